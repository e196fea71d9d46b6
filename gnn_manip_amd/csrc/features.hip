// Per-step featurisation, integrator, rollout state update and the scripted rigid-body pose.  The formulas of one row are
// step_rows.h's; the kernels here are their stand-alone and fused launches, the transposes and the host entry points.
#include "common.h"
#include "step_rows.h"

namespace gm {

int to_params(const gm_feature_desc* d, FeatParams* p, const char* who) {
    GM_REQUIRE(d != nullptr, GM_ERR_INVALID_ARGUMENT, "%s: null feature descriptor", who);
    GM_REQUIRE(d->k_steps >= 2 && d->k_steps <= 64, GM_ERR_INVALID_ARGUMENT, "%s: k_steps=%d out of range", who, d->k_steps);
    GM_REQUIRE(d->data_dim >= 4 && d->cart_col >= 0 && d->cart_col + 3 <= d->data_dim, GM_ERR_INVALID_ARGUMENT,
               "%s: bad cartesian columns", who);
    GM_REQUIRE(d->material_col >= 0 && d->material_col < d->data_dim, GM_ERR_INVALID_ARGUMENT, "%s: bad material column", who);
    GM_REQUIRE(d->control_col < 0 || d->control_col + 3 <= d->data_dim, GM_ERR_INVALID_ARGUMENT, "%s: bad control columns", who);
    GM_REQUIRE(d->conn_r > 0.0, GM_ERR_INVALID_ARGUMENT, "%s: conn_r must be > 0", who);
    p->k = d->k_steps; p->D = d->data_dim; p->cart = d->cart_col; p->mat = d->material_col; p->ctrl = d->control_col;
    p->r = (float)d->conn_r;
    for (int a = 0; a < 3; ++a) {
        p->vm[a] = d->vel_mean[a]; p->vs[a] = d->vel_std[a];
        p->am[a] = d->acc_mean[a]; p->as[a] = d->acc_std[a];
        p->lo[a] = d->lower_bounds[a]; p->hi[a] = d->upper_bounds[a];
    }
    return GM_OK;
}

// one thread per row, 256 per workgroup
template <class Kernel, class... Args>
static int launch_rows(Kernel kernel, int64_t rows, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, s, args...);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

__global__ void __launch_bounds__(256) node_features_kernel(const float* __restrict__ obs, int64_t n, FeatParams P,
                                                             float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    node_features_row(obs + i * P.D, n * P.D, P, out + i * node_feature_dim(P.k, P.ctrl));
}

// reference edge order
__global__ void __launch_bounds__(256) edge_features_kernel(const float* __restrict__ pos, int64_t stride,
                                                             const int64_t* __restrict__ snd,
                                                             const int64_t* __restrict__ rcv, int64_t e, float cr,
                                                             float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e) return;
    *reinterpret_cast<float4*>(out + i * 4) = edge_feature(pos + snd[i] * stride, pos + rcv[i] * stride, cr);
}

// same values, destination-sorted order.  The feature is (p_sender - p_receiver) / r with sender = edge_index[0]: that is
// src[p] -> dst[p] for flow 0 and dst[p] -> src[p] for flow 1 (the header records which row the structure aggregates at)
__global__ void __launch_bounds__(256) edge_features_csr_kernel(const float* __restrict__ pos, int64_t stride,
                                                                 const CsrHeader* __restrict__ hdr,
                                                                 const int* __restrict__ src, const int* __restrict__ dst,
                                                                 float cr, float* __restrict__ out) {
    const int e = hdr->n_edges;
    const bool swap = hdr->flow != 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = swap ? dst[i] : src[i], r = swap ? src[i] : dst[i];
        *reinterpret_cast<float4*>(out + i * 4) = edge_feature(pos + s * stride, pos + r * stride, cr);
    }
}

__global__ void __launch_bounds__(256) integrate_kernel(const float* __restrict__ pred, const float* __restrict__ obs,
                                                         int64_t n, FeatParams P, float* __restrict__ next_pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t fs = n * P.D;
    const float* l1 = obs + (int64_t)(P.k - 1) * fs + i * P.D + P.cart;
    const float3 nxt = integrate_row(l1, l1 - fs, pred + i * 3, P);
    next_pos[i * 3] = nxt.x; next_pos[i * 3 + 1] = nxt.y; next_pos[i * 3 + 2] = nxt.z;
}

// rollout step, fused: state_pre + node features (one thread owns row i of every frame) -- and, as the step's first launch, the
// resets of everything the step's later launches build on (StepClear: graph / destination-sort workspaces, scan states, agg).
// Rec: empty -- the scripted drive, `target` its pose -- or one RecordedDrive: the recorded control in place of the scripted one,
// and the step's record (the last frame as it then stands) written by the same thread, at the caller's row
template <class... Rec>
__global__ void __launch_bounds__(256) pre_features_kernel(float* __restrict__ obs, int64_t n, FeatParams P,
                                                            const int* __restrict__ rank, const float* __restrict__ target,
                                                            float* __restrict__ out, StepClear clr, Rec... rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    step_clear_run(clr, i, (long long)gridDim.x * blockDim.x);
    if (i >= n) return;
    const int64_t fs = n * P.D;
    float* row = obs + i * P.D;
    if constexpr (sizeof...(Rec) > 0) {
        const RecordedDrive& R = (rec, ...);
        float* last = row + (int64_t)(P.k - 1) * fs;
        const int64_t c = R.row_map ? (int64_t)R.row_map[i] : i;
        if (rank && P.ctrl >= 0 && rank[i] >= 0) recorded_control_row(last, P, R.frame + c * P.D);
        if (R.record)
            for (int d = 0; d < P.D; ++d) R.record[c * P.D + d] = last[d];
    } else if (rank && P.ctrl >= 0) {
        const int rk = rank[i];
        if (rk >= 0) control_overwrite_row(row + (int64_t)(P.k - 1) * fs, P, target ? target + (int64_t)rk * 3 : nullptr);
    }
    node_features_row(row, fs, P, out + i * node_feature_dim(P.k, P.ctrl));
}

// rollout step, fused: integrator + window shift + write-back (+ optional copy of the prediction).  Rec as above: under the
// recorded drive EVERY row takes its integrated position, then a rigid row's xyz the recorded one, and the copy of the
// prediction goes to the caller's row
template <class... Rec>
__global__ void __launch_bounds__(256) integrate_post_kernel(float* __restrict__ obs, int64_t n, FeatParams P,
                                                              const float* __restrict__ pred, const int* __restrict__ rank,
                                                              const float* __restrict__ target, float* __restrict__ pred_out, Rec... rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t fs = n * P.D;
    float* row = obs + i * P.D;
    const float* l1 = row + (int64_t)(P.k - 1) * fs + P.cart;
    if constexpr (sizeof...(Rec) > 0) {
        const RecordedDrive& R = (rec, ...);
        const int64_t c = R.row_map ? (int64_t)R.row_map[i] : i;
        if (R.pred) {
#pragma unroll
            for (int a = 0; a < 3; ++a) R.pred[c * 3 + a] = pred[i * 3 + a];
        }
        const float3 nxt = integrate_row(l1, l1 - fs, pred + i * 3, P);
        shift_write_row(row, fs, P, -1, nxt, nullptr);
        if (rank && rank[i] >= 0) recorded_pose_row(row + (int64_t)(P.k - 1) * fs, P, R.frame + c * P.D);
    } else {
        if (pred_out) {
#pragma unroll
            for (int a = 0; a < 3; ++a) pred_out[i * 3 + a] = pred[i * 3 + a];
        }
        const float3 nxt = integrate_row(l1, l1 - fs, pred + i * 3, P);
        const int rk = rank ? rank[i] : -1;
        shift_write_row(row, fs, P, rk, nxt, (rk >= 0 && target) ? target + (int64_t)rk * 3 : nullptr);
    }
}

// rank of each rigid row (material == 1) among the rigid rows; one block, running carry
__global__ void __launch_bounds__(1024) rigid_rank_kernel(const float* __restrict__ obs, int64_t n, FeatParams P,
                                                           int* __restrict__ rank, int* __restrict__ n_rigid) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const float* last = obs + (int64_t)(P.k - 1) * n * P.D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t b = 0; b < n; b += 1024) {
        int64_t i = b + threadIdx.x;
        int f = (i < n && last[i * P.D + P.mat] == 1.0f) ? 1 : 0;
        int incl = f;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int base = carry_s;
        for (int w = 0; w < wave; ++w) base += wsum[w];
        if (i < n) rank[i] = f ? base + incl - 1 : -1;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = base + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0 && n_rigid) *n_rigid = carry_s;
}

__global__ void __launch_bounds__(256) state_pre_kernel(float* __restrict__ obs, int64_t n, FeatParams P,
                                                         const int* __restrict__ rank, const float* __restrict__ target) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int rk = rank[i];
    if (rk < 0) return;
    control_overwrite_row(obs + (int64_t)(P.k - 1) * n * P.D + i * P.D, P, target ? target + (int64_t)rk * 3 : nullptr);
}

__global__ void __launch_bounds__(256) state_post_kernel(float* __restrict__ obs, int64_t n, FeatParams P,
                                                          const float* __restrict__ next_pos,
                                                          const int* __restrict__ rank, const float* __restrict__ target) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int rk = rank ? rank[i] : -1;
    const float* np = next_pos + i * 3;
    const float3 nxt = rk < 0 ? make_float3(np[0], np[1], np[2]) : make_float3(0.f, 0.f, 0.f);   // read for the rows that take it only
    shift_write_row(obs + i * P.D, n * P.D, P, rk, nxt, (rk >= 0 && target) ? target + (int64_t)rk * 3 : nullptr);
}

// one half of the recorded drive on the last frame, no shift: what = GM_RECORDED_CONTROL / GM_RECORDED_POSE
__global__ void __launch_bounds__(256) state_recorded_kernel(float* __restrict__ obs, int64_t n, FeatParams P, const int* __restrict__ rank,
                                                              const float* __restrict__ frame, const int* __restrict__ row_map, int what) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || rank[i] < 0) return;
    float* last = obs + (int64_t)(P.k - 1) * n * P.D + i * P.D;
    const float* fr = frame + (row_map ? (int64_t)row_map[i] : i) * P.D;
    if (what == GM_RECORDED_CONTROL) recorded_control_row(last, P, fr);
    else recorded_pose_row(last, P, fr);
}

// Squared-error sums of a recorded rollout, one workgroup per (step, graph).  Thread t walks the graph's rows t, t + 256, ... in
// order, then the 256 partial sums go down a fixed tree in LDS: one order of additions per (step, graph) whatever the grid, no
// atomics.  Every term is formed in float64 from the float32 inputs, without contraction into multiply-adds, so a term has the
// bits of the same expression on a host.
// Ragged: nothing (graph g owns rows [g n_per, (g + 1) n_per)), or RaggedOffsets (rows [off[g], off[g + 1]), n_per = the number of
// graphs): g is the workgroup's, so the table is read where it came, in the kernel arguments
template <typename... Ragged>
__global__ void __launch_bounds__(256) rollout_errors_kernel(const float* __restrict__ rec, const float* __restrict__ pred,
                                                              const float* __restrict__ sim, int64_t first, int64_t n, int64_t n_per,
                                                              FeatParams P, double* __restrict__ sums, Ragged... ragged) {
#pragma clang fp contract(off)
    __shared__ double red[4][256];
    const int tid = threadIdx.x;
    const int64_t graphs = sizeof...(Ragged) != 0 ? n_per : n / n_per;
    const int64_t step = blockIdx.x / graphs, g = blockIdx.x - step * graphs;
    int64_t row_lo = g * n_per, row_hi = (g + 1) * n_per;
    if constexpr (sizeof...(Ragged) != 0) ((row_lo = ragged.off[g], row_hi = ragged.off[g + 1]), ...);
    const int64_t fs = n * P.D;
    const float* rf = rec + step * fs;
    const float* gf = sim + (first + step) * fs;
    double s_all = 0.0, s_cof = 0.0, s_acc = 0.0, cnt = 0.0;
    for (int64_t r = row_lo + tid; r < row_hi; r += 256) {
        const float* a = rf + r * P.D + P.cart;
        const float* b = gf + r * P.D + P.cart;
        double e = 0.0;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double d = (double)a[x] - (double)b[x];
            e += d * d;
        }
        s_all += e;
        if (gf[r * P.D + P.mat] != 0.0f) continue;
        s_cof += e;
        cnt += 1.0;
        if (!pred) continue;
        double ea = 0.0;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double acc = ((double)b[fs + x] - 2.0 * (double)b[x]) + (double)b[x - fs];
            const double d = (double)pred[(step * n + r) * 3 + x] - (acc - (double)P.am[x]) / (double)P.as[x];
            ea += d * d;
        }
        s_acc += ea;
    }
    red[0][tid] = s_all; red[1][tid] = s_cof; red[2][tid] = s_acc; red[3][tid] = cnt;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + w];
        }
        __syncthreads();
    }
    if (tid < 4) sums[(int64_t)blockIdx.x * 4 + tid] = red[tid][0];
}

// traj_utils.py:167-194: rotation about X in the cup frame with the y/z axis swap
__global__ void __launch_bounds__(256) rigid_transform_kernel(const float* __restrict__ init, int64_t nr,
                                                               const float* __restrict__ cst, int64_t steps, float tx,
                                                               float ty, float tz, float* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nr * steps) return;
    const int64_t t = id / nr, i = id - t * nr;
    const float c = cst[t * 3], s = cst[t * 3 + 1], typ = cst[t * 3 + 2];
    const float i0 = __fsub_rn(tx, init[i * 3 + 0]);
    const float i1 = __fsub_rn(ty, init[i * 3 + 2]);
    const float i2 = __fsub_rn(tz, init[i * 3 + 1]);
    const float p0 = __fadd_rn(i0, tx);
    const float p1 = __fadd_rn(__fmaf_rn(-s, i2, __fmul_rn(c, i1)), typ);
    const float p2 = __fadd_rn(__fmaf_rn(c, i2, __fmul_rn(s, i1)), tz);
    out[id * 3 + 0] = p0;
    out[id * 3 + 2] = p1;
    out[id * 3 + 1] = p2;
}

// transpose of rigid_transform_kernel w.r.t. its per-step row (cos, sin, ty_init[1] + translation): the map is linear in it, with
// coefficients i1 = ty - init[i][2], i2 = tz - init[i][1].  One workgroup per step.  A thread walks its particles (tid, tid + 256,
// ...) in order, the 256 partial sums go down a fixed tree in LDS: no atomics, the same bits every time.  The sums are carried in
// float64 (the differences and products are then exact, the additions round at 2^-53) and rounded to float32 once at the end.
__global__ void __launch_bounds__(256) rigid_transform_bwd_kernel(const float* __restrict__ init, int64_t nr, float ty, float tz,
                                                                   const float* __restrict__ g, float* __restrict__ d_cst) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const float* gt = g + t * nr * 3;
    double dc = 0.0, ds = 0.0, dt = 0.0;
    for (int64_t i = tid; i < nr; i += 256) {
        const double i1 = (double)ty - (double)init[i * 3 + 2];
        const double i2 = (double)tz - (double)init[i * 3 + 1];
        const double g1 = gt[i * 3 + 1], g2 = gt[i * 3 + 2];   // out[.][1] = p2, out[.][2] = p1
        dc += g2 * i1 + g1 * i2;
        ds += g1 * i1 - g2 * i2;
        dt += g2;
    }
    red[0][tid] = dc; red[1][tid] = ds; red[2][tid] = dt;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) red[a][tid] += red[a][tid + w];
        }
        __syncthreads();
    }
    if (tid < 3) d_cst[t * 3 + tid] = (float)red[tid][0];
}

// ---- renumbered rollout: rows of the [k, N, D] state move as whole rows (D floats), one thread per (frame, row)
__global__ void __launch_bounds__(256) renumber_gather_kernel(const float* __restrict__ in, float* __restrict__ out, int k, int64_t n, int D,
                                                               const int* __restrict__ perm, const GraphHeader* __restrict__ ghdr,
                                                               const int* __restrict__ total_in, int* __restrict__ total_out,
                                                               const int* __restrict__ rank_caller, int* __restrict__ rank_out) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)k * n) return;
    const int64_t t = id / n, j = id - t * n;
    const int64_t src = ghdr->order_skip ? j : (int64_t)perm[j];
    const float* a = in + (t * n + src) * D;
    float* b = out + (t * n + j) * D;
    for (int d = 0; d < D; ++d) b[d] = a[d];
    if (t == 0) {
        const int tot = total_in ? total_in[src] : (int)src;
        total_out[j] = tot;
        if (rank_out) rank_out[j] = rank_caller[tot];
    }
}
__global__ void __launch_bounds__(256) renumber_scatter_kernel(const float* __restrict__ in, float* __restrict__ out, int frames, int64_t n, int D,
                                                                const int* __restrict__ total) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)frames * n) return;
    const int64_t t = id / n, j = id - t * n;
    const float* a = in + (t * n + j) * D;
    float* b = out + (t * n + (int64_t)total[j]) * D;
    for (int d = 0; d < D; ++d) b[d] = a[d];
}
int renumber_gather(const float* in, float* out, int k, int64_t n, int D, const int* perm, const void* graph_ws, const int* total_in,
                    int* total_out, const int* rank_caller, int* rank_out, hipStream_t s) {
    if (n <= 0 || k <= 0) return GM_OK;
    return launch_rows(renumber_gather_kernel, (int64_t)k * n, s, in, out, k, n, D, perm, static_cast<const GraphHeader*>(graph_ws), total_in,
                       total_out, rank_caller, rank_out);
}
int renumber_scatter(const float* in, float* out, int frames, int64_t n, int D, const int* total, hipStream_t s) {
    if (n <= 0 || frames <= 0) return GM_OK;
    return launch_rows(renumber_scatter_kernel, (int64_t)frames * n, s, in, out, frames, n, D, total);
}

int rollout_pre_features(float* obs, int64_t n, const gm_feature_desc* d, const int* rank, const float* target, float* out,
                         hipStream_t s, const StepClear* clear, const RecordedDrive* rec) {
    FeatParams P;
    int rc = to_params(d, &P, "gm_rollout_step");
    if (rc != GM_OK) return rc;
    const StepClear clr = clear ? *clear : StepClear{};
    if (rec) return launch_rows(pre_features_kernel<RecordedDrive>, n, s, obs, n, P, rank, target, out, clr, *rec);
    return launch_rows(pre_features_kernel<>, n, s, obs, n, P, rank, target, out, clr);
}

int rollout_integrate_post(float* obs, int64_t n, const gm_feature_desc* d, const float* pred, const int* rank,
                           const float* target, float* pred_out, hipStream_t s, const RecordedDrive* rec) {
    FeatParams P;
    int rc = to_params(d, &P, "gm_rollout_step");
    if (rc != GM_OK) return rc;
    if (rec) return launch_rows(integrate_post_kernel<RecordedDrive>, n, s, obs, n, P, pred, rank, target, pred_out, *rec);
    return launch_rows(integrate_post_kernel<>, n, s, obs, n, P, pred, rank, target, pred_out);
}


// ---- backward of the per-step functions (differentiable rollout step).  Each output is written in full, by one thread per row:
// no atomics, the same bits every time.

// zeros in one particle's row of every frame of a gradient window (row = its row of frame 0)
__device__ __forceinline__ void zero_window_row(float* __restrict__ row, int64_t fs, const FeatParams& P) {
    for (int t = 0; t < P.k; ++t)
        for (int d = 0; d < P.D; ++d) row[t * fs + d] = 0.f;
}

// transpose of node_features_kernel: d_obs[k][n][D] from d_out[n][F]
__global__ void __launch_bounds__(256) node_features_bwd_kernel(const float* __restrict__ obs, int64_t n, FeatParams P,
                                                                 const float* __restrict__ g, float* __restrict__ d_obs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* gi = g + i * node_feature_dim(P.k, P.ctrl);
    const int64_t fs = n * P.D;
    float* row = d_obs + i * P.D;
    zero_window_row(row, fs, P);
    // velocity t (frames t, t + 1): +g / vel_std on frame t + 1, -g / vel_std on frame t
    for (int t = 0; t < P.k; ++t) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float v = 0.f;
            if (t >= 1) v = __fdiv_rn(gi[(t - 1) * 3 + a], P.vs[a]);
            if (t + 1 < P.k) v = __fsub_rn(v, __fdiv_rn(gi[t * 3 + a], P.vs[a]));
            row[t * fs + P.cart + a] = v;
        }
    }
    const float* b = gi + 3 * (P.k - 1);
    const float* last_in = obs + (int64_t)(P.k - 1) * fs + i * P.D;
    float* last = row + (int64_t)(P.k - 1) * fs;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // the forward's own unclamped values; the gradient passes where they lie in [-1, 1] (torch.clamp's rule)
        float l, u;
        boundary_terms(last_in[P.cart + a], P, a, l, u);
        float v = last[P.cart + a];
        if (in_unit(l)) v = __fadd_rn(v, __fdiv_rn(b[a], P.r));
        if (in_unit(u)) v = __fsub_rn(v, __fdiv_rn(b[3 + a], P.r));
        last[P.cart + a] = v;
    }
    if (P.ctrl >= 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) last[P.ctrl + a] = __fdiv_rn(b[7 + a], P.vs[a]);
    }
}

// transpose of integrate_kernel: next = 2 l1 - l2 + pred * acc_std + acc_mean
__global__ void __launch_bounds__(256) integrate_bwd_kernel(const float* __restrict__ g, int64_t n, FeatParams P,
                                                             float* __restrict__ d_pred, float* __restrict__ d_obs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t fs = n * P.D;
    float* row = d_obs + i * P.D;
    zero_window_row(row, fs, P);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ga = g[i * 3 + a];
        d_pred[i * 3 + a] = __fmul_rn(ga, P.as[a]);
        row[(int64_t)(P.k - 1) * fs + P.cart + a] = __fmul_rn(2.f, ga);
        row[(int64_t)(P.k - 2) * fs + P.cart + a] = -ga;
    }
}

// transpose of state_pre_kernel on one particle row, in place on `last` = that row of the last frame of the gradient: a rigid row's
// control columns were overwritten by (target - xyz), or by xyz without a target, so their old values get nothing and xyz gets
// -+ the control gradient on top of its own; gt (or nullptr) = the row of d_rigid_target the particle owns, written in full
// (zeros without a target).  post_t (or nullptr): what state_post's transpose gave the same row of d_rigid_target, added first.
__device__ __forceinline__ void state_pre_bwd_row(float* __restrict__ last, const FeatParams& P, bool has_target, float* __restrict__ gt,
                                                  const float* __restrict__ post_t) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float gc = last[P.ctrl + a];
        const float gx = last[P.cart + a];
        last[P.cart + a] = has_target ? __fsub_rn(gx, gc) : __fadd_rn(gx, gc);
        last[P.ctrl + a] = 0.f;
        if (gt) gt[a] = has_target ? (post_t ? __fadd_rn(post_t[a], gc) : gc) : 0.f;
    }
}

// transpose of state_pre_kernel: d_before[k][n][D] from d_after[k][n][D]; one thread owns row i of every frame
__global__ void __launch_bounds__(256) state_pre_bwd_kernel(const float* __restrict__ d_after, int64_t n, FeatParams P,
                                                             const int* __restrict__ rank, int has_target, float* __restrict__ d_before,
                                                             float* __restrict__ d_target) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t fs = n * P.D;
    const float* in = d_after + i * P.D;
    float* row = d_before + i * P.D;
    for (int t = 0; t < P.k; ++t)
        for (int d = 0; d < P.D; ++d) row[t * fs + d] = in[t * fs + d];
    const int rk = rank[i];
    if (rk >= 0) state_pre_bwd_row(row + (int64_t)(P.k - 1) * fs, P, has_target != 0, d_target ? d_target + (int64_t)rk * 3 : nullptr, nullptr);
}

// transpose of state_post_kernel: frame t of the window before the update is frame t - 1 after it (frame 0 fell out: zero); the
// last frame before it also fed the last frame after it -- every column but xyz for a non-rigid row (xyz came from next_pos), the
// whole row for a rigid one, less xyz where a scripted pose replaced it -- so its gradient is the sum of those two terms
__global__ void __launch_bounds__(256) state_post_bwd_kernel(const float* __restrict__ d_after, int64_t n, FeatParams P,
                                                              const int* __restrict__ rank, int has_target, float* __restrict__ d_before,
                                                              float* __restrict__ d_next, float* __restrict__ d_target) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t fs = n * P.D;
    const float* in = d_after + i * P.D;
    float* row = d_before + i * P.D;
    for (int d = 0; d < P.D; ++d) row[d] = 0.f;
    for (int t = 1; t + 1 < P.k; ++t)
        for (int d = 0; d < P.D; ++d) row[t * fs + d] = in[(t - 1) * fs + d];
    const int rk = rank ? rank[i] : -1;
    const float* g_last = in + (int64_t)(P.k - 1) * fs;
    const float* g_prev = in + (int64_t)(P.k - 2) * fs;
    float* last = row + (int64_t)(P.k - 1) * fs;
    const bool xyz_replaced = rk < 0 || has_target;
    for (int d = 0; d < P.D; ++d) {
        const bool xyz = d >= P.cart && d < P.cart + 3;
        last[d] = (xyz && xyz_replaced) ? g_prev[d] : __fadd_rn(g_prev[d], g_last[d]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d_next[i * 3 + a] = rk < 0 ? g_last[P.cart + a] : 0.f;
        if (rk >= 0 && d_target) d_target[(int64_t)rk * 3 + a] = has_target ? g_last[P.cart + a] : 0.f;
    }
}

// the gradient of a rollout step with respect to its pre-step window, assembled: one thread owns row i of every frame and adds,
// in this order, state_post's transpose, the integrator's, the node features' and -- xyz of the last frame -- the edge features',
// and last -- every column of the last frame, g_rec given -- the caller's gradient on the step's record (the last frame after
// state_pre's overwrite, which is where this sum lives); then the transpose of state_pre on that sum (pre != 0: the step ran the
// overwrite) and the row of d_rigid_target it owns: state_post's share, then state_pre's
__global__ void __launch_bounds__(256) step_assemble_bwd_kernel(const float* __restrict__ g_post, const float* __restrict__ g_int,
                                                                 const float* __restrict__ g_nodes, const float* __restrict__ g_pos,
                                                                 const float* __restrict__ t_post, const float* __restrict__ g_rec,
                                                                 int64_t n, FeatParams P, const int* __restrict__ rank, int has_target, int pre,
                                                                 float* __restrict__ d_before, float* __restrict__ d_target) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t fs = n * P.D;
    float* row = d_before + i * P.D;
    for (int t = 0; t < P.k; ++t)
        for (int d = 0; d < P.D; ++d) {
            const int64_t at = i * P.D + t * fs + d;
            float v = __fadd_rn(__fadd_rn(g_post[at], g_int[at]), g_nodes[at]);
            if (t == P.k - 1 && d >= P.cart && d < P.cart + 3) v = __fadd_rn(v, g_pos[i * 3 + (d - P.cart)]);
            if (t == P.k - 1 && g_rec) v = __fadd_rn(v, g_rec[i * P.D + d]);
            row[t * fs + d] = v;
        }
    const int rk = rank ? rank[i] : -1;
    if (rk < 0) return;
    float* gt = d_target ? d_target + (int64_t)rk * 3 : nullptr;
    if (pre) {
        state_pre_bwd_row(row + (int64_t)(P.k - 1) * fs, P, has_target != 0, gt, t_post + (int64_t)rk * 3);
    } else if (gt) {
#pragma unroll
        for (int a = 0; a < 3; ++a) gt[a] = has_target ? t_post[(int64_t)rk * 3 + a] : 0.f;
    }
}

// edge_index [2][e] of the two sorts from the caller's separate rows
__global__ void __launch_bounds__(256) edge_pair_kernel(const int64_t* __restrict__ snd, const int64_t* __restrict__ rcv, int64_t e,
                                                         int64_t* __restrict__ ei) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e) return;
    ei[i] = snd[i];
    ei[e + i] = rcv[i];
}

// per edge, in the caller's order: the gradient on p_s, (g[0:3] + g[3] d / |d|) / r with d = (p_s - p_r) / r; 0 for the norm's
// term where |d| = 0 (torch.norm's subgradient).  An edge with an index out of range contributes nothing (the sorts leave it out).
__global__ void __launch_bounds__(256) edge_features_bwd_edge_kernel(const float* __restrict__ pos, int64_t stride,
                                                                      const int64_t* __restrict__ snd, const int64_t* __restrict__ rcv,
                                                                      int64_t n, int64_t e, float cr, const float* __restrict__ g,
                                                                      float* __restrict__ ge) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e) return;
    const int64_t s = snd[i], r = rcv[i];
    float o[3] = {0.f, 0.f, 0.f};
    if (s >= 0 && s < n && r >= 0 && r < n) {
        const float4 f = edge_feature(pos + s * stride, pos + r * stride, cr);   // the forward's (d, |d|)
        const float d[3] = {f.x, f.y, f.z};
        const float4 gv = *reinterpret_cast<const float4*>(g + i * 4);
        const float gg[3] = {gv.x, gv.y, gv.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float v = gg[a];
            if (f.w > 0.f) v = __fadd_rn(v, __fdiv_rn(__fmul_rn(gv.w, d[a]), f.w));
            o[a] = __fdiv_rn(v, cr);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) ge[i * 3 + a] = o[a];
}

// per node: + the edges it sends (segments of the sort by sender), - the edges it receives (segments of the sort by receiver),
// each segment in ascending edge id (the sorts' own order): fixed order, no atomics
__global__ void __launch_bounds__(256) edge_features_bwd_node_kernel(const int* __restrict__ snd_ptr, const int* __restrict__ snd_eid,
                                                                      const int* __restrict__ rcv_ptr, const int* __restrict__ rcv_eid,
                                                                      const float* __restrict__ ge, int64_t n, float* __restrict__ d_pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int p = snd_ptr[i], p1 = snd_ptr[i + 1]; p < p1; ++p) {
        const float* v = ge + (int64_t)snd_eid[p] * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[a] = __fadd_rn(acc[a], v[a]);
    }
    for (int p = rcv_ptr[i], p1 = rcv_ptr[i + 1]; p < p1; ++p) {
        const float* v = ge + (int64_t)rcv_eid[p] * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[a] = __fsub_rn(acc[a], v[a]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) d_pos[i * 3 + a] = acc[a];
}

// workspace of gm_edge_features_backward: the [2][e] index the sorts read, the sort by receiver (flow 0) and by sender (flow 1),
// the per-edge gradients
struct EdgeBwdWs {
    int64_t* ei;
    char *csr_rcv, *csr_snd;
    size_t csr_bytes;
    float* ge;
    size_t bytes;
};
static EdgeBwdWs carve_edge_bwd(void* ws, int64_t n, int64_t e) {
    EdgeBwdWs w;
    Carver c(ws);
    w.ei = c.take<int64_t>((size_t)2 * e);
    w.csr_bytes = gm_csr_workspace_bytes(n, e);
    w.csr_rcv = c.take<char>(w.csr_bytes);
    w.csr_snd = c.take<char>(w.csr_bytes);
    w.ge = c.take<float>((size_t)3 * e);
    w.bytes = c.used();
    return w;
}

int rollout_assemble_backward(const float* g_post, const float* g_int, const float* g_nodes, const float* g_pos, const float* t_post,
                              const float* g_rec, int64_t n, const gm_feature_desc* d, const int* rank, bool has_target, float* d_before,
                              float* d_target, hipStream_t s) {
    FeatParams P;
    int rc = to_params(d, &P, "gm_rollout_step_backward");
    if (rc != GM_OK) return rc;
    return launch_rows(step_assemble_bwd_kernel, n, s, g_post, g_int, g_nodes, g_pos, t_post, g_rec, n, P, rank, has_target ? 1 : 0,
                       (rank && P.ctrl >= 0) ? 1 : 0, d_before, d_target);
}

}  // namespace gm

using namespace gm;

extern "C" {

int gm_node_features(const float* obs, int64_t n, const gm_feature_desc* desc, float* out, void* stream) {
    gm::DevGuard dev_guard(obs);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_node_features");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n >= 0 && (n == 0 || (obs && out)), GM_ERR_INVALID_ARGUMENT, "gm_node_features: null pointer");
    if (n == 0) return GM_OK;
    return launch_rows(node_features_kernel, n, (hipStream_t)stream, obs, n, P, out);
}

int gm_edge_features(const float* pos, int64_t pos_stride, const int64_t* senders, const int64_t* receivers,
                     int64_t e, float conn_r, float* out, void* stream) {
    gm::DevGuard dev_guard(pos);
    GM_REQUIRE(e >= 0 && (e == 0 || (pos && senders && receivers && out)), GM_ERR_INVALID_ARGUMENT, "gm_edge_features: null pointer");
    GM_REQUIRE(conn_r > 0.f && pos_stride >= 3, GM_ERR_INVALID_ARGUMENT, "gm_edge_features: bad conn_r / stride");
    if (e == 0) return GM_OK;
    return launch_rows(edge_features_kernel, e, (hipStream_t)stream, pos, pos_stride, senders, receivers, e, conn_r, out);
}

int gm_edge_features_csr(const float* pos, int64_t pos_stride, const void* csr_ws, int64_t n, int64_t cap,
                         float conn_r, float* out, void* stream) {
    gm::DevGuard dev_guard(pos);
    GM_REQUIRE(pos && csr_ws && out, GM_ERR_INVALID_ARGUMENT, "gm_edge_features_csr: null pointer");
    GM_REQUIRE(conn_r > 0.f && pos_stride >= 3, GM_ERR_INVALID_ARGUMENT, "gm_edge_features_csr: bad conn_r / stride");
    if (cap == 0) return GM_OK;
    CsrWs c = carve_csr(const_cast<void*>(csr_ws), n, cap);
    int64_t nb = cdiv(cap, 256);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(edge_features_csr_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pos, pos_stride,
                       c.hdr, c.src, c.dst, conn_r, out);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

int gm_integrate(const float* pred, const float* obs, int64_t n, const gm_feature_desc* desc, float* next_pos,
                 void* stream) {
    gm::DevGuard dev_guard(obs);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_integrate");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n >= 0 && (n == 0 || (pred && obs && next_pos)), GM_ERR_INVALID_ARGUMENT, "gm_integrate: null pointer");
    if (n == 0) return GM_OK;
    return launch_rows(integrate_kernel, n, (hipStream_t)stream, pred, obs, n, P, next_pos);
}

int gm_rigid_rank(const float* obs, int64_t n, const gm_feature_desc* desc, int32_t* rank, int32_t* n_rigid_dev,
                  void* stream) {
    gm::DevGuard dev_guard(obs);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_rigid_rank");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n >= 0 && (n == 0 || (obs && rank)), GM_ERR_INVALID_ARGUMENT, "gm_rigid_rank: null pointer");
    hipLaunchKernelGGL(rigid_rank_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, obs, n, P, rank, n_rigid_dev);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

int gm_state_pre(float* obs, int64_t n, const gm_feature_desc* desc, const int32_t* rank, const float* target,
                 void* stream) {
    gm::DevGuard dev_guard(obs);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_state_pre");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(P.ctrl >= 0, GM_ERR_INVALID_ARGUMENT, "gm_state_pre: descriptor has no control columns");
    GM_REQUIRE(n >= 0 && (n == 0 || (obs && rank)), GM_ERR_INVALID_ARGUMENT, "gm_state_pre: null pointer");
    if (n == 0) return GM_OK;
    return launch_rows(state_pre_kernel, n, (hipStream_t)stream, obs, n, P, rank, target);
}

int gm_state_post(float* obs, int64_t n, const gm_feature_desc* desc, const float* next_pos, const int32_t* rank,
                  const float* target, void* stream) {
    gm::DevGuard dev_guard(obs);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_state_post");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n >= 0 && (n == 0 || (obs && next_pos)), GM_ERR_INVALID_ARGUMENT, "gm_state_post: null pointer");
    if (n == 0) return GM_OK;
    return launch_rows(state_post_kernel, n, (hipStream_t)stream, obs, n, P, next_pos, rank, target);
}

int gm_state_recorded(float* obs, int64_t n, const gm_feature_desc* desc, const int32_t* rank, const float* frame,
                      const int32_t* row_map, int what, void* stream) {
    gm::DevGuard dev_guard(obs);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_state_recorded");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(what == GM_RECORDED_CONTROL || what == GM_RECORDED_POSE, GM_ERR_INVALID_ARGUMENT,
               "gm_state_recorded: what=%d (GM_RECORDED_CONTROL = 1, GM_RECORDED_POSE = 4)", what);
    GM_REQUIRE(what != GM_RECORDED_CONTROL || P.ctrl >= 0, GM_ERR_INVALID_ARGUMENT, "gm_state_recorded: descriptor has no control columns");
    GM_REQUIRE(n >= 0 && (n == 0 || (obs && rank && frame)), GM_ERR_INVALID_ARGUMENT, "gm_state_recorded: null pointer");
    if (n == 0) return GM_OK;
    return launch_rows(state_recorded_kernel, n, (hipStream_t)stream, obs, n, P, rank, frame, row_map, what);
}

int gm_rollout_errors(const float* record_last, const float* record_pred, const float* sim, int64_t n_frames, int64_t first_frame,
                      int64_t steps, int64_t n, const gm_feature_desc* desc, double* sums, void* stream) {
    gm::DevGuard dev_guard(sums);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_rollout_errors");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(steps >= 0 && n >= 0 && n_frames >= 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_errors: negative count");
    // the acceleration target of frame f reads frames f - 1 and f + 1 of the recording
    const int64_t lo = record_pred ? 1 : 0, hi = record_pred ? n_frames - 1 : n_frames;
    GM_REQUIRE(first_frame >= lo && first_frame <= hi && steps <= hi - first_frame, GM_ERR_INVALID_ARGUMENT,
               "gm_rollout_errors: frames [%lld, %lld) outside [%lld, %lld) of the recording%s", (long long)first_frame,
               (long long)(first_frame + steps), (long long)lo, (long long)hi, record_pred ? " (record_pred needs a frame on either side)" : "");
    const int64_t n_per = graph_nodes(desc, n);
    GM_REQUIRE(n == 0 || n % n_per == 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_errors: n_nodes is not a multiple of nodes_per_graph");
    if (steps == 0 || n == 0) return GM_OK;
    GM_REQUIRE(record_last && sim && sums, GM_ERR_INVALID_ARGUMENT, "gm_rollout_errors: null pointer");
    const int64_t blocks = steps * (n / n_per);
    GM_REQUIRE(blocks < ((int64_t)1 << 31), GM_ERR_UNSUPPORTED, "gm_rollout_errors: steps * graphs overflows the grid");
    hipLaunchKernelGGL(rollout_errors_kernel<>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, record_last, record_pred, sim,
                       first_frame, n, n_per, P, sums);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

int gm_rollout_errors_ragged(const float* record_last, const float* record_pred, const float* sim, int64_t n_frames, int64_t first_frame,
                             int64_t steps, const int64_t* graph_offsets_host, int64_t n_graphs, const gm_feature_desc* desc, double* sums,
                             void* stream) {
    const char* who = "gm_rollout_errors_ragged";
    FeatParams P;
    int rc = to_params(desc, &P, who);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(desc->nodes_per_graph == 0, GM_ERR_INVALID_ARGUMENT, "%s: nodes_per_graph=%lld, must be 0 (the graphs come in graph_offsets)", who,
               (long long)desc->nodes_per_graph);
    GM_REQUIRE(record_last && sim && sums, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    RaggedOffsets R;
    rc = ragged_offsets(graph_offsets_host, n_graphs, desc->conn_r, 1, sums, who, &R);   // no graph is built: max_neighbours plays no part
    if (rc != GM_OK) return rc;
    GM_REQUIRE(steps >= 0 && n_frames >= 0, GM_ERR_INVALID_ARGUMENT, "%s: negative count", who);
    const int64_t lo = record_pred ? 1 : 0, hi = record_pred ? n_frames - 1 : n_frames;
    GM_REQUIRE(first_frame >= lo && first_frame <= hi && steps <= hi - first_frame, GM_ERR_INVALID_ARGUMENT,
               "%s: frames [%lld, %lld) outside [%lld, %lld) of the recording%s", who, (long long)first_frame,
               (long long)(first_frame + steps), (long long)lo, (long long)hi, record_pred ? " (record_pred needs a frame on either side)" : "");
    if (steps == 0) return GM_OK;
    gm::DevGuard dev_guard(sums);
    const int64_t blocks = steps * n_graphs;
    GM_REQUIRE(blocks < ((int64_t)1 << 31), GM_ERR_UNSUPPORTED, "%s: steps * graphs overflows the grid", who);
    hipLaunchKernelGGL(rollout_errors_kernel<RaggedOffsets>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, record_last, record_pred,
                       sim, first_frame, (int64_t)R.off[R.n_graphs], n_graphs, P, sums, R);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

int gm_state_pre_backward(const float* d_obs_after, int64_t n, const gm_feature_desc* desc, const int32_t* rank, int has_target,
                          float* d_obs_before, float* d_rigid_target, void* stream) {
    gm::DevGuard dev_guard(d_obs_after);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_state_pre_backward");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(P.ctrl >= 0, GM_ERR_INVALID_ARGUMENT, "gm_state_pre_backward: descriptor has no control columns");
    GM_REQUIRE(n >= 0 && (n == 0 || (d_obs_after && d_obs_before && rank)), GM_ERR_INVALID_ARGUMENT, "gm_state_pre_backward: null pointer");
    GM_REQUIRE(d_obs_after != d_obs_before || n == 0, GM_ERR_INVALID_ARGUMENT, "gm_state_pre_backward: d_obs_before must not be d_obs_after");
    if (n == 0) return GM_OK;
    return launch_rows(state_pre_bwd_kernel, n, (hipStream_t)stream, d_obs_after, n, P, rank, has_target ? 1 : 0, d_obs_before, d_rigid_target);
}

int gm_state_post_backward(const float* d_obs_after, int64_t n, const gm_feature_desc* desc, const int32_t* rank, int has_target,
                           float* d_obs_before, float* d_next_pos, float* d_rigid_target, void* stream) {
    gm::DevGuard dev_guard(d_obs_after);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_state_post_backward");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n >= 0 && (n == 0 || (d_obs_after && d_obs_before && d_next_pos)), GM_ERR_INVALID_ARGUMENT,
               "gm_state_post_backward: null pointer");
    GM_REQUIRE(d_obs_after != d_obs_before || n == 0, GM_ERR_INVALID_ARGUMENT, "gm_state_post_backward: d_obs_before must not be d_obs_after");
    if (n == 0) return GM_OK;
    return launch_rows(state_post_bwd_kernel, n, (hipStream_t)stream, d_obs_after, n, P, rank, has_target ? 1 : 0, d_obs_before, d_next_pos,
                       d_rigid_target);
}

int gm_rigid_transform(const float* rigid_init, int64_t nr, const float* cst, int64_t steps, const float ty_init[3],
                       float* out, void* stream) {
    gm::DevGuard dev_guard(rigid_init);
    GM_REQUIRE(nr >= 0 && steps >= 0 && ty_init, GM_ERR_INVALID_ARGUMENT, "gm_rigid_transform: bad sizes");
    if (nr == 0 || steps == 0) return GM_OK;
    GM_REQUIRE(rigid_init && cst && out, GM_ERR_INVALID_ARGUMENT, "gm_rigid_transform: null pointer");
    return launch_rows(rigid_transform_kernel, nr * steps, (hipStream_t)stream, rigid_init, nr, cst, steps, ty_init[0], ty_init[1], ty_init[2], out);
}


int gm_rigid_transform_backward(const float* rigid_init, int64_t nr, const float* cst, int64_t steps, const float ty_init[3],
                                const float* d_out, float* d_cst, void* stream) {
    (void)cst;   // the transform is linear in its (cos, sin, ty) rows: their values do not enter its transpose
    GM_REQUIRE(nr >= 0 && steps >= 0 && steps < ((int64_t)1 << 31) && ty_init, GM_ERR_INVALID_ARGUMENT, "gm_rigid_transform_backward: bad sizes");
    if (steps == 0) return GM_OK;
    GM_REQUIRE(d_cst && (nr == 0 || (rigid_init && d_out)), GM_ERR_INVALID_ARGUMENT, "gm_rigid_transform_backward: null pointer");
    gm::DevGuard dev_guard(d_cst);
    hipLaunchKernelGGL(rigid_transform_bwd_kernel, dim3((unsigned)steps), dim3(256), 0, (hipStream_t)stream, rigid_init, nr, ty_init[1],
                       ty_init[2], d_out, d_cst);
    GM_LAUNCH_CHECK();
    return GM_OK;
}


size_t gm_edge_features_backward_workspace_bytes(int64_t n, int64_t e) {
    if (n < 0 || e < 0) return 0;
    return carve_edge_bwd(nullptr, n, e).bytes;
}

int gm_edge_features_backward(const float* pos, int64_t pos_stride, const int64_t* senders, const int64_t* receivers, int64_t n,
                              int64_t e, float conn_r, const float* d_out, float* d_pos, void* ws, size_t ws_bytes, void* stream) {
    gm::DevGuard dev_guard(d_pos);
    GM_REQUIRE(n >= 0 && e >= 0 && n < ((int64_t)1 << 31) && e < ((int64_t)1 << 31) / 4, GM_ERR_INVALID_ARGUMENT,
               "gm_edge_features_backward: sizes out of range");
    GM_REQUIRE(n == 0 || d_pos, GM_ERR_INVALID_ARGUMENT, "gm_edge_features_backward: null pointer");
    GM_REQUIRE(e == 0 || (pos && senders && receivers && d_out && ws), GM_ERR_INVALID_ARGUMENT, "gm_edge_features_backward: null pointer");
    GM_REQUIRE(conn_r > 0.f && pos_stride >= 3, GM_ERR_INVALID_ARGUMENT, "gm_edge_features_backward: bad conn_r / stride");
    if (n == 0) return GM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (e == 0) {
        GM_HIP_CHECK(hipMemsetAsync(d_pos, 0, (size_t)n * 3 * sizeof(float), s));
        return GM_OK;
    }
    EdgeBwdWs w = carve_edge_bwd(ws, n, e);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "gm_edge_features_backward: workspace %zu < %zu", ws_bytes, w.bytes);
    const unsigned eb = (unsigned)cdiv(e, 256);
    hipLaunchKernelGGL(edge_pair_kernel, dim3(eb), dim3(256), 0, s, senders, receivers, e, w.ei);
    hipLaunchKernelGGL(edge_features_bwd_edge_kernel, dim3(eb), dim3(256), 0, s, pos, pos_stride, senders, receivers, n, e, conn_r, d_out,
                       w.ge);
    GM_LAUNCH_CHECK();
    int rc = gm::csr_from_edge_index(w.ei, n, e, 0, w.csr_rcv, w.csr_bytes, false, s);
    if (rc == GM_OK) rc = gm::csr_from_edge_index(w.ei, n, e, 1, w.csr_snd, w.csr_bytes, false, s);
    if (rc != GM_OK) return rc;
    const CsrWs cr = carve_csr(w.csr_rcv, n, e), cs = carve_csr(w.csr_snd, n, e);
    return launch_rows(edge_features_bwd_node_kernel, n, s, cs.in_ptr, cs.eid, cr.in_ptr, cr.eid, w.ge, n, d_pos);
}

int gm_node_features_backward(const float* obs, int64_t n, const gm_feature_desc* desc, const float* d_out, float* d_obs, void* stream) {
    gm::DevGuard dev_guard(obs);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_node_features_backward");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n >= 0 && (n == 0 || (obs && d_out && d_obs)), GM_ERR_INVALID_ARGUMENT, "gm_node_features_backward: null pointer");
    if (n == 0) return GM_OK;
    return launch_rows(node_features_bwd_kernel, n, (hipStream_t)stream, obs, n, P, d_out, d_obs);
}

int gm_integrate_backward(const float* d_next_pos, int64_t n, const gm_feature_desc* desc, float* d_pred, float* d_obs, void* stream) {
    gm::DevGuard dev_guard(d_next_pos);
    FeatParams P;
    int rc = to_params(desc, &P, "gm_integrate_backward");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n >= 0 && (n == 0 || (d_next_pos && d_pred && d_obs)), GM_ERR_INVALID_ARGUMENT, "gm_integrate_backward: null pointer");
    if (n == 0) return GM_OK;
    return launch_rows(integrate_bwd_kernel, n, (hipStream_t)stream, d_next_pos, n, P, d_pred, d_obs);
}

}  // extern "C"
