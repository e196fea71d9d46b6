// Debiased Sinkhorn divergence between two uniform point clouds in 3-D, on the device -- the planner's
// loss `geomloss.SamplesLoss(loss="sinkhorn", p=2, blur=.05)` (reference call sites traj_utils.py:69,279;
// SURVEY.md section 8f-2).  geomloss is not part of the reference tree (pip dependency, version not pinned,
// environment.yml:25): this restates its published algorithm (Feydy et al., "Interpolating between Optimal
// Transport and MMD using Sinkhorn Divergences", AISTATS 2019; geomloss sinkhorn_divergence.py: log-domain
// symmetric Sinkhorn with epsilon-scaling, debiasing, one final extrapolation):
//     C(x, y) = |x - y|^2 / 2,  eps schedule: diameter^2, then exp(arange(2 log diameter, 2 log blur, 2 log scaling)), blur^2
//     softmin_eps(C, h)_i = -eps log sum_j exp(h_j - C_ij / eps)
//     S = mean_i (b_x - a_x)_i + mean_j (a_y - b_y)_j
// No N x M matrix is ever stored: every softmin recomputes the distances it needs from the coordinates
// ("online" reduction): 6 flops + one exp per pair, two passes (max, then sum) -- exp-throughput bound,
// the clouds and potentials live in L2.
//
// Gradient (gm_sinkhorn_divergence_batched_backward): geomloss's convention for the tensorized backend, read from its published
// code and -- like the forward -- UNPINNED against geomloss itself.  The potentials are detached and only the last
// extrapolation is differentiated, with the right-hand cloud of every cost matrix detached (C_xy = cost(x, y.detach()),
// C_xx = cost(x, x.detach()), ...).  With a_i = 1/N, b_j = 1/M, eps = blur^2 and o[k] the input of the last extrapolation:
//     dS/dx_i = a_i (T_xx(x_i) - T_xy(x_i)),   T_xy(x_i) = sum_j softmax_j(log b_j + o[2]_j / eps - C(x_i, y_j) / eps) y_j
//                                              T_xx(x_i) = sum_k softmax_k(log a_k + o[0]_k / eps - C(x_i, x_k) / eps) x_k
//     dS/dy_j = b_j (T_yy(y_j) - T_yx(y_j))    (o[1] over y, o[3] over x)
// The output q[k] of the last extrapolation is each row's log-normaliser, so one pass suffices (sinkhorn_grad_kernel): the
// weights exp(h_j - C_ij / eps + q_i / eps) are near 1 without a running max, and dividing by their sum at the end makes the
// result independent of the rounding of q_i.  Again no N x M matrix: one exp and ~14 flops per pair, the cross and the self
// barycentre of a row in one launch.
//
// Weighted clouds (gm_sinkhorn_divergence_weighted and its backward, geomloss's loss(a, x, b, y)): the same kernels in a second
// instantiation, with log a_i / log b_j per point (sinkhorn_logw_kernel, once per call) where the uniform one has the scalar
// -log N / -log M, S = sum_i a_i (b_x - a_x)_i + sum_j b_j (a_y - b_y)_j, and the row factor a_i in the gradient.  One side may be
// uniform while the other is weighted: every launch picks its instantiation by the cloud it sums over, and with no weights at all
// every launch is the uniform one.  Weights are used as given (no normalisation, no mass-balance check: geomloss does neither) and
// are constants; a zero weight is log 0 = -inf, exactly +0 in every sum; the diameter stays the bounding box of ALL points.
#include <math.h>
#include <vector>
#include "common.h"

namespace gm {

constexpr int SK_RB = 4;  // rows per wave

// Per-pair plan of a batch (written by sinkhorn_plan_kernel, read by every launch that follows): the diameter that fixes the
// pair's epsilon schedule and the schedule's length.  Pairs of a batch have schedules of their own -- exactly what one call per
// pair would have used -- so a launch covers the batch's longest schedule and a pair whose schedule has ended passes its
// potentials through.
struct SkPlan {
    float diameter;   // of the bounding box of x_b u y_b (geomloss max_diameter), or the caller's
    int n_eps;        // length of the epsilon list: 2 + numpy.arange length; 0: both clouds are one point (loss 0); -1: non-finite input
};

// epsilon number `it` of a pair's schedule (p = 2): [diameter^2] + exp(arange(2 log diameter, 2 log blur, 2 log scaling)) + [blur^2]
__device__ __forceinline__ double sk_eps(const SkPlan& pl, int it, double blur, double scaling) {
    const double d = (double)pl.diameter;
    if (it <= 0) return d * d;
    if (it >= pl.n_eps - 1) return blur * blur;
    return exp(2.0 * log(d) + (double)(it - 1) * 2.0 * log(scaling));
}

// Softmin of pair b = blockIdx.y at epsilon number `it` of ITS schedule (it < 0: the last one; the initialisation runs at it = 0):
//   out[i] = w_old * old[i] + w_new * ( -eps * log sum_j exp(logw + f[j] / eps - |p_i - q_j|^2 / (2 eps)) )
// it >= the pair's schedule length: out = old (the pair is done with its symmetrised updates and waits for the batch).
// WEIGHTED: the cloud summed over carries per-point log-weights, lw_j = log w_j in place of logw (lw_all + b * lw_stride; a zero
// weight is -inf: it leaves the max pass alone and its term of the sum pass is exp(-inf) = +0).  The uniform instantiation
// never reads lw_all.
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) softmin_kernel(const float* __restrict__ P_all, int R, size_t p_stride, const float* __restrict__ Q_all, int S,
                                                       size_t q_stride, const float* __restrict__ f_all, float logw,
                                                       const float* __restrict__ lw_all, size_t lw_stride,
                                                       const SkPlan* __restrict__ plan, int it, float blur, float scaling,
                                                       const float* __restrict__ old_all, float w_old, float w_new, float* __restrict__ out_all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int r0 = (blockIdx.x * 4 + wave) * SK_RB;
    if (r0 >= R) return;
    const SkPlan pl = plan[b];
    const float* P = P_all + (size_t)b * p_stride;
    const float* Q = Q_all + (size_t)b * q_stride;
    const float* f = f_all ? f_all + (size_t)b * S : nullptr;
    const float* lw = WEIGHTED ? lw_all + (size_t)b * lw_stride : nullptr;
    const float* old = old_all ? old_all + (size_t)b * R : nullptr;
    float* out = out_all + (size_t)b * R;
    if (pl.n_eps <= 0 || (it >= 0 && it >= pl.n_eps)) {   // nothing to do for this pair in this launch
        if (lane < SK_RB && r0 + lane < R) out[r0 + lane] = (old && pl.n_eps > 0) ? old[r0 + lane] : 0.f;
        return;
    }
    const double eps_d = sk_eps(pl, it < 0 ? pl.n_eps - 1 : it, (double)blur, (double)scaling);
    const float inv_eps = (float)(1.0 / eps_d), eps = (float)eps_d;
    float px[SK_RB], py[SK_RB], pz[SK_RB];
#pragma unroll
    for (int r = 0; r < SK_RB; ++r) {
        const int rr = min(r0 + r, R - 1);
        px[r] = P[3 * rr];
        py[r] = P[3 * rr + 1];
        pz[r] = P[3 * rr + 2];
    }
    const float hc = 0.5f * inv_eps;
    float m[SK_RB];
#pragma unroll
    for (int r = 0; r < SK_RB; ++r) m[r] = -INFINITY;
    for (int j = lane; j < S; j += 64) {
        const float qx = Q[3 * j], qy = Q[3 * j + 1], qz = Q[3 * j + 2];
        const float h = (WEIGHTED ? lw[j] : logw) + (f ? f[j] * inv_eps : 0.f);
#pragma unroll
        for (int r = 0; r < SK_RB; ++r) {
            const float dx = px[r] - qx, dy = py[r] - qy, dz = pz[r] - qz;
            m[r] = fmaxf(m[r], h - (dx * dx + dy * dy + dz * dz) * hc);
        }
    }
#pragma unroll
    for (int r = 0; r < SK_RB; ++r)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o, 64));
    float s[SK_RB];
#pragma unroll
    for (int r = 0; r < SK_RB; ++r) s[r] = 0.f;
    for (int j = lane; j < S; j += 64) {
        const float qx = Q[3 * j], qy = Q[3 * j + 1], qz = Q[3 * j + 2];
        const float h = (WEIGHTED ? lw[j] : logw) + (f ? f[j] * inv_eps : 0.f);
#pragma unroll
        for (int r = 0; r < SK_RB; ++r) {
            const float dx = px[r] - qx, dy = py[r] - qy, dz = pz[r] - qz;
            s[r] += __expf(h - (dx * dx + dy * dy + dz * dz) * hc - m[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < SK_RB; ++r)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s[r] += __shfl_xor(s[r], o, 64);
    if (lane < SK_RB && r0 + lane < R) {
        float mm = m[0], ss = s[0];
#pragma unroll
        for (int r = 1; r < SK_RB; ++r)
            if (lane == r) { mm = m[r]; ss = s[r]; }
        const float v = -eps * (mm + __logf(ss));
        out[r0 + lane] = (old ? w_old * old[r0 + lane] : 0.f) + w_new * v;
    }
}

// One workgroup per pair: bounding box of x_b u y_b -> diameter (or the caller's) and the length of the pair's epsilon schedule;
// max_eps[0] = the batch's longest schedule (atomicMax), max_eps[1] |= 1 if a coordinate is not finite.
// WEIGHTED: the pair's weights (wa_all [B][n] and wb_all + b * wb_stride [m]; either may be null = uniform) are looked through
// as well, whether or not the diameter is given: a weight that is negative or not finite, or a cloud whose weights are all zero
// (non-negative weights sum to 0 only then), makes the pair n_eps = -1 and sets max_eps[1] |= 2.  The weights never enter the
// diameter: the bounding box is that of ALL points, as geomloss takes it.
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) sinkhorn_plan_kernel(const float* __restrict__ x_all, int n, const float* __restrict__ y_all, int m, size_t y_stride,
                                                             const float* __restrict__ wa_all, const float* __restrict__ wb_all, size_t wb_stride,
                                                             float blur, float scaling, float diameter_given, SkPlan* __restrict__ plan,
                                                             int* __restrict__ max_eps) {
    __shared__ float lo[3][256], hi[3][256];
    const int tid = threadIdx.x, b = blockIdx.x;
    if constexpr (WEIGHTED) {
        const float* wa = wa_all ? wa_all + (size_t)b * n : nullptr;
        const float* wb = wb_all ? wb_all + (size_t)b * wb_stride : nullptr;
        bool wbad = false, pos_a = !wa, pos_b = !wb;
        if (wa)
            for (int i = tid; i < n; i += 256) { wbad |= !(wa[i] >= 0.f && wa[i] < INFINITY); pos_a |= wa[i] > 0.f; }
        if (wb)
            for (int j = tid; j < m; j += 256) { wbad |= !(wb[j] >= 0.f && wb[j] < INFINITY); pos_b |= wb[j] > 0.f; }
        const int any_bad = __syncthreads_or(wbad ? 1 : 0), any_a = __syncthreads_or(pos_a ? 1 : 0), any_b = __syncthreads_or(pos_b ? 1 : 0);
        if (any_bad || !any_a || !any_b) {
            if (tid == 0) { plan[b] = SkPlan{0.f, -1}; atomicOr(max_eps + 1, 2); }
            return;
        }
    }
    const float* x = x_all + (size_t)b * n * 3;
    const float* y = y_all + (size_t)b * y_stride;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    if (!(diameter_given > 0.f)) {
        for (int i = tid; i < n + m; i += 256) {
            const float* p = i < n ? x + 3 * (size_t)i : y + 3 * (size_t)(i - n);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                bad |= !(fabsf(p[c]) < INFINITY);
                mn[c] = fminf(mn[c], p[c]);
                mx[c] = fmaxf(mx[c], p[c]);
            }
        }
    }
    if (__syncthreads_or(bad ? 1 : 0)) {
        if (tid == 0) { plan[b] = SkPlan{0.f, -1}; atomicOr(max_eps + 1, 1); }
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c][tid] = mn[c]; hi[c][tid] = mx[c]; }
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lo[c][tid] = fminf(lo[c][tid], lo[c][tid + st]);
                hi[c][tid] = fmaxf(hi[c][tid], hi[c][tid + st]);
            }
        __syncthreads();
    }
    if (tid == 0) {
        float diam = diameter_given;
        if (!(diameter_given > 0.f)) {
            float d2 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) d2 = __fadd_rn(d2, __fmul_rn(hi[c][0] - lo[c][0], hi[c][0] - lo[c][0]));
            diam = sqrtf(d2);
        }
        SkPlan pl{diam, 0};
        if (diam > 0.f) {
            const double start = 2.0 * log((double)diam), stop = 2.0 * log((double)blur), step = 2.0 * log((double)scaling);
            long long cnt = (long long)ceil((stop - start) / step);   // numpy.arange length
            cnt = cnt < 0 ? 0 : (cnt > 100000 ? 100000 : cnt);
            pl.n_eps = (int)cnt + 2;
        }
        plan[b] = pl;
        atomicMax(max_eps, pl.n_eps);
    }
}

// lw = log w, once per weighted call (a zero weight: -inf; weights the plan kernel refuses give a pair that no kernel reads them for)
__global__ void __launch_bounds__(256) sinkhorn_logw_kernel(const float* __restrict__ w, size_t len, float* __restrict__ lw) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < len) lw[e] = w[e] > 0.f ? logf(w[e]) : -INFINITY;
}

// loss_b = mean(b_x - a_x) + mean(a_y - b_y)   (one workgroup per pair, fixed order)
// WEIGHTED: loss_b = sum_i a_i (b_x - a_x)_i + sum_j b_j (a_y - b_y)_j with the weights wa_all [B][n] and wb_all + b * wb_stride [m];
// a null side is uniform and keeps its mean.
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) sinkhorn_cost_kernel(const float* __restrict__ a_x, const float* __restrict__ b_x, int n,
                                                             const float* __restrict__ a_y, const float* __restrict__ b_y, int m,
                                                             const float* __restrict__ wa_all, const float* __restrict__ wb_all, size_t wb_stride,
                                                             const SkPlan* __restrict__ plan, float* __restrict__ loss) {
    __shared__ double red[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    a_x += (size_t)b * n; b_x += (size_t)b * n; a_y += (size_t)b * m; b_y += (size_t)b * m;
    const float* wa = WEIGHTED && wa_all ? wa_all + (size_t)b * n : nullptr;
    const float* wb = WEIGHTED && wb_all ? wb_all + (size_t)b * wb_stride : nullptr;
    double s = 0.0;
    if (wa) for (int i = tid; i < n; i += 256) s += (double)wa[i] * ((double)b_x[i] - (double)a_x[i]);
    else for (int i = tid; i < n; i += 256) s += ((double)b_x[i] - (double)a_x[i]) / n;
    if (wb) for (int j = tid; j < m; j += 256) s += (double)wb[j] * ((double)a_y[j] - (double)b_y[j]);
    else for (int j = tid; j < m; j += 256) s += ((double)a_y[j] - (double)b_y[j]) / m;
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) loss[b] = plan[b].n_eps > 0 ? (float)red[0] : (plan[b].n_eps == 0 ? 0.f : NAN);
}

// Gradient of pair b = blockIdx.y on one row set P (R rows of weight 1/R) from the other cloud Q (S points) and from P itself:
//   out[i] = grad[b] * ((1/R) * (D_c[i] / W_c[i] - D_s[i] / W_s[i])) = grad[b] * (1/R) * (T_s(p_i) - T_c(p_i))     (weighted rows: a_i for 1/R)
//   W[i] = sum_j w_ij,  D[i] = sum_j w_ij (p_i - q_j),  w_ij = exp(logw + f_j / eps - |p_i - q_j|^2 / (2 eps) + g_i / eps)
// at the final eps = blur^2, with (f, g, logw) = (o[kfc], q[kgc], logw_c) over Q and (o[kfs], q[kgs], logw_s) over P, where
// o = pot[*sel] is the input of the forward's last extrapolation and q = pot[*sel ^ 1] its output.  n_eps == 0: 0; n_eps < 0: NaN.
struct SkGradPots {
    const float* p[2][4];   // the forward's two ping-pong sets (SinkhornWs::pot)
};

// W and D of the wave's SK_RB rows over the S points of Q (lanes strided over Q; wave-reduced, every lane holds the sums)
// WEIGHTED: Q's points carry the log-weights lw[j] in place of logw (a zero weight: w = exp(-inf) = +0, the point drops out).
template <bool WEIGHTED>
__device__ __forceinline__ void sk_grad_sums(const float* px, const float* py, const float* pz, const float* gn, const float* __restrict__ Q,
                                             int S, const float* __restrict__ f, float logw, const float* __restrict__ lw, float inv_eps,
                                             float* W, float (*D)[3]) {
    const float hc = 0.5f * inv_eps;
#pragma unroll
    for (int r = 0; r < SK_RB; ++r) W[r] = D[r][0] = D[r][1] = D[r][2] = 0.f;
    for (int j = threadIdx.x & 63; j < S; j += 64) {
        const float qx = Q[3 * j], qy = Q[3 * j + 1], qz = Q[3 * j + 2];
        const float h = (WEIGHTED ? lw[j] : logw) + f[j] * inv_eps;
#pragma unroll
        for (int r = 0; r < SK_RB; ++r) {
            const float dx = px[r] - qx, dy = py[r] - qy, dz = pz[r] - qz;
            const float w = __expf(h - (dx * dx + dy * dy + dz * dz) * hc + gn[r]);
            W[r] += w;
            D[r][0] += w * dx;
            D[r][1] += w * dy;
            D[r][2] += w * dz;
        }
    }
#pragma unroll
    for (int r = 0; r < SK_RB; ++r)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            W[r] += __shfl_xor(W[r], o, 64);
            D[r][0] += __shfl_xor(D[r][0], o, 64);
            D[r][1] += __shfl_xor(D[r][1], o, 64);
            D[r][2] += __shfl_xor(D[r][2], o, 64);
        }
}

// WS / WC: P / Q carry weights of their own -- log-weights lw_s_all + b * w_stride_s [R] / lw_c_all + b * w_stride_c [S] in the
// barycentres, and the row factor w_row_all + b * w_stride_s [R] = a_i in place of 1/R; a row of weight zero gets exactly 0.0.
template <bool WS, bool WC>
__global__ void __launch_bounds__(256) sinkhorn_grad_kernel(const float* __restrict__ P_all, int R, size_t p_stride, float logw_s,
                                                             const float* __restrict__ Q_all, int S, size_t q_stride, float logw_c,
                                                             const float* __restrict__ w_row_all, const float* __restrict__ lw_s_all, size_t w_stride_s,
                                                             const float* __restrict__ lw_c_all, size_t w_stride_c, SkGradPots pots, const int* __restrict__ sel, int kfc, int kgc, int kfs, int kgs,
                                                             const SkPlan* __restrict__ plan, float blur, float scaling,
                                                             const float* __restrict__ grad, float* __restrict__ out_all, size_t out_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int r0 = (blockIdx.x * 4 + wave) * SK_RB;
    if (r0 >= R) return;
    const SkPlan pl = plan[b];
    float* out = out_all + (size_t)b * out_stride;
    if (pl.n_eps <= 0) {   // one point against itself (loss 0 by definition) or non-finite input (loss NaN)
        if (lane < 3 * SK_RB && r0 + lane / 3 < R) out[3 * r0 + lane] = pl.n_eps == 0 ? 0.f : NAN;
        return;
    }
    const int o = *sel, q = o ^ 1;
    const float* P = P_all + (size_t)b * p_stride;
    const float* Q = Q_all + (size_t)b * q_stride;
    const float* fc = pots.p[o][kfc] + (size_t)b * S;
    const float* fs = pots.p[o][kfs] + (size_t)b * R;
    const float* gc = pots.p[q][kgc] + (size_t)b * R;
    const float* gs = pots.p[q][kgs] + (size_t)b * R;
    const float inv_eps = (float)(1.0 / sk_eps(pl, pl.n_eps - 1, (double)blur, (double)scaling));
    float px[SK_RB], py[SK_RB], pz[SK_RB], gcn[SK_RB], gsn[SK_RB];
#pragma unroll
    for (int r = 0; r < SK_RB; ++r) {
        const int rr = min(r0 + r, R - 1);
        px[r] = P[3 * rr];
        py[r] = P[3 * rr + 1];
        pz[r] = P[3 * rr + 2];
        gcn[r] = gc[rr] * inv_eps;
        gsn[r] = gs[rr] * inv_eps;
    }
    float Wc[SK_RB], Dc[SK_RB][3], Ws[SK_RB], Ds[SK_RB][3];
    sk_grad_sums<WC>(px, py, pz, gcn, Q, S, fc, logw_c, WC ? lw_c_all + (size_t)b * w_stride_c : nullptr, inv_eps, Wc, Dc);
    sk_grad_sums<WS>(px, py, pz, gsn, P, R, fs, logw_s, WS ? lw_s_all + (size_t)b * w_stride_s : nullptr, inv_eps, Ws, Ds);
    if (lane < 3 * SK_RB && r0 + lane / 3 < R) {
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < SK_RB; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (lane == 3 * r + c) v = Dc[r][c] / Wc[r] - Ds[r][c] / Ws[r];
        if constexpr (WS) {
            const float wr = w_row_all[(size_t)b * w_stride_s + r0 + lane / 3];
            out[3 * r0 + lane] = wr > 0.f ? grad[b] * (wr * v) : 0.f;
        } else {
            out[3 * r0 + lane] = grad[b] * ((1.f / (float)R) * v);
        }
    }
}

// dy of a cloud shared by the batch: the per-pair gradients summed in pair order, in double (deterministic, no atomics)
__global__ void __launch_bounds__(256) sinkhorn_grad_sum_kernel(const float* __restrict__ part, int B, size_t len, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= len) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)part[(size_t)b * len + e];
    out[e] = (float)s;
}


struct SinkhornWs {
    SkPlan* plan;       // [B]
    int* max_eps;       // [0] longest schedule, [1] bit 0: non-finite coordinate, bit 1: refused weights, [2] which pot set is the input of the last extrapolation
    float* pot[2][4];   // ping-pong sets of (a_x[B][n], b_y[B][m], a_y[B][m], b_x[B][n])
    float* lw_a;        // weighted calls: log a [B][n] (null: x is uniform) ...
    float* lw_b;        // ... and log b, [m] with a shared y, else [B][m] (null: y is uniform); both behind the unweighted layout
    size_t bytes;
};
static SinkhornWs carve_sinkhorn(void* ws, int64_t B, int64_t n, int64_t m, bool has_a = false, bool has_b = false, bool y_shared = false) {
    SinkhornWs w;
    Carver c(ws);
    w.plan = c.take<SkPlan>((size_t)B);
    w.max_eps = c.take<int>(4);
    for (int s = 0; s < 2; ++s) {
        w.pot[s][0] = c.take<float>((size_t)(B * n));
        w.pot[s][1] = c.take<float>((size_t)(B * m));
        w.pot[s][2] = c.take<float>((size_t)(B * m));
        w.pot[s][3] = c.take<float>((size_t)(B * n));
    }
    w.lw_a = has_a ? c.take<float>((size_t)(B * n)) : nullptr;
    w.lw_b = has_b ? c.take<float>((size_t)(y_shared ? m : B * m)) : nullptr;
    w.bytes = c.used();
    return w;
}

// The forward of every entry point (`who` names it in the messages): a / b null = that cloud is uniform and its launches are the
// uniform instantiations with the scalar -log n / -log m -- with both null, the launches of the unweighted call to the bit.
static int sinkhorn_forward(const char* who, const float* a, const float* x, int64_t batch, int64_t n, const float* b, const float* y, int64_t m,
                            int y_shared, float blur, float scaling, float diameter, float* loss_device, void* ws, size_t ws_bytes, void* stream) {
    gm::DevGuard dev_guard(x);
    GM_REQUIRE(x && y && loss_device && ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(batch >= 1 && batch < 65536, GM_ERR_INVALID_ARGUMENT, "%s: batch %lld out of range (1 .. 65535)", who, (long long)batch);
    GM_REQUIRE(n >= 1 && m >= 1 && n < ((int64_t)1 << 30) && m < ((int64_t)1 << 30), GM_ERR_INVALID_ARGUMENT,
               "%s: cloud sizes out of range (%lld, %lld)", who, (long long)n, (long long)m);
    GM_REQUIRE(blur > 0.f && scaling > 0.f && scaling < 1.f, GM_ERR_INVALID_ARGUMENT, "%s: need blur > 0 and 0 < scaling < 1", who);
    GM_REQUIRE(!(diameter > 0.f) || isfinite(diameter), GM_ERR_INVALID_ARGUMENT, "%s: diameter must be finite", who);
    SinkhornWs w = carve_sinkhorn(ws, batch, n, m, a != nullptr, b != nullptr, y_shared != 0);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    const size_t y_stride = y_shared ? 0 : (size_t)m * 3;
    const size_t was = (size_t)n, wbs = y_shared ? 0 : (size_t)m;   // strides of the weights (and their logarithms) from pair to pair
    // The plan: every pair's diameter (bounding box of its union, geomloss max_diameter -- or the caller's) and the length of its
    // epsilon schedule, on the device.  The host needs ONE number back, the batch's longest schedule = how many launches follow:
    // the only host round trip, once per batch; none when the caller names the diameter (geomloss's `diameter=` keyword).
    GM_HIP_CHECK(hipMemsetAsync(w.max_eps, 0, 4 * sizeof(int), s));
    if (a || b)
        hipLaunchKernelGGL(sinkhorn_plan_kernel<true>, dim3((unsigned)batch), dim3(256), 0, s, x, (int)n, y, (int)m, y_stride, a, b, wbs, blur, scaling,
                           diameter > 0.f ? diameter : 0.f, w.plan, w.max_eps);
    else
        hipLaunchKernelGGL(sinkhorn_plan_kernel<false>, dim3((unsigned)batch), dim3(256), 0, s, x, (int)n, y, (int)m, y_stride, a, b, wbs, blur, scaling,
                           diameter > 0.f ? diameter : 0.f, w.plan, w.max_eps);
    int n_eps = 0;
    if (diameter > 0.f) {   // the same arithmetic as the plan kernel's, on the host
        const double start = 2.0 * log((double)diameter), stop = 2.0 * log((double)blur), step = 2.0 * log((double)scaling);
        long long cnt = (long long)ceil((stop - start) / step);
        cnt = cnt < 0 ? 0 : (cnt > 100000 ? 100000 : cnt);
        n_eps = (int)cnt + 2;
    } else {
        int back[2] = {0, 0};
        GM_HIP_CHECK(hipMemcpyAsync(back, w.max_eps, sizeof(back), hipMemcpyDeviceToHost, s));
        GM_HIP_CHECK(hipStreamSynchronize(s));
        GM_REQUIRE((back[1] & 1) == 0, GM_ERR_DATA, "%s: non-finite coordinate", who);
        GM_REQUIRE((back[1] & 2) == 0, GM_ERR_DATA, "%s: weights must be finite and >= 0, and every cloud's weights must not sum to 0", who);
        n_eps = back[0];
    }
    // the set the last extrapolation reads after n_eps swaps, for the backward (which then needs no host round trip)
    GM_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(w.max_eps + 2), n_eps & 1, 1, s));
    if (a) hipLaunchKernelGGL(sinkhorn_logw_kernel, dim3((unsigned)cdiv(batch * n, 256)), dim3(256), 0, s, a, (size_t)(batch * n), w.lw_a);
    if (b) {
        const int64_t len = y_shared ? m : batch * m;
        hipLaunchKernelGGL(sinkhorn_logw_kernel, dim3((unsigned)cdiv(len, 256)), dim3(256), 0, s, b, (size_t)len, w.lw_b);
    }
    const float logwa = -logf((float)n), logwb = -logf((float)m);
    const dim3 gx((unsigned)cdiv(n, 4 * SK_RB), (unsigned)batch), gy((unsigned)cdiv(m, 4 * SK_RB), (unsigned)batch);
    const size_t xs = (size_t)n * 3;
    // softmin over the second cloud of `f` (supported there), result on the first; the instantiation goes by the cloud summed over
    auto softmin = [&](const float* P, int64_t R, size_t ps, dim3 grid, const float* Q, int64_t S, size_t qs, const float* f, float logw,
                       const float* lw, size_t lws, int it, const float* old, float w_old, float w_new, float* out) {
        if (lw)
            hipLaunchKernelGGL(softmin_kernel<true>, grid, dim3(256), 0, s, P, (int)R, ps, Q, (int)S, qs, f, logw, lw, lws, w.plan, it, blur, scaling,
                               old, w_old, w_new, out);
        else
            hipLaunchKernelGGL(softmin_kernel<false>, grid, dim3(256), 0, s, P, (int)R, ps, Q, (int)S, qs, f, logw, lw, lws, w.plan, it, blur, scaling,
                               old, w_old, w_new, out);
    };
    auto over_x = [&](const float* P, int64_t R, size_t ps, dim3 grid, const float* f, int it, const float* old, float w_old, float w_new, float* out) {
        softmin(P, R, ps, grid, x, n, xs, f, logwa, w.lw_a, was, it, old, w_old, w_new, out);
    };
    auto over_y = [&](const float* P, int64_t R, size_t ps, dim3 grid, const float* f, int it, const float* old, float w_old, float w_new, float* out) {
        softmin(P, R, ps, grid, y, m, y_stride, f, logwb, w.lw_b, wbs, it, old, w_old, w_new, out);
    };
    int cur = 0;
    {   // initialisation at the first epsilon
        float** p = w.pot[cur];
        over_x(x, n, xs, gx, nullptr, 0, nullptr, 0.f, 1.f, p[0]);         // a_x: OT(a, a)
        over_y(y, m, y_stride, gy, nullptr, 0, nullptr, 0.f, 1.f, p[1]);   // b_y: OT(b, b)
        over_x(y, m, y_stride, gy, nullptr, 0, nullptr, 0.f, 1.f, p[2]);   // a_y
        over_y(x, n, xs, gx, nullptr, 0, nullptr, 0.f, 1.f, p[3]);         // b_x
    }
    for (int it = 0; it < n_eps; ++it) {  // symmetrised updates, all four from the previous potentials
        float **o = w.pot[cur], **q = w.pot[cur ^ 1];
        over_x(x, n, xs, gx, o[0], it, o[0], 0.5f, 0.5f, q[0]);
        over_y(y, m, y_stride, gy, o[1], it, o[1], 0.5f, 0.5f, q[1]);
        over_x(y, m, y_stride, gy, o[3], it, o[2], 0.5f, 0.5f, q[2]);   // a_y from b_x
        over_y(x, n, xs, gx, o[2], it, o[3], 0.5f, 0.5f, q[3]);         // b_x from a_y
        cur ^= 1;
    }
    {   // last extrapolation at every pair's final epsilon
        float **o = w.pot[cur], **q = w.pot[cur ^ 1];
        over_x(x, n, xs, gx, o[0], -1, nullptr, 0.f, 1.f, q[0]);
        over_y(y, m, y_stride, gy, o[1], -1, nullptr, 0.f, 1.f, q[1]);
        over_x(y, m, y_stride, gy, o[3], -1, nullptr, 0.f, 1.f, q[2]);
        over_y(x, n, xs, gx, o[2], -1, nullptr, 0.f, 1.f, q[3]);
        cur ^= 1;
    }
    float** p = w.pot[cur];
    if (a || b)
        hipLaunchKernelGGL(sinkhorn_cost_kernel<true>, dim3((unsigned)batch), dim3(256), 0, s, p[0], p[3], (int)n, p[2], p[1], (int)m, a, b, wbs, w.plan,
                           loss_device);
    else
        hipLaunchKernelGGL(sinkhorn_cost_kernel<false>, dim3((unsigned)batch), dim3(256), 0, s, p[0], p[3], (int)n, p[2], p[1], (int)m, a, b, wbs, w.plan,
                           loss_device);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

static size_t sinkhorn_backward_bytes(int64_t batch, int64_t n, int64_t m, int y_shared) {
    if (batch < 0 || n < 0 || m < 0) return 0;
    Carver c(nullptr);
    if (y_shared) c.take<float>((size_t)(batch * m * 3));   // per-pair dy, summed over the batch in a second launch
    return c.used();
}

// sinkhorn_grad_kernel<ws, wc> by what the rows' own cloud (ws) and the other one (wc) carry
template <typename... Args>
static void launch_sinkhorn_grad(bool ws, bool wc, dim3 grid, hipStream_t s, Args... args) {
    if (ws && wc) hipLaunchKernelGGL((sinkhorn_grad_kernel<true, true>), grid, dim3(256), 0, s, args...);
    else if (ws) hipLaunchKernelGGL((sinkhorn_grad_kernel<true, false>), grid, dim3(256), 0, s, args...);
    else if (wc) hipLaunchKernelGGL((sinkhorn_grad_kernel<false, true>), grid, dim3(256), 0, s, args...);
    else hipLaunchKernelGGL((sinkhorn_grad_kernel<false, false>), grid, dim3(256), 0, s, args...);
}

// The backward of every entry point; a / b as in sinkhorn_forward (their logarithms are read from the forward's workspace).
static int sinkhorn_backward(const char* who, const float* a, const float* x, int64_t batch, int64_t n, const float* b, const float* y, int64_t m,
                             int y_shared, float blur, float scaling, const float* grad_loss, float* dx, float* dy, const void* fwd_ws,
                             size_t fwd_ws_bytes, void* bwd_ws, size_t bwd_ws_bytes, void* stream) {
    gm::DevGuard dev_guard(x);
    GM_REQUIRE(x && y && grad_loss && fwd_ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(batch >= 1 && batch < 65536, GM_ERR_INVALID_ARGUMENT, "%s: batch %lld out of range (1 .. 65535)", who, (long long)batch);
    GM_REQUIRE(n >= 1 && m >= 1 && n < ((int64_t)1 << 30) && m < ((int64_t)1 << 30), GM_ERR_INVALID_ARGUMENT,
               "%s: cloud sizes out of range (%lld, %lld)", who, (long long)n, (long long)m);
    GM_REQUIRE(blur > 0.f && scaling > 0.f && scaling < 1.f, GM_ERR_INVALID_ARGUMENT, "%s: need blur > 0 and 0 < scaling < 1", who);
    SinkhornWs w = carve_sinkhorn(const_cast<void*>(fwd_ws), batch, n, m, a != nullptr, b != nullptr, y_shared != 0);
    GM_REQUIRE(fwd_ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: forward workspace %zu < %zu", who, fwd_ws_bytes, w.bytes);
    const size_t need = sinkhorn_backward_bytes(batch, n, m, y_shared && dy);
    GM_REQUIRE(need == 0 || (bwd_ws && bwd_ws_bytes >= need), GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, bwd_ws ? bwd_ws_bytes : 0, need);
    hipStream_t s = (hipStream_t)stream;
    const size_t xs = (size_t)n * 3, y_stride = y_shared ? 0 : (size_t)m * 3;
    const size_t was = (size_t)n, wbs = y_shared ? 0 : (size_t)m;
    const float logwa = -logf((float)n), logwb = -logf((float)m);
    SkGradPots pots;
    for (int st = 0; st < 2; ++st)
        for (int k = 0; k < 4; ++k) pots.p[st][k] = w.pot[st][k];
    const int* sel = w.max_eps + 2;
    if (dx)   // x rows: across y with (o[2] = a_y, q[3] = b_x), within x with (o[0], q[0]) = a_x
        launch_sinkhorn_grad(a != nullptr, b != nullptr, dim3((unsigned)cdiv(n, 4 * SK_RB), (unsigned)batch), s, x, (int)n, xs, logwa, y, (int)m, y_stride,
                             logwb, a, (const float*)w.lw_a, was, (const float*)w.lw_b, wbs, pots, sel, 2, 3, 0, 0, (const SkPlan*)w.plan, blur, scaling,
                             grad_loss, dx, xs);
    if (dy) {   // y rows: across x with (o[3] = b_x, q[2] = a_y), within y with (o[1], q[1]) = b_y
        float* part = y_shared ? Carver(bwd_ws).take<float>((size_t)(batch * m * 3)) : dy;
        launch_sinkhorn_grad(b != nullptr, a != nullptr, dim3((unsigned)cdiv(m, 4 * SK_RB), (unsigned)batch), s, y, (int)m, y_stride, logwb, x, (int)n, xs,
                             logwa, b, (const float*)w.lw_b, wbs, (const float*)w.lw_a, was, pots, sel, 3, 2, 1, 1, (const SkPlan*)w.plan, blur, scaling,
                             grad_loss, part, (size_t)m * 3);
        if (y_shared)
            hipLaunchKernelGGL(sinkhorn_grad_sum_kernel, dim3((unsigned)cdiv(m * 3, 256)), dim3(256), 0, s, part, (int)batch, (size_t)m * 3, dy);
    }
    GM_LAUNCH_CHECK();
    return GM_OK;
}

}  // namespace gm

using namespace gm;

extern "C" {

size_t gm_sinkhorn_batched_workspace_bytes(int64_t batch, int64_t n, int64_t m) {
    if (batch < 0 || n < 0 || m < 0) return 0;
    return carve_sinkhorn(nullptr, batch, n, m).bytes;
}
size_t gm_sinkhorn_workspace_bytes(int64_t n, int64_t m) { return gm_sinkhorn_batched_workspace_bytes(1, n, m); }

int gm_sinkhorn_divergence_batched(const float* x, int64_t batch, int64_t n, const float* y, int64_t m, int y_shared, float blur,
                                   float scaling, float diameter, float* loss_device, void* ws, size_t ws_bytes, void* stream) {
    return sinkhorn_forward("gm_sinkhorn_divergence", nullptr, x, batch, n, nullptr, y, m, y_shared, blur, scaling, diameter, loss_device, ws, ws_bytes,
                            stream);
}

size_t gm_sinkhorn_batched_backward_workspace_bytes(int64_t batch, int64_t n, int64_t m, int y_shared) {
    return sinkhorn_backward_bytes(batch, n, m, y_shared);
}

int gm_sinkhorn_divergence_batched_backward(const float* x, int64_t batch, int64_t n, const float* y, int64_t m, int y_shared, float blur,
                                            float scaling, const float* grad_loss, float* dx, float* dy, const void* fwd_ws, size_t fwd_ws_bytes,
                                            void* bwd_ws, size_t bwd_ws_bytes, void* stream) {
    return sinkhorn_backward("gm_sinkhorn_divergence_batched_backward", nullptr, x, batch, n, nullptr, y, m, y_shared, blur, scaling, grad_loss, dx, dy,
                             fwd_ws, fwd_ws_bytes, bwd_ws, bwd_ws_bytes, stream);
}

int gm_sinkhorn_divergence(const float* x, int64_t n, const float* y, int64_t m, float blur, float scaling, float* loss_device,
                           void* ws, size_t ws_bytes, void* stream) {
    return gm_sinkhorn_divergence_batched(x, 1, n, y, m, 1, blur, scaling, 0.f, loss_device, ws, ws_bytes, stream);
}

size_t gm_sinkhorn_weighted_workspace_bytes(int64_t batch, int64_t n, int64_t m, int has_a, int has_b, int y_shared) {
    if (batch < 0 || n < 0 || m < 0) return 0;
    return carve_sinkhorn(nullptr, batch, n, m, has_a != 0, has_b != 0, y_shared != 0).bytes;
}

int gm_sinkhorn_divergence_weighted(const float* a, const float* x, int64_t batch, int64_t n, const float* b, const float* y, int64_t m, int y_shared,
                                    float blur, float scaling, float diameter, float* loss_device, void* ws, size_t ws_bytes, void* stream) {
    return sinkhorn_forward("gm_sinkhorn_divergence_weighted", a, x, batch, n, b, y, m, y_shared, blur, scaling, diameter, loss_device, ws, ws_bytes,
                            stream);
}

int gm_sinkhorn_divergence_weighted_backward(const float* a, const float* x, int64_t batch, int64_t n, const float* b, const float* y, int64_t m,
                                             int y_shared, float blur, float scaling, const float* grad_loss, float* dx, float* dy, const void* fwd_ws,
                                             size_t fwd_ws_bytes, void* bwd_ws, size_t bwd_ws_bytes, void* stream) {
    return sinkhorn_backward("gm_sinkhorn_divergence_weighted_backward", a, x, batch, n, b, y, m, y_shared, blur, scaling, grad_loss, dx, dy, fwd_ws,
                             fwd_ws_bytes, bwd_ws, bwd_ws_bytes, stream);
}

}  // extern "C"
