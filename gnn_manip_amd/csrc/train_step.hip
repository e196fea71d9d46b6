// The training step in the library: the L1 loss of examples/train_dyn.py:58-65 with its gradient, Adam on the model's own flat
// weight buffer, and gm_train_step, which strings forward, loss, backward and update together on one stream without a host
// synchronisation (host orchestration here; the model's kernels are train.hip's, reached through gm_epd_forward_train /
// gm_epd_backward).  The arithmetic of the loss and of Adam is stated in include/gnn_manip_hip.h and restated in numpy by
// tests/train_step_cases.py.  The other training mode, a loss on every frame of a rollout against a recording, is here too:
// gm_rollout_l1_loss with its transpose and gm_train_rollout_step, which runs the inference rollout keeping its windows, that loss,
// gm_rollout_backward_train (rollout_grad.hip) and the same Adam (restated by tests/train_rollout_cases.py).  Both steps are also
// available in three phases -- gm_trainer_begin, gm_train_step_accumulate / gm_train_rollout_accumulate per sample, gm_trainer_apply
// -- for an update from the mean of several samples' gradients, its norm (gm_grad_sumsq) clipped (tests/train_accum_cases.py).
// Between accumulate and apply several processes may merge their mini-batches: gm_trainer_contribution, the caller's all-gather,
// gm_trainer_reduce (gm_rank_sum: a float32 sum in rank order; tests/train_dp_cases.py).  No communication library is linked.
#include <math.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "model.h"
#include "step_rows.h"

using namespace gm;

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossGridMax = 128;   // one partial per workgroup, summed by ONE workgroup; rows past 128 * 256 are a further pass of the grid

// what the finish of a loss leaves on the device for the launches behind it
struct LossState {
    double loss;     // sum / count (NaN for count 0)
    int64_t count;   // rows counted
    float scale;     // gm_l1_loss: (float)(1.0 / count), the magnitude of every gradient element.  A rollout loss writes 0 and reads
                     // nothing here: its transpose takes each segment's scale from that segment's count
    int bad;         // how many of the samples behind `loss` forbid an update.  One sample (gm_train_step, a rollout of one
                     // segment): 1 when the edge_index was flagged or the loss is not finite; a ragged rollout batch: how many of
                     // its graphs' losses are not finite
};
static_assert(sizeof(LossState) == 24, "LossState layout");

struct LossWs {
    double* part_sum;     // [kLossGridMax]
    int64_t* part_cnt;    // [kLossGridMax]
    LossState* state;
    size_t bytes;
};
LossWs carve_loss(void* ws) {
    LossWs w;
    Carver c(ws);
    w.part_sum = c.take<double>(kLossGridMax);
    w.part_cnt = c.take<int64_t>(kLossGridMax);
    w.state = c.take<LossState>(1);
    w.bytes = c.used();
    return w;
}
__host__ __device__ inline unsigned loss_grid(int64_t rows) {
    const int64_t g = (rows + kLossThreads - 1) / kLossThreads;
    return (unsigned)(g < 1 ? 1 : (g > kLossGridMax ? kLossGridMax : g));
}

__device__ inline bool row_counts(const float* nodes, int node_dim, int mask_col, int64_t r) {
    return mask_col < 0 || nodes[(size_t)r * node_dim + mask_col] < 0.5f;
}

// The sum of 256 threads' values in a fixed tree; every thread calls it, thread 0 holds the result.
template <typename T>
__device__ inline T block_sum(T v, T* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = kLossThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

// Pass 1: a thread walks its rows (row, then column), adding the float32 values |pred - target| in float64; a workgroup's threads
// are summed in a fixed tree.  One partial per workgroup: no atomics, the same order at every run.
__global__ void __launch_bounds__(kLossThreads) l1_partials_kernel(const float* pred, const float* target, int64_t rows, int od,
                                                                   const float* nodes, int node_dim, int mask_col, double* part_sum,
                                                                   int64_t* part_cnt) {
    __shared__ double sh_s[kLossThreads];
    __shared__ int64_t sh_c[kLossThreads];
    double s = 0.0;
    int64_t cnt = 0;
    for (int64_t r = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kLossThreads) {
        if (!row_counts(nodes, node_dim, mask_col, r)) continue;
        ++cnt;
        for (int c = 0; c < od; ++c) {
            const size_t i = (size_t)r * od + c;
            s += (double)fabsf(pred[i] - target[i]);
        }
    }
    s = block_sum(s, sh_s);
    cnt = block_sum(cnt, sh_c);
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = s;
        part_cnt[blockIdx.x] = cnt;
    }
}

// Pass 2, one workgroup: the partials in a fixed tree, then the loss, the count, the gradient's scale and the skip decision.
// ha / hb (gm_train_step; else null): the two CSR headers of the forward's tape.
__global__ void __launch_bounds__(kLossThreads) l1_finish_kernel(const double* part_sum, const int64_t* part_cnt, int n_part,
                                                                 const CsrHeader* ha, const CsrHeader* hb, LossState* st, double* loss_out,
                                                                 int64_t* rows_out) {
    __shared__ double sh_s[kLossThreads];
    __shared__ int64_t sh_c[kLossThreads];
    double s = 0.0;
    int64_t cnt = 0;
    for (int i = threadIdx.x; i < n_part; i += kLossThreads) {
        s += part_sum[i];
        cnt += part_cnt[i];
    }
    s = block_sum(s, sh_s);
    cnt = block_sum(cnt, sh_c);
    if (threadIdx.x != 0) return;
    const double loss = cnt > 0 ? s / (double)cnt : (double)__builtin_nanf("");
    const bool flagged = ha && hb && ((ha->error_flags | hb->error_flags) & ERRF_BAD_EDGE_INDEX);
    st->loss = loss;
    st->count = cnt;
    st->scale = cnt > 0 ? (float)(1.0 / (double)cnt) : 0.f;
    st->bad = (flagged || !isfinite(loss)) ? 1 : 0;
    if (loss_out) *loss_out = loss;
    if (rows_out) *rows_out = cnt;
}

// Pass 3: d loss / d pred.  sign(0) = 0; a row that does not count gets 0.
__global__ void __launch_bounds__(kLossThreads) l1_grad_kernel(const float* pred, const float* target, int64_t rows, int od,
                                                               const float* nodes, int node_dim, int mask_col, const LossState* st,
                                                               float* grad) {
    const float scale = st->scale;
    for (int64_t r = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kLossThreads) {
        const bool counts = row_counts(nodes, node_dim, mask_col, r);
        for (int c = 0; c < od; ++c) {
            const size_t i = (size_t)r * od + c;
            const float d = pred[i] - target[i];
            grad[i] = !counts ? 0.f : (d > 0.f ? scale : (d < 0.f ? -scale : 0.f));
        }
    }
}

int check_loss_args(const float* pred, const float* target, int64_t rows, int od, const float* nodes, int node_dim, int mask_col,
                    const char* who) {
    GM_REQUIRE(pred && target, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(rows >= 1 && od >= 1 && rows < ((int64_t)1 << 40), GM_ERR_INVALID_ARGUMENT, "%s: sizes out of range (n_rows=%lld, out_dim=%d)", who,
               (long long)rows, od);
    GM_REQUIRE(mask_col < 0 || mask_col < node_dim, GM_ERR_INVALID_ARGUMENT, "%s: mask_col=%d outside the %d node columns", who, mask_col,
               node_dim);
    GM_REQUIRE(mask_col < 0 || nodes, GM_ERR_INVALID_ARGUMENT, "%s: null nodes with mask_col=%d", who, mask_col);
    return GM_OK;
}

// the three launches of a loss; the arguments are checked
int run_loss(const float* pred, const float* target, int64_t rows, int od, const float* nodes, int node_dim, int mask_col,
             const CsrHeader* ha, const CsrHeader* hb, const LossWs& w, double* loss_out, int64_t* rows_out, float* grad, hipStream_t s) {
    const unsigned g = loss_grid(rows);
    hipLaunchKernelGGL(l1_partials_kernel, dim3(g), dim3(kLossThreads), 0, s, pred, target, rows, od, nodes, node_dim, mask_col, w.part_sum,
                       w.part_cnt);
    GM_LAUNCH_CHECK();
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(kLossThreads), 0, s, w.part_sum, w.part_cnt, (int)g, ha, hb, w.state, loss_out, rows_out);
    GM_LAUNCH_CHECK();
    if (grad) {
        hipLaunchKernelGGL(l1_grad_kernel, dim3(g), dim3(kLossThreads), 0, s, pred, target, rows, od, nodes, node_dim, mask_col, w.state, grad);
        GM_LAUNCH_CHECK();
    }
    return GM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the rollout's loss
// The L1 loss of a rollout against recorded frames and its transpose.  Step t is scored on the last frame of the
// window the step left: windows[t + 1] for t < steps - 1, `fin` for the last step.  ONE set of kernels serves the single call
// (gm_rollout_l1_loss) and the ragged batch (gm_rollout_l1_loss_ragged): the rows are segments, one loss per segment from its own
// rows alone, and the single call is the batch of one segment [0, n) -- which is why graph g's loss in a batch is the single call's
// on g alone, bit for bit.
struct RolloutLossArgs {
    const float *windows, *fin;            // [steps,k,N,D], [k,N,D]; N: the rows of all segments
    const int32_t* rank;                   // [N] or null
    int64_t n, steps;
    int k, D, frame_dim, cart, mat;        // mat: the state's material column, < 0: off
};
// The segments and the recorded frames of each, an array of its own ([steps, n_g, frame_dim], a view into its recording).  The
// table travels by value in the kernel arguments; a kernel that needs it by a row's (divergent) graph stages it in LDS first.
struct RolloutSegments {
    RaggedOffsets R;
    const float* frames[GM_RAGGED_MAX_GRAPHS];
};
// The single call's table, made on the host: one segment [0, n) (n < 2^31) with its frames, whatever fd->nodes_per_graph says --
// a batch of equal-sized graphs is scored as ONE sample, and none of the graph builder's limits (ragged_offsets) applies.
RolloutSegments one_segment(int64_t n, const float* frames) {
    RolloutSegments S{};
    S.R.n_graphs = 1;
    for (int g = 1; g <= GM_RAGGED_MAX_GRAPHS; ++g) S.R.off[g] = (int)n;
    S.frames[0] = frames;
    return S;
}
struct SegmentRows {   // the table in LDS
    int off[GM_RAGGED_MAX_GRAPHS + 1];
    const float* frames[GM_RAGGED_MAX_GRAPHS];
};
// every thread of the workgroup calls it
__device__ inline void stage_segments(const RolloutSegments& S, SegmentRows* tab) {
    for (int t = threadIdx.x; t < S.R.n_graphs; t += blockDim.x) tab->frames[t] = S.frames[t];
    stage_ragged_offsets(S.R, tab->off);
}

__device__ inline const float* predicted_frame(const RolloutLossArgs& a, int64_t t) {
    const size_t frame = (size_t)a.n * a.D;
    return (t + 1 < a.steps ? a.windows + (size_t)(t + 1) * a.k * frame : a.fin) + (size_t)(a.k - 1) * frame;
}
// a row counts when it is not rigid and, with a material column, its flag in the last frame of windows[0] is below 0.5
__device__ inline bool rollout_row_counts(const RolloutLossArgs& a, int64_t r) {
    if (a.rank && a.rank[r] >= 0) return false;
    return a.mat < 0 || a.windows[((size_t)(a.k - 1) * a.n + r) * a.D + a.mat] < 0.5f;
}

struct GraphLoss {      // what the finish leaves per segment for the transpose
    double loss;
    int64_t count;
};
struct RolloutLossWs {
    double* part_sum;     // [n_graphs][3][kLossGridMax]: one row per axis
    int64_t* part_cnt;    // [n_graphs][kLossGridMax]
    GraphLoss* graph;     // [n_graphs]
    LossState* state;     // the call's: the segments' losses and counts added in order, bad = how many losses are not finite
    size_t bytes;
};
RolloutLossWs carve_rollout_loss(void* ws, int64_t n_graphs) {
    RolloutLossWs w;
    Carver c(ws);
    w.part_sum = c.take<double>((size_t)n_graphs * 3 * kLossGridMax);
    w.part_cnt = c.take<int64_t>((size_t)n_graphs * kLossGridMax);
    w.graph = c.take<GraphLoss>((size_t)n_graphs);
    w.state = c.take<LossState>(1);
    w.bytes = c.used();
    return w;
}

// Pass 1, l1_partials_kernel's pattern with the step as a further loop; blockIdx.y is the segment.  Segment g is walked by
// loss_grid(n_g) workgroups in that stride -- the other workgroups of the launch row leave -- so its partial sums, and everything
// behind them, depend on its own rows alone.  A thread walks its rows (row, then step, then axis) and adds the float32 values
// |pred - frame| in float64, one sum per axis; a workgroup's threads are summed in a fixed tree.
__global__ void __launch_bounds__(kLossThreads) rollout_l1_partials_kernel(RolloutLossArgs a, RolloutSegments S, double* part_sum,
                                                                           int64_t* part_cnt) {
    __shared__ double sh_s[kLossThreads];
    __shared__ int64_t sh_c[kLossThreads];
    const int g = blockIdx.y;
    const int64_t lo = S.R.off[g], n_g = S.R.off[g + 1] - lo;
    const unsigned grid = loss_grid(n_g);
    if (blockIdx.x >= grid) return;
    const float* frames = S.frames[g];
    double s[3] = {0.0, 0.0, 0.0};
    int64_t cnt = 0;
    for (int64_t q = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; q < n_g; q += (int64_t)grid * kLossThreads) {
        const int64_t r = lo + q;
        if (!rollout_row_counts(a, r)) continue;
        ++cnt;
        for (int64_t t = 0; t < a.steps; ++t) {
            const float* p = predicted_frame(a, t) + (size_t)r * a.D + a.cart;
            const float* f = frames + ((size_t)t * n_g + q) * a.frame_dim + a.cart;
            for (int c = 0; c < 3; ++c) s[c] += (double)fabsf(p[c] - f[c]);
        }
    }
    for (int c = 0; c < 3; ++c) {
        const double v = block_sum(s[c], sh_s);
        if (threadIdx.x == 0) part_sum[((size_t)g * 3 + c) * kLossGridMax + blockIdx.x] = v;
    }
    cnt = block_sum(cnt, sh_c);
    if (threadIdx.x == 0) part_cnt[(size_t)g * kLossGridMax + blockIdx.x] = cnt;
}

struct PosScale { double s[3]; };

// Pass 2, ONE workgroup, the segments in order: loss_g = (s_0 / scale_0 + s_1 / scale_1 + s_2 / scale_2) / (steps * count_g) from
// the segment's own partials in a fixed tree; then the call's state, the losses and counts added in segment order.
__global__ void __launch_bounds__(kLossThreads) rollout_l1_finish_kernel(const double* part_sum, const int64_t* part_cnt, RaggedOffsets R,
                                                                         int64_t steps, PosScale ps, GraphLoss* graph, LossState* st,
                                                                         double* losses_out, int64_t* rows_out) {
    __shared__ double sh_s[kLossThreads];
    __shared__ int64_t sh_c[kLossThreads];
    double total = 0.0;      // thread 0's
    int64_t rows = 0;
    int bad = 0;
    for (int g = 0; g < R.n_graphs; ++g) {
        const int n_part = (int)loss_grid(R.off[g + 1] - R.off[g]);
        double s[3];
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            for (int i = threadIdx.x; i < n_part; i += kLossThreads) v += part_sum[((size_t)g * 3 + c) * kLossGridMax + i];
            s[c] = block_sum(v, sh_s);
        }
        int64_t cnt = 0;
        for (int i = threadIdx.x; i < n_part; i += kLossThreads) cnt += part_cnt[(size_t)g * kLossGridMax + i];
        cnt = block_sum(cnt, sh_c);
        if (threadIdx.x != 0) continue;
        const double terms = (double)steps * (double)cnt;
        const double loss = cnt > 0 ? ((s[0] / ps.s[0] + s[1] / ps.s[1]) + s[2] / ps.s[2]) / terms : (double)__builtin_nanf("");
        graph[g].loss = loss;
        graph[g].count = cnt;
        if (losses_out) losses_out[g] = loss;
        if (rows_out) rows_out[g] = cnt;
        total = g == 0 ? loss : total + loss;
        rows += cnt;
        bad += isfinite(loss) ? 0 : 1;
    }
    if (threadIdx.x != 0) return;
    st->loss = total;
    st->count = rows;
    st->scale = 0.f;
    st->bad = bad;
}

// Pass 3: the transpose, every element of d_records [steps,N,D] and d_final [k,N,D] written.  blockIdx.y is the [N,D] slab: slab
// j < steps is d_records[j], which takes step j - 1's gradient (slab 0: zeros); slab steps + f is frame f of d_final, whose last frame
// takes the last step's.  An element is sign(pred - frame) * (float)(1.0 / ((scale_c * steps) * count_g)) on the xyz columns of a
// counted row, with sign(0) = 0, and 0 everywhere else; the row's segment (one segment: no search) decides the count and the frame.
__global__ void __launch_bounds__(kLossThreads) rollout_l1_grad_kernel(RolloutLossArgs a, RolloutSegments S, PosScale ps, const GraphLoss* graph,
                                                                       float* d_records, float* d_final) {
    __shared__ SegmentRows tab;
    __shared__ float sg[GM_RAGGED_MAX_GRAPHS][3];
    for (int g = threadIdx.x; g < S.R.n_graphs; g += blockDim.x) {
        const int64_t cnt = graph[g].count;
        for (int c = 0; c < 3; ++c) sg[g][c] = cnt > 0 ? (float)(1.0 / ((ps.s[c] * (double)a.steps) * (double)cnt)) : 0.f;
    }
    stage_segments(S, &tab);
    const int64_t slab = blockIdx.y;
    const size_t frame = (size_t)a.n * a.D;
    float* out = slab < a.steps ? d_records + (size_t)slab * frame : d_final + (size_t)(slab - a.steps) * frame;
    const int64_t t = slab < a.steps ? slab - 1 : (slab == a.steps + a.k - 1 ? a.steps - 1 : -1);
    const float* pred = t >= 0 ? predicted_frame(a, t) : nullptr;
    for (int64_t r = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * kLossThreads) {
        const int g = staged_graph_of_row(tab.off, S.R.n_graphs, r);
        const int64_t lo = tab.off[g], n_g = tab.off[g + 1] - lo;
        const bool counts = t >= 0 && graph[g].count > 0 && rollout_row_counts(a, r);
        for (int c = 0; c < a.D; ++c) {
            float v = 0.f;
            const int ax = c - a.cart;
            if (counts && ax >= 0 && ax < 3) {
                const float d = pred[(size_t)r * a.D + c] - tab.frames[g][((size_t)t * n_g + (r - lo)) * a.frame_dim + c];
                v = d > 0.f ? sg[g][ax] : (d < 0.f ? -sg[g][ax] : 0.f);
            }
            out[(size_t)r * a.D + c] = v;
        }
    }
}

// The scripted poses of a recorded drive: trajectory[t][rigid_rank[r]] = xyz(frames of r's segment [t][r - its first row]); ranks
// are global.
__global__ void __launch_bounds__(kLossThreads) recorded_poses_kernel(RolloutSegments S, int frame_dim, int cart, const int32_t* rank,
                                                                      int64_t n, int64_t n_rigid, float* trajectory) {
    __shared__ SegmentRows tab;
    stage_segments(S, &tab);
    const int64_t r = (int64_t)blockIdx.x * kLossThreads + threadIdx.x, t = blockIdx.y;
    if (r >= n) return;
    const int64_t j = rank[r];
    if (j < 0 || j >= n_rigid) return;
    const int g = staged_graph_of_row(tab.off, S.R.n_graphs, r);
    const int64_t lo = tab.off[g], n_g = tab.off[g + 1] - lo;
    const float* f = tab.frames[g] + ((size_t)t * n_g + (r - lo)) * frame_dim + cart;
    float* o = trajectory + ((size_t)t * n_rigid + j) * 3;
    o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
}

constexpr int64_t kRolloutStepsMax = 32768;   // the step is a grid dimension of the launches above

int check_rollout_loss_args(const gm_feature_desc* fd, int64_t n, int64_t steps, int frame_dim, int material_col, const double* pos_scale,
                            const char* who) {
    GM_REQUIRE(fd, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(steps >= 1 && steps <= kRolloutStepsMax, GM_ERR_INVALID_ARGUMENT, "%s: steps=%lld outside 1..%lld", who, (long long)steps,
               (long long)kRolloutStepsMax);
    GM_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && fd->k_steps >= 2 && fd->k_steps <= 64 && fd->data_dim >= 4 && fd->cart_col >= 0 &&
                   fd->cart_col + 3 <= fd->data_dim,
               GM_ERR_INVALID_ARGUMENT, "%s: sizes out of range (n_nodes=%lld, k_steps=%d, data_dim=%d, cart_col=%d)", who, (long long)n,
               fd->k_steps, fd->data_dim, fd->cart_col);
    GM_REQUIRE((frame_dim == fd->data_dim || frame_dim == fd->data_dim - 3) && fd->cart_col + 3 <= frame_dim, GM_ERR_INVALID_ARGUMENT,
               "%s: frame_dim=%d is neither data_dim=%d nor data_dim - 3 with the xyz columns inside", who, frame_dim, fd->data_dim);
    GM_REQUIRE(material_col < fd->data_dim, GM_ERR_INVALID_ARGUMENT, "%s: material_col=%d outside the %d state columns", who, material_col,
               fd->data_dim);
    for (int c = 0; pos_scale && c < 3; ++c)
        GM_REQUIRE(pos_scale[c] == pos_scale[c] && pos_scale[c] != 0.0, GM_ERR_INVALID_ARGUMENT, "%s: pos_scale[%d] is zero or NaN", who, c);
    return GM_OK;
}

// the launches of a rollout loss: partials, finish and, with d_records / d_final (both or neither), the transpose.  The arguments
// are checked; a.n: the rows of all segments.
int run_rollout_loss(const RolloutLossArgs& a, const RolloutSegments& S, const double* pos_scale, const RolloutLossWs& w, double* losses_out,
                     int64_t* rows_out, float* d_records, float* d_final, hipStream_t s) {
    PosScale ps{{1.0, 1.0, 1.0}};
    for (int c = 0; pos_scale && c < 3; ++c) ps.s[c] = pos_scale[c];
    unsigned gmax = 1;
    for (int g = 0; g < S.R.n_graphs; ++g) gmax = std::max(gmax, loss_grid(S.R.off[g + 1] - S.R.off[g]));
    hipLaunchKernelGGL(rollout_l1_partials_kernel, dim3(gmax, (unsigned)S.R.n_graphs), dim3(kLossThreads), 0, s, a, S, w.part_sum, w.part_cnt);
    GM_LAUNCH_CHECK();
    hipLaunchKernelGGL(rollout_l1_finish_kernel, dim3(1), dim3(kLossThreads), 0, s, w.part_sum, w.part_cnt, S.R, a.steps, ps, w.graph, w.state,
                       losses_out, rows_out);
    GM_LAUNCH_CHECK();
    if (d_records && d_final) {
        hipLaunchKernelGGL(rollout_l1_grad_kernel, dim3(loss_grid(a.n), (unsigned)(a.steps + a.k)), dim3(kLossThreads), 0, s, a, S, ps, w.graph,
                           d_records, d_final);
        GM_LAUNCH_CHECK();
    }
    return GM_OK;
}
// the table and the frame pointers of a ragged loss, checked
int ragged_loss_table(const char* who, const gm_feature_desc* fd, const int64_t* offsets_host, int64_t n_graphs, int K, const void* ws,
                      const float* const* frames_host, RolloutSegments* S) {
    GM_REQUIRE(frames_host, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    const int rc = ragged_scene_table(who, fd, offsets_host, n_graphs, K, ws, &S->R);
    if (rc != GM_OK) return rc;
    for (int g = 0; g < GM_RAGGED_MAX_GRAPHS; ++g) {
        S->frames[g] = g < S->R.n_graphs ? frames_host[g] : nullptr;
        GM_REQUIRE(g >= S->R.n_graphs || S->frames[g], GM_ERR_INVALID_ARGUMENT, "%s: null pointer (frames[%d])", who, g);
    }
    return GM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- Adam
struct TrainerRecord {   // the 32-byte device record gm_trainer_record copies out
    int64_t steps_applied, steps_skipped;
    double beta1_pow, beta2_pow;
};
static_assert(sizeof(TrainerRecord) == 32, "TrainerRecord layout");
struct AdamScalars {     // what the prepare launch leaves for the flat launch
    float step, s2;
    int skip;
    float gscale;        // gm_trainer_apply: what multiplies every gradient element first (the mean and the clip)
};
static_assert(sizeof(AdamScalars) == 16, "AdamScalars layout");
struct AccumRecord {     // the 48-byte device record of a mini-batch gm_trainer_accum_record copies out
    int64_t samples, bad;
    double loss_sum, sumsq, grad_norm, scale;
};
static_assert(sizeof(AccumRecord) == 48, "AccumRecord layout");

__global__ void trainer_record_set_kernel(TrainerRecord* rec, int64_t applied, int64_t skipped, int keep_skipped, double b1p, double b2p) {
    rec->steps_applied = applied;
    if (!keep_skipped) rec->steps_skipped = skipped;
    rec->beta1_pow = b1p;
    rec->beta2_pow = b2p;
}

// One thread: the step's float64 scalars.  The powers are RUNNING PRODUCTS, so that a host loop reproduces them exactly.
__global__ void adam_prepare_kernel(const LossState* st, TrainerRecord* rec, AdamScalars* sc, double beta1, double beta2, double lr,
                                    double* loss_out) {
    if (loss_out) *loss_out = st->loss;
    sc->skip = st->bad != 0;
    if (st->bad) {
        rec->steps_skipped += 1;
        return;
    }
    const double b1p = rec->beta1_pow * beta1, b2p = rec->beta2_pow * beta2;
    rec->beta1_pow = b1p;
    rec->beta2_pow = b2p;
    rec->steps_applied += 1;
    sc->step = (float)(lr / (1.0 - b1p));
    sc->s2 = (float)sqrt(1.0 - b2p);
}

// gm_trainer_begin: an empty mini-batch.  sumsq stays 0 (finite) where no norm is asked for.
__global__ void accum_reset_kernel(AccumRecord* acc) {
    acc->samples = 0;
    acc->bad = 0;
    acc->loss_sum = 0.0;
    acc->sumsq = 0.0;
    acc->grad_norm = (double)__builtin_nanf("");
    acc->scale = (double)__builtin_nanf("");
}

// One thread: the samples behind a loss join the mini-batch together, in arrival order -- one sample, or the n_samples graphs of
// a ragged rollout batch (st->loss their sum).
__global__ void accum_add_batch_kernel(const LossState* st, AccumRecord* acc, int n_samples) {
    acc->samples += n_samples;
    acc->bad += st->bad;
    acc->loss_sum += st->loss;
}

// The float64 sum of squares, l1_partials_kernel's shape.  Pass 1: a thread walks its 16-byte groups in a fixed stride, then its
// elements of the scalar tail, squaring and adding in float64; a workgroup's threads are summed in a fixed tree.  x is 16-byte aligned.
__global__ void __launch_bounds__(kLossThreads) sumsq_partials_kernel(const float* x, size_t count, double* part) {
    __shared__ double sh[kLossThreads];
    const size_t n4 = count >> 2, t = (size_t)blockIdx.x * kLossThreads + threadIdx.x, nt = (size_t)gridDim.x * kLossThreads;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    double s = 0.0;
    for (size_t i = t; i < n4; i += nt) {
        const float4 v = x4[i];
        s += (double)v.x * (double)v.x;
        s += (double)v.y * (double)v.y;
        s += (double)v.z * (double)v.z;
        s += (double)v.w * (double)v.w;
    }
    for (size_t i = (n4 << 2) + t; i < count; i += nt) s += (double)x[i] * (double)x[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Pass 2, one workgroup: the partials in a fixed tree.
__global__ void __launch_bounds__(kLossThreads) sumsq_finish_kernel(const double* part, int n_part, double* out) {
    __shared__ double sh[kLossThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_part; i += kLossThreads) s += part[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) *out = s;
}

unsigned sumsq_grid(size_t count) {
    const int64_t g = cdiv((int64_t)cdiv((int64_t)count, 4), kLossThreads);
    return (unsigned)(g < 1 ? 1 : (g > kLossGridMax ? kLossGridMax : g));
}
int run_sumsq(const float* x, size_t count, double* part, double* out, hipStream_t s) {
    const unsigned g = sumsq_grid(count);
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3(g), dim3(kLossThreads), 0, s, x, count, part);
    GM_LAUNCH_CHECK();
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(kLossThreads), 0, s, part, (int)g, out);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

// One thread: gm_trainer_apply's float64 scalars -- the mean's and the clip's scale, the skip decision, then adam_prepare_kernel's.
// have_norm: acc->sumsq holds this mini-batch's sum of squares.  clip: max_norm is in force.
__global__ void apply_prepare_kernel(AccumRecord* acc, TrainerRecord* rec, AdamScalars* sc, double beta1, double beta2, double lr,
                                     double max_norm, int clip, int have_norm, double* loss_out, double* norm_out) {
    const double S = (double)acc->samples;
    const double norm = have_norm ? sqrt(acc->sumsq) / S : (double)__builtin_nanf("");
    double coef = 1.0;
    if (clip) {
        const double c = max_norm / (norm + 1e-6);
        coef = c < 1.0 ? c : 1.0;
    }
    const float scale = (float)(coef / S);
    acc->grad_norm = norm;
    acc->scale = (double)scale;
    if (norm_out) *norm_out = norm;
    const int skip = (acc->bad > 0 || !isfinite(acc->sumsq)) ? 1 : 0;
    sc->skip = skip;
    sc->gscale = scale;
    if (loss_out) *loss_out = skip ? (double)__builtin_nanf("") : acc->loss_sum / S;
    if (skip) {
        rec->steps_skipped += 1;
        return;
    }
    const double b1p = rec->beta1_pow * beta1, b2p = rec->beta2_pow * beta2;
    rec->beta1_pow = b1p;
    rec->beta2_pow = b2p;
    rec->steps_applied += 1;
    sc->step = (float)(lr / (1.0 - b1p));
    sc->s2 = (float)sqrt(1.0 - b2p);
}

struct AdamConsts { float b1, o1, b2, o2, eps; };

// gm_trainer_apply's first operation on an element, rounded on its own
__device__ inline float scaled_gradient(float g, float scale) {
#pragma clang fp contract(off)
    const float g1 = scale * g;
    return g1;
}

// One element, every float32 operation rounded on its own: no contraction into fused multiply-adds in this function.
__device__ inline void adam_element(float& p, float& m, float& v, float g, const AdamConsts& k, float step, float s2) {
#pragma clang fp contract(off)
    const float m1 = k.b1 * m;
    const float m2 = k.o1 * g;
    m = m1 + m2;
    const float v1 = k.b2 * v;
    const float v2 = k.o2 * g;
    const float v3 = v2 * g;
    v = v1 + v3;
    const float den = sqrtf(v) / s2;
    const float den2 = den + k.eps;
    const float q = m / den2;
    const float u = step * q;
    p = p - u;
}

// The flat launch over the model's weight buffer: 16-byte accesses, a scalar tail for a count that is no multiple of 4.  A skipped
// step returns before it touches anything.  kScaled (gm_trainer_apply): every gradient element is multiplied by sc->gscale first.
template <bool kScaled>
__global__ void __launch_bounds__(256) adam_flat_kernel(float* p, float* m, float* v, const float* g, size_t count, AdamConsts k,
                                                         const AdamScalars* sc) {
    if (sc->skip) return;
    const float step = sc->step, s2 = sc->s2, gs = kScaled ? sc->gscale : 1.f;
    const size_t n4 = count >> 2, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (size_t i = t; i < n4; i += nt) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        float4 gg = g4[i];
        if (kScaled) {
            gg.x = scaled_gradient(gg.x, gs); gg.y = scaled_gradient(gg.y, gs);
            gg.z = scaled_gradient(gg.z, gs); gg.w = scaled_gradient(gg.w, gs);
        }
        adam_element(pp.x, mm.x, vv.x, gg.x, k, step, s2);
        adam_element(pp.y, mm.y, vv.y, gg.y, k, step, s2);
        adam_element(pp.z, mm.z, vv.z, gg.z, k, step, s2);
        adam_element(pp.w, mm.w, vv.w, gg.w, k, step, s2);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    for (size_t i = (n4 << 2) + t; i < count; i += nt) adam_element(p[i], m[i], v[i], kScaled ? scaled_gradient(g[i], gs) : g[i], k, step, s2);
}

// ---------------------------------------------------------------------------------------------------------------- data-parallel exchange
struct ContributionTail {   // the 32 bytes behind a contribution's gradients
    int64_t samples, bad;
    double loss_sum;
    int64_t steps_applied;
};
static_assert(sizeof(ContributionTail) == 32, "ContributionTail layout");
constexpr int kRankSumWorldMax = 64;

// gm_rank_sum: dst[i] = ((src[i] + src[stride + i]) + src[2 * stride + i]) + ..., every add a float32 add of its own, in rank order.
// An element is summed by one thread from its first rank to its last: nothing depends on the grid.  adam_flat_kernel's walk: 16-byte
// groups in a grid stride, then the scalar tail.  (Unrolling the rank loop for 4 and 8 ranks was measured and bought nothing.)
__global__ void __launch_bounds__(256) rank_sum_kernel(const float* src, size_t count, int world, size_t stride, float* dst) {
    const size_t n4 = count >> 2, s4 = stride >> 2, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
    const float4* x4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (size_t i = t; i < n4; i += nt) {
        float4 a = x4[i];
        for (int r = 1; r < world; ++r) {
            const float4 v = x4[(size_t)r * s4 + i];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        d4[i] = a;
    }
    for (size_t i = (n4 << 2) + t; i < count; i += nt) {
        float a = src[i];
        for (int r = 1; r < world; ++r) a += src[(size_t)r * stride + i];
        dst[i] = a;
    }
}

int run_rank_sum(const float* src, size_t count, int world, size_t stride, float* dst, hipStream_t s) {
    const size_t g = cdiv((int64_t)(count / 4 + 1), 256);
    hipLaunchKernelGGL(rank_sum_kernel, dim3((unsigned)(g > 2048 ? 2048 : g)), dim3(256), 0, s, src, count, world, stride, dst);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

// One thread: the tail of a contribution.  A poisoned one reports no sample and one bad one.
__global__ void contribution_tail_kernel(const AccumRecord* acc, const TrainerRecord* rec, ContributionTail* tail, int poisoned) {
    tail->samples = poisoned ? 0 : acc->samples;
    tail->bad = poisoned ? 1 : acc->bad;
    tail->loss_sum = poisoned ? 0.0 : acc->loss_sum;
    tail->steps_applied = rec->steps_applied;
}

// One thread: the merged mini-batch record of gm_trainer_reduce from the ranks' tails, in rank order.
__global__ void reduce_record_kernel(const char* contributions, int world, size_t stride_bytes, size_t tail_off, int64_t samples_total,
                                     AccumRecord* acc) {
    const ContributionTail* first = reinterpret_cast<const ContributionTail*>(contributions + tail_off);
    int64_t samples = first->samples, bad = first->bad;
    double loss_sum = first->loss_sum;
    bool in_step = true;
    for (int r = 1; r < world; ++r) {
        const ContributionTail* tail = reinterpret_cast<const ContributionTail*>(contributions + (size_t)r * stride_bytes + tail_off);
        samples += tail->samples;
        bad += tail->bad;
        loss_sum += tail->loss_sum;
        if (tail->steps_applied != first->steps_applied) in_step = false;
    }
    if (!in_step) bad += 1;                    // replicas out of step
    if (samples != samples_total) bad += 1;    // not the mini-batch the caller sharded
    acc->samples = samples;
    acc->bad = bad;
    acc->loss_sum = loss_sum;
    acc->sumsq = 0.0;
    acc->grad_norm = (double)__builtin_nanf("");
    acc->scale = (double)__builtin_nanf("");
}

}  // namespace

struct gm_trainer {
    gm_model* m = nullptr;   // not owned: the caller destroys the trainer first
    double beta1 = 0.9, beta2 = 0.999, eps = 1e-8;
    size_t count = 0;        // floats from the start of m->raw to the end of its last tensor: what Adam walks
    size_t alloc = 0;        // floats of m->raw (each tensor starts on 16 bytes), and of each buffer below
    float *exp_avg = nullptr, *exp_avg_sq = nullptr, *grad = nullptr;   // laid out like m->raw; the gaps stay zero
    TrainerRecord* rec = nullptr;
    AdamScalars* sc = nullptr;
    void* loss_ws = nullptr;   // gm_l1_loss's workspace of gm_train_step
    AccumRecord* acc = nullptr;    // the mini-batch's record
    double* norm_part = nullptr;   // [kLossGridMax]: the partials of the gradient norm
    int64_t pending = -1;          // host side of a mini-batch: samples accumulated since gm_trainer_begin; < 0: none begun
    std::vector<const float*> T;   // tensor t of m->raw
    std::vector<float*> G;         // its gradient: what gm_epd_backward takes as grads[t]
};

namespace {

struct StepWs {
    char* tape;   // first: the tape's CSR header is the workspace's first 16 bytes (the edge_index verdict)
    char* bwd;
    float *out, *go;
    size_t tape_bytes, bwd_bytes, bytes;
};
StepWs carve_step(void* ws, const gm_model_desc* d, int64_t n, int64_t e) {
    StepWs w;
    w.tape_bytes = gm_train_tape_bytes(d, n, e);
    w.bwd_bytes = gm_train_backward_workspace_bytes(d, n, e);
    Carver c(ws);
    w.tape = c.take<char>(w.tape_bytes);
    w.bwd = c.take<char>(w.bwd_bytes);
    const size_t od = (size_t)n * (d->out_dim > 0 ? d->out_dim : 1);
    w.out = c.take<float>(od);
    w.go = c.take<float>(od);
    w.bytes = c.used();
    return w;
}

// gm_train_rollout_step's workspace.  The windows come first: window t < steps is the state before step t, window `steps` the state
// the forward left.
struct RolloutStepWs {
    float *windows, *d_records, *d_final, *d_obs0, *trajectory;
    char *loss, *rollout, *sweep;
    size_t rollout_bytes, sweep_bytes, bytes;
};
bool rollout_step_sizes_ok(const gm_model_desc* d, const gm_feature_desc* fd, int64_t n, int64_t n_rigid, int K, int64_t steps) {
    return d && fd && n >= 1 && n_rigid >= 0 && n_rigid <= n && K >= 1 && steps >= 1 && steps <= kRolloutStepsMax && fd->k_steps >= 2 &&
           fd->k_steps <= 64 && fd->data_dim >= 4 && n < ((int64_t)1 << 31) / K;
}
// n_graphs: the segments of the loss (1: gm_train_rollout_step's; a ragged batch: its graphs)
RolloutStepWs carve_rollout_step(void* ws, const gm_model_desc* d, const gm_feature_desc* fd, int64_t n, int64_t n_rigid, int K,
                                 int64_t steps, int64_t n_graphs) {
    RolloutStepWs w;
    const size_t window = (size_t)fd->k_steps * n * fd->data_dim;
    w.rollout_bytes = gm_rollout_workspace_bytes(d, n, K);
    w.sweep_bytes = gm_rollout_backward_workspace_bytes(d, fd, n, K);
    Carver c(ws);
    w.windows = c.take<float>((size_t)(steps + 1) * window);
    w.d_records = c.take<float>((size_t)steps * n * fd->data_dim);
    w.d_final = c.take<float>(window);
    w.d_obs0 = c.take<float>(window);
    w.trajectory = c.take<float>((size_t)steps * n_rigid * 3);
    w.loss = c.take<char>(carve_rollout_loss(nullptr, n_graphs).bytes);
    w.rollout = c.take<char>(w.rollout_bytes);
    w.sweep = c.take<char>(w.sweep_bytes);
    w.bytes = c.used();
    return w;
}

// One Adam step on the trainer's gradients under the skip decision a loss left in `st`; the model's images follow the new weights.
template <bool kScaled>
int adam_flat(gm_trainer* t, hipStream_t s) {
    const AdamConsts k{(float)t->beta1, (float)(1.0 - t->beta1), (float)t->beta2, (float)(1.0 - t->beta2), (float)t->eps};
    const size_t g = cdiv((int64_t)(t->count / 4 + 1), 256);
    hipLaunchKernelGGL(adam_flat_kernel<kScaled>, dim3((unsigned)(g > 2048 ? 2048 : g)), dim3(256), 0, s, t->m->raw, t->exp_avg,
                       t->exp_avg_sq, t->grad, t->count, k, t->sc);
    GM_LAUNCH_CHECK();
    return weights_changed_in_place(t->m, s);
}
int adam_update(gm_trainer* t, const LossState* st, double lr, double* loss_out, hipStream_t s) {
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(1), 0, s, st, t->rec, t->sc, t->beta1, t->beta2, lr, loss_out);
    GM_LAUNCH_CHECK();
    return adam_flat<false>(t, s);
}

// The samples behind a loss join the pending mini-batch: the device record, then the host count.
int accumulate_samples(gm_trainer* t, const LossState* st, int64_t samples, hipStream_t s) {
    hipLaunchKernelGGL(accum_add_batch_kernel, dim3(1), dim3(1), 0, s, st, t->acc, (int)samples);
    GM_LAUNCH_CHECK();
    t->pending += samples;
    return GM_OK;
}

// What gm_train_step and gm_train_step_accumulate refuse before any device call.
int check_step_args(const gm_trainer* t, const float* nodes, int64_t n, const float* edge_attr, const int64_t* edge_index, int64_t e,
                    const float* target, int mask_col, double lr, const void* ws, size_t ws_bytes, const char* who) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", who);
    const gm_model* m = t->m;
    GM_REQUIRE(n >= 1 && e >= 0 && n < ((int64_t)1 << 31) && e < ((int64_t)1 << 31) / m->H, GM_ERR_INVALID_ARGUMENT,
               "%s: sizes out of range (n=%lld, e=%lld)", who, (long long)n, (long long)e);
    GM_REQUIRE(nodes && target && ws && (e == 0 || (edge_attr && edge_index)), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(mask_col < 0 || mask_col < m->d.node_dim, GM_ERR_INVALID_ARGUMENT, "%s: mask_col=%d outside the %d node columns", who,
               mask_col, m->d.node_dim);
    GM_REQUIRE(lr == lr, GM_ERR_INVALID_ARGUMENT, "%s: lr is NaN", who);
    const size_t need = carve_step(nullptr, &m->d, n, e).bytes;
    GM_REQUIRE(ws_bytes >= need, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
    return GM_OK;
}

// A batch's forward, loss and backward into the trainer's gradients (clear: zeroed first; else added to); the loss's state is left
// in the trainer's loss workspace.  The arguments are checked.
int step_gradients(gm_trainer* t, const float* nodes, int64_t n, const float* edge_attr, const int64_t* edge_index, int64_t e,
                   const float* target, int mask_col, bool clear, double* loss_out, void* ws, hipStream_t s) {
    gm_model* m = t->m;
    const StepWs w = carve_step(ws, &m->d, n, e);
    const int nt = (int)t->T.size(), od = m->d.out_dim;
    const LossWs lw = carve_loss(t->loss_ws);
    if (clear) GM_HIP_CHECK(hipMemsetAsync(t->grad, 0, t->alloc * sizeof(float), s));
    int rc = gm_epd_forward_train(m, nodes, n, edge_attr, edge_index, e, w.out, w.tape, w.tape_bytes, s);
    if (rc != GM_OK) return rc;
    // the tape begins with the destination sort's workspace, the source sort's follows it (train_model.hip: take_csr): the two
    // headers that carry the edge_index verdict
    const CsrHeader* ha = reinterpret_cast<const CsrHeader*>(w.tape);
    const CsrHeader* hb = reinterpret_cast<const CsrHeader*>(w.tape + align_up(gm_csr_workspace_bytes(n, e), 256));
    rc = run_loss(w.out, target, n, od, nodes, m->d.node_dim, mask_col, ha, hb, lw, loss_out, nullptr, w.go, s);
    if (rc != GM_OK) return rc;
    return gm_epd_backward(m, t->T.data(), nt, nodes, edge_attr, n, e, w.go, t->G.data(), w.tape, w.tape_bytes, w.bwd, w.bwd_bytes, s);
}

float* flat_of(const gm_trainer* t, int what) {
    switch (what) {
        case GM_TRAINER_PARAMS: return t->m->raw;
        case GM_TRAINER_EXP_AVG: return t->exp_avg;
        case GM_TRAINER_EXP_AVG_SQ: return t->exp_avg_sq;
        case GM_TRAINER_GRADS: return t->grad;
        default: return nullptr;
    }
}
int check_tensor_list(const gm_trainer* t, const void* const* tensors, int n_tensors, const char* who) {
    const int nt = (int)t->m->raw_jobs.size();
    GM_REQUIRE(n_tensors == nt, GM_ERR_INVALID_ARGUMENT, "%s: expected %d tensors, got %d", who, nt, n_tensors);
    for (int i = 0; i < nt; ++i) GM_REQUIRE(tensors[i], GM_ERR_INVALID_ARGUMENT, "%s: tensor %d is null", who, i);
    return GM_OK;
}

}  // namespace

extern "C" {

size_t gm_l1_loss_workspace_bytes(int64_t n_rows, int out_dim) {
    if (n_rows < 1 || out_dim < 1) return 0;
    return carve_loss(nullptr).bytes;
}

int gm_l1_loss(const float* pred, const float* target, int64_t n_rows, int out_dim, const float* nodes, int node_dim, int mask_col,
               double* loss_out, int64_t* rows_counted_out, float* grad_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_loss_args(pred, target, n_rows, out_dim, nodes, node_dim, mask_col, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(loss_out && ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    const LossWs w = carve_loss(ws);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", __func__, ws_bytes, w.bytes);
    gm::DevGuard dev_guard(pred);
    return run_loss(pred, target, n_rows, out_dim, nodes, node_dim, mask_col, nullptr, nullptr, w, loss_out, rows_counted_out, grad_out,
                    (hipStream_t)stream);
}

int gm_trainer_create(gm_model* m, double beta1, double beta2, double eps, void* stream, gm_trainer** out) {
    GM_REQUIRE(!m || m->packed_t3, GM_ERR_UNSUPPORTED, "%s: the training kernels are instantiated for hidden_size 64 / 128 / 256", __func__);
    GM_REQUIRE(m, GM_ERR_INVALID_ARGUMENT, "%s: null model", __func__);
    GM_REQUIRE(out, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    GM_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, GM_ERR_INVALID_ARGUMENT,
               "%s: betas (%g, %g) outside [0, 1) or eps %g negative", __func__, beta1, beta2, eps);
    gm::DevGuard dev_guard(m->raw);
    hipStream_t s = (hipStream_t)stream;
    gm_trainer* t = new gm_trainer();
    t->m = m;
    t->beta1 = beta1; t->beta2 = beta2; t->eps = eps;
    for (const VecJob& j : m->raw_jobs) {
        t->T.push_back(m->raw + j.dst_off);
        t->count = j.dst_off + (size_t)j.count;
        t->alloc = j.dst_off + (((size_t)j.count + 3) & ~(size_t)3);
    }
    const size_t loss_bytes = carve_loss(nullptr).bytes;
    const size_t fb = t->alloc * sizeof(float);
    if (hipMalloc(&t->exp_avg, fb) != hipSuccess || hipMalloc(&t->exp_avg_sq, fb) != hipSuccess || hipMalloc(&t->grad, fb) != hipSuccess ||
        hipMalloc(&t->rec, sizeof(TrainerRecord)) != hipSuccess || hipMalloc(&t->sc, sizeof(AdamScalars)) != hipSuccess ||
        hipMalloc(&t->loss_ws, loss_bytes) != hipSuccess || hipMalloc(&t->acc, sizeof(AccumRecord)) != hipSuccess ||
        hipMalloc(&t->norm_part, kLossGridMax * sizeof(double)) != hipSuccess) {
        gm::set_error("%s: hipMalloc failed", __func__);
        gm_trainer_destroy(t);
        return GM_ERR_HIP;
    }
    for (const VecJob& j : m->raw_jobs) t->G.push_back(t->grad + j.dst_off);
    int rc = [&]() -> int {
        GM_HIP_CHECK(hipMemsetAsync(t->exp_avg, 0, fb, s));
        GM_HIP_CHECK(hipMemsetAsync(t->exp_avg_sq, 0, fb, s));
        GM_HIP_CHECK(hipMemsetAsync(t->grad, 0, fb, s));
        GM_HIP_CHECK(hipMemsetAsync(t->sc, 0, sizeof(AdamScalars), s));
        hipLaunchKernelGGL(trainer_record_set_kernel, dim3(1), dim3(1), 0, s, t->rec, (int64_t)0, (int64_t)0, 0, 1.0, 1.0);
        GM_LAUNCH_CHECK();
        hipLaunchKernelGGL(accum_reset_kernel, dim3(1), dim3(1), 0, s, t->acc);
        GM_LAUNCH_CHECK();
        return GM_OK;
    }();
    if (rc != GM_OK) {
        gm_trainer_destroy(t);
        return rc;
    }
    *out = t;
    return GM_OK;
}

void gm_trainer_destroy(gm_trainer* t) {
    if (!t) return;
    for (void* p : std::initializer_list<void*>{t->exp_avg, t->exp_avg_sq, t->grad, t->rec, t->sc, t->loss_ws, t->acc, t->norm_part})
        (void)hipFree(p);
    delete t;
}

size_t gm_train_step_workspace_bytes(const gm_model_desc* desc, int64_t n, int64_t e) {
    if (!desc || n < 1 || e < 0) return 0;
    return carve_step(nullptr, desc, n, e).bytes;
}

int gm_train_step(gm_trainer* t, const float* nodes, int64_t n, const float* edge_attr, const int64_t* edge_index, int64_t e,
                  const float* target, int mask_col, double lr, double* loss_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_step_args(t, nodes, n, edge_attr, edge_index, e, target, mask_col, lr, ws, ws_bytes, __func__);
    if (rc != GM_OK) return rc;
    gm::DevGuard dev_guard(nodes);
    hipStream_t s = (hipStream_t)stream;
    t->pending = -1;   // the gradients are cleared: a mini-batch that was pending is gone
    rc = step_gradients(t, nodes, n, edge_attr, edge_index, e, target, mask_col, true, nullptr, ws, s);
    if (rc != GM_OK) return rc;
    return adam_update(t, carve_loss(t->loss_ws).state, lr, loss_out, s);
}

int gm_trainer_begin(gm_trainer* t, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    gm::DevGuard dev_guard(t->grad);
    hipStream_t s = (hipStream_t)stream;
    t->pending = -1;
    GM_HIP_CHECK(hipMemsetAsync(t->grad, 0, t->alloc * sizeof(float), s));
    hipLaunchKernelGGL(accum_reset_kernel, dim3(1), dim3(1), 0, s, t->acc);
    GM_LAUNCH_CHECK();
    t->pending = 0;
    return GM_OK;
}

int gm_train_step_accumulate(gm_trainer* t, const float* nodes, int64_t n, const float* edge_attr, const int64_t* edge_index, int64_t e,
                             const float* target, int mask_col, double* loss_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_step_args(t, nodes, n, edge_attr, edge_index, e, target, mask_col, 0.0, ws, ws_bytes, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(t->pending >= 0, GM_ERR_INVALID_ARGUMENT, "%s: no mini-batch begun (gm_trainer_begin)", __func__);
    gm::DevGuard dev_guard(nodes);
    hipStream_t s = (hipStream_t)stream;
    const int64_t pending = t->pending;
    t->pending = -1;   // until the sample has joined: a failure below leaves the mini-batch undefined
    rc = step_gradients(t, nodes, n, edge_attr, edge_index, e, target, mask_col, false, loss_out, ws, s);
    if (rc != GM_OK) return rc;
    t->pending = pending;
    return accumulate_samples(t, carve_loss(t->loss_ws).state, 1, s);
}

int gm_trainer_apply(gm_trainer* t, double lr, double max_grad_norm, double* loss_out, double* grad_norm_out, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    GM_REQUIRE(lr == lr, GM_ERR_INVALID_ARGUMENT, "%s: lr is NaN", __func__);
    GM_REQUIRE(max_grad_norm == max_grad_norm, GM_ERR_INVALID_ARGUMENT, "%s: max_grad_norm is NaN", __func__);
    GM_REQUIRE(t->pending >= 0, GM_ERR_INVALID_ARGUMENT, "%s: no mini-batch begun (gm_trainer_begin)", __func__);
    GM_REQUIRE(t->pending >= 1, GM_ERR_INVALID_ARGUMENT, "%s: no sample accumulated", __func__);
    gm::DevGuard dev_guard(t->grad);
    hipStream_t s = (hipStream_t)stream;
    const int clip = (max_grad_norm > 0.0 && max_grad_norm <= 1.7976931348623157e308) ? 1 : 0;
    const int have_norm = (clip || grad_norm_out) ? 1 : 0;
    t->pending = -1;   // one update per mini-batch
    if (have_norm) {
        int rc = run_sumsq(t->grad, t->count, t->norm_part, &t->acc->sumsq, s);
        if (rc != GM_OK) return rc;
    }
    hipLaunchKernelGGL(apply_prepare_kernel, dim3(1), dim3(1), 0, s, t->acc, t->rec, t->sc, t->beta1, t->beta2, lr, max_grad_norm, clip,
                       have_norm, loss_out, grad_norm_out);
    GM_LAUNCH_CHECK();
    return adam_flat<true>(t, s);
}

int gm_trainer_accum_record(const gm_trainer* t, void* record_host, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    GM_REQUIRE(record_host, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    gm::DevGuard dev_guard(t->acc);
    GM_HIP_CHECK(hipMemcpyAsync(record_host, t->acc, sizeof(AccumRecord), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return GM_OK;
}

size_t gm_grad_sumsq_workspace_bytes(int64_t count) {
    if (count < 1) return 0;
    return kLossGridMax * sizeof(double);
}

int gm_grad_sumsq(const float* x, int64_t count, double* sumsq_out, void* ws, size_t ws_bytes, void* stream) {
    GM_REQUIRE(x && sumsq_out && ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    GM_REQUIRE(count >= 1 && count < ((int64_t)1 << 40), GM_ERR_INVALID_ARGUMENT, "%s: count=%lld out of range", __func__, (long long)count);
    GM_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)ws & 7) == 0, GM_ERR_INVALID_ARGUMENT, "%s: x must lie on 16 bytes, ws on 8", __func__);
    const size_t need = gm_grad_sumsq_workspace_bytes(count);
    GM_REQUIRE(ws_bytes >= need, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", __func__, ws_bytes, need);
    gm::DevGuard dev_guard(x);
    return run_sumsq(x, (size_t)count, static_cast<double*>(ws), sumsq_out, (hipStream_t)stream);
}

int gm_rank_sum(const float* src, int64_t count, int world, int64_t stride_floats, float* dst, void* stream) {
    GM_REQUIRE(src && dst, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    GM_REQUIRE(count >= 1 && count < ((int64_t)1 << 40), GM_ERR_INVALID_ARGUMENT, "%s: count=%lld out of range", __func__, (long long)count);
    GM_REQUIRE(world >= 1 && world <= kRankSumWorldMax, GM_ERR_INVALID_ARGUMENT, "%s: world=%d outside 1..%d", __func__, world,
               kRankSumWorldMax);
    GM_REQUIRE(stride_floats >= count && (stride_floats & 3) == 0, GM_ERR_INVALID_ARGUMENT,
               "%s: stride_floats=%lld below count=%lld or no multiple of 4", __func__, (long long)stride_floats, (long long)count);
    GM_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, GM_ERR_INVALID_ARGUMENT, "%s: src and dst must lie on 16 bytes",
               __func__);
    gm::DevGuard dev_guard(src);
    return run_rank_sum(src, (size_t)count, world, (size_t)stride_floats, dst, (hipStream_t)stream);
}

size_t gm_trainer_contribution_bytes(const gm_trainer* t) {
    if (!t) return 0;
    return t->alloc * sizeof(float) + sizeof(ContributionTail);
}

int gm_trainer_contribution(gm_trainer* t, void* out_dev, size_t out_bytes, int poisoned, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    GM_REQUIRE(out_dev, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    const size_t need = gm_trainer_contribution_bytes(t), grad_bytes = t->alloc * sizeof(float);
    GM_REQUIRE(out_bytes >= need, GM_ERR_INVALID_ARGUMENT, "%s: out_bytes %zu < %zu", __func__, out_bytes, need);
    GM_REQUIRE(((uintptr_t)out_dev & 15) == 0, GM_ERR_INVALID_ARGUMENT, "%s: out_dev must lie on 16 bytes", __func__);
    GM_REQUIRE(poisoned || t->pending >= 0, GM_ERR_INVALID_ARGUMENT, "%s: no mini-batch begun (gm_trainer_begin)", __func__);
    gm::DevGuard dev_guard(t->grad);
    hipStream_t s = (hipStream_t)stream;
    char* out = static_cast<char*>(out_dev);
    if (poisoned) {
        GM_HIP_CHECK(hipMemsetAsync(out, 0, grad_bytes, s));
    } else {
        GM_HIP_CHECK(hipMemcpyAsync(out, t->grad, grad_bytes, hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(contribution_tail_kernel, dim3(1), dim3(1), 0, s, t->acc, t->rec, reinterpret_cast<ContributionTail*>(out + grad_bytes),
                       poisoned ? 1 : 0);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

int gm_trainer_reduce(gm_trainer* t, const void* contributions_dev, int world, size_t stride_bytes, int64_t samples_total_host,
                      void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    GM_REQUIRE(contributions_dev, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    GM_REQUIRE(world >= 1 && world <= kRankSumWorldMax, GM_ERR_INVALID_ARGUMENT, "%s: world=%d outside 1..%d", __func__, world,
               kRankSumWorldMax);
    const size_t need = gm_trainer_contribution_bytes(t), grad_bytes = t->alloc * sizeof(float);
    GM_REQUIRE(stride_bytes >= need && (stride_bytes & 15) == 0, GM_ERR_INVALID_ARGUMENT,
               "%s: stride_bytes=%zu below %zu or no multiple of 16", __func__, stride_bytes, need);
    GM_REQUIRE(((uintptr_t)contributions_dev & 15) == 0, GM_ERR_INVALID_ARGUMENT, "%s: contributions_dev must lie on 16 bytes", __func__);
    GM_REQUIRE(samples_total_host >= 1, GM_ERR_INVALID_ARGUMENT, "%s: samples_total_host=%lld below 1", __func__,
               (long long)samples_total_host);
    GM_REQUIRE(t->pending >= 0, GM_ERR_INVALID_ARGUMENT, "%s: no mini-batch begun (gm_trainer_begin)", __func__);
    gm::DevGuard dev_guard(t->grad);
    hipStream_t s = (hipStream_t)stream;
    t->pending = -1;   // until the merged mini-batch stands
    int rc = run_rank_sum(static_cast<const float*>(contributions_dev), t->alloc, world, stride_bytes / sizeof(float), t->grad, s);
    if (rc != GM_OK) return rc;
    hipLaunchKernelGGL(reduce_record_kernel, dim3(1), dim3(1), 0, s, static_cast<const char*>(contributions_dev), world, stride_bytes,
                       grad_bytes, samples_total_host, t->acc);
    GM_LAUNCH_CHECK();
    t->pending = samples_total_host;
    return GM_OK;
}

size_t gm_rollout_l1_loss_workspace_bytes(int64_t n_nodes, int64_t steps) {
    if (n_nodes < 1 || steps < 1 || steps > kRolloutStepsMax) return 0;
    return carve_rollout_loss(nullptr, 1).bytes;
}

int gm_rollout_l1_loss(const float* windows, const float* final_state, const float* frames, int frame_dim, int64_t steps, int64_t n,
                       const gm_feature_desc* fd, const int32_t* rigid_rank, int material_col, const double* pos_scale, double* loss_out,
                       int64_t* rows_counted_out, float* d_records, float* d_final, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_rollout_loss_args(fd, n, steps, frame_dim, material_col, pos_scale, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(windows && final_state && frames && loss_out && ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    GM_REQUIRE((d_records != nullptr) == (d_final != nullptr), GM_ERR_INVALID_ARGUMENT, "%s: d_records and d_final go together", __func__);
    const RolloutLossWs w = carve_rollout_loss(ws, 1);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", __func__, ws_bytes, w.bytes);
    gm::DevGuard dev_guard(windows);
    const RolloutLossArgs a{windows, final_state, rigid_rank, n, steps, fd->k_steps, fd->data_dim, frame_dim, fd->cart_col,
                            material_col < 0 ? -1 : material_col};
    return run_rollout_loss(a, one_segment(n, frames), pos_scale, w, loss_out, rows_counted_out, d_records, d_final, (hipStream_t)stream);
}

size_t gm_rollout_l1_loss_ragged_workspace_bytes(int64_t n_graphs) {
    if (n_graphs < 1 || n_graphs > GM_RAGGED_MAX_GRAPHS) return 0;
    return carve_rollout_loss(nullptr, n_graphs).bytes;
}

int gm_rollout_l1_loss_ragged(const float* windows, const float* final_state, const float* const* frames_host, int frame_dim, int64_t steps,
                              const int64_t* graph_offsets_host, int64_t n_graphs, const gm_feature_desc* fd, const int32_t* rigid_rank,
                              int material_col, const double* pos_scale, double* losses_out, int64_t* rows_counted_out, float* d_records,
                              float* d_final, void* ws, size_t ws_bytes, void* stream) {
    RolloutSegments S;
    int rc = ragged_loss_table(__func__, fd, graph_offsets_host, n_graphs, 1, ws, frames_host, &S);
    if (rc != GM_OK) return rc;
    const int64_t n = S.R.off[S.R.n_graphs];
    rc = check_rollout_loss_args(fd, n, steps, frame_dim, material_col, pos_scale, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(windows && final_state && losses_out, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    GM_REQUIRE((d_records != nullptr) == (d_final != nullptr), GM_ERR_INVALID_ARGUMENT, "%s: d_records and d_final go together", __func__);
    const RolloutLossWs w = carve_rollout_loss(ws, n_graphs);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", __func__, ws_bytes, w.bytes);
    gm::DevGuard dev_guard(windows);
    const RolloutLossArgs a{windows, final_state, rigid_rank, n, steps, fd->k_steps, fd->data_dim, frame_dim, fd->cart_col,
                            material_col < 0 ? -1 : material_col};
    return run_rollout_loss(a, S, pos_scale, w, losses_out, rows_counted_out, d_records, d_final, (hipStream_t)stream);
}

size_t gm_train_rollout_step_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n, int64_t n_rigid, int K,
                                             int64_t steps) {
    if (!rollout_step_sizes_ok(desc, fdesc, n, n_rigid, K, steps)) return 0;
    return carve_rollout_step(nullptr, desc, fdesc, n, n_rigid, K, steps, 1).bytes;
}

size_t gm_train_rollout_ragged_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n_total, int64_t n_rigid_total,
                                               int64_t n_graphs, int K, int64_t steps) {
    if (n_graphs < 1 || n_graphs > GM_RAGGED_MAX_GRAPHS || n_total < n_graphs) return 0;
    if (!rollout_step_sizes_ok(desc, fdesc, n_total, n_rigid_total, K, steps)) return 0;
    return carve_rollout_step(nullptr, desc, fdesc, n_total, n_rigid_total, K, steps, n_graphs).bytes;
}

// A training sample, or a mini-batch of them, on a rollout: gm_train_rollout_step (mode kRolloutEvaluate for update == 0,
// kRolloutStep), gm_train_rollout_accumulate (kRolloutAccumulate) and, with a batch, gm_train_rollout_accumulate_ragged
// (kRolloutAccumulate / kRolloutEvaluate): the windows of the batch's graphs side by side as ONE ragged rollout, one loss per graph,
// one sweep and one update of the mini-batch's record.
enum { kRolloutEvaluate = 0, kRolloutStep = 1, kRolloutAccumulate = 2 };
struct RaggedBatch {   // checked (ragged_loss_table); its rows are n
    const int64_t* offsets_host;
    int64_t n_graphs;
    RolloutSegments S;
};
// batch == null: one sample, its recording in `frames`, its loss into loss_out (optional).  Else one loss per graph (required).
static int train_rollout(gm_trainer* t, const float* obs0, int64_t n, const RaggedBatch* batch, const gm_feature_desc* fd, int K,
                         const int32_t* rigid_rank, int64_t n_rigid, const float* frames, int frame_dim, int64_t steps, int material_col,
                         const double* pos_scale, double lr, int mode, double* loss_out, void* ws, size_t ws_bytes, void* stream,
                         const char* who) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", who);
    gm_model* m = t->m;
    int rc = check_rollout_loss_args(fd, n, steps, frame_dim, material_col, pos_scale, who);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(rollout_step_sizes_ok(&m->d, fd, n, n_rigid, K, steps), GM_ERR_INVALID_ARGUMENT,
               "%s: sizes out of range (n_nodes=%lld, n_rigid=%lld, max_neighbours=%d)", who, (long long)n, (long long)n_rigid, K);
    GM_REQUIRE(obs0 && ws && (batch ? loss_out != nullptr : frames != nullptr) && (rigid_rank || n_rigid == 0), GM_ERR_INVALID_ARGUMENT,
               "%s: null pointer", who);
    GM_REQUIRE(lr == lr, GM_ERR_INVALID_ARGUMENT, "%s: lr is NaN", who);
    rc = gm::check_model_for_scene(m->d, fd, who);
    if (rc != GM_OK) return rc;
    const int64_t samples = batch ? batch->n_graphs : 1;
    const RolloutStepWs w = carve_rollout_step(ws, &m->d, fd, n, n_rigid, K, steps, samples);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.bytes);
    GM_REQUIRE(mode != kRolloutAccumulate || t->pending >= 0, GM_ERR_INVALID_ARGUMENT, "%s: no mini-batch begun (gm_trainer_begin)", who);
    gm::DevGuard dev_guard(obs0);
    hipStream_t s = (hipStream_t)stream;
    const bool update = mode != kRolloutEvaluate;
    const int64_t pending = t->pending;
    if (update) t->pending = -1;   // a step clears the gradients; a failing accumulate leaves the mini-batch undefined
    const size_t window = (size_t)fd->k_steps * n * fd->data_dim;
    const bool scripted = n_rigid > 0;
    const float* trajectory = scripted ? w.trajectory : nullptr;
    const RolloutSegments S = batch ? batch->S : one_segment(n, frames);

    // 1. the recorded poses of the rigid rows as one trajectory [steps, n_rigid, 3]: ranks are global
    if (scripted) {
        hipLaunchKernelGGL(recorded_poses_kernel, dim3((unsigned)cdiv(n, kLossThreads), (unsigned)steps), dim3(kLossThreads), 0, s, S, frame_dim,
                           fd->cart_col, rigid_rank, n, n_rigid, w.trajectory);
        GM_LAUNCH_CHECK();
    }
    // 2. the inference rollout, each step in place on a copy of the window before it: window t stays behind as step t's pre-step window
    GM_HIP_CHECK(hipMemcpyAsync(w.windows, obs0, window * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int64_t i = 0; i < steps; ++i) {
        float* next = w.windows + (size_t)(i + 1) * window;
        GM_HIP_CHECK(hipMemcpyAsync(next, next - window, window * sizeof(float), hipMemcpyDeviceToDevice, s));
        const float* poses = scripted ? trajectory + (size_t)i * n_rigid * 3 : nullptr;
        rc = batch ? gm_rollout_step_ragged(m, next, batch->offsets_host, batch->n_graphs, fd, K, rigid_rank, poses, nullptr, w.rollout,
                                            w.rollout_bytes, stream)
                   : gm_rollout_step(m, next, n, fd, K, rigid_rank, poses, nullptr, w.rollout, w.rollout_bytes, stream);
        if (rc != GM_OK) return rc;
    }
    // 3. the loss (one per graph of a batch, and the state of all), and for an update its transpose
    const RolloutLossArgs a{w.windows, w.windows + (size_t)steps * window, rigid_rank, n, steps, fd->k_steps, fd->data_dim, frame_dim,
                            fd->cart_col, material_col < 0 ? -1 : material_col};
    const RolloutLossWs lw = carve_rollout_loss(w.loss, samples);
    rc = run_rollout_loss(a, S, pos_scale, lw, loss_out, nullptr, update ? w.d_records : nullptr, update ? w.d_final : nullptr, s);
    if (rc != GM_OK || !update) return rc;
    // 4. the reverse sweep into the trainer's gradients (a step clears them first), then Adam under gm_train_step's skip rule, or the
    //    samples join the pending mini-batch in one launch on its record
    if (mode == kRolloutStep) GM_HIP_CHECK(hipMemsetAsync(t->grad, 0, t->alloc * sizeof(float), s));
    const int nt = (int)t->T.size();
    const int64_t n_targets = scripted ? steps : 0;
    rc = batch ? gm_rollout_backward_train_ragged(m, t->T.data(), nt, w.windows, batch->offsets_host, batch->n_graphs, fd, K, rigid_rank,
                                                  trajectory, n_targets, n_rigid, steps, w.d_final, w.d_records, t->G.data(), w.d_obs0,
                                                  nullptr, w.sweep, w.sweep_bytes, stream)
               : gm_rollout_backward_train(m, t->T.data(), nt, w.windows, n, fd, K, rigid_rank, trajectory, n_targets, n_rigid, steps,
                                           w.d_final, w.d_records, t->G.data(), w.d_obs0, nullptr, w.sweep, w.sweep_bytes, stream);
    if (rc != GM_OK) return rc;
    if (mode == kRolloutStep) return adam_update(t, lw.state, lr, loss_out, s);
    t->pending = pending;
    return accumulate_samples(t, lw.state, samples, s);
}

int gm_train_rollout_step(gm_trainer* t, const float* obs0, int64_t n, const gm_feature_desc* fd, int K, const int32_t* rigid_rank,
                          int64_t n_rigid, const float* frames, int frame_dim, int64_t steps, int material_col, const double* pos_scale,
                          double lr, int update, double* loss_out, void* ws, size_t ws_bytes, void* stream) {
    return train_rollout(t, obs0, n, nullptr, fd, K, rigid_rank, n_rigid, frames, frame_dim, steps, material_col, pos_scale, lr,
                         update ? kRolloutStep : kRolloutEvaluate, loss_out, ws, ws_bytes, stream, __func__);
}

int gm_train_rollout_accumulate(gm_trainer* t, const float* obs0, int64_t n, const gm_feature_desc* fd, int K, const int32_t* rigid_rank,
                                int64_t n_rigid, const float* frames, int frame_dim, int64_t steps, int material_col,
                                const double* pos_scale, double* loss_out, void* ws, size_t ws_bytes, void* stream) {
    return train_rollout(t, obs0, n, nullptr, fd, K, rigid_rank, n_rigid, frames, frame_dim, steps, material_col, pos_scale, 0.0,
                         kRolloutAccumulate, loss_out, ws, ws_bytes, stream, __func__);
}

int gm_train_rollout_accumulate_ragged(gm_trainer* t, const float* obs0, const int64_t* graph_offsets_host, int64_t n_graphs,
                                       const gm_feature_desc* fd, int K, const int32_t* rigid_rank, int64_t n_rigid,
                                       const float* const* frames_host, int frame_dim, int64_t steps, int material_col,
                                       const double* pos_scale, int update, double* losses_out, void* ws, size_t ws_bytes, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    RaggedBatch batch{graph_offsets_host, n_graphs, {}};
    const int rc = ragged_loss_table(__func__, fd, graph_offsets_host, n_graphs, K, ws, frames_host, &batch.S);
    if (rc != GM_OK) return rc;
    return train_rollout(t, obs0, batch.S.R.off[batch.S.R.n_graphs], &batch, fd, K, rigid_rank, n_rigid, nullptr, frame_dim, steps, material_col,
                         pos_scale, 0.0, update ? kRolloutAccumulate : kRolloutEvaluate, losses_out, ws, ws_bytes, stream, __func__);
}

int gm_trainer_record(const gm_trainer* t, void* record_host, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    GM_REQUIRE(record_host, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    gm::DevGuard dev_guard(t->rec);
    GM_HIP_CHECK(hipMemcpyAsync(record_host, t->rec, sizeof(TrainerRecord), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return GM_OK;
}

int gm_trainer_export(const gm_trainer* t, int what, float* const* tensors_out, int n_tensors, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    GM_REQUIRE(tensors_out, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    const float* flat = flat_of(t, what);
    GM_REQUIRE(flat, GM_ERR_INVALID_ARGUMENT, "%s: unknown what=%d", __func__, what);
    int rc = check_tensor_list(t, reinterpret_cast<const void* const*>(tensors_out), n_tensors, __func__);
    if (rc != GM_OK) return rc;
    gm::DevGuard dev_guard(flat);
    hipStream_t s = (hipStream_t)stream;
    if (what == GM_TRAINER_PARAMS) {   // the weights may have been loaded on another stream
        rc = weights_ready_on(t->m, s);
        if (rc != GM_OK) return rc;
    }
    for (int i = 0; i < n_tensors; ++i) {
        const VecJob& j = t->m->raw_jobs[(size_t)i];
        GM_HIP_CHECK(hipMemcpyAsync(tensors_out[i], flat + j.dst_off, (size_t)j.count * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return GM_OK;
}

int gm_trainer_import(gm_trainer* t, int what, const float* const* tensors_in, int n_tensors, int64_t step_count, void* stream) {
    GM_REQUIRE(t, GM_ERR_INVALID_ARGUMENT, "%s: null trainer", __func__);
    GM_REQUIRE(tensors_in, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    float* flat = flat_of(t, what);
    GM_REQUIRE(flat && what != GM_TRAINER_GRADS, GM_ERR_INVALID_ARGUMENT, "%s: %s what=%d", __func__,
               flat ? "the gradients are an output," : "unknown", what);
    int rc = check_tensor_list(t, reinterpret_cast<const void* const*>(tensors_in), n_tensors, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(what != GM_TRAINER_EXP_AVG || (step_count >= 0 && step_count < ((int64_t)1 << 40)), GM_ERR_INVALID_ARGUMENT,
               "%s: step_count=%lld out of range", __func__, (long long)step_count);
    if (what == GM_TRAINER_PARAMS) return gm_model_update(t->m, tensors_in, n_tensors, 1, stream);   // copies, then re-packs the images
    gm::DevGuard dev_guard(flat);
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < n_tensors; ++i) {
        const VecJob& j = t->m->raw_jobs[(size_t)i];
        GM_HIP_CHECK(hipMemcpyAsync(flat + j.dst_off, tensors_in[i], (size_t)j.count * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (what == GM_TRAINER_EXP_AVG) {
        // the powers as the steps themselves would have left them: running products.  A product ends at a FIXED POINT of the rounded
        // multiplication -- zero for a beta up to 0.5, a non-zero denormal above it (0.9: 2.47e-323, 0.999: 2.465e-321; both reached
        // by step 737,741) -- and the device's own products stop at the same one, so the loop ends once neither product changes.
        double b1p = 1.0, b2p = 1.0;
        for (int64_t i = 0; i < step_count && !(b1p * t->beta1 == b1p && b2p * t->beta2 == b2p); ++i) { b1p *= t->beta1; b2p *= t->beta2; }
        hipLaunchKernelGGL(trainer_record_set_kernel, dim3(1), dim3(1), 0, s, t->rec, step_count, (int64_t)0, 1, b1p, b2p);
        GM_LAUNCH_CHECK();
    }
    return GM_OK;
}

}  // extern "C"
