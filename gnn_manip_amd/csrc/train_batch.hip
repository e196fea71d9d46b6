// Training batches from resident recordings: what CoffeeDataset.sample, random_walk_noise, _process_noisy / _process_simple and the
// collate do for a batch of samples (coffee_dataset.py:82-102, utils.py:96-115, collate_utils.py:29-40,68-87,169-193), in two
// phases around the one number the host has to learn, the edge count.  Phase 1 is one row kernel (window, control columns, noise,
// node features, target, packed positions) in front of the batched radius-graph build; phase 2 is the graph's own edge emission and
// the edge features.  The formulas of a row are step_rows.h's, the graph and its edges are graph.hip's and features.hip's.
// Samples of different sizes (the _ragged entry points) take the same launches: the sizes ride in the kernel arguments, the row
// kernel and the graph build have a compile-time variant that reads them, and every equal-sized instantiation stays as it was.
#include "common.h"
#include "step_rows.h"

namespace gm {
namespace {

// The window's k is a template parameter: a thread keeps the xyz of its k frames and its 3 (k - 1) noise terms in registers, and
// every loop over them unrolls.  (With a run-time k the two arrays are indexed dynamically and live in scratch.)
constexpr int kTrainBatchMaxK = 8;

struct TrainBatchRecord {   // the workspace's first 16 bytes
    int n_edges;
    int error_flags;
    int reserved[2];
};

struct TrainBatchWs {
    TrainBatchRecord* rec;
    float* pos;    // [batch * N, 3] the noisy last positions, packed: what the graph build and the edge features read
    char* graph;   // the radius graph's workspace
    size_t graph_bytes, bytes;
};
TrainBatchWs carve_train_batch(void* ws, int64_t rows, int max_nb) {
    TrainBatchWs w;
    Carver c(ws);
    w.rec = c.take<TrainBatchRecord>(1);
    w.pos = c.take<float>((size_t)rows * 3);
    w.graph_bytes = carve_graph(nullptr, rows, max_nb).bytes;
    w.graph = c.take<char>(w.graph_bytes);
    w.bytes = c.used();
    return w;
}

struct TrainBatchFrames {   // by value in the kernel arguments: no copy, no allocation
    const float* p[GM_TRAIN_BATCH_MAX];
};
struct TrainBatchSizes {    // of a ragged batch, by value too: sample b has n[b] rows and owns rows [off[b], off[b] + n[b])
    int n[GM_TRAIN_BATCH_MAX];
    int off[GM_TRAIN_BATCH_MAX];
};
enum : int { NOISE_NONE = 0, NOISE_SAMPLE = 1, NOISE_DRAW = 2 };
struct TrainBatchArgs {
    FeatParams P;          // of the window
    int rec_dim;           // columns of a recording row
    int noise;             // NOISE_*
    float noise_scale;     // (float)(noise_std / sqrt(k - 1))
    unsigned key[2];       // Philox key: seed, low word first
    unsigned long long first_stream;
    long long n;           // nodes per graph
    const float* noise_sample;
    float *nodes, *target, *windows, *pos;
    TrainBatchRecord* rec;
};

// Philox4x32-10 (Salmon et al., SC'11), in place on the counter
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// The Box-Muller pair of two words: u1 in (0, 1], u2 in [0, 1), both exact in float32
__device__ __forceinline__ void box_muller(unsigned w_even, unsigned w_odd, float& z0, float& z1) {
    const float u1 = __fmul_rn((float)((w_even >> 8) + 1u), 0x1p-24f);
    const float u2 = __fmul_rn((float)(w_odd >> 8), 0x1p-24f);
    const float rad = __fsqrt_rn(__fmul_rn(-2.f, logf(u1)));
    float sn, cs;
    sincosf(__fmul_rn(6.2831855f, u2), &sn, &cs);
    z0 = __fmul_rn(rad, cs);
    z1 = __fmul_rn(rad, sn);
}

// The rows of sample b and its first row in the batch: A.n and (unused) 0, or with the sizes of a ragged batch theirs
template <typename... Sizes>
__device__ __forceinline__ long long sample_rows(const TrainBatchArgs& A, long long b, const Sizes&... sizes) {
    if constexpr (sizeof...(Sizes) != 0) return (sizes.n[b], ...);
    else return A.n;
}
template <typename... Sizes>
__device__ __forceinline__ long long sample_first_row(long long b, const Sizes&... sizes) {
    if constexpr (sizeof...(Sizes) != 0) return (sizes.off[b], ...);
    else return 0;
}

// One thread per (sample blockIdx.y, particle): reads the particle's k + 1 recording rows, writes its window rows (if asked), its
// node-feature row, its target row and its packed noisy last position.  Sizes: nothing (every sample has A.n rows: the instantiation
// behind gm_train_batch_build), or TrainBatchSizes -- the grid's x is then sized for the largest sample and a thread past its
// sample's rows returns; a sample's blocks of windows / noise_sample / nodes / target begin at its first row instead of at b * n
template <int K, typename... Sizes>
__global__ void __launch_bounds__(256) train_batch_kernel(TrainBatchFrames F, TrainBatchArgs A, Sizes... sizes) {
    constexpr bool RAGGED = sizeof...(Sizes) != 0;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (!RAGGED)
        if (i >= A.n) return;
    const long long b = blockIdx.y, n = sample_rows(A, b, sizes...), first = sample_first_row(b, sizes...);
    if constexpr (RAGGED)
        if (i >= n) return;
    const FeatParams& P = A.P;
    const int R = A.rec_dim;
    const long long rfs = n * R;             // frame strides of the recording and of the window
    const long long wfs = n * P.D;
    const float* rec = F.p[b] + i * R;       // the particle's row of the window's first frame
    float* win;
    if constexpr (RAGGED) win = A.windows ? A.windows + first * K * P.D + i * P.D : nullptr;
    else win = A.windows ? A.windows + b * K * wfs + i * P.D : nullptr;
    bool bad = false;

    float nxt[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        nxt[a] = rec[K * rfs + P.cart + a];
        bad |= !isfinite(nxt[a]);
    }

    // the velocity noise of frame steps 1 .. K - 1, term q = 3 (t - 1) + a
    constexpr int NQ = 3 * (K - 1);
    float nz[NQ];
    if (A.noise == NOISE_SAMPLE) {
        const float* ns;
        if constexpr (RAGGED) ns = A.noise_sample + (first * (K - 1) + i) * 3;
        else ns = A.noise_sample + (b * (K - 1) * n + i) * 3;
#pragma unroll
        for (int q = 0; q < NQ; ++q) nz[q] = ns[(long long)(q / 3) * n * 3 + q % 3];
    } else if (A.noise == NOISE_DRAW) {
        const unsigned long long stream = A.first_stream + (unsigned long long)b;
#pragma unroll
        for (int j = 0; j < (NQ + 3) / 4; ++j) {
            unsigned c[4] = {(unsigned)i, (unsigned)j, (unsigned)stream, (unsigned)(stream >> 32)};
            philox4x32_10(c, A.key[0], A.key[1]);
            float z[4];
            box_muller(c[0], c[1], z[0], z[1]);
            box_muller(c[2], c[3], z[2], z[3]);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (4 * j + l < NQ) nz[4 * j + l] = __fmul_rn(z[l], A.noise_scale);
        }
    } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) nz[q] = 0.f;
    }

    // loc: the noisy xyz of the K frames, then the last frame's material and control -- the window as node_features_row reads it
    // (frame stride 3, xyz at 0, and behind the last frame's xyz its material at 3 and its control at 4)
    float loc[3 * K + 4];
    float vel[3] = {0.f, 0.f, 0.f}, seq[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const float* r = rec + t * rfs;
        const float m = r[P.mat];
        float ctl[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = r[P.cart + a];
            bad |= !isfinite(x);
            // the control of a rigid row: the way to the next position, from the CLEAN positions (dataset.py:104-108)
            ctl[a] = (m != 1.f) ? 0.f : __fsub_rn(nxt[a], x);
            // running sums of the noise, added left to right; the first term of a sum is the term itself (utils.py:104-112)
            if (t == 1) {
                vel[a] = nz[a];
                seq[a] = vel[a];
            } else if (t > 1) {
                vel[a] = __fadd_rn(vel[a], nz[3 * (t - 1) + a]);
                seq[a] = __fadd_rn(seq[a], vel[a]);
            }
            float xn = x;
            if (A.noise != NOISE_NONE) xn = __fadd_rn(x, t == 0 ? 0.f : seq[a]);
            bad |= !isfinite(xn);
            loc[3 * t + a] = xn;
        }
        if (win) {
            float* w = win + t * wfs;
            for (int d = 0; d < R; ++d) w[d] = r[d];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                w[P.cart + a] = loc[3 * t + a];
                if (P.ctrl >= 0) w[P.ctrl + a] = ctl[a];
            }
        }
        if (t == K - 1) {
            loc[3 * K] = m;
#pragma unroll
            for (int a = 0; a < 3; ++a) loc[3 * K + 1 + a] = ctl[a];
        }
    }

    FeatParams Q = P;
    Q.k = K;
    Q.cart = 0;
    Q.mat = 3;
    Q.ctrl = P.ctrl >= 0 ? 4 : -1;
    long long row;
    if constexpr (RAGGED) row = first + i;
    else row = b * n + i;
    node_features_row(loc, 3, Q, A.nodes + row * node_feature_dim(K, P.ctrl));

    float nn[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) nn[a] = A.noise != NOISE_NONE ? __fadd_rn(nxt[a], seq[a]) : nxt[a];
    const float3 tg = target_row(nn, loc + 3 * (K - 1), loc + 3 * (K - 2), P);
    A.target[row * 3] = tg.x; A.target[row * 3 + 1] = tg.y; A.target[row * 3 + 2] = tg.z;
#pragma unroll
    for (int a = 0; a < 3; ++a) A.pos[row * 3 + a] = loc[3 * (K - 1) + a];
    if (bad) atomicOr(&A.rec->error_flags, ERRF_NONFINITE_POS);
}

// A.n: the rows of every sample, or with `sizes` those of the largest
template <int K, typename... Sizes>
int launch_train_batch(const TrainBatchFrames& F, const TrainBatchArgs& A, int64_t batch, hipStream_t s, const Sizes&... sizes) {
    const auto kernel = train_batch_kernel<K, Sizes...>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(A.n, 256), (unsigned)batch), dim3(256), 0, s, F, A, sizes...);
    GM_LAUNCH_CHECK();
    return GM_OK;
}
template <typename... Sizes>
int launch_train_batch_k(int k, const TrainBatchFrames& F, const TrainBatchArgs& A, int64_t batch, hipStream_t s, const Sizes&... sizes) {
    switch (k) {
        case 2: return launch_train_batch<2>(F, A, batch, s, sizes...);
        case 3: return launch_train_batch<3>(F, A, batch, s, sizes...);
        case 4: return launch_train_batch<4>(F, A, batch, s, sizes...);
        case 5: return launch_train_batch<5>(F, A, batch, s, sizes...);
        case 6: return launch_train_batch<6>(F, A, batch, s, sizes...);
        case 7: return launch_train_batch<7>(F, A, batch, s, sizes...);
        default: return launch_train_batch<8>(F, A, batch, s, sizes...);
    }
}

// what both phases check of (fdesc, batch, N, max_neighbours), in front of any device call
int check_batch_shape(const gm_feature_desc* fdesc, int64_t batch, int64_t n, FeatParams* P, const char* who) {
    int rc = to_params(fdesc, P, who);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(batch >= 1 && batch <= GM_TRAIN_BATCH_MAX, GM_ERR_INVALID_ARGUMENT, "%s: batch=%lld outside 1..%d", who, (long long)batch,
               GM_TRAIN_BATCH_MAX);
    GM_REQUIRE(n >= 1, GM_ERR_INVALID_ARGUMENT, "%s: nodes_per_graph=%lld < 1", who, (long long)n);
    return GM_OK;
}

// the graph builder's own limits on the batch's rows and on max_neighbours, as this entry point's refusal
int check_graph_limits(int64_t rows, int64_t n, double conn_r, int max_nb, const void* ws, const char* who) {
    if (radius_graph_check_args(static_cast<const float*>(ws), 3, rows, n, conn_r, max_nb, ws) == GM_OK) return GM_OK;
    char why[384];
    snprintf(why, sizeof(why), "%s", gm_last_error());
    set_error("%s: %s", who, why);
    return GM_ERR_INVALID_ARGUMENT;
}

// The sizes of a ragged batch as the two tables the kernels take, behind the checks of the sizes and of the graph builder's limits
// on their total; *largest: the rows of the largest sample
int batch_tables(const int64_t* sizes, int64_t batch, double conn_r, int max_nb, const void* ws, const char* who, RaggedOffsets* R,
                 TrainBatchSizes* S, int64_t* largest) {
    int64_t off[GM_TRAIN_BATCH_MAX + 1] = {0};
    *largest = 0;
    for (int64_t b = 0; b < batch; ++b) {
        GM_REQUIRE(sizes[b] >= 1, GM_ERR_INVALID_ARGUMENT, "%s: sizes[%lld]=%lld < 1", who, (long long)b, (long long)sizes[b]);
        GM_REQUIRE(sizes[b] < (int64_t)1 << 30, GM_ERR_INVALID_ARGUMENT, "%s: sizes[%lld]=%lld out of range (the rows of a batch < 2^30)", who,
                   (long long)b, (long long)sizes[b]);
        off[b + 1] = off[b] + sizes[b];
        *largest = sizes[b] > *largest ? sizes[b] : *largest;
    }
    const int rc = ragged_offsets(off, batch, conn_r, max_nb, ws, who, R);
    if (rc != GM_OK) return rc;
    for (int64_t b = 0; b < GM_TRAIN_BATCH_MAX; ++b) {
        S->n[b] = b < batch ? (int)sizes[b] : 0;
        S->off[b] = R->off[b];
    }
    return GM_OK;
}

// Phase 1 of both entry points.  ragged: the samples have sizes[b] rows (n is not read); else n rows each (sizes is not read)
int train_batch_build(const char* who, bool ragged, const float* const* first_frames, const int64_t* sizes, int64_t batch, int64_t n,
                      int rec_dim, const gm_feature_desc* fdesc, int max_neighbours, double noise_std, uint64_t seed, uint64_t first_stream,
                      const float* noise_sample, float* nodes, float* target, float* windows, void* ws, size_t ws_bytes, void* stream) {
    TrainBatchArgs A{};
    int rc = check_batch_shape(fdesc, batch, ragged ? 1 : n, &A.P, who);
    if (rc != GM_OK) return rc;
    const FeatParams& P = A.P;
    GM_REQUIRE(first_frames && nodes && target && ws && (sizes || !ragged), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    TrainBatchFrames F{};
    for (int64_t b = 0; b < batch; ++b) {
        GM_REQUIRE(first_frames[b], GM_ERR_INVALID_ARGUMENT, "%s: null pointer (first_frames[%lld])", who, (long long)b);
        F.p[b] = first_frames[b];
    }
    // the window is the recording's columns, or those and the dataset's three control columns behind them
    GM_REQUIRE(rec_dim >= 4 && ((P.ctrl < 0 && P.D == rec_dim) || (P.ctrl == rec_dim && P.D == rec_dim + 3)), GM_ERR_INVALID_ARGUMENT,
               "%s: data_dim=%d, control_col=%d do not describe the window of a recording of %d columns (data_dim == rec_dim without "
               "control columns, control_col == rec_dim and data_dim == rec_dim + 3 with them)", who, P.D, P.ctrl, rec_dim);
    GM_REQUIRE(P.cart + 3 <= rec_dim && P.mat < rec_dim, GM_ERR_INVALID_ARGUMENT, "%s: position / material columns outside the recording's %d",
               who, rec_dim);
    GM_REQUIRE(P.k <= kTrainBatchMaxK, GM_ERR_UNSUPPORTED, "%s: k_steps=%d unsupported (2..%d: the window lives in registers)", who, P.k,
               kTrainBatchMaxK);
    GM_REQUIRE(noise_std == noise_std, GM_ERR_INVALID_ARGUMENT, "%s: noise_std is NaN", who);
    int64_t rows = batch * n;
    RaggedOffsets R;
    TrainBatchSizes S;
    if (ragged) {
        rc = batch_tables(sizes, batch, fdesc->conn_r, max_neighbours, ws, who, &R, &S, &n);   // n: the grid's, the largest sample
        rows = rc == GM_OK ? R.off[batch] : 0;
    } else {
        rc = check_graph_limits(rows, n, fdesc->conn_r, max_neighbours, ws, who);
    }
    if (rc != GM_OK) return rc;
    TrainBatchWs w = carve_train_batch(ws, rows, max_neighbours);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_INVALID_ARGUMENT, "%s: workspace %zu < %zu", who, ws_bytes, w.bytes);

    gm::DevGuard dev_guard(ws);
    hipStream_t s = (hipStream_t)stream;
    A.rec_dim = rec_dim;
    A.noise = noise_sample ? NOISE_SAMPLE : (noise_std > 0.0 ? NOISE_DRAW : NOISE_NONE);
    A.noise_scale = (float)(noise_std / sqrt((double)(P.k - 1)));
    A.key[0] = (unsigned)seed;
    A.key[1] = (unsigned)(seed >> 32);
    A.first_stream = first_stream;
    A.n = n;
    A.noise_sample = noise_sample;
    A.nodes = nodes; A.target = target; A.windows = windows; A.pos = w.pos;
    A.rec = w.rec;

    // four parts, the same launches whether the sizes are equal or not: one clear, one row kernel, the graph build (bounding box,
    // cell assignment, cell scan, cell fill, two neighbour kernels), one scan of the counts
    GraphWs g = carve_graph(w.graph, rows, max_neighbours);
    StepClear clr;
    rc = graph_clear_jobs(clr, g, rows);
    if (rc == GM_OK) rc = clr.add(reinterpret_cast<int*>(w.rec), 4, 0);
    if (rc == GM_OK) rc = launch_step_clear(clr, s);
    if (rc != GM_OK) return rc;
    rc = ragged ? launch_train_batch_k(P.k, F, A, batch, s, S) : launch_train_batch_k(P.k, F, A, batch, s);
    if (rc == GM_OK)
        rc = ragged ? radius_graph_build_ragged_core(w.pos, 3, R, fdesc->conn_r, max_neighbours, g, nullptr, nullptr, 0, s)
                    : radius_graph_build_core(w.pos, 3, rows, n, fdesc->conn_r, max_neighbours, g, nullptr, nullptr, 0, s);
    if (rc != GM_OK) return rc;
    const ScanJob sj{g.cnt, g.out_ptr, (long long)rows + 1, &w.rec->n_edges, g.scan_cnt};   // E goes to the record
    return scan_lookback(&sj, 1, s);
}

// Phase 2 of both entry points: the graph's edge emission reads a ragged workspace as any other
int train_batch_edges(const char* who, bool ragged, const void* ws, const int64_t* sizes, int64_t batch, int64_t n, const gm_feature_desc* fdesc,
                      int max_neighbours, int64_t n_edges, int64_t* edge_index, float* edge_attr, void* stream) {
    FeatParams P;
    int rc = check_batch_shape(fdesc, batch, ragged ? 1 : n, &P, who);
    if (rc != GM_OK) return rc;
    int64_t rows = batch * n;
    if (ragged) {
        GM_REQUIRE(ws && sizes, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
        RaggedOffsets R;
        TrainBatchSizes S;
        rc = batch_tables(sizes, batch, fdesc->conn_r, max_neighbours, ws, who, &R, &S, &n);
        if (rc != GM_OK) return rc;
        rows = R.off[batch];
    }
    GM_REQUIRE(n_edges >= 0 && n_edges <= rows * (int64_t)max_neighbours, GM_ERR_INVALID_ARGUMENT,
               "%s: n_edges=%lld outside 0..%s * max_neighbours", who, (long long)n_edges, ragged ? "total rows" : "batch * nodes_per_graph");
    GM_REQUIRE(ws && (n_edges == 0 || (edge_index && edge_attr)), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (!ragged) rc = check_graph_limits(rows, n, fdesc->conn_r, max_neighbours, ws, who);
    if (rc != GM_OK || n_edges == 0) return rc;
    const TrainBatchWs w = carve_train_batch(const_cast<void*>(ws), rows, max_neighbours);
    rc = gm_radius_graph_edges(w.graph, rows, max_neighbours, edge_index, edge_index + n_edges, n_edges, stream);
    if (rc != GM_OK) return rc;
    return gm_edge_features(w.pos, 3, edge_index, edge_index + n_edges, n_edges, P.r, edge_attr, stream);
}

}  // namespace
}  // namespace gm

using namespace gm;

extern "C" {

size_t gm_train_batch_ragged_workspace_bytes(const gm_feature_desc* fdesc, int64_t total_rows, int64_t batch, int max_neighbours) {
    if (!fdesc || batch < 1 || batch > GM_TRAIN_BATCH_MAX || total_rows < batch || total_rows >= (int64_t)1 << 30) return 0;
    if (max_neighbours < 1 || max_neighbours > 160 || total_rows * max_neighbours >= (int64_t)1 << 31) return 0;
    return carve_train_batch(nullptr, total_rows, max_neighbours).bytes;   // the sizes travel in the kernel arguments
}

int gm_train_batch_build_ragged(const float* const* first_frames, const int64_t* sizes, int64_t batch, int rec_dim, const gm_feature_desc* fdesc,
                                int max_neighbours, double noise_std, uint64_t seed, uint64_t first_stream, const float* noise_sample,
                                float* nodes, float* target, float* windows, void* ws, size_t ws_bytes, void* stream) {
    return train_batch_build("gm_train_batch_build_ragged", true, first_frames, sizes, batch, 0, rec_dim, fdesc, max_neighbours, noise_std, seed,
                             first_stream, noise_sample, nodes, target, windows, ws, ws_bytes, stream);
}

int gm_train_batch_edges_ragged(const void* ws, const int64_t* sizes, int64_t batch, const gm_feature_desc* fdesc, int max_neighbours,
                                int64_t n_edges, int64_t* edge_index, float* edge_attr, void* stream) {
    return train_batch_edges("gm_train_batch_edges_ragged", true, ws, sizes, batch, 0, fdesc, max_neighbours, n_edges, edge_index, edge_attr,
                             stream);
}

size_t gm_train_batch_workspace_bytes(const gm_feature_desc* fdesc, int64_t batch, int64_t n, int max_neighbours) {
    if (!fdesc || batch < 1 || batch > GM_TRAIN_BATCH_MAX || n < 1 || n >= ((int64_t)1 << 30) / batch) return 0;
    if (max_neighbours < 1 || max_neighbours > 160 || batch * n * max_neighbours >= (int64_t)1 << 31) return 0;
    return carve_train_batch(nullptr, batch * n, max_neighbours).bytes;
}

int gm_train_batch_build(const float* const* first_frames, int64_t batch, int64_t n, int rec_dim, const gm_feature_desc* fdesc,
                         int max_neighbours, double noise_std, uint64_t seed, uint64_t first_stream, const float* noise_sample,
                         float* nodes, float* target, float* windows, void* ws, size_t ws_bytes, void* stream) {
    return train_batch_build("gm_train_batch_build", false, first_frames, nullptr, batch, n, rec_dim, fdesc, max_neighbours, noise_std, seed,
                             first_stream, noise_sample, nodes, target, windows, ws, ws_bytes, stream);
}

int gm_train_batch_edges(const void* ws, int64_t batch, int64_t n, const gm_feature_desc* fdesc, int max_neighbours, int64_t n_edges,
                         int64_t* edge_index, float* edge_attr, void* stream) {
    return train_batch_edges("gm_train_batch_edges", false, ws, nullptr, batch, n, fdesc, max_neighbours, n_edges, edge_index, edge_attr, stream);
}

int gm_train_batch_status(const int32_t* record_host, int64_t* n_edges_host) {
    GM_REQUIRE(record_host, GM_ERR_INVALID_ARGUMENT, "gm_train_batch_status: null pointer");
    TrainBatchRecord h;
    memcpy(&h, record_host, sizeof(h));
    if (n_edges_host) *n_edges_host = h.n_edges;
    GM_REQUIRE(!(h.error_flags & ERRF_NONFINITE_POS), GM_ERR_DATA, "training batch: non-finite position in a recorded frame or in the noise");
    return GM_OK;
}

int gm_train_batch_num_edges(const void* ws, int64_t* n_edges_host, void* stream) {
    GM_REQUIRE(ws && n_edges_host, GM_ERR_INVALID_ARGUMENT, "gm_train_batch_num_edges: null pointer");
    gm::DevGuard dev_guard(ws);
    TrainBatchRecord h;
    GM_HIP_CHECK(hipMemcpyAsync(&h, ws, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return gm_train_batch_status(reinterpret_cast<const int32_t*>(&h), n_edges_host);
}

}  // extern "C"
