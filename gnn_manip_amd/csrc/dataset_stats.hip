// Moments of a resident recording: count, mean and M2 of the velocities p[t+1] - p[t] and of the accelerations
// (p[t+2] - p[t+1]) - (p[t+1] - p[t]) per axis, and the range of the positions -- what the normalisation vectors of metadata.json
// are made of.  HBM-bound: every position is read once, everything else lives in registers.
//
// Replaces the reduction of simulation/generate_metadata.py:24-45 (np.diff, np.diff again, mean and np.std over the stacked rows).
//
// Numerics: differences in float64 from the float32 positions; every thread runs Welford's update on its samples, shifted by the
// first velocity / acceleration of the first counted row (a sample of the data: the running means then have the size of the spread,
// not of the drift, so a mean far above the spread costs nothing); threads, waves, workgroups and the workgroups' partials are
// merged by Chan's formula in a fixed order.  No floating-point atomics: the same input gives the same bits.
#include "common.h"

namespace gm {
namespace {

constexpr int kStatsThreads = 256;
constexpr int kStatsGridMax = GM_RECORDING_STATS_MAX_WORKGROUPS;
constexpr int kStatsRec = GM_RECORDING_STATS_DOUBLES;   // a partial has the layout of the result (shifted means)
constexpr size_t kStatsShiftBytes = 256;                // the workspace's first array: 6 doubles

// (count, mean, M2) of the velocities and the accelerations on three axes -- the counts are the same on every axis -- and the
// positions' range
struct Moments {
    double nv, na;
    double vm[3], vM[3], am[3], aM[3];
    float lo[3], hi[3];
};

__device__ __forceinline__ Moments moments_empty() {
    Moments m;
    m.nv = m.na = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        m.vm[a] = m.vM[a] = m.am[a] = m.aM[a] = 0.0;
        m.lo[a] = __builtin_inff();
        m.hi[a] = -__builtin_inff();
    }
    return m;
}

// Chan, Golub, LeVeque: (na, ma, Ma) + (nb, mb, Mb).  wb = nb / n, wab = na * nb / n (0 where n == 0)
__device__ __forceinline__ void chan(double& ma, double& Ma, double mb, double Mb, double wb, double wab) {
    const double d = mb - ma;
    ma = ma + d * wb;
    Ma = (Ma + Mb) + (d * d) * wab;
}

__device__ __forceinline__ void moments_merge(Moments& x, const Moments& y) {
    const double nv = x.nv + y.nv, na = x.na + y.na;
    const double wv = nv > 0.0 ? y.nv / nv : 0.0, wvv = nv > 0.0 ? x.nv * y.nv / nv : 0.0;
    const double wa = na > 0.0 ? y.na / na : 0.0, waa = na > 0.0 ? x.na * y.na / na : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        chan(x.vm[a], x.vM[a], y.vm[a], y.vM[a], wv, wvv);
        chan(x.am[a], x.aM[a], y.am[a], y.aM[a], wa, waa);
        x.lo[a] = fminf(x.lo[a], y.lo[a]);
        x.hi[a] = fmaxf(x.hi[a], y.hi[a]);
    }
    x.nv = nv;
    x.na = na;
}

__device__ __forceinline__ Moments moments_shfl_xor(const Moments& x, int o) {
    Moments y;
    y.nv = __shfl_xor(x.nv, o, 64);
    y.na = __shfl_xor(x.na, o, 64);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        y.vm[a] = __shfl_xor(x.vm[a], o, 64);
        y.vM[a] = __shfl_xor(x.vM[a], o, 64);
        y.am[a] = __shfl_xor(x.am[a], o, 64);
        y.aM[a] = __shfl_xor(x.aM[a], o, 64);
        y.lo[a] = __shfl_xor(x.lo[a], o, 64);
        y.hi[a] = __shfl_xor(x.hi[a], o, 64);
    }
    return y;
}

// record layout (include/gnn_manip_hip.h): 8 doubles per axis
__device__ __forceinline__ void moments_store(const Moments& m, double* rec) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double* r = rec + 8 * a;
        r[0] = m.nv; r[1] = m.vm[a]; r[2] = m.vM[a];
        r[3] = m.na; r[4] = m.am[a]; r[5] = m.aM[a];
        r[6] = (double)m.lo[a]; r[7] = (double)m.hi[a];
    }
}
__device__ __forceinline__ Moments moments_load(const double* rec) {
    Moments m;
    m.nv = rec[0];
    m.na = rec[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double* r = rec + 8 * a;
        m.vm[a] = r[1]; m.vM[a] = r[2];
        m.am[a] = r[4]; m.aM[a] = r[5];
        m.lo[a] = (float)r[6]; m.hi[a] = (float)r[7];
    }
    return m;
}

// The 256 threads' moments: lanes of a wave by the xor butterfly, the four waves in order by thread 0, which holds the result.
__device__ __forceinline__ Moments moments_block(Moments m, Moments* sh /*[4]*/) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const Moments y = moments_shfl_xor(m, o);
        moments_merge(m, y);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kStatsThreads / 64; ++w) moments_merge(m, sh[w]);
    return m;
}

struct StatsArgs {
    const float* rec;
    int64_t n_frames, n_nodes;
    int data_dim, cart0, dim, material_col;
    float material_value;
    double* shift;   // [6] in the workspace: the velocity shifts, then the acceleration shifts
};

__device__ __forceinline__ bool stats_row_counts(const StatsArgs& A, int64_t node) {
    return A.material_col < 0 || A.rec[node * A.data_dim + A.material_col] == A.material_value;
}

// Pass 0, one workgroup: the shifts -- the first velocity and the first acceleration of the FIRST COUNTED row, a sample of the data
// that is merged later.  Any finite value serves (the shifts only decide how large the running means are); a non-finite one is
// replaced by 0, and so are the shifts when no row is counted.  The rows are searched 256 at a time, in order.
__global__ void __launch_bounds__(kStatsThreads) stats_shift_kernel(StatsArgs A) {
    __shared__ long long first[kStatsThreads / 64];
    long long row = -1;
    for (int64_t base = 0; base < A.n_nodes; base += kStatsThreads) {
        const int64_t node = base + threadIdx.x;
        const bool hit = node < A.n_nodes && stats_row_counts(A, node);
        const unsigned long long m = __ballot(hit);
        if ((threadIdx.x & 63) == 0) first[threadIdx.x >> 6] = m ? (long long)(base + (threadIdx.x & ~63) + __builtin_ctzll(m)) : -1;
        __syncthreads();
        for (int w = kStatsThreads / 64 - 1; w >= 0; --w) row = first[w] >= 0 ? first[w] : row;
        __syncthreads();
        if (row >= 0) break;   // uniform: every thread read the same four words
    }
    if (threadIdx.x >= 3) return;
    const int a = threadIdx.x;
    double kv = 0.0, ka = 0.0;
    if (a < A.dim && row >= 0) {
        const int64_t fs = A.n_nodes * A.data_dim, at = row * A.data_dim + A.cart0 + a;
        const double p0 = (double)A.rec[at], p1 = (double)A.rec[fs + at], p2 = (double)A.rec[2 * fs + at];
        const double v0 = p1 - p0, a0 = (p2 - p1) - v0;
        kv = isfinite(v0) ? v0 : 0.0;
        ka = isfinite(a0) ? a0 : 0.0;
    }
    A.shift[a] = kv;
    A.shift[3 + a] = ka;
}

__device__ __forceinline__ void stats_shift(const StatsArgs& A, double* kv, double* ka) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        kv[a] = A.shift[a];
        ka[a] = A.shift[3 + a];
    }
}

// Pass 1.  A thread walks the frames of a node with the last position and the last velocity in registers, then goes on to its next
// node (grid stride); one partial per workgroup.
__global__ void __launch_bounds__(kStatsThreads) stats_partials_kernel(StatsArgs A, double* part) {
    __shared__ Moments sh[kStatsThreads / 64];
    double kv[3], ka[3];
    stats_shift(A, kv, ka);
    Moments m = moments_empty();
    const int64_t fs = A.n_nodes * A.data_dim;
    for (int64_t node = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x; node < A.n_nodes; node += (int64_t)gridDim.x * kStatsThreads) {
        if (!stats_row_counts(A, node)) continue;
        const float* row = A.rec + node * A.data_dim;
        double prev[3], vel[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            prev[a] = vel[a] = 0.0;
            if (a >= A.dim) continue;
            const float p = row[A.cart0 + a];
            m.lo[a] = fminf(m.lo[a], p);
            m.hi[a] = fmaxf(m.hi[a], p);
            prev[a] = (double)p;
        }
        for (int64_t t = 1; t < A.n_frames; ++t) {
            row += fs;
            m.nv += 1.0;
            const double iv = 1.0 / m.nv;
            if (t >= 2) m.na += 1.0;
            const double ia = 1.0 / m.na;   // used from t == 2 on
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (a >= A.dim) continue;
                const float p = row[A.cart0 + a];
                m.lo[a] = fminf(m.lo[a], p);
                m.hi[a] = fmaxf(m.hi[a], p);
                const double v = (double)p - prev[a];
                if (t >= 2) {
                    const double x = (v - vel[a]) - ka[a];
                    const double d = x - m.am[a];
                    m.am[a] += d * ia;
                    m.aM[a] += d * (x - m.am[a]);
                }
                const double x = v - kv[a];
                const double d = x - m.vm[a];
                m.vm[a] += d * iv;
                m.vM[a] += d * (x - m.vm[a]);
                prev[a] = (double)p;
                vel[a] = v;
            }
        }
    }
    m = moments_block(m, sh);
    if (threadIdx.x == 0) moments_store(m, part + (size_t)blockIdx.x * kStatsRec);
}

// Pass 2, one workgroup: thread i merges partials i, i + 256, ... in index order, the threads as in pass 1; the shifts go back on
// the means.  An axis whose mean is not finite reports a non-finite range as well; axes past `dim` report zeros.
__global__ void __launch_bounds__(kStatsThreads) stats_finish_kernel(StatsArgs A, const double* part, int n_part, double* out) {
    __shared__ Moments sh[kStatsThreads / 64];
    Moments m = moments_empty();
    for (int i = threadIdx.x; i < n_part; i += kStatsThreads) moments_merge(m, moments_load(part + (size_t)i * kStatsRec));
    m = moments_block(m, sh);
    if (threadIdx.x != 0) return;
    double kv[3], ka[3];
    stats_shift(A, kv, ka);
    const double nan = (double)__builtin_nanf("");
    for (int a = 0; a < 3; ++a) {
        double* r = out + 8 * a;
        if (a >= A.dim) {
            for (int q = 0; q < 8; ++q) r[q] = 0.0;
            continue;
        }
        const double vm = m.nv > 0.0 ? kv[a] + m.vm[a] : 0.0, am = m.na > 0.0 ? ka[a] + m.am[a] : 0.0;
        const bool ok = isfinite(vm) && isfinite(am);
        r[0] = m.nv; r[1] = vm; r[2] = m.vM[a];
        r[3] = m.na; r[4] = am; r[5] = m.aM[a];
        r[6] = ok ? (double)m.lo[a] : nan;
        r[7] = ok ? (double)m.hi[a] : nan;
    }
}

unsigned stats_grid(int64_t n_nodes) {
    const int64_t g = cdiv(n_nodes, kStatsThreads);
    return (unsigned)(g < 1 ? 1 : (g > kStatsGridMax ? kStatsGridMax : g));
}
// the recording's floats are addressed in int64; the bound keeps every byte offset far inside it
bool stats_sizes_ok(int64_t n_frames, int64_t n_nodes) {
    return n_frames >= 3 && n_nodes >= 1 && n_frames < ((int64_t)1 << 31) && n_nodes < ((int64_t)1 << 31) &&
           n_frames * n_nodes < ((int64_t)1 << 44);
}

}  // namespace
}  // namespace gm

using namespace gm;

extern "C" {

size_t gm_recording_stats_workspace_bytes(int64_t n_frames, int64_t n_nodes) {
    if (!stats_sizes_ok(n_frames, n_nodes)) return 0;
    return kStatsShiftBytes + (size_t)stats_grid(n_nodes) * kStatsRec * sizeof(double);   // the shifts, then one partial per workgroup
}

int gm_recording_stats(const float* rec, int64_t n_frames, int64_t n_nodes, int data_dim, int cart0, int dim, int material_col,
                       float material_value, double* out_device, void* ws, size_t ws_bytes, void* stream) {
    GM_REQUIRE(rec && out_device && ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    GM_REQUIRE(n_frames >= 3, GM_ERR_INVALID_ARGUMENT, "%s: n_frames=%lld < 3 (no acceleration exists)", __func__, (long long)n_frames);
    GM_REQUIRE(n_nodes >= 1, GM_ERR_INVALID_ARGUMENT, "%s: n_nodes=%lld < 1", __func__, (long long)n_nodes);
    GM_REQUIRE(stats_sizes_ok(n_frames, n_nodes), GM_ERR_INVALID_ARGUMENT, "%s: n_frames=%lld, n_nodes=%lld out of range", __func__,
               (long long)n_frames, (long long)n_nodes);
    GM_REQUIRE(dim >= 1 && dim <= 3, GM_ERR_INVALID_ARGUMENT, "%s: dim=%d outside 1..3", __func__, dim);
    GM_REQUIRE(data_dim >= 1 && data_dim <= (1 << 16) && cart0 >= 0 && cart0 + dim <= data_dim, GM_ERR_INVALID_ARGUMENT,
               "%s: columns cart0=%d .. cart0+dim=%d outside data_dim=%d", __func__, cart0, cart0 + dim, data_dim);
    GM_REQUIRE(material_col < data_dim, GM_ERR_INVALID_ARGUMENT, "%s: material_col=%d outside data_dim=%d", __func__, material_col, data_dim);
    GM_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out_device & 7) == 0, GM_ERR_INVALID_ARGUMENT, "%s: ws and out must lie on 8 bytes",
               __func__);
    const size_t need = gm_recording_stats_workspace_bytes(n_frames, n_nodes);
    GM_REQUIRE(ws_bytes >= need, GM_ERR_INVALID_ARGUMENT, "%s: workspace %zu < %zu", __func__, ws_bytes, need);
    gm::DevGuard dev_guard(rec);
    hipStream_t s = (hipStream_t)stream;
    const StatsArgs A{rec, n_frames, n_nodes, data_dim, cart0, dim, material_col < 0 ? -1 : material_col, material_value,
                      static_cast<double*>(ws)};
    const unsigned g = stats_grid(n_nodes);
    double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + kStatsShiftBytes);
    hipLaunchKernelGGL(stats_shift_kernel, dim3(1), dim3(kStatsThreads), 0, s, A);
    hipLaunchKernelGGL(stats_partials_kernel, dim3(g), dim3(kStatsThreads), 0, s, A, part);
    GM_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(kStatsThreads), 0, s, A, part, (int)g, out_device);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

}  // extern "C"
