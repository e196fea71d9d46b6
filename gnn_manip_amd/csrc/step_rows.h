// The per-row formulas of a rollout step, each stated once: the stand-alone kernels (features.hip, graph.hip) call one of them, the
// fused kernels of gm_rollout_step compose them -- which is why a fused step equals the chain of stand-alone entry points bit for bit.
// All float32 element-wise work; operations are written with the _rn intrinsics so that no multiply-add is contracted: the results
// are bit-identical to the reference's separate torch ops wherever the reference's own op order is defined.
#pragma once
#include "common.h"

namespace gm {

struct FeatParams {
    int k, D, cart, mat, ctrl;
    float r;
    float vm[3], vs[3], am[3], as[3], lo[3], hi[3];
};

// A descriptor checked and turned into the kernels' parameters (features.hip); `who` opens the message of a refusal
int to_params(const gm_feature_desc* d, FeatParams* p, const char* who);

// The radius-graph build behind its resets (graph.hip, graph_clear_jobs): grid phase and neighbour search into g.cnt / g.nbr; the
// scan of g.cnt (-> g.out_ptr, E) is the caller's.  radius_graph_check_args: the limits gm_radius_graph_build_batched puts on its
// arguments.  Declared here, not in common.h, for the callers that compose a build with their own row kernels (train_batch.hip).
int radius_graph_check_args(const float* pos, int64_t pos_stride, int64_t n, int64_t n_per, double conn_r, int K, const void* ws);
int radius_graph_build_core(const float* pos, int64_t pos_stride, int64_t n, int64_t n_per, double conn_r, int K, const GraphWs& g,
                            int* indeg, int* slot, int flow, hipStream_t s);

// The graphs of a ragged build (gm_radius_graph_build_ragged): graph g owns rows [off[g], off[g + 1]).  The table travels by value
// in the kernel arguments -- no copy, no allocation; the one kernel that needs the graph of a row stages it in LDS.
struct RaggedOffsets {
    int n_graphs;
    int off[GM_RAGGED_MAX_GRAPHS + 1];
};
// host offsets -> table, behind every check gm_radius_graph_build_ragged makes of them and of the other arguments (`who` opens
// the message of a refusal); radius_graph_build_ragged_core: radius_graph_build_core with the graph of a row from the table
int ragged_offsets(const int64_t* offsets_host, int64_t n_graphs, double conn_r, int K, const void* ws, const char* who, RaggedOffsets* out);
// What every _ragged rollout, sweep and loss entry point checks before anything else: fd and ws given, a descriptor of ONE scene
// per graph (nodes_per_graph == 0), then ragged_offsets
int ragged_scene_table(const char* who, const gm_feature_desc* fd, const int64_t* offsets_host, int64_t n_graphs, int K, const void* ws,
                       RaggedOffsets* out);
int radius_graph_build_ragged_core(const float* pos, int64_t pos_stride, const RaggedOffsets& R, double conn_r, int K, const GraphWs& g,
                                   int* indeg, int* slot, int flow, hipStream_t s);
// radius_graph_build_fused / csr_from_graph_fused (common.h) for the graphs of a table: the rollout step's graph path of a ragged batch
int radius_graph_build_fused_ragged(const float* pos, int64_t pos_stride, const RaggedOffsets& R, double conn_r, int K, void* graph_ws,
                                    size_t graph_ws_bytes, void* csr_ws, size_t csr_ws_bytes, int flow, hipStream_t s);
int csr_from_graph_fused_ragged(const void* graph_ws, const RaggedOffsets& R, int K, void* csr_ws, size_t csr_ws_bytes, const float* pos,
                                int64_t pos_stride, float conn_r, float* edge_attr, int flow, hipStream_t s);

// Width of a scene's node features: 3 (k_steps - 1) velocities, 6 boundary terms, the material, and 3 more with control columns
__host__ __device__ static inline int node_feature_dim(int k_steps, int control_col) { return 3 * (k_steps - 1) + 7 + (control_col >= 0 ? 3 : 0); }
inline int node_feature_dim(const gm_feature_desc* fd) { return node_feature_dim(fd->k_steps, fd->control_col); }
// Nodes of one graph of a batch of equal-sized scenes stored back to back (nodes_per_graph == 0: one scene of n nodes)
inline int64_t graph_nodes(const gm_feature_desc* fd, int64_t n) { return fd->nodes_per_graph > 0 ? fd->nodes_per_graph : n; }

#if defined(__HIPCC__)
// The table of a ragged build comes by value in the kernel arguments; a search by a divergent index needs it in memory, so the
// workgroup stages it in LDS first (every thread of the workgroup calls this).
__device__ __forceinline__ void stage_ragged_offsets(const RaggedOffsets& R, int* s_off /* LDS, n_graphs + 1 ints */) {
    for (int t = threadIdx.x; t <= R.n_graphs; t += blockDim.x) s_off[t] = R.off[t];
    __syncthreads();
}
// The graph of row i in a staged table: the g with s_off[g] <= i < s_off[g + 1].  One graph: no iteration.
__device__ __forceinline__ int staged_graph_of_row(const int* s_off, int n_graphs, int64_t i) {
    int lo = 0, hi = n_graphs;   // off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)s_off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
// The graph of row i of a ragged build, staging included (every thread of the workgroup calls this).
__device__ __forceinline__ int ragged_graph_of_row(const RaggedOffsets& R, int64_t i) {
    __shared__ int s_off[GM_RAGGED_MAX_GRAPHS + 1];
    stage_ragged_offsets(R, s_off);
    return staged_graph_of_row(s_off, R.n_graphs, i);
}

// [(p_s - p_r) / r, |.|] of one edge, ps / pr = the xyz of its sender (edge_index[0]) / receiver (utils.py:43-61)
__device__ __forceinline__ float4 edge_feature(const float* __restrict__ ps, const float* __restrict__ pr, float cr) {
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = __fdiv_rn(__fsub_rn(ps[a], pr[a]), cr);
    float q = __fmul_rn(d[0], d[0]);
    q = __fadd_rn(q, __fmul_rn(d[1], d[1]));
    q = __fadd_rn(q, __fmul_rn(d[2], d[2]));
    return make_float4(d[0], d[1], d[2], __fsqrt_rn(q));
}

// Distance of x to the lower (l) and from the upper (u) bound of one axis in units of r, before the clamp: the forward clamps both
// to [-1, 1] (unit_clamp), the backward passes a gradient where they lie inside (in_unit: torch.clamp's rule)
__device__ __forceinline__ void boundary_terms(float x, const FeatParams& P, int a, float& l, float& u) {
    l = __fdiv_rn(__fsub_rn(x, P.lo[a]), P.r);
    u = __fdiv_rn(__fsub_rn(P.hi[a], x), P.r);
}
__device__ __forceinline__ float unit_clamp(float v) { return fminf(fmaxf(v, -1.f), 1.f); }
__device__ __forceinline__ bool in_unit(float v) { return v >= -1.f && v <= 1.f; }

// Node features of one particle, row = its row of frame 0, fs = the frame stride, o = its node_feature_dim floats: the k - 1
// velocities (utils.py:27-40), the clamped boundary terms and the material (collate_utils.py:195-208), the control (217-232)
__device__ __forceinline__ void node_features_row(const float* __restrict__ row, int64_t fs, const FeatParams& P, float* __restrict__ o) {
    float prev[3], cur[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) prev[a] = row[P.cart + a];
    for (int t = 1; t < P.k; ++t) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            cur[a] = row[t * fs + P.cart + a];
            o[(t - 1) * 3 + a] = __fdiv_rn(__fsub_rn(__fsub_rn(cur[a], prev[a]), P.vm[a]), P.vs[a]);
            prev[a] = cur[a];
        }
    }
    float* b = o + 3 * (P.k - 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l, u;
        boundary_terms(cur[a], P, a, l, u);
        b[a] = unit_clamp(l);
        b[3 + a] = unit_clamp(u);
    }
    const float* last = row + (int64_t)(P.k - 1) * fs;
    b[6] = last[P.mat];
    if (P.ctrl >= 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) b[7 + a] = __fdiv_rn(__fsub_rn(last[P.ctrl + a], P.vm[a]), P.vs[a]);
    }
}

// Control of one rigid particle, last = its row of the last frame, tgt = its scripted xyz or nullptr: the way to the target, or
// without one its current xyz (rollout_utils.py:40-47 / traj_utils.py:126-134)
__device__ __forceinline__ void control_overwrite_row(float* __restrict__ last, const FeatParams& P, const float* __restrict__ tgt) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float cur = last[P.cart + a];
        last[P.ctrl + a] = tgt ? __fsub_rn(tgt[a], cur) : cur;
    }
}

// The recorded drive (compute_rollout's ground-truth mode): fr = the particle's row of the recorded frame of this step.
// Before the step the control columns of a rigid particle take the recording's (rollout_utils.py:45) ...
__device__ __forceinline__ void recorded_control_row(float* __restrict__ last, const FeatParams& P, const float* __restrict__ fr) {
#pragma unroll
    for (int a = 0; a < 3; ++a) last[P.ctrl + a] = fr[P.ctrl + a];
}
// ... and after it, on the new last frame, its xyz takes the xyz of the SAME recorded frame (rollout_utils.py:60: the pose lags
// the window by one step); the row's other columns are what the shift left there
__device__ __forceinline__ void recorded_pose_row(float* __restrict__ last, const FeatParams& P, const float* __restrict__ fr) {
#pragma unroll
    for (int a = 0; a < 3; ++a) last[P.cart + a] = fr[P.cart + a];
}

// Next xyz of one particle from its xyz in the last two frames (l1, l2) and its predicted, normalised acceleration:
// l1 + ((l1 - l2) + (pred * acc_std + acc_mean)) (rollout_utils.py:145-158)
__device__ __forceinline__ float3 integrate_row(const float* __restrict__ l1, const float* __restrict__ l2, const float* __restrict__ pred,
                                                const FeatParams& P) {
    float nxt[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float acc = __fadd_rn(__fmul_rn(pred[a], P.as[a]), P.am[a]);
        const float lv = __fsub_rn(l1[a], l2[a]);
        nxt[a] = __fadd_rn(l1[a], __fadd_rn(lv, acc));
    }
    return make_float3(nxt[0], nxt[1], nxt[2]);
}

// Training target of one particle: its normalised acceleration from the xyz that follows the window (nxt) and its xyz in the last
// two frames (l1, l2), (((nxt - 2 l1) + l2) - acc_mean) / acc_std in compute_target's op order (utils.py:10-24,
// collate_utils.py:150-159) -- integrate_row's inverse up to rounding
__device__ __forceinline__ float3 target_row(const float* __restrict__ nxt, const float* __restrict__ l1, const float* __restrict__ l2,
                                             const FeatParams& P) {
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float acc = __fadd_rn(__fsub_rn(nxt[a], __fmul_rn(2.f, l1[a])), l2[a]);
        t[a] = __fdiv_rn(__fsub_rn(acc, P.am[a]), P.as[a]);
    }
    return make_float3(t[0], t[1], t[2]);
}

// Window shift and write-back of one particle, row = its row of frame 0: frame t takes frame t + 1, then the last frame's xyz takes
// nxt (rk < 0: not rigid; by value, so that a fused caller's stays in registers) or the scripted tgt
// (rollout_utils.py:53-61 / traj_utils.py:146-152)
__device__ __forceinline__ void shift_write_row(float* __restrict__ row, int64_t fs, const FeatParams& P, int rk, float3 nxt,
                                                const float* __restrict__ tgt) {
    for (int t = 0; t + 1 < P.k; ++t)
        for (int d = 0; d < P.D; ++d) row[t * fs + d] = row[(t + 1) * fs + d];
    float* last = row + (int64_t)(P.k - 1) * fs + P.cart;
    if (rk < 0) {
        last[0] = nxt.x; last[1] = nxt.y; last[2] = nxt.z;
    } else if (tgt) {
#pragma unroll
        for (int a = 0; a < 3; ++a) last[a] = tgt[a];
    }  // rigid row without a scripted pose keeps its pre-step row (traj_utils.py:150-152)
}
#endif

}  // namespace gm
