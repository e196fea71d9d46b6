// Argument block and launcher of the edge MLP kernels (mlp.hip), used by model.hip.
#pragma once
#include "common.h"

namespace gm {

// gm_model_set_precision (ABI values): how the inference kernels form a Linear's products on the fp16 matrix pipe (hmma_dev.h).
// Every launcher picks its kernel's instantiation from the `precision` of its argument block; nothing else depends on it.
constexpr int kPrecisionF32 = 0;   // three partial products per multiply: fp32 accuracy
constexpr int kPrecisionF16 = 1;   // one: weights and inputs of every Linear rounded to fp16, fp32 accumulation

// What the edge kernels read: launch_edge_sys / launch_edge_sys_enc (hedge.h) take it as is, the streamed path copies it into an
// HmEdgeArgs (hmlp.h).
struct EdgeArgs {
    const CsrHeader* hdr;  // device-side edge count (rollout path) or nullptr
    int n_edges_host;
    const int* dst;        // [E] aggregation node per sorted position (processor only)
    const int* src;        // [E]
    const int* eid;        // [E] row of e_in for sorted position p, or nullptr: row = p
    const int* eid_out;    // [E] row of e_out (and of the residual read), or nullptr: row = p
    const float* P;        // [N][2H]  P_i (+b1) | P_j
    const float* e_in;     // processor: [E][H]; encoder: raw edge_attr [E][k1]
    float* e_out;          // [E][H]
    float* agg;            // [N][H] pre-zeroed, or nullptr
    float* side;           // [n_groups][H] head partials of the scatter-add (hedge.h), sys / hm kernels
    const float* wstream_h3; // fp16 hi / lo image of the systolic kernel (hedge.h), or nullptr
    const float* wstream_hm; // fp16 hi / lo Linear images of this MLP for the streamed kernels (hmlp.h)
    const int* edge_blocks;  // block / chunk tables of the edge list (carve_edge_blocks), or nullptr
    int64_t n_nodes_tab;     // n_nodes the tables were carved for
    ProfState* prof;         // timing of this launch (gm_model_profile), or nullptr
    const float* ln_g;
    const float* ln_b;
    float eps;
    int residual;          // e_out = e' + e_in
    int discard_e_out;     // nobody reads e_out after this launch (the last step of a forward): a kernel may leave it unwritten
    int P_prescaled;       // P was written times the systolic kernel's weight scale T1 (HmNodeArgs::p_scale): that kernel's launch
    int k1;                // encoder: edge_dim
    int h_valid;           // the model's hidden_size (<= the width H the kernel runs at; LayerNorm statistics are over these features)
    int zero_pad_rows;     // systolic encoder: e_out is a forward's latent array -- keep kEdgePadRows zero rows behind row n_edges (hedge.h)
    int precision;         // kPrecisionF32 / kPrecisionF16 (the model's)
};

#ifdef __HIPCC__
// The Linear in front of a LayerNorm is held with the common offset of its outputs taken off -- of every column of W over the
// outputs, and of the bias: the LayerNorm removes it anyway, and removed here it never meets a float32 sum, where an offset c on a
// deviation sigma costs c / sigma ulps (tests/layernorm_cases.py: offset(c)).  What is taken off is the COARSE part of the mean: its
// nearest multiple of g, the power of two with 2 s < g <= 4 s, s the largest deviation from the mean.  Weights whose mean is below
// their own spread -- any initialisation, most trained layers -- give 0 and are held as they are, bit for bit; an offset beyond the
// spread is removed down to at most 2 s.  s = 0 (all entries equal): the mean itself, so nothing is left.
__device__ __forceinline__ float coarse_mean(double mean, float spread) {
    if (!(spread > 0.f)) return (float)mean;
    if (!(spread < 1.0e30f)) return 0.f;
    int ex;
    (void)frexpf(spread, &ex);                  // spread in [2^(ex-1), 2^ex)
    const double g = ldexp(1.0, ex + 1);
    return (float)(rint(mean / g) * g);
}
// of n floats at p[0], p[stride], ..
__device__ __forceinline__ float coarse_mean_of(const float* p, size_t stride, int n) {
    if (n <= 0) return 0.f;
    double a = 0.0;
    for (int r = 0; r < n; ++r) a += (double)p[(size_t)r * stride];
    a /= (double)n;
    float s = 0.f;
    for (int r = 0; r < n; ++r) s = fmaxf(s, fabsf((float)((double)p[(size_t)r * stride] - a)));
    return coarse_mean(a, s);
}
#endif

struct VecJob {
    const float* src;
    size_t dst_off;
    int count;   // floats copied
    int zero_to; // destination floats [count, zero_to) are zeroed (padding), 0 = none
    int center;  // the bias in front of a LayerNorm as the training kernels read it: b - coarse_mean(b)
};
constexpr int kVecJobsMax = 96;   // (a batch is a kernel argument: 96 jobs of 32 bytes)
struct VecJobs {
    int n;
    VecJob job[kVecJobsMax];
};
int launch_vec_batch(const VecJobs& jobs, float* base, hipStream_t s);
// sys: the systolic form (hedge.hip) that the forward's route chose for this MLP, else the streamed one (hmlp.hip)
int launch_edge(int H, int NL, bool enc, bool sys, const EdgeArgs& a, int64_t edge_capacity, hipStream_t s);

}  // namespace gm
