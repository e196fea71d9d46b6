// Launch of the edge MLP kernels (+ the batched vector copy of a weight load).  Which form an MLP takes is decided once per
// forward (model.hip: route_forward):
//   processor phi_e (and the edge encoder of the rollout path) at hidden 128 / num_layers 2  -> systolic fp16 x 3 kernels (hedge.hip)
//   everything else                                                                         -> streamed fp16 x 3 kernels (hmlp.hip)
// Reference semantics: EncProcDecGNN.forward / _process / _build_mlp, gnn_manip/models/epd_gnn.py:72-105.
#include <string.h>
#include "common.h"
#include "mlp.h"

#include "hedge.h"
#include "hmlp.h"

namespace gm {

// ------------------------------------------------------------------------------------------
// copies of small vectors / raw tensors into the model's own buffers (one launch for many)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vec_batch_kernel(VecJobs J, float* __restrict__ base) {
    const VecJob j = J.job[blockIdx.x];   // blockIdx.y: slice of the tensor (a weight matrix is 16k .. 49k floats: not one workgroup's job)
    // (a centred job is a bias: at most a few hundred floats, walked by every thread in the same order -- redundant on purpose, the
    // pack is no hot path; 0 leaves the bits alone)
    const float off = j.center ? coarse_mean_of(j.src, 1, j.count) : 0.f;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < max(j.count, j.zero_to); i += gridDim.y * blockDim.x)
        base[j.dst_off + i] = i < j.count ? (float)((double)j.src[i] - (double)off) : 0.f;
}

int launch_vec_batch(const VecJobs& jobs, float* base, hipStream_t s) {
    if (jobs.n <= 0) return GM_OK;
    hipLaunchKernelGGL(vec_batch_kernel, dim3(jobs.n, 16), dim3(256), 0, s, jobs, base);
    GM_LAUNCH_CHECK();
    return GM_OK;
}

// ------------------------------------------------------------------------------------------
// edge MLP launcher
// ------------------------------------------------------------------------------------------
int launch_edge(int H, int NL, bool enc, bool sys, const EdgeArgs& a, int64_t edge_capacity, hipStream_t s) {
    if (edge_capacity <= 0) return GM_OK;
    if (sys && enc) return launch_edge_sys_enc(a, s);
    if (sys) return launch_edge_sys(a, carve_edge_blocks(const_cast<int*>(a.edge_blocks), a.n_nodes_tab, edge_capacity), edge_capacity, s);
    HmEdgeArgs h{};
    h.hdr = a.hdr; h.n_edges_host = a.n_edges_host; h.dst = a.dst; h.src = a.src; h.eid = a.eid; h.eid_out = a.eid_out;
    h.P = a.P; h.e_in = a.e_in; h.e_out = a.e_out; h.agg = a.agg; h.w = a.wstream_hm; h.ln_g = a.ln_g; h.ln_b = a.ln_b;
    h.eps = a.eps; h.residual = a.residual; h.discard_e_out = a.discard_e_out; h.k1 = a.k1; h.nl = NL; h.prof = a.prof;
    h.h_valid = a.h_valid;
    h.precision = a.precision;
    h.flags = a.hdr ? const_cast<int*>(&a.hdr->error_flags) : nullptr;
    if (!enc) {
        const EdgeBlocks t = carve_edge_blocks(const_cast<int*>(a.edge_blocks), a.n_nodes_tab, edge_capacity);
        h.blk = t.blk; h.tab = t.hdr; h.head = t.head; h.side = a.side;
    }
    return launch_edge_hm(H, enc, h, s);
}

}  // namespace gm
