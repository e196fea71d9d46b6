// Model handle shared by model.hip (inference) and train_model.hip (training).
#pragma once
#include <mutex>
#include <vector>
#include "common.h"
#include "hmlp.h"
#include "mlp.h"
#include "step_rows.h"
#include "train.h"

namespace gm {
// choices of gm_model_set_edge_kernel (ABI values; 1 .. 4 were the round-1 fp32 / bf16 x 6 kernels, removed in round 5)
enum EdgeKernel : int {
    EK_AUTO = 0,      // the systolic kernels where they exist and the graph fits them, the systolic node path from kSysNodeMinNodes
    EK_SYS = 5,       // as EK_AUTO; needs the systolic images (hidden 128, num_layers 2)
    EK_HM = 6,        // the streamed kernels everywhere
    EK_SYS_ALL = 7,   // as EK_SYS, and the systolic node path at any graph size
};

// One MLP of the state_dict (epd_gnn.py:63-84): tensors [base, end) = W_0, b_0, .., W_NL, b_NL [, gamma, beta]; `in` inputs of
// Linear 0, `out` outputs of Linear NL, hidden_size between them; normed: ends in a LayerNorm (all but the decoder)
struct MlpSpec { int base, end, in, out; bool normed; };
// One chain's forward weight stream in packed_t3: where it starts and how many stages the chain walks -- `stages` on its own,
// `stages_tail` with the next step's [W_i | W_j] that follow it (node streams whose kernel may run the projection tail; else 0)
struct TStream { size_t off = 0; int stages = 0, stages_tail = 0; };
// the model's MLPs in state_dict order: edge encoder, node encoder, the edge and node MLP of each step, the decoder
std::vector<MlpSpec> model_mlps(const gm_model_desc& d);

// What a rollout step (model.hip) and its backward (rollout_grad.hip) ask of a model for a scene: its node features' width
// (step_rows.h) and a 3-D scene's edge features and accelerations; `who`: the entry point, for the message
static inline int check_model_for_scene(const gm_model_desc& d, const gm_feature_desc* fd, const char* who) {
    const int F = node_feature_dim(fd);
    GM_REQUIRE(d.node_dim == F, GM_ERR_INVALID_ARGUMENT, "%s: model node_dim=%d but features give %d", who, d.node_dim, F);
    GM_REQUIRE(d.edge_dim == 4 && d.out_dim == 3, GM_ERR_INVALID_ARGUMENT, "%s: needs edge_dim=4, out_dim=3 (3-D scene)", who);
    return GM_OK;
}
}  // namespace gm

struct gm_model {
    gm_model_desc d;
    int H, NL, M;                 // H: the model's hidden_size
    int Hp = 0;                   // the width the inference kernels run at: H zero-padded to 64 / 128 / 256 (hm_padded_hidden)
    int ci = 0, cj = 1, ce = 2;   // column block of phi_e's first Linear that multiplies h_i, h_j, e (gm_model_desc.col_*)
    int ch = 0, ca = 1;           // column block of phi_v's first Linear for h, agg (gm_model_desc.node_agg_first)
    std::vector<gm::MlpSpec> mlp;   // gm::model_mlps(d)
    const gm::MlpSpec& edge_mlp(int k) const { return mlp[2 + 2 * k]; }
    const gm::MlpSpec& node_mlp(int k) const { return mlp[3 + 2 * k]; }
    // Every buffer below is laid out, and every job that fills it planned, once by gm_model_create (plan_weights); a load
    // launches the jobs.  Offsets are in floats from the buffer's base.
    // The model's own copy of the raw tensors (device).  A weight update refreshes it and the cheap images (vec, the training
    // streams); the inference images (packed_hm, packed_h3) are re-packed from it by the first inference call that follows
    // (ensure_inference_images): a training loop, which updates the weights every step, never pays for them.
    float* raw = nullptr;
    std::vector<gm::VecJob> raw_jobs;   // one per tensor: where it goes (each load supplies the source)
    float* vec = nullptr;     // per-MLP contiguous [bias_0..bias_NL, ln_gamma, ln_beta]
    std::vector<gm::VecJob> vec_jobs;
    size_t v_enc_edge, v_enc_node, v_dec;   // start of each MLP's block
    std::vector<size_t> v_edge, v_node;
    // bf16 x 3 weight streams of the training kernels (train.hip), hidden 64 / 128 / 256 only: MLP after MLP, stages of kStageFloatsB3
    float* packed_t3 = nullptr;
    std::vector<gm::PackTJob> t_jobs;
    gm::TStream t_enc_edge, t_enc_node, t_dec;
    std::vector<gm::TStream> t_edge, t_node, t_proj;   // t_proj: [W_i | W_j] of step k, the tail of the node encoder (k = 0) or node step k - 1
    float* packed_hm = nullptr;  // fp16 hi / lo image of every Linear (hmlp.h)
    std::vector<gm::PackHmJob> hm_jobs;   // host copy of hm_jobs_dev
    gm::PackHmJob* hm_jobs_dev = nullptr;
    float* hm_stats = nullptr;
    size_t hm_enc_edge = 0, hm_enc_node = 0, hm_enc_node_tail = 0;
    std::vector<size_t> hm_edge, hm_node, hm_node_tail, hm_node_q;   // hm_node_q: Q = h W_h^T + b1 of node step k (hedge.h)
    // fp16 hi / lo images of the systolic kernels (hedge.h), hidden 128 / num_layers 2 only: the M processor edge MLPs, the edge
    // encoder, then the M processor node MLPs (agg block of Linear 1 | Linear 2 | Linear 3)
    float* packed_h3 = nullptr;
    std::vector<gm::PackH3Job> h3_jobs;
    size_t h3_enc = 0;
    std::vector<size_t> h3_edge, h3_node;
    bool infer_stale = true;
    std::mutex lazy_mu;
    gm::ProfState* prof = nullptr;  // gm_model_profile
    int edge_kernel = gm::EK_AUTO;   // gm_model_set_edge_kernel: which kernels the forwards of this model may take (gm::EdgeKernel)
    bool node_fusion = true;         // gm_model_set_node_fusion: the systolic node path runs a step's node MLP and projections as one launch
    int precision = gm::kPrecisionF32;   // gm_model_set_precision: partial products of the inference kernels (training never reads it)
    // Every copy / pack of the weights is queued on the stream of the call that triggered it; `ready` is recorded behind the last
    // one.  An entry point that runs on ANOTHER stream waits for it there (weights_ready_on), so a model may be loaded on one
    // stream and used on others.  (The other direction -- a weight update while a forward on another stream still reads the old
    // images -- is the caller's to order, like any write to memory a queued kernel reads.)
    hipEvent_t ready = nullptr;
    hipStream_t ready_stream = nullptr;
};
int ensure_inference_images(const gm_model* m, hipStream_t s);   // model.hip; called by every inference entry point
int weights_ready_on(const gm_model* m, hipStream_t s);          // model.hip; called by every entry point that reads the packed weights
// model.hip; a kernel queued on s has rewritten m->raw (train_step.hip: Adam works on it): what a load does after its copy -- vec and
// the training streams re-packed on s, the inference images stale, `ready` recorded
int weights_changed_in_place(gm_model* m, hipStream_t s);

