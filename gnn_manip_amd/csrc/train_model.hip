// Training entry points: forward with activation tape and backward of the whole
// encode-process-decode model (host orchestration; kernels in train.hip / mlp.hip).
// Reference call sites: examples/train_dyn.py:45-72 (model.forward -> loss.backward -> Adam),
// gnn_manip/models/epd_gnn.py:86-105 (forward wiring the gradients flow back through).
#include <vector>
#include "common.h"
#include "mlp.h"
#include "model.h"
#include "train.h"

using namespace gm;

namespace {

// The destination-sorted edges (aggregation index i = edge_index[1]) and the source-grouped view of the sorted list.  It starts
// every tape that has one: epd_gnn.py (_HeaderWatch) reads the edge_index verdict from the destination sort's header at byte 0.
struct TrainCsr {
    CsrWs dst, src;   // each view's header starts its csr workspace
    int64_t* ei2;     // [2][e] the sorted list with its rows swapped: the input of the source sort
};
TrainCsr take_csr(Carver& c, int64_t n, int64_t e) {
    TrainCsr t;
    const size_t bytes = gm_csr_workspace_bytes(n, e);
    t.dst = carve_csr(c.take<char>(bytes), n, e);
    t.src = carve_csr(c.take<char>(bytes), n, e);
    t.ei2 = c.take<int64_t>((size_t)2 * e);
    return t;
}
int build_csr(const TrainCsr& t, const int64_t* edge_index, int64_t n, int64_t e, int flow, hipStream_t s) {
    int rc = gm::csr_from_edge_index(edge_index, n, e, flow, t.dst.hdr, t.dst.bytes, false, s);
    if (rc == GM_OK) rc = launch_swap_index(t.dst.src, e, t.ei2, s);
    if (rc == GM_OK) rc = gm::csr_from_edge_index(t.ei2, n, e, 0, t.src.hdr, t.src.bytes, false, s);
    return rc;
}

TapePtr take_tape(Carver& c, int64_t rows, int H, int NL, bool normed) {
    TapePtr t{};
    t.a = c.take<float>((size_t)NL * rows * H);   // post-ReLU outputs of Linear 1 .. NL, one [rows][H] array each
    t.mask = c.take<uint32_t>((size_t)NL * rows * (H / 32));
    if (normed) {
        t.xhat = c.take<float>((size_t)rows * H);
        t.rstd = c.take<float>((size_t)rows);
    }
    return t;
}

struct EncTape {
    TapePtr ee, en;
};
struct StepTape {   // one processor step
    float* agg;
    TapePtr te, tn;
};

struct Tape {
    TrainCsr csr;
    std::vector<float*> h, e;   // block inputs: h[0..M], e[0..M]
    std::vector<StepTape> step;
    float* P;
    EncTape enc;
    TapePtr dec;
    size_t bytes;
};

Tape carve_tape(void* ws, const gm_model_desc* d, int64_t n, int64_t e) {
    Tape t;
    const int H = d->hidden_size, M = d->m_steps, NL = d->num_layers;
    Carver c(ws);
    t.csr = take_csr(c, n, e);
    t.h.resize(M + 1);
    t.e.resize(M + 1);
    t.step.resize(M);
    for (int k = 0; k <= M; ++k) t.h[k] = c.take<float>((size_t)n * H);
    for (int k = 0; k <= M; ++k) t.e[k] = c.take<float>((size_t)e * H);
    for (int k = 0; k < M; ++k) t.step[k].agg = c.take<float>((size_t)n * H);
    t.P = c.take<float>((size_t)n * 2 * H);
    t.enc.ee = take_tape(c, e, H, NL, true);
    t.enc.en = take_tape(c, n, H, NL, true);
    for (int k = 0; k < M; ++k) {
        t.step[k].te = take_tape(c, e, H, NL, true);
        t.step[k].tn = take_tape(c, n, H, NL, true);
    }
    t.dec = take_tape(c, n, H, NL, false);
    t.bytes = c.used();
    return t;
}

// ---- tapes of the two standalone blocks (torch_graphnet API surface)
struct GiTape {
    EncTape enc;
    size_t bytes;
};
GiTape carve_gi_tape(void* ws, int H, int NL, int64_t n, int64_t e) {
    GiTape t;
    Carver c(ws);
    t.enc.ee = take_tape(c, e, H, NL, true);
    t.enc.en = take_tape(c, n, H, NL, true);
    t.bytes = c.used();
    return t;
}
struct InTape {
    TrainCsr csr;
    float* P;
    StepTape st;
    size_t bytes;
};
InTape carve_in_tape(void* ws, int H, int NL, int64_t n, int64_t e) {
    InTape t;
    Carver c(ws);
    t.csr = take_csr(c, n, e);
    t.P = c.take<float>((size_t)n * 2 * H);
    t.st.agg = c.take<float>((size_t)n * H);
    t.st.te = take_tape(c, e, H, NL, true);
    t.st.tn = take_tape(c, n, H, NL, true);
    t.bytes = c.used();
    return t;
}

// One backward chain's slot of BwdWs::packT: where its transposed stream starts, the stages the sizing walk reserved for it and
// the stages the last pack put there -- which is what the chain launched on it walks (0: nothing packed, the launch refuses)
struct Slot { size_t off = 0; int cap = 0, stages = 0; };

struct BwdWs {
    float *packT, *dz, *dzn, *de, *dh, *dagg, *Gi, *Gj, *part;
    float* go;          // the upstream gradient as the chains read it: zero when the forward's edge_index was flagged (gate_grad_out_kernel)
    size_t dz_stride;   // floats between dz_l and dz_(l+1) (l = 1 .. NL + 1)
    float* dzl(int l) const { return dz + (size_t)(l - 1) * dz_stride; }
    // the node-sized chains of the model backward (node MLPs, node encoder) leave their dz in a set of their own, so that the
    // weight-gradient jobs over an edge chain's dz and those over the node chain's that follows run as ONE batch
    size_t dzn_stride;
    float* dznl(int l) const { return dzn + (size_t)(l - 1) * dzn_stride; }
    // slots of packT, one per backward chain (PackBwd)
    Slot dec, enc_edge, enc_node;
    std::vector<Slot> edge, node;
    size_t bytes;
};

// The transposed images of the backward chains, each MLP's Linears in the order its chain consumes them: the one place that knows
// what a slot of BwdWs::packT holds.  With a model (m, T) it queues the pack jobs of the slots it is asked for and counts the
// stages it puts in each.  Without one (carve_bwd, which asks for every optional part) the same walk only lays the slots out, back
// to back.  k: the step whose tensors are packed; j: its slot (a block's is 0).
struct PackBwd {
    const gm_model_desc& d;
    BwdWs& b;
    const gm_model* m;   // nullptr: the sizing walk
    const float* const* T;
    hipStream_t s;
    const int H = d.hidden_size, NL = d.num_layers;
    PackTJobs jobs{};
    int rc = GM_OK;
    size_t laid = 0;     // sizing walk: floats of packT laid out so far
    int flush() {   // also when a batch is full
        if (rc == GM_OK && jobs.n > 0) rc = launch_pack_b3_batch(jobs, b.packT, s);
        jobs.n = 0;
        return rc;
    }
    // what only the real pack looks up: Linear l of MLP i (gm_model::mlp), the first column of block c (gm_model::ci ..) of a Linear 1
    const float* W(int i, int l) const { return m ? T[m->mlp[i].base + 2 * l] : nullptr; }
    int col(int gm_model::*c) const { return m ? m->*c * H : 0; }
    Slot& begin(Slot& sl) { if (m) sl.stages = 0; else sl = {laid, 0, 0}; return sl; }
    void job(Slot& sl, const float* W, int w_rows, int ld, int col0, int ksub, int center = 0) {
        const int st = layer_stages_b3(w_rows, ksub);
        if (!m) { sl.cap += st; laid = sl.off + (size_t)sl.cap * kStageFloatsB3; return; }
        if (rc == GM_OK) rc = [&]() -> int {
            GM_REQUIRE(sl.stages + st <= sl.cap, GM_ERR_WORKSPACE, "backward pack: %d stages into a slot laid out for %d", sl.stages + st, sl.cap);
            return GM_OK;
        }();
        if (rc != GM_OK) return;
        if (jobs.n == kPackTJobsMax) flush();
        PackTJob& j = jobs.job[jobs.n++];
        j.W = W; j.w_rows = w_rows; j.ld = ld; j.col0 = col0; j.ksub = ksub; j.fwd = 0; j.center = center;
        j.dst_off = sl.off + (size_t)sl.stages * kStageFloatsB3;
        sl.stages += st;
    }
    // the hidden Linears NL + 1 .. 2 of MLP i, which ends in a LayerNorm: the Linear in front of it centred, as in the forward's stream
    void hidden(Slot& sl, int i) { for (int l = NL; l >= 1; --l) job(sl, W(i, l), H, H, 0, H, l == NL); }
    void ij(Slot& sl, int k) {   // W_i, W_j: the column blocks of step k's first edge Linear that multiply h_i, h_j
        job(sl, W(2 + 2 * k, 0), H, 3 * H, col(&gm_model::ci), H);
        job(sl, W(2 + 2 * k, 0), H, 3 * H, col(&gm_model::cj), H);
    }
    // an encoder (MLP i).  ij: in front, step 0's W_i^T, W_j^T (the model's node encoder: its chain also takes that step's Gi / Gj);
    // input: behind, W_1^T for the gradient w.r.t. the raw features (block API)
    void enc(Slot& slot, int i, int k1, bool with_ij, bool input) {
        Slot& sl = begin(slot);
        if (with_ij) ij(sl, 0);
        hidden(sl, i);
        if (input) job(sl, W(i, 0), H, k1, 0, k1);
    }
    void dec() {
        const int i = 2 + 2 * d.m_steps;
        Slot& sl = begin(b.dec);
        job(sl, W(i, NL), d.out_dim, H, 0, H);
        for (int l = NL - 1; l >= 0; --l) job(sl, W(i, l), H, H, 0, H);
    }
    void edge(int k, int j) {
        Slot& sl = begin(b.edge[j]);
        hidden(sl, 2 + 2 * k);
        job(sl, W(2 + 2 * k, 0), H, 3 * H, col(&gm_model::ce), H);
    }
    void node(int k, int j) {
        Slot& sl = begin(b.node[j]);
        if (j + 1 < (int)b.node.size()) ij(sl, k + 1);   // a step with a next one: its chain also takes that step's Gi / Gj
        hidden(sl, 3 + 2 * k);
        job(sl, W(3 + 2 * k, 0), H, 2 * H, col(&gm_model::ch), H);
        job(sl, W(3 + 2 * k, 0), H, 2 * H, col(&gm_model::ca), H);
    }
    // a block's projection backward: step k's W_i^T, W_j^T alone, in the node encoder's slot (which a block's backward does not use)
    void proj(int k) { ij(begin(b.enc_node), k); }
    void enc_node(bool with_ij, bool input) { enc(b.enc_node, 1, d.node_dim, with_ij, input); }
    void enc_edge(bool input) { enc(b.enc_edge, 0, d.edge_dim, false, input); }
};

BwdWs carve_bwd(void* ws, const gm_model_desc* d, int64_t n, int64_t e) {
    BwdWs b;
    const int H = d->hidden_size, M = d->m_steps, NL = d->num_layers;
    b.edge.resize(M);
    b.node.resize(M);
    PackBwd lay{*d, b, nullptr, nullptr, nullptr};
    lay.dec();
    for (int k = 0; k < M; ++k) {
        lay.node(k, k);
        lay.edge(k, k);
    }
    lay.enc_node(true, true);
    lay.enc_edge(true);
    Carver c(ws);
    b.packT = c.take<float>(lay.laid);
    const int64_t R = n > e ? n : e;
    b.dz_stride = align_up((size_t)R * H, 64);
    b.dz = c.take<float>((size_t)(NL + 1) * b.dz_stride);
    b.dzn_stride = align_up((size_t)n * H, 64);
    b.dzn = c.take<float>((size_t)(NL + 1) * b.dzn_stride);
    b.de = c.take<float>((size_t)e * H);
    b.dh = c.take<float>((size_t)n * H);
    b.dagg = c.take<float>((size_t)n * H);
    b.Gi = c.take<float>((size_t)n * H);
    b.Gj = c.take<float>((size_t)n * H);
    b.part = c.take<float>(wgrad_partial_floats(H));
    b.go = c.take<float>((size_t)n * (d->out_dim > 0 ? d->out_dim : 1));
    b.bytes = c.used();
    return b;
}
// backward scratch of a single block: same carve as the whole model with one processor step
BwdWs carve_block_bwd(void* ws, const gm_model_desc* d, int64_t n, int64_t e) {
    gm_model_desc d1 = *d;
    d1.m_steps = 1;
    return carve_bwd(ws, &d1, n, e);
}

// The launches of one backward call after its images are packed.  Every call does nothing once rc holds an error.
// grads == nullptr: an inputs-only backward (gm_epd_backward_inputs_only).  No weight-gradient job is enqueued (so every flush is
// empty and launches nothing), and the chains get no dgamma / dbeta, which is the launch argument that makes their epilogue skip
// the LayerNorm parameter sums (train.hip: A.ln_part).  The dz chains, the segment sums and the dx tails are the same launches on
// the same operands: a tile's results do not depend on which workgroup walks it.
struct BwdRun {
    const gm_model* m;
    float* const* grads;
    const BwdWs& b;
    hipStream_t s;
    WgradBatch wb;   // weight-gradient jobs run a batch per launch; flushed before anything overwrites their operands
    int rc = GM_OK;
    BwdRun(const gm_model* m_, float* const* grads_, const BwdWs& b_, hipStream_t s_) : m(m_), grads(grads_), b(b_), s(s_) {
        wgrad_batch_init(wb, b.part, m->H, s);
    }
    float* g(int i) const { return grads ? grads[i] : nullptr; }   // gradient tensor i, or nullptr in an inputs-only backward
    void wgrad(const float* dz, int ldz, int Mo, const float* X, int ldx, int K, const int* xidx, int64_t rows, float* out, int ldw,
               int col0, float* db) {
        if (rc == GM_OK && grads) rc = wgrad_enqueue(wb, dz, ldz, Mo, X, ldx, K, xidx, rows, out, ldw, col0, db);
    }
    // sl: the slot the chain's stream was packed into.  flush: the chain overwrites operands of the waiting jobs
    void launch(int kind, TrainBwdArgs a, const Slot& sl, bool flush) {
        a.wstream = b.packT + sl.off; a.wstages = sl.stages;
        if (rc == GM_OK && flush) rc = wgrad_flush(wb);
        if (rc == GM_OK) rc = launch_train_bwd(m->H, kind, a, s, &wb);
    }
    // dW = dz_(l+1)^T a_l (+ the bias) of Linears l + 1 = top + 1 .. 2 of the MLP whose chain `a` just ran
    void tail(const TrainBwdArgs& a, int base, int top) {
        for (int l = top; l >= 1; --l)
            wgrad(a.dz + (size_t)l * a.dz_stride, m->H, m->H, a.tape.a + (size_t)(l - 1) * a.rows * m->H, m->H, m->H, nullptr, a.rows,
                  g(base + 2 * l), m->H, 0, g(base + 2 * l + 1));
    }
    // the LayerNorm and dz fields of a normed MLP's chain: its LayerNorm parameter gradients are summed inside the chain kernel and
    // reduced by wb's next flush; node_set: dz goes to the node-sized set (BwdWs::dzn), which no waiting job reads
    void set_normed(TrainBwdArgs& a, int base, size_t voff, bool node_set) const {
        const int NL = m->NL;
        a.ln_g = m->vec + voff + (size_t)(NL + 1) * m->H;
        a.dgamma = g(base + 2 * (NL + 1)); a.dbeta = g(base + 2 * (NL + 1) + 1);
        a.dz = node_set ? b.dzn : b.dz; a.dz_stride = node_set ? b.dzn_stride : b.dz_stride; a.nl = NL;
    }
    // a normed MLP's chain and the weight gradients of its Linears 2 .. NL + 1 (Linear 1's differ at every call site).  A chain
    // that writes the edge-sized dz set flushes first; one that writes the node-sized set adds its jobs to the waiting ones.
    void chain(int kind, TrainBwdArgs a, const Slot& sl, int base, size_t voff, bool node_set) {
        set_normed(a, base, voff, node_set);
        launch(kind, a, sl, !node_set);
        tail(a, base, m->NL);
    }
    // node-level sums of an edge chain's dz_1 (G_i over each edge's destination, G_j over its source): everything the factorised
    // Linear 1 needs -- its W_i / W_j gradients (input h) here, the input gradient W_i^T G_i + W_j^T G_j in the next node chain
    void ij_grads(const TrainCsr& csr, const float* h, int be, int64_t n) {
        if (rc == GM_OK)
            rc = launch_segment_sum_pair(m->H, csr.dst.in_ptr, nullptr, csr.src.in_ptr, csr.src.eid, b.dzl(1), nullptr, nullptr, b.Gi, b.Gj,
                                         n, s);
        wgrad(b.Gi, m->H, m->H, h, m->H, m->H, nullptr, n, g(be), 3 * m->H, m->ci * m->H, nullptr);
        wgrad(b.Gj, m->H, m->H, h, m->H, m->H, nullptr, n, g(be), 3 * m->H, m->cj * m->H, nullptr);
    }
    int finish() {
        if (rc == GM_OK) rc = wgrad_flush(wb);
        return rc;
    }
};

// A training forward does not synchronise: an edge_index entry outside [0, n) is flagged by the destination sort in the tape's CSR
// headers and reported at a later forward / status() (epd_gnn.py).  Until then the step must not do damage: the flagged forward's
// output is NaN (the loss shows it) and its backward produces exactly zero gradients (the upstream gradient is gated to zero), so
// the optimiser step that runs before the error surfaces leaves the weights where a raise at the forward would have left them.
__global__ void __launch_bounds__(256) poison_if_flagged_kernel(const CsrHeader* a, const CsrHeader* b, float* out, size_t count) {
    if (!((a->error_flags | b->error_flags) & ERRF_BAD_EDGE_INDEX)) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) out[i] = __builtin_nanf("");
}
__global__ void __launch_bounds__(256) gate_grad_out_kernel(const CsrHeader* a, const CsrHeader* b, const float* g, float* out, size_t count) {
    const bool bad = ((a->error_flags | b->error_flags) & ERRF_BAD_EDGE_INDEX) != 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) out[i] = bad ? 0.f : g[i];
}
unsigned small_grid(size_t count) {
    const size_t g = (count + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 512 ? 512 : g));
}

// The checks every training entry point starts with, before any device call.
int check_model(const gm_model* m, int64_t n, int64_t e, const char* who) {
    GM_REQUIRE(!m || m->packed_t3, GM_ERR_UNSUPPORTED, "%s: the training kernels are instantiated for hidden_size 64 / 128 / 256", who);
    GM_REQUIRE(m, GM_ERR_INVALID_ARGUMENT, "%s: null model", who);
    GM_REQUIRE(n >= 1 && e >= 0 && n < ((int64_t)1 << 31) && e < ((int64_t)1 << 31) / m->H, GM_ERR_INVALID_ARGUMENT,
               "%s: sizes out of range (n=%lld, e=%lld)", who, (long long)n, (long long)e);
    return GM_OK;
}
// a backward's state_dict: all of it, and the tensors and gradients [lo, hi) of the MLPs it reads non-null (grads == nullptr: an
// inputs-only backward has none)
int check_tensors(const gm_model* m, const float* const* T, float* const* grads, int n_tensors, int lo, int hi, const char* who) {
    const int nt = gm_model_num_tensors(&m->d);
    GM_REQUIRE(n_tensors == nt, GM_ERR_INVALID_ARGUMENT, "%s: expected %d tensors, got %d", who, nt, n_tensors);
    for (int i = lo; i < hi; ++i) GM_REQUIRE(T[i] && (!grads || grads[i]), GM_ERR_INVALID_ARGUMENT, "%s: tensor / gradient %d is null", who, i);
    return GM_OK;
}
// after the entry point's own checks: the caller's buffers are large enough, the kernels set up, the weight streams ready on s
int ready_to_launch(const gm_model* m, size_t tape_bytes, size_t tape_need, size_t ws_bytes, size_t ws_need, hipStream_t s, const char* who) {
    GM_REQUIRE(tape_bytes >= tape_need, GM_ERR_WORKSPACE, "%s: tape %zu < %zu", who, tape_bytes, tape_need);
    GM_REQUIRE(ws_bytes >= ws_need, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, ws_need);
    int rc = train_kernels_init();
    if (rc != GM_OK) return rc;
    return weights_ready_on(m, s);   // the weight streams may have been packed on another stream (model.h)
}

// the MLP's forward stream; tail: the chain runs on into the next step's [W_i | W_j] behind it (TrainFwdArgs::P_out)
void set_stream(const gm_model* m, TrainFwdArgs& a, const TStream& t, bool tail) {
    a.wstream = m->packed_t3 + t.off; a.wstages = tail ? t.stages_tail : t.stages;
}
void set_normed(const gm_model* m, TrainFwdArgs& a, size_t voff) {
    const float* v = m->vec + voff;
    const int H = m->H, NL = m->NL;
    a.bias = v; a.bias_tail = v + H; a.ln_g = v + (size_t)(NL + 1) * H; a.ln_b = v + (size_t)(NL + 2) * H; a.eps = m->d.ln_eps; a.nl = NL;
}

// The two encoders.  rowidx: the edge_attr row of each destination-sorted edge (nullptr: the caller's order); P: the node
// encoder's tail writes step 0's P = h_0 [W_i | W_j]^T (+ b1) there (nullptr: no tail).
int fwd_encoders(const gm_model* m, int64_t n, int64_t e, const float* x, const float* edge_attr, const int* rowidx, const EncTape& t,
                 float* h_out, float* e_out, float* P, hipStream_t s) {
    TrainFwdArgs ea{};
    ea.rows = (int)e; ea.x_in = edge_attr; ea.rowidx = rowidx; ea.k1 = m->d.edge_dim;
    set_stream(m, ea, m->t_enc_edge, false); set_normed(m, ea, m->v_enc_edge);
    ea.tape = t.ee; ea.out = e_out;
    TrainFwdArgs na{};
    na.rows = (int)n; na.x_in = x; na.k1 = m->d.node_dim;
    set_stream(m, na, m->t_enc_node, P != nullptr); set_normed(m, na, m->v_enc_node);
    na.tape = t.en; na.out = h_out;
    if (P) { na.P_out = P; na.proj_bias = m->vec + m->v_edge[0]; }
    int rc = launch_train_fwd(m->H, TK_ENC_EDGE, ea, s);
    if (rc == GM_OK) rc = launch_train_fwd(m->H, TK_ENC_NODE, na, s);
    return rc;
}

// Processor step k: edge MLP -> segment sum of its LayerNorm output -> node MLP.  rowidx: the e_in / e_out row of each sorted
// edge (nullptr: the sorted order); residual: out = MLP(x) + x; tail: the node MLP then writes step k + 1's P over P.
int fwd_step(const gm_model* m, int k, const CsrWs& c, int64_t n, int64_t e, const float* h, const float* e_in, float* P,
             const StepTape& st, float* h_out, float* e_out, const int* rowidx, int residual, bool tail, hipStream_t s) {
    TrainFwdArgs ea{};
    ea.rows = (int)e; ea.x_in = e_in; ea.rowidx = rowidx; ea.dst = c.dst; ea.src = c.src; ea.P = P;
    set_stream(m, ea, m->t_edge[k], false); set_normed(m, ea, m->v_edge[k]);
    ea.tape = st.te; ea.out = e_out; ea.residual = residual;
    TrainFwdArgs na{};
    na.rows = (int)n; na.x_in = h; na.agg = st.agg;
    set_stream(m, na, m->t_node[k], tail); set_normed(m, na, m->v_node[k]);
    na.tape = st.tn; na.out = h_out; na.residual = residual;
    if (tail) { na.P_out = P; na.proj_bias = m->vec + m->v_edge[k + 1]; }
    int rc = launch_train_fwd(m->H, TK_PROC_EDGE, ea, s);
    // agg_i = sum over edges into i of e' = gamma * sum xhat + deg * beta
    if (rc == GM_OK) rc = launch_segment_sum_pair(m->H, c.in_ptr, nullptr, nullptr, nullptr, st.te.xhat, ea.ln_g, ea.ln_b, st.agg, nullptr, n, s);
    if (rc == GM_OK) rc = launch_train_fwd(m->H, TK_PROC_NODE, na, s);
    return rc;
}

}  // namespace

extern "C" {

size_t gm_train_tape_bytes(const gm_model_desc* desc, int64_t n, int64_t e) {
    if (!desc || n < 0 || e < 0) return 0;
    return carve_tape(nullptr, desc, n, e).bytes;
}

size_t gm_train_backward_workspace_bytes(const gm_model_desc* desc, int64_t n, int64_t e) {
    if (!desc || n < 0 || e < 0) return 0;
    return carve_bwd(nullptr, desc, n, e).bytes;
}

int gm_epd_forward_train(const gm_model* m, const float* nodes, int64_t n, const float* edge_attr, const int64_t* edge_index,
                         int64_t e, float* out, void* tape, size_t tape_bytes, void* stream) {
    int rc = check_model(m, n, e, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(nodes && out && tape && (e == 0 || (edge_attr && edge_index)), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    gm::DevGuard dev_guard(nodes);
    hipStream_t s = (hipStream_t)stream;
    const int M = m->M;
    Tape t = carve_tape(tape, &m->d, n, e);
    rc = ready_to_launch(m, tape_bytes, t.bytes, 0, 0, s, __func__);
    if (rc != GM_OK) return rc;
    rc = build_csr(t.csr, edge_index, n, e, m->d.flow, s);
    if (rc != GM_OK) return rc;
    rc = fwd_encoders(m, n, e, nodes, edge_attr, t.csr.dst.eid, t.enc, t.h[0], t.e[0], t.P, s);
    if (rc != GM_OK) return rc;
    for (int k = 0; k < M; ++k) {
        rc = fwd_step(m, k, t.csr.dst, n, e, t.h[k], t.e[k], t.P, t.step[k], t.h[k + 1], t.e[k + 1], nullptr, 1, k + 1 < M, s);
        if (rc != GM_OK) return rc;
    }
    {
        TrainFwdArgs a{};
        a.rows = (int)n; a.x_in = t.h[M]; set_stream(m, a, m->t_dec, false);
        a.bias = m->vec + m->v_dec; a.bias_tail = a.bias + m->H; a.nl = m->NL;
        a.tape = t.dec; a.out = out; a.out_dim = m->d.out_dim;
        rc = launch_train_fwd(m->H, TK_DEC, a, s);
        if (rc != GM_OK) return rc;
    }
    {   // a flagged edge_index: the prediction is NaN, not a plausible number computed on a different graph
        const size_t cnt = (size_t)n * m->d.out_dim;
        hipLaunchKernelGGL(poison_if_flagged_kernel, dim3(small_grid(cnt)), dim3(256), 0, s, t.csr.dst.hdr, t.csr.src.hdr, out, cnt);
        GM_LAUNCH_CHECK();
    }
    return GM_OK;
}

// The whole model's backward.  d_nodes / d_edge_attr (either may be null): the encoders' chains run on through W_1^T into the raw
// input rows (TrainBwdArgs::dx_in); the parameter gradients are the same launches on the same operands either way.
// grads == nullptr (inputs_only): the input gradients alone (BwdRun).
static int epd_backward(const gm_model* m, const float* const* T, int n_tensors, const float* nodes, const float* edge_attr, int64_t n,
                        int64_t e, const float* grad_out, float* const* grads, float* d_nodes, float* d_edge_attr, void* tape,
                        size_t tape_bytes, void* ws, size_t ws_bytes, void* stream, const char* who, bool inputs_only = false) {
    GM_REQUIRE(!inputs_only || d_nodes || d_edge_attr, GM_ERR_INVALID_ARGUMENT, "%s: d_nodes and d_edge_attr are both null", who);
    int rc = check_model(m, n, e, who);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(T && (grads || inputs_only) && nodes && grad_out && tape && ws && (e == 0 || edge_attr), GM_ERR_INVALID_ARGUMENT,
               "%s: null pointer", who);
    rc = check_tensors(m, T, grads, n_tensors, 0, n_tensors, who);
    if (rc != GM_OK) return rc;
    gm::DevGuard dev_guard(nodes);
    hipStream_t s = (hipStream_t)stream;
    const int H = m->H, NL = m->NL, M = m->M, OD = m->d.out_dim;
    Tape t = carve_tape(tape, &m->d, n, e);
    BwdWs b = carve_bwd(ws, &m->d, n, e);
    rc = ready_to_launch(m, tape_bytes, t.bytes, ws_bytes, b.bytes, s, who);
    if (rc != GM_OK) return rc;
    BwdRun bw(m, grads, b, s);
    const CsrWs& c = t.csr.dst;

    // ---- transposed operand images of every Linear on the backward path (batched: a few launches)
    PackBwd pk{m->d, b, m, T, s};
    pk.dec();
    for (int k = 0; k < M; ++k) {
        pk.node(k, k);
        pk.edge(k, k);
    }
    pk.enc_node(true, d_nodes != nullptr);
    pk.enc_edge(d_edge_attr != nullptr);
    rc = pk.flush();
    if (rc != GM_OK) return rc;

    // ---- the upstream gradient as the chains see it: zero for a forward whose edge_index was flagged (see gate_grad_out_kernel)
    {
        const size_t cnt = (size_t)n * OD;
        hipLaunchKernelGGL(gate_grad_out_kernel, dim3(small_grid(cnt)), dim3(256), 0, s, c.hdr, t.csr.src.hdr, grad_out, b.go, cnt);
        GM_LAUNCH_CHECK();
    }
    // ---- decoder
    {
        const int bd = m->mlp.back().base;
        TrainBwdArgs a{};
        a.rows = (int)n; a.dY = b.go; a.out_dim = OD; a.tape = t.dec;
        a.dz = b.dz; a.dz_stride = b.dz_stride; a.nl = NL; a.dx = b.dh;
        bw.launch(TB_DEC, a, b.dec, true);
        bw.wgrad(b.go, OD, OD, t.dec.a + (size_t)(NL - 1) * n * H, H, H, nullptr, n, bw.g(bd + 2 * NL), H, 0, bw.g(bd + 2 * NL + 1));
        bw.tail(a, bd, NL - 1);
        bw.wgrad(b.dzl(1), H, H, t.h[M], H, H, nullptr, n, bw.g(bd), H, 0, bw.g(bd + 1));
    }
    // ---- processor blocks, last to first
    for (int k = M - 1; k >= 0; --k) {
        const bool has_next = k + 1 < M;
        const int be = m->edge_mlp(k).base, bn = m->node_mlp(k).base;
        {
            TrainBwdArgs a{};
            a.rows = (int)n; a.dY = b.dh; a.Gi = has_next ? b.Gi : nullptr; a.Gj = has_next ? b.Gj : nullptr; a.tape = t.step[k].tn;
            a.dx_resid = b.dh; a.dx = b.dh; a.dagg_out = b.dagg;
            // node-sized dz set: the waiting jobs read the edge-sized one, Gi / Gj and tapes -- nothing this chain writes
            bw.chain(TB_NODE, a, b.node[k], bn, m->v_node[k], true);
            bw.wgrad(b.dznl(1), H, H, t.h[k], H, H, nullptr, n, bw.g(bn), 2 * H, m->ch * H, bw.g(bn + 1));
            bw.wgrad(b.dznl(1), H, H, t.step[k].agg, H, H, nullptr, n, bw.g(bn), 2 * H, m->ca * H, nullptr);
        }
        {
            TrainBwdArgs a{};
            a.rows = (int)e; a.dY = has_next ? b.de : nullptr; a.dagg = b.dagg; a.dst = c.dst; a.tape = t.step[k].te;
            a.dx = b.de; a.residual = 1;
            bw.chain(TB_EDGE, a, b.edge[k], be, m->v_edge[k], false);
            bw.wgrad(b.dzl(1), H, H, t.e[k], H, H, nullptr, e, bw.g(be), 3 * H, m->ce * H, bw.g(be + 1));
            bw.ij_grads(t.csr, t.h[k], be, n);
        }
    }
    // ---- encoders
    {
        TrainBwdArgs a{};
        a.rows = (int)n; a.dY = b.dh; a.Gi = b.Gi; a.Gj = b.Gj; a.tape = t.enc.en;
        a.dx_in = d_nodes; a.k1 = m->d.node_dim;
        const int bn = m->mlp[1].base;
        bw.chain(TB_ENC, a, b.enc_node, bn, m->v_enc_node, true);   // as the node MLPs
        bw.wgrad(b.dznl(1), H, H, nodes, m->d.node_dim, m->d.node_dim, nullptr, n, bw.g(bn), m->d.node_dim, 0, bw.g(bn + 1));
    }
    if (e > 0) {
        TrainBwdArgs a{};
        a.rows = (int)e; a.dY = b.de; a.tape = t.enc.ee;
        a.dx_in = d_edge_attr; a.k1 = m->d.edge_dim; a.dxidx = c.eid;   // sorted row p came from the caller's row eid[p]: a permutation
        const int be = m->mlp[0].base;
        bw.chain(TB_ENC, a, b.enc_edge, be, m->v_enc_edge, false);
        bw.wgrad(b.dzl(1), H, H, edge_attr, m->d.edge_dim, m->d.edge_dim, c.eid, e, bw.g(be), m->d.edge_dim, 0, bw.g(be + 1));
    }
    return bw.finish();
}

int gm_epd_backward(const gm_model* m, const float* const* T, int n_tensors, const float* nodes, const float* edge_attr, int64_t n,
                    int64_t e, const float* grad_out, float* const* grads, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                    void* stream) {
    return epd_backward(m, T, n_tensors, nodes, edge_attr, n, e, grad_out, grads, nullptr, nullptr, tape, tape_bytes, ws, ws_bytes, stream,
                        __func__);
}

// carve_bwd lays every slot out with its optional parts, the encoders' transposed W_1 images among them: the same carve serves
size_t gm_train_backward_inputs_workspace_bytes(const gm_model_desc* desc, int64_t n, int64_t e) {
    if (!desc || n < 0 || e < 0) return 0;
    return carve_bwd(nullptr, desc, n, e).bytes;
}

int gm_epd_backward_inputs(const gm_model* m, const float* const* T, int n_tensors, const float* nodes, const float* edge_attr, int64_t n,
                           int64_t e, const float* grad_out, float* const* grads, float* d_nodes, float* d_edge_attr, void* tape,
                           size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
    return epd_backward(m, T, n_tensors, nodes, edge_attr, n, e, grad_out, grads, d_nodes, d_edge_attr, tape, tape_bytes, ws, ws_bytes,
                        stream, __func__);
}

int gm_epd_backward_inputs_only(const gm_model* m, const float* const* T, int n_tensors, const float* nodes, const float* edge_attr,
                                int64_t n, int64_t e, const float* grad_out, float* d_nodes, float* d_edge_attr, void* tape,
                                size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
    return epd_backward(m, T, n_tensors, nodes, edge_attr, n, e, grad_out, nullptr, d_nodes, d_edge_attr, tape, tape_bytes, ws, ws_bytes,
                        stream, __func__, true);
}


// ------------------------------------------------------------------------------------------
// standalone blocks under autograd (the torch_graphnet surface, call sites epd_gnn.py:88,101)
// ------------------------------------------------------------------------------------------
size_t gm_block_tape_bytes(const gm_model_desc* desc, int interaction_network, int64_t n, int64_t e) {
    if (!desc || n < 0 || e < 0) return 0;
    return interaction_network ? carve_in_tape(nullptr, desc->hidden_size, desc->num_layers, n, e).bytes : carve_gi_tape(nullptr, desc->hidden_size, desc->num_layers, n, e).bytes;
}

size_t gm_block_backward_workspace_bytes(const gm_model_desc* desc, int64_t n, int64_t e) {
    if (!desc || n < 0 || e < 0) return 0;
    return carve_block_bwd(nullptr, desc, n, e).bytes;
}

int gm_graph_independent_forward_train(const gm_model* m, const float* x, int64_t n, const float* edge_attr, int64_t e, float* h_out,
                                       float* e_out, void* tape, size_t tape_bytes, void* stream) {
    int rc = check_model(m, n, e, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(x && h_out && tape && (e == 0 || (edge_attr && e_out)), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    gm::DevGuard dev_guard(x ? (const void*)x : (const void*)edge_attr);
    hipStream_t s = (hipStream_t)stream;
    GiTape t = carve_gi_tape(tape, m->H, m->NL, n, e);
    rc = ready_to_launch(m, tape_bytes, t.bytes, 0, 0, s, __func__);
    if (rc != GM_OK) return rc;
    return fwd_encoders(m, n, e, x, edge_attr, nullptr, t.enc, h_out, e_out, nullptr, s);
}

int gm_graph_independent_backward(const gm_model* m, const float* const* T, int n_tensors, const float* x, const float* edge_attr, int64_t n,
                                  int64_t e, const float* dh, const float* de, float* dx, float* dedge_attr, float* const* grads,
                                  void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_model(m, n, e, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(T && grads && x && dh && tape && ws && (e == 0 || (edge_attr && de)), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    const int H = m->H, NL = m->NL;
    const MlpSpec &ee = m->mlp[0], &en = m->mlp[1];
    rc = check_tensors(m, T, grads, n_tensors, ee.base, en.end, __func__);
    if (rc != GM_OK) return rc;
    gm::DevGuard dev_guard(x ? (const void*)x : (const void*)edge_attr);
    hipStream_t s = (hipStream_t)stream;
    GiTape t = carve_gi_tape(tape, H, NL, n, e);
    BwdWs b = carve_block_bwd(ws, &m->d, n, e);
    rc = ready_to_launch(m, tape_bytes, t.bytes, ws_bytes, b.bytes, s, __func__);
    if (rc != GM_OK) return rc;
    BwdRun bw(m, grads, b, s);
    PackBwd pk{m->d, b, m, T, s};
    pk.enc_node(false, dx != nullptr);
    pk.enc_edge(dedge_attr != nullptr);
    rc = pk.flush();
    if (rc != GM_OK) return rc;
    auto run = [&](int base, const TapePtr& tp, int64_t rows, const float* dY, size_t voff, const Slot& sl, const float* X, int k1, float* dxin) {
        if (rows <= 0) return;
        TrainBwdArgs a{};
        a.rows = (int)rows; a.dY = dY; a.tape = tp; a.dx_in = dxin; a.k1 = k1;
        bw.chain(TB_ENC, a, sl, base, voff, false);
        bw.wgrad(b.dzl(1), H, H, X, k1, k1, nullptr, rows, bw.g(base), k1, 0, bw.g(base + 1));
    };
    run(en.base, t.enc.en, n, dh, m->v_enc_node, b.enc_node, x, m->d.node_dim, dx);
    run(ee.base, t.enc.ee, e, de, m->v_enc_edge, b.enc_edge, edge_attr, m->d.edge_dim, dedge_attr);
    return bw.finish();
}

int gm_interaction_network_forward_train(const gm_model* m, int k, const float* h, int64_t n, const float* e_in, const int64_t* edge_index,
                                         int64_t e, float* h_out, float* e_out, void* tape, size_t tape_bytes, void* stream) {
    int rc = check_model(m, n, e, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(k >= 0 && k < m->M, GM_ERR_INVALID_ARGUMENT, "%s: block %d out of range", __func__, k);
    GM_REQUIRE(h && h_out && tape && (e == 0 || (e_in && e_out && edge_index)), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", __func__);
    gm::DevGuard dev_guard(h);
    hipStream_t s = (hipStream_t)stream;
    InTape t = carve_in_tape(tape, m->H, m->NL, n, e);
    rc = ready_to_launch(m, tape_bytes, t.bytes, 0, 0, s, __func__);
    if (rc != GM_OK) return rc;
    rc = build_csr(t.csr, edge_index, n, e, m->d.flow, s);
    if (rc != GM_OK) return rc;
    {
        TrainFwdArgs pa{};   // P = [h W_i^T + b1 | h W_j^T] of this block's edge MLP
        pa.rows = (int)n; pa.x_in = h; pa.bias = m->vec + m->v_edge[k]; pa.out = t.P; pa.nl = m->NL; set_stream(m, pa, m->t_proj[k], false);
        rc = launch_train_fwd(m->H, TK_PROJ, pa, s);
        if (rc != GM_OK) return rc;
    }
    return fwd_step(m, k, t.csr.dst, n, e, h, e_in, t.P, t.st, h_out, e_out, t.csr.dst.eid, 0, false, s);
}

int gm_interaction_network_backward(const gm_model* m, int k, const float* const* T, int n_tensors, const float* h, const float* e_in,
                                    int64_t n, int64_t e, const float* dh_out, const float* de_out, float* dh_in, float* de_in,
                                    float* const* grads, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_model(m, n, e, __func__);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(k >= 0 && k < m->M, GM_ERR_INVALID_ARGUMENT, "%s: block %d out of range", __func__, k);
    GM_REQUIRE(T && grads && h && dh_out && dh_in && tape && ws && (e == 0 || (e_in && de_out && de_in)), GM_ERR_INVALID_ARGUMENT,
               "%s: null pointer", __func__);
    const int H = m->H, be = m->edge_mlp(k).base, bn = m->node_mlp(k).base;
    rc = check_tensors(m, T, grads, n_tensors, be, m->node_mlp(k).end, __func__);
    if (rc != GM_OK) return rc;
    gm::DevGuard dev_guard(h);
    hipStream_t s = (hipStream_t)stream;
    InTape t = carve_in_tape(tape, H, m->NL, n, e);
    BwdWs b = carve_block_bwd(ws, &m->d, n, e);
    rc = ready_to_launch(m, tape_bytes, t.bytes, ws_bytes, b.bytes, s, __func__);
    if (rc != GM_OK) return rc;
    BwdRun bw(m, grads, b, s);
    const CsrWs& c = t.csr.dst;
    PackBwd pk{m->d, b, m, T, s};
    pk.node(k, 0);
    pk.edge(k, 0);
    pk.proj(k);
    rc = pk.flush();
    if (rc != GM_OK) return rc;
    // node MLP: dY = dh_out (no residual inside the block); dx = W_h^T dz1 -> b.dh, dagg -> b.dagg
    {
        TrainBwdArgs a{};
        a.rows = (int)n; a.dY = dh_out; a.tape = t.st.tn; a.dx = b.dh; a.dagg_out = b.dagg;
        bw.chain(TB_NODE, a, b.node[0], bn, m->v_node[k], false);
        bw.wgrad(b.dzl(1), H, H, h, H, H, nullptr, n, bw.g(bn), 2 * H, m->ch * H, bw.g(bn + 1));
        bw.wgrad(b.dzl(1), H, H, t.st.agg, H, H, nullptr, n, bw.g(bn), 2 * H, m->ca * H, nullptr);
    }
    if (e > 0) {
        TrainBwdArgs a{};
        a.rows = (int)e; a.dY = de_out; a.dyidx = c.eid; a.dagg = b.dagg; a.dst = c.dst; a.tape = t.st.te;
        a.dx = de_in; a.dxidx = c.eid;
        bw.chain(TB_EDGE, a, b.edge[0], be, m->v_edge[k], false);
        bw.wgrad(b.dzl(1), H, H, e_in, H, H, c.eid, e, bw.g(be), 3 * H, m->ce * H, bw.g(be + 1));
    }
    bw.ij_grads(t.csr, h, be, n);
    // dh_in = W_h^T dz1 (node MLP) + W_i^T G_i + W_j^T G_j (edge MLP, factorised layer 1)
    TrainBwdArgs a{};
    a.rows = (int)n; a.dY = b.dh; a.Gi = b.Gi; a.Gj = b.Gj; a.dx = dh_in;
    bw.launch(TB_PROJ, a, b.enc_node, true);
    return bw.rc;
}

}  // extern "C"
