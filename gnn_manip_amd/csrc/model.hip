// Model handle (packed weight image), forward orchestration and the device-resident rollout step.
// Host-side C++ only: the kernels it launches live in the other .hip files.
#include <algorithm>
#include <vector>
#include "common.h"
#include "mlp.h"
#include "model.h"
#include "train.h"
#include "hedge.h"
#include "hmlp.h"

using namespace gm;

std::vector<MlpSpec> gm::model_mlps(const gm_model_desc& d) {
    const int H = d.hidden_size, NL = d.num_layers;
    std::vector<MlpSpec> mlp;
    auto add = [&](int in, int out, bool normed) {
        const int base = mlp.empty() ? 0 : mlp.back().end;
        mlp.push_back({base, base + 2 * (NL + 1) + (normed ? 2 : 0), in, out, normed});
    };
    add(d.edge_dim, H, true);
    add(d.node_dim, H, true);
    for (int k = 0; k < d.m_steps; ++k) {
        add(3 * H, H, true);
        add(2 * H, H, true);
    }
    add(H, d.out_dim, false);
    return mlp;
}

namespace {

int check_desc(const gm_model_desc* d, const char* who) {
    GM_REQUIRE(d != nullptr, GM_ERR_INVALID_ARGUMENT, "%s: null model descriptor", who);
    // the reference's two ctor asserts (epd_gnn.py:26-27)
    GM_REQUIRE(d->num_layers >= 2, GM_ERR_INVALID_ARGUMENT, "The number of layers num_layers must be at least 2");
    GM_REQUIRE(d->m_steps >= 1, GM_ERR_INVALID_ARGUMENT, "The number of m_steps message pasting steps must be at least 1");
    GM_REQUIRE(hm_padded_hidden(d->hidden_size) > 0, GM_ERR_UNSUPPORTED,
               "%s: hidden_size=%d: supported are 1 .. 256 (run zero-padded at width 64, 128 or 256)", who, d->hidden_size);
    GM_REQUIRE(d->num_layers <= 16, GM_ERR_UNSUPPORTED, "%s: num_layers=%d: at most 16", who, d->num_layers);
    GM_REQUIRE(d->edge_dim >= 1 && d->edge_dim <= 8, GM_ERR_UNSUPPORTED, "%s: edge_dim=%d unsupported (1..8)", who, d->edge_dim);
    GM_REQUIRE(d->node_dim >= 1 && d->node_dim <= 32, GM_ERR_UNSUPPORTED, "%s: node_dim=%d unsupported (1..32)", who, d->node_dim);
    GM_REQUIRE(d->out_dim >= 1 && d->out_dim <= 4, GM_ERR_UNSUPPORTED, "%s: out_dim=%d unsupported (1..4)", who, d->out_dim);
    GM_REQUIRE(d->ln_eps > 0.f, GM_ERR_INVALID_ARGUMENT, "%s: ln_eps must be > 0", who);
    GM_REQUIRE(d->flow == 0 || d->flow == 1, GM_ERR_INVALID_ARGUMENT, "%s: flow must be 0 (aggregate at edge_index[1]) or 1", who);
    GM_REQUIRE(d->node_agg_first == 0 || d->node_agg_first == 1, GM_ERR_INVALID_ARGUMENT, "%s: node_agg_first must be 0 or 1", who);
    if (d->col_i || d->col_j || d->col_e) {
        const int a = d->col_i, b = d->col_j, c = d->col_e;
        GM_REQUIRE(a >= 0 && a < 3 && b >= 0 && b < 3 && c >= 0 && c < 3 && a != b && a != c && b != c, GM_ERR_INVALID_ARGUMENT,
                   "%s: col_i, col_j, col_e must be a permutation of 0, 1, 2", who);
    }
    return GM_OK;
}

struct FwdWs {
    float *h, *P, *agg, *side, *e;
    float* Q;   // [N][H]: the h half of the next node MLP's first Linear (systolic node path)
    size_t bytes;
};
// cap_e: rows of the latent edge array held here (0: the caller's); cap_side: edge capacity the side buffer of the
// scatter-add's head partials is sized for (hedge.h)
FwdWs carve_fwd(void* ws, int H, int64_t n, int64_t cap_e, int64_t cap_side) {
    FwdWs f;
    Carver c(ws);
    f.h = c.take<float>((size_t)n * H);
    f.P = c.take<float>((size_t)n * 2 * H);
    f.agg = c.take<float>((size_t)n * H);
    f.side = c.take<float>(edge_groups_max(n, cap_side) * H);
    f.e = c.take<float>((size_t)(cap_e > 0 ? cap_e + kEdgePadRows : 0) * H);   // + zero rows behind the list (hedge.h)
    f.Q = c.take<float>((size_t)n * H);
    f.bytes = c.used();
    return f;
}

struct WeightSizes { size_t raw, vec, t3, hm, h3; };   // floats of each buffer plan_weights lays out

// The one walk over the model's weights: where each raw tensor goes, then the layout of every image, the jobs that pack it from
// the raw copy and the offsets the forward and training code read.  Called with the buffers still null it only sizes them;
// gm_model_create calls it again once they are allocated, and every load launches the jobs it planned.
WeightSizes plan_weights(gm_model* m) {
    // H: the width the kernels run at (hidden_size zero-padded to 64 / 128 / 256: strides, image sizes); Hv: the model's hidden_size
    const int H = m->Hp, Hv = m->H, NL = m->NL, M = m->M;
    const MlpSpec &enc_edge = m->mlp[0], &enc_node = m->mlp[1], &dec = m->mlp.back();
    WeightSizes z{};
    for (auto* v : {&m->t_proj, &m->t_edge, &m->t_node}) v->assign(M, TStream{});
    for (auto* v : {&m->v_edge, &m->v_node, &m->hm_edge, &m->hm_node, &m->hm_node_tail,
                    &m->hm_node_q, &m->h3_edge, &m->h3_node})
        v->assign(M, 0);
    std::vector<const float*> T;   // the raw copy of each tensor
    m->raw_jobs.clear();
    for (const MlpSpec& p : m->mlp) {
        auto put = [&](int count) {
            m->raw_jobs.push_back({nullptr, z.raw, count, 0});
            T.push_back(m->raw + z.raw);
            z.raw += ((size_t)count + 3) & ~(size_t)3;
        };
        for (int l = 0; l <= NL; ++l) {
            const int out = l == NL ? p.out : Hv, in = l == 0 ? p.in : Hv;
            put(out * in);
            put(out);
        }
        if (p.normed) { put(Hv); put(Hv); }
    }

    // biases + LayerNorm vectors (training, LayerNorm of every kernel), zero on the padded features, which therefore stay exactly zero
    m->vec_jobs.clear();
    auto vecs = [&](const MlpSpec& p) {
        const size_t start = z.vec;
        auto put = [&](int ti, int count, int width, int center = 0) {
            m->vec_jobs.push_back({T[ti], z.vec, count, count < width ? width : 0, center});
            z.vec += width;
        };
        // (the bias in front of a LayerNorm is kept centred, like that Linear's training images: PackTJob::center)
        for (int l = 0; l <= NL; ++l) put(p.base + 2 * l + 1, l == NL ? p.out : Hv, p.normed || l < NL ? H : 32, p.normed && l == NL);
        if (p.normed) { put(p.base + 2 * NL + 2, Hv, H); put(p.base + 2 * NL + 3, Hv, H); }
        return start;
    };
    m->v_enc_edge = vecs(enc_edge);
    m->v_enc_node = vecs(enc_node);
    for (int k = 0; k < M; ++k) {
        m->v_edge[k] = vecs(m->edge_mlp(k));
        m->v_node[k] = vecs(m->node_mlp(k));
    }
    m->v_dec = vecs(dec);

    // bf16 x 3 streams of the training kernels, for the widths they exist for: the forward Linears in the order the chains consume them
    m->t_jobs.clear();
    if (Hv == 64 || Hv == 128 || Hv == 256) {
        TStream* cur = nullptr;   // the stream being laid out: begin() opens it, every Linear packed from there on counts into it
        auto begin = [&](TStream& t) { t = {z.t3, 0, 0}; cur = &t; };
        auto t3 = [&](int ti, int out_rows, int ld, int col0, int k, int center = 0) {
            m->t_jobs.push_back({T[ti], k, ld, col0, out_rows, 1, center, z.t3});
            cur->stages += layer_stages_b3(k, out_rows);
            z.t3 += (size_t)layer_stages_b3(k, out_rows) * kStageFloatsB3;
        };
        auto hidden3 = [&](const MlpSpec& p) { for (int l = 1; l <= NL; ++l) t3(p.base + 2 * l, l == NL ? p.out : H, H, 0, H, p.normed && l == NL); };
        auto whole3 = [&](const MlpSpec& p) { t3(p.base, H, p.in, 0, p.in); hidden3(p); };   // Linear 0 in one block: encoders, decoder
        begin(m->t_enc_edge);
        whole3(enc_edge);
        begin(m->t_enc_node);
        whole3(enc_node);
        for (int k = 0; k < M; ++k) {
            const MlpSpec &e = m->edge_mlp(k), &n = m->node_mlp(k);
            TStream& before = k == 0 ? m->t_enc_node : m->t_node[k - 1];   // ends where [W_i | W_j] begin: its projection tail runs on into them
            begin(m->t_proj[k]);
            t3(e.base, H, 3 * H, m->ci * H, H);   // W_i
            t3(e.base, H, 3 * H, m->cj * H, H);   // W_j
            before.stages_tail = before.stages + m->t_proj[k].stages;
            begin(m->t_edge[k]);
            t3(e.base, H, 3 * H, m->ce * H, H);   // W_e
            hidden3(e);
            begin(m->t_node[k]);
            t3(n.base, H, 2 * H, m->ch * H, H);   // W_h
            t3(n.base, H, 2 * H, m->ca * H, H);   // W_agg
            hidden3(n);
        }
        begin(m->t_dec);
        whole3(dec);
    }

    // fp16 hi / lo images of every Linear (hmlp.h); consecutive Linears of an MLP form a scale chain
    std::vector<PackHmJob>& jobs = m->hm_jobs;
    jobs.clear();
    int prev = -1;   // job whose output feeds the next lin() (-1: the next one heads a chain)
    float head_rms = 1.f;
    auto lin = [&](int ti, int ld, int col0a, int col0b, int out_valid, int out_pad, int out_seg, int k_valid, int k_pad, int k_seg,
                   bool with_bias, int bias_n, int gain_col0 = 0, int gain_cols = 0) {
        PackHmJob j{};
        j.W = T[ti]; j.ld = ld; j.bias = with_bias ? T[ti + 1] : nullptr; j.bias_n = bias_n;
        j.out_valid = out_valid; j.out_pad = out_pad; j.out_seg = out_seg;
        j.k_valid = k_valid; j.k_pad = k_pad; j.k_seg = k_seg; j.col0[0] = col0a; j.col0[1] = col0b;
        j.pred = prev; j.in_rms = head_rms; j.gain_col0 = gain_col0; j.gain_cols = gain_cols;
        j.dst = m->packed_hm + z.hm;
        z.hm += hm_lin_floats(out_pad, k_pad);
        prev = (int)jobs.size();
        jobs.push_back(j);
    };
    auto head = [&](float rms) { prev = -1; head_rms = rms; };
    auto hh = [&](int ti) { lin(ti, Hv, 0, 0, Hv, H, H, Hv, H, H, true, Hv); };
    // Linears 1 .. NL of an MLP that ends in a LayerNorm (the decoder's are queued one by one): the last one is packed centred
    auto hidden = [&](const MlpSpec& p) {
        for (int l = 1; l <= NL; ++l) hh(p.base + 2 * l);
        jobs.back().center = 1;
    };
    auto proj = [&](int k) {   // P = h [W_i | W_j]^T + [b1 | 0] of processor step k: a chain of its own (input h)
        head(1.f);
        lin(m->edge_mlp(k).base, 3 * Hv, m->ci * Hv, m->cj * Hv, Hv, 2 * H, H, Hv, H, H, true, Hv);
    };
    m->hm_enc_edge = z.hm;
    head(kHmRawInputRms);   // raw edge features: per-row power-of-two scale in the kernel
    lin(enc_edge.base, enc_edge.in, 0, 0, Hv, H, H, enc_edge.in, 16, 16, true, Hv);
    hidden(enc_edge);
    m->hm_enc_node = z.hm;
    head(kHmRawInputRms);
    lin(enc_node.base, enc_node.in, 0, 0, Hv, H, H, enc_node.in, 32, 32, true, Hv);
    hidden(enc_node);
    m->hm_enc_node_tail = z.hm;
    proj(0);
    for (int k = 0; k < M; ++k) {
        const MlpSpec &e = m->edge_mlp(k), &n = m->node_mlp(k);
        m->hm_edge[k] = z.hm;
        head(1.f);
        // the e block; b1 lives in P_i.  Its pre-activation also takes h_i and h_j: the gain is that of the whole [H x 3H] Linear
        lin(e.base, 3 * Hv, m->ce * Hv, 0, Hv, H, H, Hv, H, H, false, 0, 0, 3 * Hv);
        hidden(e);
        m->hm_node[k] = z.hm;
        head(1.f);
        lin(n.base, 2 * Hv, m->ch * Hv, m->ca * Hv, Hv, H, H, Hv, 2 * H, H, true, Hv);
        hidden(n);
        m->hm_node_tail[k] = z.hm;
        if (k + 1 < M) proj(k + 1);
        else {
            head(1.f);
            for (int l = 0; l < NL; ++l) hh(dec.base + 2 * l);
            lin(dec.base + 2 * NL, Hv, 0, 0, dec.out, 32, 32, Hv, H, H, true, dec.out);
        }
    }
    for (int k = 0; k < M; ++k) {   // Q = h W_h^T + b1 of node step k (systolic node path): a chain of its own, input h
        m->hm_node_q[k] = z.hm;
        head(1.f);
        lin(m->node_mlp(k).base, 2 * Hv, m->ch * Hv, 0, Hv, H, H, Hv, H, H, true, Hv);
    }

    // fp16 hi / lo images of the systolic kernels (hidden 128, num_layers 2): the M processor edge MLPs, the edge encoder, then
    // the node MLPs (the agg block of Linear 1, whose h block is Q; Linear 2; Linear 3)
    m->h3_jobs.clear();
    if (Hv == 128 && NL == 2) {
        auto h3 = [&](size_t& slot, const MlpSpec& p, int W1_col0, int W1_ld, int enc_k1) {
            const float* const* W = &T[p.base];   // W_0, b_0, W_1, b_1, W_2, b_2, gamma, beta
            PackH3Job j{};
            j.W1 = W[0]; j.b1 = W[1]; j.W2 = W[2]; j.b2 = W[3]; j.W3 = W[4]; j.b3 = W[5]; j.gamma = W[6]; j.beta = W[7];
            j.W1_col0 = W1_col0; j.W1_ld = W1_ld; j.enc_k1 = enc_k1; j.dst = m->packed_h3 + z.h3;
            m->h3_jobs.push_back(j);
            slot = z.h3;
            z.h3 += h3_image_floats();
        };
        for (int k = 0; k < M; ++k) h3(m->h3_edge[k], m->edge_mlp(k), m->ce * H, 0, 0);
        h3(m->h3_enc, enc_edge, 0, 0, enc_edge.in);
        for (int k = 0; k < M; ++k) h3(m->h3_node[k], m->node_mlp(k), m->ca * H, 2 * H, 0);
    }
    return z;
}

// Runs the jobs a batch (Batch::job) at a time, in order
template <class Batch, class Job>
int launch_batches(const std::vector<Job>& jobs, int (*launch)(const Batch&, float*, hipStream_t), float* base, hipStream_t s) {
    Batch b;
    const size_t cap = sizeof(b.job) / sizeof(b.job[0]);
    for (size_t i = 0; i < jobs.size(); i += cap) {
        b.n = (int)std::min(cap, jobs.size() - i);
        std::copy_n(jobs.begin() + i, b.n, b.job);
        const int rc = launch(b, base, s);
        if (rc != GM_OK) return rc;
    }
    return GM_OK;
}

// vec and the training streams: every load packs them from the raw copy
int pack_common(const gm_model* m, hipStream_t s) {
    int rc = launch_batches(m->vec_jobs, launch_vec_batch, m->vec, s);
    if (rc == GM_OK && m->packed_t3) rc = launch_batches(m->t_jobs, launch_pack_b3_batch, m->packed_t3, s);
    return rc;
}

// packed_hm and packed_h3: the first inference call after a load packs them (ensure_inference_images)
int pack_inference(const gm_model* m, hipStream_t s) {
    int rc = pack_hm(m->hm_jobs.data(), (int)m->hm_jobs.size(), m->hm_jobs_dev, m->hm_stats, s);
    if (rc != GM_OK || !m->packed_h3) return rc;
    const int n_edge = m->M + 1;   // the edge images (the steps', the encoder's), then the node images
    rc = pack_h3(m->h3_jobs.data(), n_edge, s);
    if (rc == GM_OK) rc = pack_h3(m->h3_jobs.data() + n_edge, m->M, s);
    return rc;
}

// `ready` = everything queued for the model's images so far, on stream s (model.h)
int mark_ready(gm_model* m, hipStream_t s) {
    if (!m->ready) GM_HIP_CHECK(hipEventCreateWithFlags(&m->ready, hipEventDisableTiming));
    GM_HIP_CHECK(hipEventRecord(m->ready, s));
    m->ready_stream = s;
    return GM_OK;
}

// The raw tensors are first copied into the model's own device buffer (host- or device-resident callers alike), then the cheap
// images are packed from that copy; the inference images follow on first use (ensure_inference_images).
int load_weights(gm_model* m, const float* const* T, int nt, bool on_device, hipStream_t s) {
    GM_REQUIRE(nt == (int)m->raw_jobs.size(), GM_ERR_INVALID_ARGUMENT, "model: expected %zu tensors, got %d", m->raw_jobs.size(), nt);
    for (int i = 0; i < nt; ++i) GM_REQUIRE(T[i] != nullptr, GM_ERR_INVALID_ARGUMENT, "model: tensor %d is null", i);
    std::lock_guard<std::mutex> guard(m->lazy_mu);
    int rc = GM_OK;
    if (on_device) {
        std::vector<VecJob> jobs = m->raw_jobs;
        for (int i = 0; i < nt; ++i) jobs[(size_t)i].src = T[i];
        rc = launch_batches(jobs, launch_vec_batch, m->raw, s);
    } else {
        for (int i = 0; i < nt && rc == GM_OK; ++i) {
            const VecJob& j = m->raw_jobs[(size_t)i];
            if (hipMemcpyAsync(m->raw + j.dst_off, T[i], (size_t)j.count * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) {
                gm::set_error("model: copy of tensor %d to the device failed", i);
                rc = GM_ERR_HIP;
            }
        }
        if (rc == GM_OK) (void)hipStreamSynchronize(s);   // the caller's host buffers may go away when this returns
    }
    if (rc != GM_OK) return rc;
    m->infer_stale = true;
    rc = pack_common(m, s);
    if (rc == GM_OK) rc = mark_ready(m, s);
    return rc;
}

}  // namespace

int ensure_inference_images(const gm_model* cm, hipStream_t s) {
    gm_model* m = const_cast<gm_model*>(cm);
    std::lock_guard<std::mutex> guard(m->lazy_mu);
    // the copy / common pack (and an earlier inference pack) may have been queued on another stream: this one waits for them
    if (m->ready && s != m->ready_stream) GM_HIP_CHECK(hipStreamWaitEvent(s, m->ready, 0));
    if (!m->infer_stale) return GM_OK;
    int rc = pack_inference(m, s);
    if (rc == GM_OK) rc = mark_ready(m, s);   // the images are complete once THIS lands: other streams wait for it
    if (rc == GM_OK) m->infer_stale = false;
    return rc;
}

int weights_changed_in_place(gm_model* m, hipStream_t s) {
    std::lock_guard<std::mutex> guard(m->lazy_mu);
    m->infer_stale = true;
    int rc = pack_common(m, s);
    if (rc == GM_OK) rc = mark_ready(m, s);
    return rc;
}

int weights_ready_on(const gm_model* cm, hipStream_t s) {
    gm_model* m = const_cast<gm_model*>(cm);
    std::lock_guard<std::mutex> guard(m->lazy_mu);
    if (m->ready && s != m->ready_stream) GM_HIP_CHECK(hipStreamWaitEvent(s, m->ready, 0));
    return GM_OK;
}

extern "C" {

int gm_padded_hidden_size(int hidden_size) { return hm_padded_hidden(hidden_size); }

int gm_model_num_tensors(const gm_model_desc* d) {
    if (!d) return 0;
    return gm::model_mlps(*d).back().end;
}

int gm_model_create(const gm_model_desc* desc, const float* const* tensors, int n_tensors, int on_device, void* stream,
                    gm_model** out) {
    gm::DevGuard dev_guard((on_device && tensors) ? tensors[0] : nullptr);
    GM_REQUIRE(out && tensors, GM_ERR_INVALID_ARGUMENT, "gm_model_create: null pointer");
    int rc = check_desc(desc, "gm_model_create");
    if (rc != GM_OK) return rc;
    gm_model* m = new gm_model();
    m->d = *desc;
    m->H = desc->hidden_size;
    m->Hp = hm_padded_hidden(desc->hidden_size);   // width the kernels run at (buffers, images); m->H: the model's
    m->NL = desc->num_layers; m->M = desc->m_steps;
    if (desc->col_i || desc->col_j || desc->col_e) { m->ci = desc->col_i; m->cj = desc->col_j; m->ce = desc->col_e; }
    if (desc->node_agg_first) { m->ch = 1; m->ca = 0; }
    m->mlp = model_mlps(*desc);
    const WeightSizes z = plan_weights(m);
    auto alloc = [](auto** p, size_t count) { return count == 0 || hipMalloc(p, count * sizeof(**p)) == hipSuccess; };
    if (!alloc(&m->raw, z.raw) || !alloc(&m->vec, z.vec) || !alloc(&m->packed_t3, z.t3) || !alloc(&m->packed_hm, z.hm) ||
        !alloc(&m->packed_h3, z.h3) || !alloc(&m->hm_jobs_dev, m->hm_jobs.size()) || !alloc(&m->hm_stats, 4 * m->hm_jobs.size())) {
        gm::set_error("gm_model_create: hipMalloc failed");
        gm_model_destroy(m);
        return GM_ERR_HIP;
    }
    plan_weights(m);   // now with the buffers: the job lists point into them
    rc = load_weights(m, tensors, n_tensors, on_device != 0, (hipStream_t)stream);
    if (rc != GM_OK) {
        gm_model_destroy(m);
        return rc;
    }
    *out = m;
    return GM_OK;
}

int gm_model_update(gm_model* m, const float* const* tensors, int n_tensors, int on_device, void* stream) {
    gm::DevGuard dev_guard((on_device && tensors) ? tensors[0] : nullptr);
    GM_REQUIRE(m && tensors, GM_ERR_INVALID_ARGUMENT, "gm_model_update: null pointer");
    return load_weights(m, tensors, n_tensors, on_device != 0, (hipStream_t)stream);
}

void gm_model_destroy(gm_model* m) {
    if (!m) return;
    for (void* p : std::initializer_list<void*>{m->raw, m->vec, m->packed_t3, m->packed_hm, m->packed_h3, m->hm_jobs_dev, m->hm_stats})
        (void)hipFree(p);
    if (m->ready) (void)hipEventDestroy(m->ready);
    delete m->prof;
    delete m;
}

size_t gm_forward_workspace_bytes(const gm_model_desc* desc, int64_t n, int64_t cap) {
    if (!desc || n < 0 || cap < 0) return 0;
    return carve_fwd(nullptr, hm_padded_hidden(desc->hidden_size), n, cap, cap).bytes;
}

size_t gm_block_workspace_bytes(const gm_model_desc* desc, int64_t n, int64_t cap) {
    if (!desc || n < 0 || cap < 0) return 0;
    return carve_fwd(nullptr, hm_padded_hidden(desc->hidden_size), n, 0, cap).bytes;
}

}  // extern "C"

namespace {

// Which form each MLP of one forward takes: decided once per forward, followed by every launch of it.  The systolic kernels
// (hedge.h) exist for hidden 128 / num_layers 2 (packed_h3); the streamed ones (hmlp.h) take every other launch.
struct Route {
    bool sys_enc;    // edge encoder: sys_enc_kernel, which zeroes the pad rows behind the edge list itself (else hm_edge_kernel)
    bool sys_edge;   // processor edge: sys_edge_kernel, which reads P pre-scaled by its image's T1 (else hm_edge_kernel)
    bool sys_node;   // processor node: sys_node_kernel + sys_proj_kernel, then the streamed decoder (else hm_node_kernel and its tail)
};
enum class Entry { Fused, Independent, Block };   // gm_epd_forward / gm_rollout_step, gm_graph_independent_forward, gm_interaction_network_forward
// attr_sorted: the raw edge features are in sorted order (no eid gather); n_per_graph: nodes of ONE graph of a block-diagonal batch, or n
Route route_forward(const gm_model* m, Entry entry, int64_t n, int64_t n_per_graph, int64_t cap, bool attr_sorted) {
    // the systolic kernels need rows in sorted order behind a CSR header's device-side edge count: the fused forward's (the
    // independent forward has no header, a block forward reads its edge rows through eid)
    const bool sys = entry == Entry::Fused && m->packed_h3 && m->edge_kernel != EK_HM;
    Route r;
    r.sys_enc = sys && attr_sorted && m->d.edge_dim == 4;
    r.sys_edge = sys && cap > 0 && edge_sys_fits(n, cap);   // larger graphs than its 32-bit offsets cover take the streamed kernel
    // by the size of ONE graph, not of the batch (batch invariance: hedge.h, kSysNodeMinNodes)
    r.sys_node = r.sys_edge && (m->edge_kernel == EK_SYS_ALL || (n_per_graph > 0 ? n_per_graph : n) >= kSysNodeMinNodes);
    return r;
}

// LayerNorm of the MLP whose vec block starts at voff ([bias_0 .. bias_NL, gamma, beta])
template <class A>
void set_ln(const gm_model* m, A& a, size_t voff) {
    const float* v = m->vec + voff;
    a.ln_g = v + (size_t)(m->NL + 1) * m->Hp; a.ln_b = v + (size_t)(m->NL + 2) * m->Hp; a.eps = m->d.ln_eps;
}

EdgeArgs enc_edge_args(const gm_model* m, const float* edge_attr, const int* eid, const CsrHeader* hdr, int e_host, float* e_out) {
    EdgeArgs a{};
    a.hdr = hdr; a.n_edges_host = e_host; a.eid = eid;
    a.e_in = edge_attr; a.e_out = e_out; a.k1 = m->d.edge_dim;
    a.wstream_hm = m->packed_hm + m->hm_enc_edge;
    a.wstream_h3 = m->packed_h3 ? m->packed_h3 + m->h3_enc : nullptr;
    a.prof = m->prof;
    a.precision = m->precision;
    set_ln(m, a, m->v_enc_edge);
    a.h_valid = m->H;
    return a;
}
EdgeArgs proc_edge_args(const gm_model* m, int k, const CsrWs& c, int64_t n, const int* eid, const float* P, const float* e_in,
                        float* e_out, float* agg, float* side, int residual) {
    EdgeArgs a{};
    a.hdr = c.hdr; a.dst = c.dst; a.src = c.src; a.eid = eid; a.eid_out = eid;
    a.P = P; a.e_in = e_in; a.e_out = e_out; a.agg = agg; a.side = side; a.residual = residual;
    a.wstream_hm = m->packed_hm + m->hm_edge[k];
    a.wstream_h3 = m->packed_h3 ? m->packed_h3 + m->h3_edge[k] : nullptr;
    a.edge_blocks = c.blocks;
    a.n_nodes_tab = n;
    a.prof = m->prof;
    a.precision = m->precision;
    set_ln(m, a, m->v_edge[k]);
    a.h_valid = m->H;
    return a;
}

// The streamed node kernel (hmlp.h, launch_node_hm): mode 0 the encoder, mode 1 a processor step, mode 2 a tail alone.
HmNodeArgs node_args(const gm_model* m, int64_t n, const float* x_in, int* flags) {
    HmNodeArgs a{};
    a.n_nodes = (int)n; a.x_in = x_in; a.nl = m->NL; a.h_valid = m->H; a.flags = flags; a.prof = m->prof;
    a.precision = m->precision;
    return a;
}
HmNodeArgs enc_node_args(const gm_model* m, int64_t n, const float* x, float* h_out, int* flags) {
    HmNodeArgs a = node_args(m, n, x, flags);
    a.k1 = m->d.node_dim; a.h_out = h_out;
    a.w = m->packed_hm + m->hm_enc_node;
    set_ln(m, a, m->v_enc_node);
    return a;
}
// node MLP of step k on [h | agg], agg completed by the head partials of the edge kernel's scatter-add (hedge.h) in the same launch
HmNodeArgs proc_node_args(const gm_model* m, int k, const CsrWs& c, int64_t n, int64_t cap, const float* h, const float* agg,
                          const float* side, float* h_out, int residual) {
    HmNodeArgs a = node_args(m, n, h, &c.hdr->error_flags);
    a.agg = agg; a.h_out = h_out; a.residual = residual;
    a.w = m->packed_hm + m->hm_node[k];
    set_ln(m, a, m->v_node[k]);
    const EdgeBlocks t = carve_edge_blocks(c.blocks, n, cap);
    a.stitch = t.stitch; a.head = t.head; a.side = side; a.tab = t.hdr;
    return a;
}
// the tail behind a node MLP: the projection P of edge step `next` (< M), or the decoder (next == M).  p_scaled: the systolic edge
// kernel takes that step, and P leaves at its weight scale
void set_tail(const gm_model* m, HmNodeArgs& a, int next, float* P, float* out, bool p_scaled) {
    a.w_tail = m->packed_hm + (next == 0 ? m->hm_enc_node_tail : m->hm_node_tail[next - 1]);
    if (next < m->M) {
        a.tail = 1;
        a.P_out = P;
        a.p_scale = p_scaled ? edge_sys_p_scale(m->packed_h3 + m->h3_edge[next]) : nullptr;
    } else {
        a.tail = 2;
        a.dec_out = out;
        a.out_dim = m->d.out_dim;
    }
}
HmNodeArgs tail_args(const gm_model* m, int next, int64_t n, const float* h, float* P, float* out, int* flags) {
    HmNodeArgs a = node_args(m, n, h, flags);
    set_tail(m, a, next, P, out, false);
    return a;
}

// agg_cleared: the caller's first launch has zeroed agg (the rollout step's StepClear); n_per_graph: nodes of ONE graph of a
// block-diagonal batch of equal-sized graphs (the kernel choice must not depend on how many graphs share the call), or n
int epd_forward_impl(const gm_model* m, const float* nodes, int64_t n, const float* edge_attr, int attr_is_csr_order,
                     const void* csr_ws, int64_t cap, float* out, void* fwd_ws, size_t fwd_ws_bytes, void* stream, bool agg_cleared,
                     int64_t n_per_graph) {
    gm::DevGuard dev_guard(out);
    GM_REQUIRE(m && csr_ws && fwd_ws, GM_ERR_INVALID_ARGUMENT, "gm_epd_forward: null pointer");
    GM_REQUIRE(n >= 0 && cap >= 0 && n < ((int64_t)1 << 31) && cap < ((int64_t)1 << 31), GM_ERR_INVALID_ARGUMENT, "gm_epd_forward: sizes out of range");
    if (n == 0) return GM_OK;
    GM_REQUIRE(nodes && out && (edge_attr || cap == 0), GM_ERR_INVALID_ARGUMENT, "gm_epd_forward: null tensor");
    const int H = m->Hp, NL = m->NL, M = m->M;   // the padded width: every latent array has this row stride
    FwdWs f = carve_fwd(fwd_ws, H, n, cap, cap);
    GM_REQUIRE(fwd_ws_bytes >= f.bytes, GM_ERR_WORKSPACE, "gm_epd_forward: workspace %zu < %zu", fwd_ws_bytes, f.bytes);
    CsrWs c = carve_csr(const_cast<void*>(csr_ws), n, cap);
    int* flags = &c.hdr->error_flags;
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_inference_images(m, s);
    if (rc != GM_OK) return rc;
    const Route route = route_forward(m, Entry::Fused, n, n_per_graph, cap, attr_is_csr_order != 0);
    {
        EdgeArgs ee = enc_edge_args(m, edge_attr, attr_is_csr_order ? nullptr : c.eid, c.hdr, 0, f.e);
        ee.zero_pad_rows = 1;
        rc = launch_edge(H, NL, true, route.sys_enc, ee, cap, s);
    }
    if (rc != GM_OK) return rc;
    if (cap > 0 && !route.sys_enc) {
        ProfScope prof(m->prof, PROF_REST, s);
        rc = zero_edge_pad_rows(c.hdr, f.e, H, s);
        if (rc != GM_OK) return rc;
    }
    // The systolic node path (hedge.h) takes the h half of its node MLP's first Linear as Q, written with P by the projection kernel
    // behind every step.
    auto proj_args = [&](int k) {   // h -> P of edge step k, Q of node step k
        ProjSysArgs pa{};
        pa.h = f.h; pa.P = f.P; pa.Q = f.Q; pa.n = (int)n; pa.flags = flags; pa.prof = m->prof;
        pa.precision = m->precision;
        pa.img_p = m->packed_hm + (k == 0 ? m->hm_enc_node_tail : m->hm_node_tail[k - 1]);
        pa.img_q = m->packed_hm + m->hm_node_q[k];
        pa.scale_p = edge_sys_p_scale(m->packed_h3 + m->h3_edge[k]);
        pa.scale_q = edge_sys_p_scale(m->packed_h3 + m->h3_node[k]);
        return pa;
    };
    {
        HmNodeArgs na = enc_node_args(m, n, nodes, f.h, flags);
        if (!route.sys_node) set_tail(m, na, 0, f.P, out, route.sys_edge);
        rc = launch_node_hm(H, 0, na, s);
    }
    if (rc == GM_OK && route.sys_node) rc = launch_proj_sys(proj_args(0), s);
    if (rc != GM_OK) return rc;
    // agg is zeroed once (nodes without in-edges read zeros; rows with in-edges are stored whole by every edge launch)
    if (!agg_cleared) {
        ProfScope prof(m->prof, PROF_REST, s);
        GM_HIP_CHECK(hipMemsetAsync(f.agg, 0, (size_t)n * H * sizeof(float), s));
    }
    for (int k = 0; k < M; ++k) {
        EdgeArgs ea = proc_edge_args(m, k, c, n, nullptr, f.P, f.e, f.e, f.agg, f.side, 1);
        ea.discard_e_out = k + 1 == M;   // the decoder reads h only (epd_gnn.py:96): the last step's e + e' is never looked at
        ea.P_prescaled = route.sys_edge;
        rc = launch_edge(H, NL, false, route.sys_edge, ea, cap, s);
        if (rc != GM_OK) return rc;
        if (route.sys_node) {
            // head partials of the scatter-add into agg, the node MLP (h in place), then the next step's projections (one launch with the
            // node MLP, or two: gm_model_set_node_fusion) -- or the decoder
            rc = launch_agg_stitch(f.agg, f.side, carve_edge_blocks(c.blocks, n, cap), n, m->prof, s);
            NodeSysArgs ns{};
            ns.h = f.h; ns.agg = f.agg; ns.Q = f.Q; ns.h_out = f.h; ns.image = m->packed_h3 + m->h3_node[k];
            ns.n = (int)n; ns.flags = flags; ns.eps = m->d.ln_eps; ns.prof = m->prof;
            ns.precision = m->precision;
            const bool fused = k + 1 < M && m->node_fusion;
            if (rc == GM_OK) rc = fused ? launch_node_proj_sys(ns, proj_args(k + 1), s) : launch_node_sys(ns, s);
            if (rc == GM_OK && k + 1 < M && !fused) rc = launch_proj_sys(proj_args(k + 1), s);
            if (rc == GM_OK && k + 1 == M) rc = launch_node_hm(H, 2, tail_args(m, M, n, f.h, f.P, out, flags), s);
        } else {
            HmNodeArgs a = proc_node_args(m, k, c, n, cap, f.h, f.agg, f.side, f.h, 1);
            set_tail(m, a, k + 1, f.P, out, route.sys_edge);
            rc = launch_node_hm(H, 1, a, s);
        }
        if (rc != GM_OK) return rc;
    }
    return GM_OK;
}
}  // namespace

extern "C" {

int gm_epd_forward(const gm_model* m, const float* nodes, int64_t n, const float* edge_attr, int attr_is_csr_order,
                   const void* csr_ws, int64_t cap, float* out, void* fwd_ws, size_t fwd_ws_bytes, void* stream) {
    return epd_forward_impl(m, nodes, n, edge_attr, attr_is_csr_order, csr_ws, cap, out, fwd_ws, fwd_ws_bytes, stream, false, n);
}

int gm_graph_independent_forward(const gm_model* m, const float* x, int64_t n, const float* edge_attr, int64_t e,
                                 float* h_out, float* e_out, void* stream) {
    gm::DevGuard dev_guard(x ? (const void*)x : (const void*)edge_attr);
    GM_REQUIRE(m, GM_ERR_INVALID_ARGUMENT, "gm_graph_independent_forward: null model");
    GM_REQUIRE(n >= 0 && e >= 0 && n < ((int64_t)1 << 31) && e < ((int64_t)1 << 31), GM_ERR_INVALID_ARGUMENT, "sizes out of range");
    GM_REQUIRE((n == 0 || (x && h_out)) && (e == 0 || (edge_attr && e_out)), GM_ERR_INVALID_ARGUMENT, "gm_graph_independent_forward: null tensor");
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_inference_images(m, s);
    if (rc != GM_OK) return rc;
    const Route route = route_forward(m, Entry::Independent, n, n, e, true);
    rc = launch_edge(m->Hp, m->NL, true, route.sys_enc, enc_edge_args(m, edge_attr, nullptr, nullptr, (int)e, e_out), e, s);
    if (rc != GM_OK || n == 0) return rc;
    return launch_node_hm(m->Hp, 0, enc_node_args(m, n, x, h_out, nullptr), s);
}

int gm_interaction_network_forward(const gm_model* m, int k, const float* h, int64_t n, const float* e,
                                   const void* csr_ws, int64_t cap, float* h_out, float* e_out, void* fwd_ws,
                                   size_t fwd_ws_bytes, void* stream) {
    gm::DevGuard dev_guard(h);
    GM_REQUIRE(m && csr_ws && fwd_ws, GM_ERR_INVALID_ARGUMENT, "gm_interaction_network_forward: null pointer");
    GM_REQUIRE(k >= 0 && k < m->M, GM_ERR_INVALID_ARGUMENT, "gm_interaction_network_forward: block %d out of range", k);
    GM_REQUIRE(n >= 0 && cap >= 0 && n < ((int64_t)1 << 31) && cap < ((int64_t)1 << 31), GM_ERR_INVALID_ARGUMENT, "sizes out of range");
    if (n == 0) return GM_OK;
    GM_REQUIRE(h && h_out && (cap == 0 || (e && e_out)), GM_ERR_INVALID_ARGUMENT, "gm_interaction_network_forward: null tensor");
    const int H = m->Hp, NL = m->NL;
    FwdWs f = carve_fwd(fwd_ws, H, n, 0, cap);  // P, agg and the side buffer are used
    GM_REQUIRE(fwd_ws_bytes >= f.bytes, GM_ERR_WORKSPACE, "gm_interaction_network_forward: workspace %zu < %zu", fwd_ws_bytes, f.bytes);
    CsrWs c = carve_csr(const_cast<void*>(csr_ws), n, cap);
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_inference_images(m, s);
    if (rc != GM_OK) return rc;
    const Route route = route_forward(m, Entry::Block, n, n, cap, false);
    // projection P = h [W_i | W_j]^T (+ b1): the tail section of the preceding node stream
    rc = launch_node_hm(H, 2, tail_args(m, k, n, h, f.P, nullptr, &c.hdr->error_flags), s);
    if (rc != GM_OK) return rc;
    GM_HIP_CHECK(hipMemsetAsync(f.agg, 0, (size_t)n * H * sizeof(float), s));
    rc = launch_edge(H, NL, false, route.sys_edge, proc_edge_args(m, k, c, n, c.eid, f.P, e, e_out, f.agg, f.side, 0), cap, s);
    if (rc != GM_OK) return rc;
    return launch_node_hm(H, 1, proc_node_args(m, k, c, n, cap, h, f.agg, f.side, h_out, 0), s);
}

// ------------------------------------------------------------------------------------------
// rollout step
// ------------------------------------------------------------------------------------------
}  // extern "C"

namespace {
struct RolloutWs {
    void *graph, *csr, *fwd;
    float *x, *edge_attr, *pred;
    size_t graph_bytes, csr_bytes, fwd_bytes, bytes;
};
RolloutWs carve_rollout(void* ws, const gm_model_desc* d, int64_t n, int K) {
    RolloutWs r;
    const int64_t cap = n * K;
    r.graph_bytes = gm_graph_workspace_bytes(n, K);
    r.csr_bytes = gm_csr_workspace_bytes(n, cap);
    r.fwd_bytes = gm_forward_workspace_bytes(d, n, cap);
    Carver c(ws);
    r.graph = c.take<char>(r.graph_bytes);
    r.csr = c.take<char>(r.csr_bytes);
    r.fwd = c.take<char>(r.fwd_bytes);
    r.x = c.take<float>((size_t)n * 32);
    r.edge_attr = c.take<float>((size_t)cap * 4);
    r.pred = c.take<float>((size_t)n * 4);
    r.bytes = c.used();
    return r;
}
// scratch of a renumbered rollout (gm_rollout, renumber_every > 0): two copies of the state (a re-ordering reads one and writes the
// other), the row maps that go with them, the order and the rigid ranks of the current copy
struct RenumberWs {
    float* state[2];
    int* total[2];
    int *perm, *rank;
    size_t bytes;
};
RenumberWs carve_renumber(void* ws, const gm_feature_desc* fd, int64_t n) {
    RenumberWs w;
    Carver c(ws);
    const size_t st = (size_t)fd->k_steps * n * fd->data_dim;
    w.state[0] = c.take<float>(st);
    w.state[1] = c.take<float>(st);
    w.total[0] = c.take<int>(n);
    w.total[1] = c.take<int>(n);
    w.perm = c.take<int>(n);
    w.rank = c.take<int>(n);
    w.bytes = c.used();
    return w;
}
}  // namespace

extern "C" {

int gm_model_set_edge_kernel(gm_model* m, int choice) {
    GM_REQUIRE(m, GM_ERR_INVALID_ARGUMENT, "gm_model_set_edge_kernel: null model");
    GM_REQUIRE(choice >= EK_AUTO && choice <= EK_SYS_ALL, GM_ERR_INVALID_ARGUMENT, "gm_model_set_edge_kernel: choice %d out of range", choice);
    GM_REQUIRE(choice == EK_AUTO || choice >= EK_SYS, GM_ERR_UNSUPPORTED,
               "gm_model_set_edge_kernel: choices 1..4 (the round-1 fp32 / bf16 x 6 kernels) were removed from the library (round 5)");
    GM_REQUIRE((choice != EK_SYS && choice != EK_SYS_ALL) || m->packed_h3, GM_ERR_UNSUPPORTED, "gm_model_set_edge_kernel: the systolic kernel is for hidden_size 128, num_layers 2");
    m->edge_kernel = choice;
    return GM_OK;
}

int gm_model_set_node_fusion(gm_model* m, int on) {
    GM_REQUIRE(m, GM_ERR_INVALID_ARGUMENT, "gm_model_set_node_fusion: null model");
    m->node_fusion = on != 0;
    return GM_OK;
}

int gm_model_set_precision(gm_model* m, int precision) {
    GM_REQUIRE(m, GM_ERR_INVALID_ARGUMENT, "gm_model_set_precision: null model");
    GM_REQUIRE(precision == GM_PRECISION_F32 || precision == GM_PRECISION_F16, GM_ERR_INVALID_ARGUMENT,
               "gm_model_set_precision: precision %d (GM_PRECISION_F32 = 0, GM_PRECISION_F16 = 1)", precision);
    m->precision = precision;
    return GM_OK;
}

int gm_model_profile(gm_model* m, int kind_mask) {
    GM_REQUIRE(m, GM_ERR_INVALID_ARGUMENT, "gm_model_profile: null model");
    if (!m->prof) {
        if (!kind_mask) return GM_OK;
        m->prof = new ProfState();
    }
    for (int k = 0; k < PROF_KINDS; ++k)
        if (((kind_mask & ~m->prof->mask) >> k) & 1) m->prof->count[k] = m->prof->dropped[k] = 0;  // newly enabled kinds start from zero
    m->prof->mask = kind_mask;
    return GM_OK;
}

int gm_model_profile_query(const gm_model* m, int kind, int64_t* launches, double* total_ms) {
    GM_REQUIRE(m && kind >= 0 && kind < PROF_KINDS && launches && total_ms, GM_ERR_INVALID_ARGUMENT, "gm_model_profile_query: bad argument");
    *launches = 0;
    *total_ms = 0.0;
    const ProfState* p = m->prof;
    if (!p) return GM_OK;
    // scopes beyond the kind's PROF_MAX event pairs were not timed: the count comes back NEGATIVE (minus the scopes opened) and the
    // total covers the first PROF_MAX only -- a caller that divides by steps must not use it
    *launches = p->dropped[kind] ? -(int64_t)(p->count[kind] + p->dropped[kind]) : p->count[kind];
    for (int i = 0; i < p->count[kind]; ++i) {
        GM_HIP_CHECK(hipEventSynchronize(p->stop[kind][i]));
        float ms = 0.f;
        GM_HIP_CHECK(hipEventElapsedTime(&ms, p->start[kind][i], p->stop[kind][i]));
        *total_ms += ms;
    }
    return GM_OK;
}

size_t gm_rollout_workspace_bytes(const gm_model_desc* desc, int64_t n, int K) {
    if (!desc || n < 0 || K < 1) return 0;
    return carve_rollout(nullptr, desc, n, K).bytes;
}

}  // extern "C"

namespace {
int64_t ragged_min_rows(const gm::RaggedOffsets& R) {
    int64_t lo = R.off[1] - R.off[0];
    for (int g = 1; g < R.n_graphs; ++g) lo = std::min<int64_t>(lo, R.off[g + 1] - R.off[g]);
    return lo;
}

// gm_rollout_step under either drive: the scripted one (rigid_target, pred_acc_out) or -- rec given -- the recorded one
// R (or nullptr: graphs of fd->nodes_per_graph rows): the graphs of a ragged batch, n = R->off[R->n_graphs]
int rollout_step_impl(const gm_model* m, float* obs, int64_t n, const gm_feature_desc* fd, int K, const int32_t* rigid_rank,
                      const float* rigid_target, float* pred_acc_out, const gm::RecordedDrive* rec, void* ws, size_t ws_bytes,
                      void* stream, const gm::RaggedOffsets* R = nullptr) {
    gm::DevGuard dev_guard(obs);
    GM_REQUIRE(m && obs && fd && ws, GM_ERR_INVALID_ARGUMENT, "gm_rollout_step: null pointer");
    int rc = gm::check_model_for_scene(m->d, fd, "gm_rollout_step");
    if (rc != GM_OK) return rc;
    GM_REQUIRE(n < ((int64_t)1 << 31) / (K > 0 ? K : 1), GM_ERR_UNSUPPORTED, "gm_rollout_step: n*max_neighbours overflows int32");
    RolloutWs r = carve_rollout(ws, &m->d, n, K);
    GM_REQUIRE(ws_bytes >= r.bytes, GM_ERR_WORKSPACE, "gm_rollout_step: workspace %zu < %zu", ws_bytes, r.bytes);
    if (n == 0) return GM_OK;
    const int64_t cap = n * K;
    hipStream_t hs = (hipStream_t)stream;
    // state_pre + node features in one launch -- which also resets what the step's later launches build on: the graph and
    // destination-sort workspaces (headers, cell counts, in-degrees, scan states, stitch table) and the forward's agg rows
    {
        StepClear clr;
        rc = graph_clear_jobs(clr, carve_graph(r.graph, n, K), n);
        if (rc == GM_OK) rc = csr_clear_jobs(clr, carve_csr(r.csr, n, cap), n, m->d.flow);
        FwdWs f = carve_fwd(r.fwd, m->Hp, n, cap, cap);
        if (rc == GM_OK) rc = clr.add(reinterpret_cast<int*>(f.agg), (long long)n * m->Hp, 0);
        if (rc != GM_OK) return rc;
        ProfScope prof(m->prof, PROF_REST, hs);
        rc = gm::rollout_pre_features(obs, n, fd, rigid_rank, rigid_target, r.x, hs, &clr, rec);
    }
    if (rc != GM_OK) return rc;
    const float* last_pos = obs + (size_t)(fd->k_steps - 1) * n * fd->data_dim + fd->cart_col;
    {   // the in-degree count of the destination sort rides in the neighbour search
        ProfScope prof(m->prof, PROF_GRAPH, hs);
        rc = R ? gm::radius_graph_build_fused_ragged(last_pos, fd->data_dim, *R, fd->conn_r, K, r.graph, r.graph_bytes, r.csr, r.csr_bytes,
                                                     m->d.flow, hs)
               : gm::radius_graph_build_fused(last_pos, fd->data_dim, n, gm::graph_nodes(fd, n), fd->conn_r, K,
                                              r.graph, r.graph_bytes, r.csr, r.csr_bytes, m->d.flow, hs);
    }
    if (rc != GM_OK) return rc;
    // destination sort; the edge features and the block tables are written by the same pass that fixes each segment's order
    {
        ProfScope prof(m->prof, PROF_REST, hs);
        rc = R ? gm::csr_from_graph_fused_ragged(r.graph, *R, K, r.csr, r.csr_bytes, last_pos, fd->data_dim, (float)fd->conn_r, r.edge_attr,
                                                 m->d.flow, hs)
               : gm::csr_from_graph_fused(r.graph, n, K, r.csr, r.csr_bytes, last_pos, fd->data_dim, (float)fd->conn_r, r.edge_attr,
                                          m->d.flow, hs);
    }
    if (rc != GM_OK) return rc;
    // a ragged batch routes by its smallest graph (hedge.h, kSysNodeMinNodes)
    rc = epd_forward_impl(m, r.x, n, r.edge_attr, 1, r.csr, cap, r.pred, r.fwd, r.fwd_bytes, stream, true,
                          R ? ragged_min_rows(*R) : gm::graph_nodes(fd, n));
    if (rc != GM_OK) return rc;
    // integrator + window shift + write-back (+ copy of the prediction) in one launch
    ProfScope prof(m->prof, PROF_REST, hs);
    return gm::rollout_integrate_post(obs, n, fd, r.pred, rigid_rank, rigid_target, pred_acc_out, hs, rec);
}
}  // namespace

extern "C" {

int gm_rollout_step(const gm_model* m, float* obs, int64_t n, const gm_feature_desc* fd, int K, const int32_t* rigid_rank,
                    const float* rigid_target, float* pred_acc_out, void* ws, size_t ws_bytes, void* stream) {
    return rollout_step_impl(m, obs, n, fd, K, rigid_rank, rigid_target, pred_acc_out, nullptr, ws, ws_bytes, stream);
}

int gm_rollout_step_ragged(const gm_model* m, float* obs, const int64_t* graph_offsets_host, int64_t n_graphs, const gm_feature_desc* fd, int K,
                           const int32_t* rigid_rank, const float* rigid_target, float* pred_acc_out, void* ws, size_t ws_bytes,
                           void* stream) {
    gm::RaggedOffsets R;
    const int rc = gm::ragged_scene_table("gm_rollout_step_ragged", fd, graph_offsets_host, n_graphs, K, ws, &R);
    if (rc != GM_OK) return rc;
    GM_REQUIRE(m && obs, GM_ERR_INVALID_ARGUMENT, "gm_rollout_step_ragged: null pointer");
    const size_t need = carve_rollout(nullptr, &m->d, R.off[R.n_graphs], K).bytes;
    GM_REQUIRE(ws_bytes >= need, GM_ERR_WORKSPACE, "gm_rollout_step_ragged: workspace %zu < %zu", ws_bytes, need);
    return rollout_step_impl(m, obs, R.off[R.n_graphs], fd, K, rigid_rank, rigid_target, pred_acc_out, nullptr, ws, ws_bytes, stream, &R);
}

size_t gm_rollout_renumber_workspace_bytes(const gm_feature_desc* fd, int64_t n) {
    if (!fd || n < 0 || fd->k_steps < 1 || fd->data_dim < 1) return 0;
    return carve_renumber(nullptr, fd, n).bytes;
}

}  // extern "C"

namespace {
// What moves the rigid rows of a rollout: scripted poses (gm_rollout: targets) or the frames of a recording (gm_rollout_recorded:
// frames).  The loop below is the one loop of both.
struct RolloutDrive {
    const float* targets = nullptr;   // [n_targets, n_rigid, 3]
    int64_t n_targets = 0, n_rigid = 0;
    const float* frames = nullptr;    // [steps, N, D], the caller's numbering
    float* record_pred = nullptr;     // [steps, N, 3] or nullptr (recorded drive only)
};
int rollout_loop(const char* who, const gm_model* m, float* obs, int64_t n, const gm_feature_desc* fd, int K, const int32_t* rigid_rank,
                 const RolloutDrive& drive, int64_t steps, float* record_last, int64_t renumber_every, void* renumber_ws,
                 size_t renumber_ws_bytes, void* ws, size_t ws_bytes, void* stream, const gm::RaggedOffsets* R = nullptr) {
    hipStream_t hs = (hipStream_t)stream;
    const float* rigid_targets = drive.targets;
    const int64_t n_targets = drive.n_targets, n_rigid = drive.n_rigid;
    const size_t frame = (size_t)n * fd->data_dim;
    const bool renum = renumber_every > 0 && n > 0 && steps > 0;
    RenumberWs rw{};
    RolloutWs r{};
    if (renum) {
        GM_REQUIRE(renumber_ws, GM_ERR_INVALID_ARGUMENT, "%s: renumber_every > 0 needs renumber_ws (gm_rollout_renumber_workspace_bytes)", who);
        rw = carve_renumber(renumber_ws, fd, n);
        GM_REQUIRE(renumber_ws_bytes >= rw.bytes, GM_ERR_WORKSPACE, "%s: renumber workspace %zu < %zu", who, renumber_ws_bytes, rw.bytes);
        GM_REQUIRE(n < ((int64_t)1 << 31) / (K > 0 ? K : 1), GM_ERR_UNSUPPORTED, "%s: n*max_neighbours overflows int32", who);
        r = carve_rollout(ws, &m->d, n, K);
        GM_REQUIRE(ws_bytes >= r.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, r.bytes);
    }
    // The renumbered rollout works on a copy of the state whose rows are in grid-cell order (gm::cell_order: the radius graph's own
    // grid; scenes of a batch stay apart), re-ordered every `renumber_every` steps: state[j] is the caller's row total[j], its rigid
    // rank is the caller's (rank values only index the pose arrays: any order does), records and the final state go back through
    // `total`.  A radius graph does not depend on the numbering and every per-node / per-edge function is numbering-free, so what
    // changes is the order in which a node's incoming messages are summed: float32 rounding (tests: 2e-6 of the plain engine).
    float* state = obs;            // the array the steps run on
    const int* rank = rigid_rank;
    const int* total = nullptr;    // row of the caller's state that row j of `state` is (nullptr: the identity)
    int flip = 0;
    for (int64_t i = 0; i < steps; ++i) {
        if (renum && i % renumber_every == 0) {
            const float* last_pos = state + (size_t)(fd->k_steps - 1) * frame + fd->cart_col;
            int rc = gm::cell_order(last_pos, fd->data_dim, n, gm::graph_nodes(fd, n), fd->conn_r, K, r.graph,
                                    r.graph_bytes, rw.perm, hs);
            if (rc != GM_OK) return rc;
            rc = gm::renumber_gather(state, rw.state[flip], fd->k_steps, n, fd->data_dim, rw.perm, r.graph, total, rw.total[flip],
                                     rigid_rank, rigid_rank ? rw.rank : nullptr, hs);
            if (rc != GM_OK) return rc;
            state = rw.state[flip];
            total = rw.total[flip];
            rank = rigid_rank ? rw.rank : nullptr;
            flip ^= 1;
        }
        if (drive.frames) {
            // the recorded drive: control overwrite, record, pose and the copy of the prediction ride in the step's two fused
            // launches, reaching the caller's arrays through `total`
            const gm::RecordedDrive rec{drive.frames + (size_t)i * frame, total, record_last ? record_last + (size_t)i * frame : nullptr,
                                        drive.record_pred ? drive.record_pred + (size_t)i * n * 3 : nullptr};
            int rc = rollout_step_impl(m, state, n, fd, K, rank, nullptr, nullptr, &rec, ws, ws_bytes, stream, R);
            if (rc != GM_OK) return rc;
            continue;
        }
        float* last = state + (size_t)(fd->k_steps - 1) * frame;
        // traj_utils.py:126-134: steps past the scripted trajectory keep the rigid body where it is (control = 0 displacement)
        const float* target = i < n_targets ? rigid_targets + (size_t)i * n_rigid * 3 : nullptr;
        if (record_last) {  // the reference records the last frame after the control overwrite (rollout_utils.py:49, traj_utils.py:137)
            // a descriptor without control columns has nothing to overwrite: the record is the last frame as it stands
            int rc = fd->control_col >= 0 ? gm_state_pre(state, n, fd, rank, target, stream) : GM_OK;
            if (rc != GM_OK) return rc;
            if (total) rc = gm::renumber_scatter(last, record_last + (size_t)i * frame, 1, n, fd->data_dim, total, hs);
            else GM_HIP_CHECK(hipMemcpyAsync(record_last + (size_t)i * frame, last, frame * sizeof(float), hipMemcpyDeviceToDevice, hs));
            if (rc != GM_OK) return rc;
        }
        int rc = rollout_step_impl(m, state, n, fd, K, rank, target, nullptr, nullptr, ws, ws_bytes, stream, R);
        if (rc != GM_OK) return rc;
    }
    if (total) return gm::renumber_scatter(state, obs, fd->k_steps, n, fd->data_dim, total, hs);
    return GM_OK;
}
}  // namespace

extern "C" {

int gm_rollout(const gm_model* m, float* obs, int64_t n, const gm_feature_desc* fd, int K, const int32_t* rigid_rank,
               const float* rigid_targets, int64_t n_targets, int64_t n_rigid, int64_t steps, float* record_last,
               int64_t renumber_every, void* renumber_ws, size_t renumber_ws_bytes, void* ws, size_t ws_bytes, void* stream) {
    gm::DevGuard dev_guard(obs);
    GM_REQUIRE(m && obs && fd && ws, GM_ERR_INVALID_ARGUMENT, "gm_rollout: null pointer");
    GM_REQUIRE(steps >= 0 && n_targets >= 0 && n_rigid >= 0 && renumber_every >= 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout: negative count");
    // a scene without rigid rows has an empty trajectory ([steps, 0, 3]: a null pointer); the reference's loop runs on it unchanged
    GM_REQUIRE(rigid_targets || n_targets == 0 || n_rigid == 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout: n_targets > 0 without rigid_targets");
    GM_REQUIRE(!rigid_targets || rigid_rank, GM_ERR_INVALID_ARGUMENT, "gm_rollout: rigid_targets need rigid_rank");
    RolloutDrive drive;
    drive.targets = rigid_targets; drive.n_targets = n_targets; drive.n_rigid = n_rigid;
    return rollout_loop("gm_rollout", m, obs, n, fd, K, rigid_rank, drive, steps, record_last, renumber_every, renumber_ws, renumber_ws_bytes,
                        ws, ws_bytes, stream);
}

// compute_rollout's ground-truth mode (rollout_utils.py:38-61, args.cma_traj None): gm_rollout's loop under the recorded drive.
// Step i takes the control columns of frames[i] before it runs (:45) and the xyz of the SAME frames[i] after it (:60): the pose
// lags the window by one step, as the reference's does.
int gm_rollout_recorded(const gm_model* m, float* obs, int64_t n, const gm_feature_desc* fd, int K, const int32_t* rigid_rank,
                        const float* frames, int64_t steps, float* record_last, float* record_pred, int64_t renumber_every,
                        void* renumber_ws, size_t renumber_ws_bytes, void* ws, size_t ws_bytes, void* stream) {
    gm::DevGuard dev_guard(obs);
    GM_REQUIRE(m && obs && fd && ws, GM_ERR_INVALID_ARGUMENT, "gm_rollout_recorded: null pointer");
    GM_REQUIRE(steps >= 0 && renumber_every >= 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_recorded: negative count");
    GM_REQUIRE(frames || steps == 0 || n == 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_recorded: steps > 0 without frames");
    if (steps == 0 || n <= 0) return GM_OK;
    RolloutDrive drive;
    drive.frames = frames; drive.record_pred = record_pred;
    return rollout_loop("gm_rollout_recorded", m, obs, n, fd, K, rigid_rank, drive, steps, record_last, renumber_every, renumber_ws,
                        renumber_ws_bytes, ws, ws_bytes, stream);
}

// gm_rollout / gm_rollout_recorded on graphs of any sizes: the same loop and launches, the table in every step's graph path, no
// renumbering.  The workspace is checked here, before the first launch, so that a refusal leaves every output as it was.
int gm_rollout_ragged(const gm_model* m, float* obs, const int64_t* graph_offsets_host, int64_t n_graphs, const gm_feature_desc* fd, int K,
                      const int32_t* rigid_rank, const float* rigid_targets, int64_t n_targets, int64_t n_rigid, int64_t steps,
                      float* record_last, void* ws, size_t ws_bytes, void* stream) {
    gm::RaggedOffsets R;
    const int rc = gm::ragged_scene_table("gm_rollout_ragged", fd, graph_offsets_host, n_graphs, K, ws, &R);
    if (rc != GM_OK) return rc;
    gm::DevGuard dev_guard(obs);
    GM_REQUIRE(m && obs, GM_ERR_INVALID_ARGUMENT, "gm_rollout_ragged: null pointer");
    GM_REQUIRE(steps >= 0 && n_targets >= 0 && n_rigid >= 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_ragged: negative count");
    GM_REQUIRE(rigid_targets || n_targets == 0 || n_rigid == 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_ragged: n_targets > 0 without rigid_targets");
    GM_REQUIRE(!rigid_targets || rigid_rank, GM_ERR_INVALID_ARGUMENT, "gm_rollout_ragged: rigid_targets need rigid_rank");
    const int64_t n = R.off[R.n_graphs];
    const size_t need = carve_rollout(nullptr, &m->d, n, K).bytes;
    GM_REQUIRE(ws_bytes >= need, GM_ERR_WORKSPACE, "gm_rollout_ragged: workspace %zu < %zu", ws_bytes, need);
    RolloutDrive drive;
    drive.targets = rigid_targets; drive.n_targets = n_targets; drive.n_rigid = n_rigid;
    return rollout_loop("gm_rollout_ragged", m, obs, n, fd, K, rigid_rank, drive, steps, record_last, 0, nullptr, 0, ws, ws_bytes, stream, &R);
}

int gm_rollout_recorded_ragged(const gm_model* m, float* obs, const int64_t* graph_offsets_host, int64_t n_graphs, const gm_feature_desc* fd,
                               int K, const int32_t* rigid_rank, const float* frames, int64_t steps, float* record_last, float* record_pred,
                               void* ws, size_t ws_bytes, void* stream) {
    gm::RaggedOffsets R;
    const int rc = gm::ragged_scene_table("gm_rollout_recorded_ragged", fd, graph_offsets_host, n_graphs, K, ws, &R);
    if (rc != GM_OK) return rc;
    gm::DevGuard dev_guard(obs);
    GM_REQUIRE(m && obs, GM_ERR_INVALID_ARGUMENT, "gm_rollout_recorded_ragged: null pointer");
    GM_REQUIRE(steps >= 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_recorded_ragged: negative count");
    GM_REQUIRE(frames || steps == 0, GM_ERR_INVALID_ARGUMENT, "gm_rollout_recorded_ragged: steps > 0 without frames");
    const int64_t n = R.off[R.n_graphs];
    const size_t need = carve_rollout(nullptr, &m->d, n, K).bytes;
    GM_REQUIRE(ws_bytes >= need, GM_ERR_WORKSPACE, "gm_rollout_recorded_ragged: workspace %zu < %zu", ws_bytes, need);
    if (steps == 0) return GM_OK;
    RolloutDrive drive;
    drive.frames = frames; drive.record_pred = record_pred;
    return rollout_loop("gm_rollout_recorded_ragged", m, obs, n, fd, K, rigid_rank, drive, steps, record_last, 0, nullptr, 0, ws, ws_bytes,
                        stream, &R);
}

int gm_rollout_status(const void* ws, const gm_model_desc* desc, int64_t n, int K, int64_t* n_edges_host, void* stream) {
    gm::DevGuard dev_guard(ws);
    GM_REQUIRE(ws && desc && n_edges_host, GM_ERR_INVALID_ARGUMENT, "gm_rollout_status: null pointer");
    RolloutWs r = carve_rollout(const_cast<void*>(ws), desc, n, K);
    int rc = gm_radius_graph_num_edges(r.graph, n_edges_host, stream);
    if (rc != GM_OK) return rc;
    int64_t e2 = 0;
    return gm_csr_num_edges(r.csr, &e2, stream);
}

}  // extern "C"
