// The reverse sweep of a rollout in the library: the vector-Jacobian product of one rollout step with respect to its pre-step
// window and scripted pose -- and, for a caller that trains, the model's parameters; without `grads` they are constants -- and the
// loop of it over the windows a forward kept, with an optional gradient on every step's record.  A step is composed of the
// library's own entry points -- nothing here has a kernel of its own but the assembly of the window's gradient (features.hip:
// step_assemble_bwd_kernel), so every number is the one a caller of those entry points would get.
#include "common.h"
#include "model.h"
#include "step_rows.h"

namespace gm {
// features.hip
int rollout_assemble_backward(const float* g_post, const float* g_int, const float* g_nodes, const float* g_pos, const float* t_post,
                              const float* g_rec, int64_t n, const gm_feature_desc* d, const int* rank, bool has_target, float* d_before,
                              float* d_target, hipStream_t s);
}  // namespace gm

namespace {

struct StepBwdWs {
    float *pre, *nodes, *edge_attr, *pred;                 // the forward: window after state_pre, features, prediction
    int64_t* ei;                                           // [2][E], E <= cap
    void *graph, *tape, *bwd, *edge_bwd;
    size_t graph_bytes, tape_bytes, bwd_bytes, edge_bwd_bytes;
    float *d_next, *d_pred, *d_nodes, *d_edge_attr, *d_pos, *t_post;
    float *g_post, *g_int, *g_nodes;                       // [k,N,D] each: the three window-sized contributions
    size_t bytes;
};

StepBwdWs carve_step_bwd(void* ws, const gm_model_desc* d, const gm_feature_desc* fd, int64_t n, int K) {
    StepBwdWs w;
    const int64_t cap = n * K;
    const size_t window = (size_t)fd->k_steps * n * fd->data_dim;
    const size_t F = (size_t)gm::node_feature_dim(fd);
    gm::Carver c(ws);
    w.pre = c.take<float>(window);
    w.nodes = c.take<float>((size_t)n * F);
    w.edge_attr = c.take<float>((size_t)cap * 4);
    w.pred = c.take<float>((size_t)n * 3);
    w.ei = c.take<int64_t>((size_t)2 * cap);
    w.graph_bytes = gm_graph_workspace_bytes(n, K);
    w.tape_bytes = gm_train_tape_bytes(d, n, cap);
    w.bwd_bytes = gm_train_backward_inputs_workspace_bytes(d, n, cap);
    w.edge_bwd_bytes = gm_edge_features_backward_workspace_bytes(n, cap);
    w.graph = c.take<char>(w.graph_bytes);
    w.tape = c.take<char>(w.tape_bytes);
    w.bwd = c.take<char>(w.bwd_bytes);
    w.edge_bwd = c.take<char>(w.edge_bwd_bytes);
    w.d_next = c.take<float>((size_t)n * 3);
    w.d_pred = c.take<float>((size_t)n * 3);
    w.d_nodes = c.take<float>((size_t)n * F);
    w.d_edge_attr = c.take<float>((size_t)cap * 4);
    w.d_pos = c.take<float>((size_t)n * 3);
    w.t_post = c.take<float>((size_t)n * 3);
    w.g_post = c.take<float>(window);
    w.g_int = c.take<float>(window);
    w.g_nodes = c.take<float>(window);
    w.bytes = c.used();
    return w;
}

// the sweep's workspace: the step's, and the two gradient windows that take turns as d_obs_after / d_obs_before
struct SweepWs {
    void* step;
    size_t step_bytes;
    float* g[2];
    size_t bytes;
};
SweepWs carve_sweep(void* ws, const gm_model_desc* d, const gm_feature_desc* fd, int64_t n, int K) {
    SweepWs w;
    gm::Carver c(ws);
    w.step_bytes = carve_step_bwd(nullptr, d, fd, n, K).bytes;
    w.step = c.take<char>(w.step_bytes);
    const size_t window = (size_t)fd->k_steps * n * fd->data_dim;
    w.g[0] = c.take<float>(window);
    w.g[1] = c.take<float>(window);
    w.bytes = c.used();
    return w;
}

bool sizes_ok(const gm_model_desc* d, const gm_feature_desc* fd, int64_t n, int K) {
    return d && fd && n >= 0 && K >= 1 && fd->k_steps >= 2 && fd->k_steps <= 64 && fd->data_dim >= 4 && n < ((int64_t)1 << 31) / K;
}

}  // namespace

extern "C" {

size_t gm_rollout_step_backward_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n, int K) {
    if (!sizes_ok(desc, fdesc, n, K)) return 0;
    return carve_step_bwd(nullptr, desc, fdesc, n, K).bytes;
}

// both step entry points; `who` names the one that was called in its messages.  R (or nullptr: graphs of fd->nodes_per_graph rows): the
// graphs of a ragged batch -- the step's graph is then gm_radius_graph_build_ragged's; everything else is per row or per edge
static int step_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* obs_before, int64_t n,
                         const gm_feature_desc* fd, int K, const int32_t* rigid_rank, const float* rigid_target, const float* d_obs_after,
                         const float* d_record, float* const* grads, float* d_obs_before, float* d_rigid_target, int64_t* n_edges_host,
                         void* ws, size_t ws_bytes, void* stream, const char* who, const gm::RaggedOffsets* R = nullptr) {
    gm::DevGuard dev_guard(obs_before);
    GM_REQUIRE(m && tensors && fd && ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(sizes_ok(&m->d, fd, n, K), GM_ERR_INVALID_ARGUMENT, "%s: sizes out of range", who);
    GM_REQUIRE(n == 0 || (obs_before && d_obs_after && d_obs_before), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(!rigid_target || rigid_rank, GM_ERR_INVALID_ARGUMENT, "%s: rigid_target needs rigid_rank", who);
    int rc = gm::check_model_for_scene(m->d, fd, who);
    if (rc != GM_OK) return rc;
    StepBwdWs w = carve_step_bwd(ws, &m->d, fd, n, K);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.bytes);
    if (n_edges_host) *n_edges_host = 0;
    if (n == 0) return GM_OK;
    hipStream_t hs = (hipStream_t)stream;
    const size_t window = (size_t)fd->k_steps * n * fd->data_dim;
    const bool has_target = rigid_target != nullptr;
    const bool pre = rigid_rank && fd->control_col >= 0;   // gm_rollout_step's own condition for the overwrite
    const float conn_r = (float)fd->conn_r;

    // ---- the step's forward again, out of place, with the training forward's tape
    GM_HIP_CHECK(hipMemcpyAsync(w.pre, obs_before, window * sizeof(float), hipMemcpyDeviceToDevice, hs));
    if (pre) {
        rc = gm_state_pre(w.pre, n, fd, rigid_rank, rigid_target, stream);
        if (rc != GM_OK) return rc;
    }
    rc = gm_node_features(w.pre, n, fd, w.nodes, stream);
    if (rc != GM_OK) return rc;
    const float* last_pos = w.pre + (size_t)(fd->k_steps - 1) * n * fd->data_dim + fd->cart_col;
    if (R) {
        int64_t off[GM_RAGGED_MAX_GRAPHS + 1];
        for (int g = 0; g <= R->n_graphs; ++g) off[g] = R->off[g];
        rc = gm_radius_graph_build_ragged(last_pos, fd->data_dim, off, R->n_graphs, fd->conn_r, K, w.graph, w.graph_bytes, stream);
    } else {
        rc = gm_radius_graph_build_batched(last_pos, fd->data_dim, n, gm::graph_nodes(fd, n), fd->conn_r, K, w.graph,
                                           w.graph_bytes, stream);
    }
    if (rc != GM_OK) return rc;
    int64_t e = 0;
    rc = gm_radius_graph_num_edges(w.graph, &e, stream);   // the one number read back: the training forward takes E on the host
    if (rc != GM_OK) return rc;
    GM_REQUIRE(e >= 0 && e <= n * K, GM_ERR_DATA, "%s: edge count %lld outside [0, %lld]", who, (long long)e, (long long)(n * K));
    if (n_edges_host) *n_edges_host = e;
    int64_t *senders = w.ei, *receivers = w.ei + e;
    rc = gm_radius_graph_edges(w.graph, n, K, senders, receivers, e, stream);
    if (rc != GM_OK) return rc;
    rc = gm_edge_features(last_pos, fd->data_dim, senders, receivers, e, conn_r, w.edge_attr, stream);
    if (rc != GM_OK) return rc;
    rc = gm_epd_forward_train(m, w.nodes, n, w.edge_attr, w.ei, e, w.pred, w.tape, w.tape_bytes, stream);
    if (rc != GM_OK) return rc;

    // ---- the transposes, last function first
    rc = gm_state_post_backward(d_obs_after, n, fd, rigid_rank, has_target, w.g_post, w.d_next, w.t_post, stream);
    if (rc != GM_OK) return rc;
    rc = gm_integrate_backward(w.d_next, n, fd, w.d_pred, w.g_int, stream);
    if (rc != GM_OK) return rc;
    // the same dz chains and input tails either way (d_nodes / d_edge_attr are bit-equal); with grads, the weight-gradient launches too
    if (grads)
        rc = gm_epd_backward_inputs(m, tensors, n_tensors, w.nodes, w.edge_attr, n, e, w.d_pred, grads, w.d_nodes,
                                    e > 0 ? w.d_edge_attr : nullptr, w.tape, w.tape_bytes, w.bwd, w.bwd_bytes, stream);
    else
        rc = gm_epd_backward_inputs_only(m, tensors, n_tensors, w.nodes, w.edge_attr, n, e, w.d_pred, w.d_nodes,
                                         e > 0 ? w.d_edge_attr : nullptr, w.tape, w.tape_bytes, w.bwd, w.bwd_bytes, stream);
    if (rc != GM_OK) return rc;
    rc = gm_node_features_backward(w.pre, n, fd, w.d_nodes, w.g_nodes, stream);
    if (rc != GM_OK) return rc;
    rc = gm_edge_features_backward(last_pos, fd->data_dim, senders, receivers, n, e, conn_r, w.d_edge_attr, w.d_pos, w.edge_bwd,
                                   w.edge_bwd_bytes, stream);
    if (rc != GM_OK) return rc;
    // the sum of the four (and of d_record, when given), state_pre's transpose and both shares of d_rigid_target: one launch, one
    // thread per particle row
    return gm::rollout_assemble_backward(w.g_post, w.g_int, w.g_nodes, w.d_pos, w.t_post, d_record, n, fd, rigid_rank, has_target,
                                         d_obs_before, d_rigid_target, hs);
}

int gm_rollout_step_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* obs_before, int64_t n,
                             const gm_feature_desc* fd, int K, const int32_t* rigid_rank, const float* rigid_target,
                             const float* d_obs_after, float* d_obs_before, float* d_rigid_target, int64_t* n_edges_host, void* ws,
                             size_t ws_bytes, void* stream) {
    return step_backward(m, tensors, n_tensors, obs_before, n, fd, K, rigid_rank, rigid_target, d_obs_after, nullptr, nullptr, d_obs_before,
                         d_rigid_target, n_edges_host, ws, ws_bytes, stream, __func__);
}

int gm_rollout_step_backward_train(const gm_model* m, const float* const* tensors, int n_tensors, const float* obs_before, int64_t n,
                                   const gm_feature_desc* fd, int K, const int32_t* rigid_rank, const float* rigid_target,
                                   const float* d_obs_after, const float* d_record, float* const* grads, float* d_obs_before,
                                   float* d_rigid_target, int64_t* n_edges_host, void* ws, size_t ws_bytes, void* stream) {
    return step_backward(m, tensors, n_tensors, obs_before, n, fd, K, rigid_rank, rigid_target, d_obs_after, d_record, grads, d_obs_before,
                         d_rigid_target, n_edges_host, ws, ws_bytes, stream, __func__);
}

size_t gm_rollout_backward_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n, int K) {
    if (!sizes_ok(desc, fdesc, n, K)) return 0;
    return carve_sweep(nullptr, desc, fdesc, n, K).bytes;
}

static int sweep_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* windows, int64_t n,
                          const gm_feature_desc* fd, int K, const int32_t* rigid_rank, const float* trajectory, int64_t n_targets,
                          int64_t n_rigid, int64_t steps, const float* d_final, const float* d_records, float* const* grads, float* d_obs0,
                          float* d_trajectory, void* ws, size_t ws_bytes, void* stream, const char* who, const gm::RaggedOffsets* R = nullptr) {
    gm::DevGuard dev_guard(d_final);
    GM_REQUIRE(m && tensors && fd && ws, GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(steps >= 0 && n_targets >= 0 && n_rigid >= 0, GM_ERR_INVALID_ARGUMENT, "%s: negative count", who);
    GM_REQUIRE(sizes_ok(&m->d, fd, n, K), GM_ERR_INVALID_ARGUMENT, "%s: sizes out of range", who);
    GM_REQUIRE(n == 0 || (d_final && d_obs0 && (windows || steps == 0)), GM_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    GM_REQUIRE(trajectory || n_targets == 0 || n_rigid == 0, GM_ERR_INVALID_ARGUMENT, "%s: n_targets > 0 without trajectory", who);
    GM_REQUIRE(!trajectory || rigid_rank, GM_ERR_INVALID_ARGUMENT, "%s: a trajectory needs rigid_rank", who);
    GM_REQUIRE(n_rigid <= n, GM_ERR_INVALID_ARGUMENT, "%s: n_rigid=%lld > n_nodes=%lld", who, (long long)n_rigid, (long long)n);
    SweepWs w = carve_sweep(ws, &m->d, fd, n, K);
    GM_REQUIRE(ws_bytes >= w.bytes, GM_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.bytes);
    hipStream_t hs = (hipStream_t)stream;
    const size_t window = (size_t)fd->k_steps * n * fd->data_dim;
    const size_t pose = (size_t)n_rigid * 3;
    const size_t record = (size_t)n * fd->data_dim;
    // rows of steps the sweep does not visit (at or past `steps`) are zeros; the others are overwritten below
    if (d_trajectory && trajectory && n_targets * pose > 0)
        GM_HIP_CHECK(hipMemsetAsync(d_trajectory, 0, (size_t)n_targets * pose * sizeof(float), hs));
    if (n == 0) return GM_OK;
    // a step's own messages name the step entry point this sweep is the loop of
    const char* step_who = (d_records || grads) ? "gm_rollout_step_backward_train" : "gm_rollout_step_backward";
    const float* g_after = d_final;
    for (int64_t t = steps - 1; t >= 0; --t) {
        // gm_rollout's rule: step t is driven by pose t, steps past the trajectory keep the rigid body in place (no target)
        const bool scripted = trajectory && t < n_targets && n_rigid > 0;
        float* g_before = t == 0 ? d_obs0 : w.g[t & 1];
        // grads: every step accumulates into the same buffers, so step steps - 1 adds first and step 0 last (a fixed order)
        int rc = step_backward(m, tensors, n_tensors, windows + (size_t)t * window, n, fd, K, rigid_rank,
                               scripted ? trajectory + (size_t)t * pose : nullptr, g_after, d_records ? d_records + (size_t)t * record : nullptr,
                               grads, g_before, scripted && d_trajectory ? d_trajectory + (size_t)t * pose : nullptr, nullptr, w.step,
                               w.step_bytes, stream, step_who, R);
        if (rc != GM_OK) return rc;
        g_after = g_before;
    }
    if (steps == 0 && d_obs0 != d_final) GM_HIP_CHECK(hipMemcpyAsync(d_obs0, d_final, window * sizeof(float), hipMemcpyDeviceToDevice, hs));
    return GM_OK;
}

int gm_rollout_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* windows, int64_t n,
                        const gm_feature_desc* fd, int K, const int32_t* rigid_rank, const float* trajectory, int64_t n_targets,
                        int64_t n_rigid, int64_t steps, const float* d_final, float* d_obs0, float* d_trajectory, void* ws, size_t ws_bytes,
                        void* stream) {
    return sweep_backward(m, tensors, n_tensors, windows, n, fd, K, rigid_rank, trajectory, n_targets, n_rigid, steps, d_final, nullptr,
                          nullptr, d_obs0, d_trajectory, ws, ws_bytes, stream, __func__);
}

int gm_rollout_backward_train(const gm_model* m, const float* const* tensors, int n_tensors, const float* windows, int64_t n,
                              const gm_feature_desc* fd, int K, const int32_t* rigid_rank, const float* trajectory, int64_t n_targets,
                              int64_t n_rigid, int64_t steps, const float* d_final, const float* d_records, float* const* grads,
                              float* d_obs0, float* d_trajectory, void* ws, size_t ws_bytes, void* stream) {
    return sweep_backward(m, tensors, n_tensors, windows, n, fd, K, rigid_rank, trajectory, n_targets, n_rigid, steps, d_final, d_records,
                          grads, d_obs0, d_trajectory, ws, ws_bytes, stream, __func__);
}

// The two training sweeps on graphs of any sizes (the table as in gm_radius_graph_build_ragged, fd->nodes_per_graph == 0): still one
// edge-count read per step, for the whole batch.  d_record / d_records and grads both NULL: the plain vector-Jacobian product.
int gm_rollout_step_backward_train_ragged(const gm_model* m, const float* const* tensors, int n_tensors, const float* obs_before,
                                          const int64_t* graph_offsets_host, int64_t n_graphs, const gm_feature_desc* fd, int K,
                                          const int32_t* rigid_rank, const float* rigid_target, const float* d_obs_after, const float* d_record,
                                          float* const* grads, float* d_obs_before, float* d_rigid_target, int64_t* n_edges_host, void* ws,
                                          size_t ws_bytes, void* stream) {
    gm::RaggedOffsets R;
    const int rc = gm::ragged_scene_table(__func__, fd, graph_offsets_host, n_graphs, K, ws, &R);
    if (rc != GM_OK) return rc;
    return step_backward(m, tensors, n_tensors, obs_before, R.off[R.n_graphs], fd, K, rigid_rank, rigid_target, d_obs_after, d_record, grads,
                         d_obs_before, d_rigid_target, n_edges_host, ws, ws_bytes, stream, __func__, &R);
}

int gm_rollout_backward_train_ragged(const gm_model* m, const float* const* tensors, int n_tensors, const float* windows,
                                     const int64_t* graph_offsets_host, int64_t n_graphs, const gm_feature_desc* fd, int K,
                                     const int32_t* rigid_rank, const float* trajectory, int64_t n_targets, int64_t n_rigid, int64_t steps,
                                     const float* d_final, const float* d_records, float* const* grads, float* d_obs0, float* d_trajectory,
                                     void* ws, size_t ws_bytes, void* stream) {
    gm::RaggedOffsets R;
    const int rc = gm::ragged_scene_table(__func__, fd, graph_offsets_host, n_graphs, K, ws, &R);
    if (rc != GM_OK) return rc;
    return sweep_backward(m, tensors, n_tensors, windows, R.off[R.n_graphs], fd, K, rigid_rank, trajectory, n_targets, n_rigid, steps, d_final,
                          d_records, grads, d_obs0, d_trajectory, ws, ws_bytes, stream, __func__, &R);
}

}  // extern "C"
