/*
 * gnn_manip_hip.h -- C ABI of libgnnmanip_hip.so: the MI355X (gfx950) rollout engine for
 * gnn-manip's encode-process-decode particle simulator.
 *
 * The reference (dblanm/gnn-manip) is pure Python and has no FFI of its own; its boundary is
 * the duck-typed call surface listed in SURVEY.md section 8b.  Every entry point below names
 * the reference function it replaces (paths relative to the reference checkout).  The Python
 * host layer in gnn_manip_amd/ binds these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is DEVICE memory unless the name ends
 *     in _host; the caller (PyTorch) owns every buffer and every workspace;
 *   - nothing is allocated per call; gm_model_create() allocates the packed weight image once;
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns without
 *     synchronising, unless documented otherwise;
 *   - return value: GM_OK (0) or a negative gm_status; gm_last_error() returns a thread-local
 *     message for the last failure.  Nothing throws or aborts across this boundary.
 *   - threading / streams: the stateless entry points are re-entrant.  A gm_model handle is NOT: it packs its inference
 *     operand images lazily, on the stream of the first inference call after gm_model_create / gm_model_update, so one
 *     handle is used from one thread and its update and inference calls go to ONE stream (or the caller orders the
 *     streams itself); use one handle per thread / stream otherwise (the reference's callers are single-threaded on one
 *     stream: rollout_utils.py:97-102, train_dyn.py:45-72).
 */
#ifndef GNN_MANIP_HIP_H
#define GNN_MANIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gm_status {
    GM_OK = 0,
    GM_ERR_INVALID_ARGUMENT = -1,
    GM_ERR_UNSUPPORTED = -2,   /* e.g. hidden size the kernels are not instantiated for */
    GM_ERR_HIP = -3,           /* a HIP runtime call failed */
    GM_ERR_WORKSPACE = -4,     /* workspace too small */
    GM_ERR_DATA = -5           /* device-side data error (non-finite position, bad index) */
} gm_status;

typedef struct gm_model gm_model; /* opaque */

const char* gm_last_error(void);
int gm_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Radius graph.   Replaces get_connectivity(pos_nodes, conn_r, max_neighbours)
 *                 gnn_manip/utils/utils.py:64-93  (sklearn KDTree.query_radius semantics:
 *                 float64 squared distance, d2 <= r*r, ascending distance, first max_nb kept,
 *                 ties broken on the smaller index).
 *                 max_neighbours: 1 .. 160 (the general kernel's candidate lists live in LDS), else GM_ERR_UNSUPPORTED;
 *                 a batch whose n_nodes is not a multiple of nodes_per_graph: GM_ERR_INVALID_ARGUMENT.
 * ------------------------------------------------------------------------------------------ */
size_t gm_graph_workspace_bytes(int64_t n_nodes, int max_neighbours);

/* Build per-query neighbour lists into the workspace.  pos points at x of node 0; node i is at
 * pos + i*pos_stride (floats), so the xyz columns of a [N, D] state row can be passed directly. */
int gm_radius_graph_build(const float* pos, int64_t pos_stride, int64_t n_nodes, double conn_r,
                          int max_neighbours, void* graph_ws, size_t graph_ws_bytes, void* stream);

/* Same for a batch of equal-sized graphs stored back to back (node i belongs to graph i / nodes_per_graph):
 * no edge crosses graphs -- the batch of collate_utils.py:68-87 (edge indices offset by N*i, :76). */
int gm_radius_graph_build_batched(const float* pos, int64_t pos_stride, int64_t n_nodes, int64_t nodes_per_graph,
                                  double conn_r, int max_neighbours, void* graph_ws, size_t graph_ws_bytes, void* stream);

/* Same for n_graphs graphs of ANY sizes stored back to back (an addition to ABI 7): graph g owns rows
 * [graph_offsets_host[g], graph_offsets_host[g + 1]), n_nodes = graph_offsets_host[n_graphs] -- the batch torch_geometric's
 * loader collates (edge indices offset by the running node count).  The result is gm_radius_graph_build's on each graph alone
 * with the graph's row offset on its indices: the edge list equals the concatenation of the per-graph lists bit for bit, ties
 * included (a graph's rows keep their order, so (d2, index) ranks the same), and with all sizes equal it is
 * gm_radius_graph_build_batched's.  graph_offsets_host is a HOST array; the offsets travel by value in the kernel arguments
 * (no copy, no allocation, no host synchronisation), which is why a build takes at most GM_RAGGED_MAX_GRAPHS graphs.  Refused
 * with GM_ERR_INVALID_ARGUMENT and a "gm_radius_graph_build_ragged: ..." message, before any device call: n_graphs outside
 * 1..GM_RAGGED_MAX_GRAPHS, graph_offsets_host[0] != 0, a graph of fewer than 1 row, a null pointer, n_nodes >= 2^30,
 * max_neighbours outside 1..160, n_nodes * max_neighbours >= 2^31, conn_r <= 0, pos_stride < 3, a workspace below
 * gm_graph_ragged_workspace_bytes (which is 0 for such arguments).
 * The workspace has the layout of gm_graph_workspace_bytes(n_nodes, max_neighbours) -- nothing but the kernels reads the offsets
 * -- so gm_radius_graph_num_edges and gm_radius_graph_edges(graph_ws, n_nodes, max_neighbours, ...) read it as they read any
 * other.  Its device header reports nodes_per_graph = n_nodes: gm_csr_from_graph(_flow) on a ragged workspace lays out its
 * block tables as for ONE graph, which is exactly what a collated edge_index gets from gm_csr_from_edge_index. */
#define GM_RAGGED_MAX_GRAPHS 64 /* == GM_TRAIN_BATCH_MAX */
size_t gm_graph_ragged_workspace_bytes(int64_t n_nodes, int64_t n_graphs, int max_neighbours);
int gm_radius_graph_build_ragged(const float* pos, int64_t pos_stride, const int64_t* graph_offsets_host /*[n_graphs+1]*/,
                                 int64_t n_graphs, double conn_r, int max_neighbours, void* graph_ws, size_t graph_ws_bytes,
                                 void* stream);

/* Synchronises `stream`; returns E and the device error flags of the last build. */
int gm_radius_graph_num_edges(const void* graph_ws, int64_t* n_edges_host, void* stream);

/* Emit the reference-ordered edge list: grouped by sender (= query node) ascending, distance
 * ascending inside a group.  senders/receivers: int64[capacity], capacity >= E. */
int gm_radius_graph_edges(const void* graph_ws, int64_t n_nodes, int max_neighbours,
                          int64_t* senders, int64_t* receivers, int64_t capacity, void* stream);

/* Neighbour census (an addition to ABI 7; the reference has no counterpart: get_connectivity, utils.py:64-93, keeps the nearest
 * max_neighbours of a query and drops the rest without a word).  counts_device[i] = the number of nodes gm_radius_graph_build
 * would list for query i if it had no cap: the nodes j (i itself among them) with float64 d2 <= conn_r * conn_r, d2 accumulated
 * x -> y -> z with separately rounded products and sums -- the build's own predicate, evaluated by the build's own code over the
 * build's own cell list.  Hence min(counts[i], max_neighbours) is the out-degree the build gives node i, and counts[i] >
 * max_neighbours says that row i is truncated at that cap.  Counts only: no candidate lists, so no 160 limit.  A row with a
 * non-finite coordinate counts 0 and is counted by nobody.  One graph; pos / pos_stride as in gm_radius_graph_build.  The
 * workspace has the layout of gm_graph_workspace_bytes(n_nodes, 1), and gm_neighbour_census_workspace_bytes returns its size (0
 * for n_nodes outside 1 .. 2^30 - 1); it is written before it is read.  No host synchronisation.  Refused with
 * GM_ERR_INVALID_ARGUMENT and a "gm_neighbour_census: ..." message, before any device call: a null pointer, n_nodes outside
 * 1 .. 2^30 - 1, conn_r <= 0, pos_stride < 3, a workspace below the query. */
size_t gm_neighbour_census_workspace_bytes(int64_t n_nodes);
int gm_neighbour_census(const float* pos, int64_t pos_stride, int64_t n_nodes, double conn_r, int32_t* counts_device /*[N]*/,
                        void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Destination-sorted edge structure (the engine's internal edge order).
 * Aggregation index i = edge_index[1], source j = edge_index[0] (PyG source_to_target, see
 * DESIGN.md).  Edges are grouped by i; inside a group ascending original edge id (stable).
 * ------------------------------------------------------------------------------------------ */
size_t gm_csr_workspace_bytes(int64_t n_nodes, int64_t edge_capacity);
int gm_csr_from_graph(const void* graph_ws, int64_t n_nodes, int max_neighbours,
                      void* csr_ws, size_t csr_ws_bytes, void* stream);
int gm_csr_from_edge_index(const int64_t* edge_index /* [2,E] row-major */, int64_t n_nodes,
                           int64_t n_edges, void* csr_ws, size_t csr_ws_bytes, void* stream);
/* The same with the aggregation index chosen by `flow` (gm_model_desc.flow): 0 = edge_index[1] (default), 1 = edge_index[0]. */
int gm_csr_from_graph_flow(const void* graph_ws, int64_t n_nodes, int max_neighbours, int flow,
                           void* csr_ws, size_t csr_ws_bytes, void* stream);
int gm_csr_from_edge_index_flow(const int64_t* edge_index, int64_t n_nodes, int64_t n_edges, int flow,
                                void* csr_ws, size_t csr_ws_bytes, void* stream);
/* Synchronises; copies E and error flags to the host. */
int gm_csr_num_edges(const void* csr_ws, int64_t* n_edges_host, void* stream);
/* The same verdict from a HOST copy of the workspace's first 16 bytes (its header: n_edges, error flags, flow, pad) -- for callers
 * that copy the header asynchronously behind their work and poll for it instead of synchronising.  No device access.  The tape of
 * gm_epd_forward_train and of gm_interaction_network_forward_train begins with the csr workspace of that forward: the same
 * 16 bytes tell whether its edge_index held an entry outside [0, n_nodes) (such edges are left out). */
int gm_csr_header_status(const int32_t* header_host /*[4]*/, int64_t* n_edges_host /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Features.
 * gm_edge_features      replaces get_edges_displacement   gnn_manip/utils/utils.py:43-61
 *                       out[e] = [(p[s]-p[r])/conn_r, ||.||], reference edge order.
 * gm_edge_features_csr  same values in the destination-sorted order of a csr workspace (sender = edge_index[0] whatever
 *                       `flow` the workspace was built with: the header records it).
 * gm_node_features      replaces GraphBoundedMultimaterial(Control).compute_nodes
 *                       gnn_manip/utils/collate_utils.py:195-208,217-232 (+ get_nodes_vel,
 *                       utils.py:27-40).  obs: [k, N, D] float32 row-major.
 * ------------------------------------------------------------------------------------------ */
int gm_edge_features(const float* pos, int64_t pos_stride, const int64_t* senders,
                     const int64_t* receivers, int64_t n_edges, float conn_r, float* out /*[E,4]*/,
                     void* stream);
int gm_edge_features_csr(const float* pos, int64_t pos_stride, const void* csr_ws, int64_t n_nodes,
                         int64_t edge_capacity, float conn_r, float* out /*[cap,4]*/, void* stream);

typedef struct gm_feature_desc {
    double conn_r;          /* connectivity radius as the Python float the reference passes: the radius
                               test runs in float64 on it, float32 feature divisions on (float)conn_r */
    int32_t k_steps;        /* frames in the window (6) */
    int32_t data_dim;       /* D: columns per particle row (8 with control, 5 without) */
    int32_t cart_col;       /* first of the 3 contiguous position columns (2) */
    int32_t material_col;   /* (1) */
    int32_t control_col;    /* first of the 3 contiguous control columns (5), or -1: no control */
    int32_t nodes_per_graph; /* rollout of a batch of equal-sized scenes stored back to back (candidates); 0: one scene */
    float vel_mean[3], vel_std[3];
    float acc_mean[3], acc_std[3];
    float lower_bounds[3], upper_bounds[3];
} gm_feature_desc;

int gm_node_features(const float* obs, int64_t n_nodes, const gm_feature_desc* desc,
                     float* out /* [N, 3*(k-1)+6+1(+3)] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Integrator + rollout state update.
 * gm_integrate     replaces get_position_from_prediction  gnn_manip/utils/rollout_utils.py:145-158
 * gm_state_pre     replaces rollout_utils.py:40-47 == traj_utils.py:126-134: control columns of the
 *                  rigid rows (material == 1) of the last frame <- rigid_target - current xyz.
 *                  A descriptor without control columns (control_col < 0) has nothing to overwrite:
 *                  called on its own, gm_state_pre rejects it (GM_ERR_INVALID_ARGUMENT); gm_rollout_step
 *                  and gm_rollout skip the overwrite, and gm_rollout's record is then the last frame
 *                  as it stands.
 * gm_state_post    replaces rollout_utils.py:53-61 == traj_utils.py:146-152: window shift, write
 *                  p_{t+1}, overwrite rigid rows' xyz with the scripted pose.
 * rigid_target: [N_rigid,3] poses in rigid-row order; rigid_rank: int32[N] = rank of row among
 * rigid rows (or -1), built once per scene by gm_rigid_rank.
 * gm_rigid_transform replaces compute_particles_tmatrix    gnn_manip/utils/traj_utils.py:167-194
 * ------------------------------------------------------------------------------------------ */
int gm_integrate(const float* pred_acc /*[N,3]*/, const float* obs, int64_t n_nodes,
                 const gm_feature_desc* desc, float* next_pos /*[N,3]*/, void* stream);
int gm_rigid_rank(const float* obs, int64_t n_nodes, const gm_feature_desc* desc, int32_t* rigid_rank,
                  int32_t* n_rigid_dev, void* stream);
int gm_state_pre(float* obs, int64_t n_nodes, const gm_feature_desc* desc, const int32_t* rigid_rank,
                 const float* rigid_target /* or NULL: control <- current xyz (traj_utils.py:131) */,
                 void* stream);
int gm_state_post(float* obs, int64_t n_nodes, const gm_feature_desc* desc, const float* next_pos,
                  const int32_t* rigid_rank, const float* rigid_target /* or NULL */, void* stream);
int gm_rigid_transform(const float* rigid_init /*[Nr,3]*/, int64_t n_rigid, const float* rot_cs_ty
                       /* [T,3] host-computed (cos, sin, ty_init[1]+translation) float32 */,
                       int64_t n_steps, const float ty_init[3], float* out /*[T,Nr,3]*/, void* stream);

/* Transpose of gm_rigid_transform with respect to its per-step rows: d_rot_cs_ty [T,3] from d_out [T,Nr,3].  With
 * i1 = ty_init[1] - init[i][2], i2 = ty_init[2] - init[i][1] and g = d_out[t][i]:
 *   d_cos = sum_i (g[2] i1 + g[1] i2),  d_sin = sum_i (g[1] i1 - g[2] i2),  d_ty = sum_i g[2].
 * The transform is linear in its rows, so rot_cs_ty itself is not read (it may be NULL).  One workgroup per step, the sum over the
 * rigid particles in a fixed order carried in float64 and rounded once: no float atomics, the same call twice gives the same bits.
 * The output is written in full; n_rigid = 0 writes zeros. */
int gm_rigid_transform_backward(const float* rigid_init /*[Nr,3]*/, int64_t n_rigid, const float* rot_cs_ty /*[T,3] or NULL*/,
                                int64_t n_steps, const float ty_init[3], const float* d_out /*[T,Nr,3]*/,
                                float* d_rot_cs_ty /*[T,3]*/, void* stream);

/* Backward of the per-step functions (a differentiable rollout step).  Every output is WRITTEN IN FULL, not accumulated, by one
 * thread per row in a fixed order: no float atomics, the same call twice gives the same bits; no host synchronisation.
 * nodes_per_graph of the descriptor plays no part.
 * gm_edge_features_backward: d_pos [N,3] (dense rows) from d_out [E,4].  With d = (p_s - p_r) / r and g = d_out[e] the edge gives
 *   (g[0:3] + g[3] d / |d|) / r to its sender and the negative to its receiver; where |d| = 0 (the self edge every node has) the
 *   norm's term is 0, the subgradient torch.norm uses.  A node sums the edges it sends, then subtracts the edges it receives, each
 *   group in ascending edge id (segmented sums over the destination sorts with flow 1 and flow 0, built in `ws`).  Any edge list
 *   works: hubs, duplicates, isolated nodes (zero rows), any order; an edge with an index outside [0, N) contributes nothing.
 * gm_node_features_backward: d_obs [k,N,D] from d_out [N,F], the transpose of gm_node_features.  Velocity columns give
 *   +-1/vel_std to the two frames of their difference; the six boundary columns give +-1/conn_r to the last frame where the
 *   UNCLAMPED value lies in [-1, 1] (torch.clamp's rule: the ends included) and nothing elsewhere; the material column gives
 *   nothing; control columns give 1/vel_std to the last frame's control columns.  Columns no feature reads are zero.
 * gm_integrate_backward: d_pred [N,3] = g acc_std and d_obs [k,N,D]: +2g on frame k-1, -g on frame k-2 in the position columns,
 *   zero everywhere else, g = d_next_pos [N,3]. */
size_t gm_edge_features_backward_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int gm_edge_features_backward(const float* pos, int64_t pos_stride, const int64_t* senders, const int64_t* receivers,
                              int64_t n_nodes, int64_t n_edges, float conn_r, const float* d_out /*[E,4]*/,
                              float* d_pos /*[N,3]*/, void* ws, size_t ws_bytes, void* stream);
int gm_node_features_backward(const float* obs, int64_t n_nodes, const gm_feature_desc* desc,
                              const float* d_out /*[N,F]*/, float* d_obs /*[k,N,D]*/, void* stream);
int gm_integrate_backward(const float* d_next_pos /*[N,3]*/, int64_t n_nodes, const gm_feature_desc* desc,
                          float* d_pred /*[N,3]*/, float* d_obs /*[k,N,D]*/, void* stream);

/* Transposes of the two state updates (the reverse sweep of a rollout): the gradient with respect to the window BEFORE the update,
 * d_obs_before [k,N,D], from the gradient with respect to the window after it, d_obs_after [k,N,D] (another buffer).  Both are
 * linear maps of the window, so no state is read: has_target says whether the update was given a rigid_target.  Outputs are
 * written in full by one thread per particle row; d_rigid_target [N_rigid,3] may be NULL, and without a target it is written as
 * zeros.  Every element is a copy, a negation or a sum of two float32 terms: no float atomics, the same bits every time.
 * gm_state_pre_backward: a rigid row's control columns were overwritten with (target - xyz), or xyz without a target: their old
 *   values get zero, xyz gets its own gradient MINUS (with a target) or PLUS (without) the control columns' gradient, and
 *   d_rigid_target gets the control columns' gradient.  Every other element is copied.  A descriptor without control columns is
 *   refused, as by gm_state_pre.
 * gm_state_post_backward: frame 0 gets zero (it fell out of the window), frame t gets frame t - 1 of d_obs_after, and the last
 *   frame gets frame k - 2 PLUS frame k - 1 of d_obs_after in the columns it passed on: every column but xyz for a non-rigid row,
 *   whose xyz gradient is d_next_pos [N,3]; the whole row for a rigid row without a target (zero d_next_pos); every column but
 *   xyz for a rigid row with one, whose xyz gradient is d_rigid_target.  rigid_rank NULL: no rigid rows, d_rigid_target untouched. */
int gm_state_pre_backward(const float* d_obs_after, int64_t n_nodes, const gm_feature_desc* desc, const int32_t* rigid_rank,
                          int has_target, float* d_obs_before, float* d_rigid_target /* [N_rigid,3] or NULL */, void* stream);
int gm_state_post_backward(const float* d_obs_after, int64_t n_nodes, const gm_feature_desc* desc,
                           const int32_t* rigid_rank /* or NULL */, int has_target, float* d_obs_before, float* d_next_pos /*[N,3]*/,
                           float* d_rigid_target /* [N_rigid,3] or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Model.  Replaces EncProcDecGNN.__init__/_build_mlp + load_state_dict
 *         gnn_manip/models/epd_gnn.py:13-49,72-84 ; rollout_utils.py:137-139.
 * tensors_host_or_dev: the model's parameters in state_dict order (encoder.phi_edge.*,
 * encoder.phi_node.*, processor.k.phi_edge.*, processor.k.phi_node.*, decoder.*; inside an MLP:
 * Linear weight [out,in] row-major, bias, ..., LayerNorm weight, bias).  They are copied and
 * repacked into the MFMA operand image; the caller's tensors are not referenced afterwards.
 *
 * Numeric domain.  The reference computes every Linear in float32.  The inference kernels form the same float32 products
 * on the fp16 matrix pipe: each operand is a pair of fp16 numbers (22 significant bits), three exact partial products per
 * multiply, float32 accumulation.  An fp16 pair represents |x| < 65504 and keeps full precision down to 2^-3, so the
 * kernels hold every operand at a power-of-two scale chosen from the weights (nothing is rounded by it): hidden
 * activations ride at an rms near 2^4 (4096-fold headroom) whatever the scale of the weights -- scaling (W_l, b_l) by s and W_(l+1) by 1/s
 * changes no operand bit -- and each raw node / edge feature row is scaled by its own maximum, so features of any
 * magnitude (1e-30 .. 1e30) are as accurate as in float32.  Latents (h, e, agg: LayerNorm outputs and their sums) enter at
 * their natural magnitude: fine from ~2^-8 to 65504.  A value outside the representable range is never clamped: the
 * kernel that meets it sets a flag in the CSR header of that forward and gm_csr_num_edges / gm_rollout_status return
 * GM_ERR_DATA ("fp16 split range exceeded"); the outputs of that forward are then invalid.  A float32 evaluation would
 * also stay finite for magnitudes up to 3.4e38: that part of its domain is not covered.
 *
 * Numeric domain of the fp16 mode (gm_model_set_precision(m, GM_PRECISION_F16); inference entry points only).  Every Linear
 * multiplies its weights and its inputs ROUNDED TO fp16 (round to nearest even; 11 significant bits) and accumulates the exact
 * products in float32: one matrix instruction per multiply instead of three.  Everything else is as above and stays float32: the
 * power-of-two scales, the biases, P and Q as initial accumulators, LayerNorm, residuals, the scatter-add and its summation order,
 * the latents in memory.  An operand is rounded AT its scale: the packed weights t W, the hidden activations U x, a raw feature row
 * times its own power of two.  That is the rounding of the unscaled value only while both are fp16 normals (>= 2^-14; below, fp16's
 * spacing is 2^-24 whatever the value).  Rows or first-Linear weights of magnitude 1e-4 keep all 11 bits here and would lose them
 * rounded as they stand; an entry more than 2^20 below its row's maximum keeps about 31 - k bits at 2^-k of it.  The weight images are the same (the mode reads their hi halves), so the
 * switch needs no re-pack.  Expect a decoder output about 1e-3 of its largest element away from float64 after 10 message-passing
 * steps (float32: 1e-6): enough to rank rollout candidates, not for parity.  The range is the same: a value of magnitude >= 65520 in an
 * operand image becomes +-inf, the row check of every kernel counts +-inf like NaN, the same flag is raised (GM_ERR_DATA, "fp16 split
 * range exceeded") and the prediction of that forward comes out NaN, never a plausible finite number; a non-finite input row of
 * gm_graph_independent_forward comes out as a NaN row and leaves the other rows' bits alone.
 *
 * Numeric domain of the training entry points (gm_epd_forward_train / gm_epd_backward*, the *_forward_train / *_backward block
 * entry points).  They form the float32 products on the bf16 matrix pipe: every operand -- weight, activation, gradient -- is
 * split into three bf16 parts, which keep float32's whole exponent range, and accumulated in float32.  No operand is scaled and
 * no range is searched, so ANY finite float32 magnitude is supported, in the forward and in the backward (gradients of 1e-9 and
 * 1e+5 in one array included), and nothing is flagged or clamped.  A rescaling by a power of two is bit-exact: grad_out * 2^k
 * gives every gradient * 2^k; (W_l, b_l) * s with W_(l+1) / s, or features * c with the encoders' first weights / c, give the
 * same prediction bit for bit and the gradients of the rescaled tensors times the inverse factor (as long as no value leaves
 * float32's normal range).  A non-finite input feature or parameter gives NaN rows exactly where a float32 evaluation has them
 * -- the row itself, and the rows its edges carry it to -- and leaves every other row's bits alone (the chains' ReLU passes a
 * NaN on and records the unit as active, as relu / threshold_backward do); the loss and the parameter gradients of such a step
 * are non-finite as in float32.  tests/test_gpu_train_domain.py holds the kernels to this.
 * ------------------------------------------------------------------------------------------ */
typedef struct gm_model_desc {
    int32_t node_dim, edge_dim, out_dim;
    int32_t hidden_size;   /* 1 .. 256 (epd_gnn.py:13-14 takes any int); see gm_padded_hidden_size */
    int32_t num_layers;    /* >= 2: hidden layers per MLP (epd_gnn.py:26) */
    int32_t m_steps;       /* >= 1 */
    float ln_eps;          /* 1e-5; the eps of every LayerNorm of the model.  Must be > 0: 0, negative and NaN are refused */
    /* Convention of the torch_graphnet.InteractionNetwork block, whose source is absent from the reference tree
     * (.gitmodules:1-3).  All zero = the default of DESIGN.md section 2 (BASELINE.json north_star wording, PyG
     * source_to_target).  Exposed so that a checkpoint trained with another convention can be matched. */
    int32_t flow;          /* 0: j = edge_index[0], aggregation index i = edge_index[1]; 1: i = edge_index[0], j = edge_index[1] */
    int32_t col_i, col_j, col_e; /* column block (0, 1, 2) of phi_e's first Linear that multiplies h_i, h_j, e; all zero = (0, 1, 2) */
    int32_t node_agg_first; /* 0: phi_v(cat[h, agg]); 1: phi_v(cat[agg, h]) */
} gm_model_desc;

/* The kernels are instantiated for the widths 64, 128 and 256; a model of another hidden size h <= 256 runs
 * zero-padded at the next of them: weights, biases and LayerNorm vectors are padded with zeros when they are packed, LayerNorm
 * statistics are taken over the h features that exist (the Linear in front of a LayerNorm is packed centred over its outputs,
 * so the statistics are a mean square and zero padding adds nothing), the padded features stay exactly zero.  Returns that width (0:
 * unsupported).  It is the ROW STRIDE of every latent array that crosses this interface: h / e of
 * gm_graph_independent_forward and gm_interaction_network_forward (inputs zero-padded by the caller, outputs padded with
 * zeros); gm_epd_forward and the rollout entry points have no latent arguments.  Training entry points: hidden 64 / 128 / 256. */
int gm_padded_hidden_size(int hidden_size);

int gm_model_num_tensors(const gm_model_desc* desc);
int gm_model_create(const gm_model_desc* desc, const float* const* tensors, int n_tensors,
                    int tensors_on_device, void* stream, gm_model** out);
/* create / update copy the tensors into the model (stream-ordered for device tensors; host tensors are read before the call
 * returns): the caller's buffers are not referenced afterwards.  The operand images of the training kernels are packed by the
 * call itself; those of the inference kernels by the first inference call that follows (on that call's stream) -- a training
 * loop, which updates the weights every step, never pays for them. */
int gm_model_update(gm_model* m, const float* const* tensors, int n_tensors, int tensors_on_device,
                    void* stream);
void gm_model_destroy(gm_model* m);

/* Processor edge kernel of THIS model (no reference counterpart; diagnostics / A-B measurements).  0 = automatic
 * (the systolic fp16 x 3 kernel for hidden 128 / num_layers 2 in the fused forward, else the
 * streamed one); 5 = systolic fp16 x 3 where it applies, else 6; 6 = streamed fp16 x 3 (hmlp.hip; every MLP of the
 * model, any supported size); 7 = as 5, and the processor NODE MLPs in the systolic form too (node kernel + projection kernel,
 * hedge.hip) whatever the graph's size -- 0 takes those for graphs of 49152 nodes or more (one graph of a batch counts, not the batch), where a workgroup has blocks enough to pipeline.  1..4 were round 1's fp32 / bf16 x 6 kernels: removed from the library in round 5
 * (GM_ERR_UNSUPPORTED).  No environment variable is read: the choice belongs to the handle. */
int gm_model_set_edge_kernel(gm_model* m, int choice);
/* The systolic node path of THIS model (diagnostics / A-B measurements, like the choice above): on != 0 (the default) runs a
 * processor step's node MLP and the next step's projections as one launch (sys_node_proj_kernel), 0 as the two launches it is
 * made of.  The results are the same bit for bit. */
int gm_model_set_node_fusion(gm_model* m, int on);
/* Arithmetic of the INFERENCE kernels of THIS model (see "Numeric domain" above): GM_PRECISION_F32 (the default: three partial
 * products per multiply, float32 accuracy) or GM_PRECISION_F16 (one: weights and inputs of every Linear rounded to fp16, float32
 * accumulation).  It covers gm_epd_forward, gm_graph_independent_forward, gm_interaction_network_forward, gm_rollout_step and
 * gm_rollout; which kernels a forward takes (gm_model_set_edge_kernel) does not depend on it.  It does NOT touch the training
 * entry points (*_train, every backward), the Sinkhorn loss or the graph build: gm_rollout_step_backward / gm_rollout_backward of a
 * GM_PRECISION_F16 model re-run and differentiate the FLOAT32 step at the states the fp16 forward visited.  The choice belongs to the
 * handle (no process-global state, no environment variable), takes effect at the next call and may change between any two calls
 * (the caller orders it against calls in flight on other threads, like a weight update).  A null model or any other value:
 * GM_ERR_INVALID_ARGUMENT. */
enum { GM_PRECISION_F32 = 0, GM_PRECISION_F16 = 1 };
int gm_model_set_precision(gm_model* m, int precision);

size_t gm_forward_workspace_bytes(const gm_model_desc* desc, int64_t n_nodes, int64_t edge_capacity);
/* workspace of gm_interaction_network_forward (the latent edge arrays are the caller's) */
size_t gm_block_workspace_bytes(const gm_model_desc* desc, int64_t n_nodes, int64_t edge_capacity);

/* EncProcDecGNN.forward(nodes, edge_attr, edge_index)   epd_gnn.py:86-105.
 * edge_attr is in the CALLER's edge order; the csr workspace (built from the same edge_index or
 * from the radius graph) carries the permutation.  edge_attr_is_csr_order != 0 says edge_attr is
 * already destination-sorted (rollout path). */
int gm_epd_forward(const gm_model* m, const float* nodes /*[N,node_dim]*/, int64_t n_nodes,
                   const float* edge_attr /*[E,edge_dim]*/, int edge_attr_is_csr_order,
                   const void* csr_ws, int64_t edge_capacity, float* out /*[N,out_dim]*/,
                   void* fwd_ws, size_t fwd_ws_bytes, void* stream);

/* torch_graphnet.GraphIndependent call site epd_gnn.py:88 -- (phi_node(x), phi_edge(e)).
 * torch_graphnet.InteractionNetwork call site epd_gnn.py:101 -- (h', e'), no residual.
 * `block` = -1: encoder; 0..m_steps-1: processor block.  Outputs in the caller's edge order.
 * Range violations of the fp16 split (see "Numeric domain" above): gm_interaction_network_forward flags them in the header of
 * its csr workspace like the fused forward (gm_csr_num_edges returns GM_ERR_DATA).  gm_graph_independent_forward has no such
 * header: there a violating row -- a non-finite input feature, or a range violation further on -- comes out as NaN in every
 * feature (the kernels carry a per-row poison term from every Linear's accumulators into the LayerNorm), which is how the caller
 * sees it; the other rows are unaffected. */
int gm_graph_independent_forward(const gm_model* m, const float* x, int64_t n_nodes, const float* edge_attr,
                                 int64_t n_edges, float* h_out, float* e_out, void* stream);
int gm_interaction_network_forward(const gm_model* m, int block, const float* h, int64_t n_nodes,
                                   const float* e, const void* csr_ws, int64_t edge_capacity,
                                   float* h_out, float* e_out, void* fwd_ws, size_t fwd_ws_bytes,
                                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Training: what examples/train_dyn.py:45-72 does with the model --
 * `model.forward(x, edge_attr, edge_index)` under autograd, `loss.backward()`, optimiser step.
 * gm_epd_forward_train == EncProcDecGNN.forward (epd_gnn.py:86-105) that also records the activation
 * tape in the caller's buffer (gm_train_tape_bytes); edge_index is the caller's int64 [2, E]
 * (j = row 0, aggregation index i = row 1).  gm_epd_backward consumes the tape and ACCUMULATES the
 * gradient of every parameter into grads[t] (same order and shapes as the `tensors` of
 * gm_model_create; the caller zeroes them), given grad_out = dLoss/d(out) [N, out_dim].  `tensors`
 * are the parameter values the forward ran with (device pointers).  Inputs x / edge_attr get no
 * gradient here (they are data in train_dyn.py; gm_epd_backward_inputs returns them).  Weight gradients are reduced in a fixed order
 * (deterministic, like the bias and LayerNorm-parameter gradients: no atomics on the backward path). */
size_t gm_train_tape_bytes(const gm_model_desc* desc, int64_t n_nodes, int64_t n_edges);
size_t gm_train_backward_workspace_bytes(const gm_model_desc* desc, int64_t n_nodes, int64_t n_edges);
int gm_epd_forward_train(const gm_model* m, const float* nodes, int64_t n_nodes, const float* edge_attr,
                         const int64_t* edge_index, int64_t n_edges, float* out, void* tape,
                         size_t tape_bytes, void* stream);
int gm_epd_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* nodes,
                    const float* edge_attr, int64_t n_nodes, int64_t n_edges, const float* grad_out,
                    float* const* grads, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                    void* stream);

/* gm_epd_backward that also returns the gradient w.r.t. the model's inputs (a differentiable rollout step; a frozen model in a
 * planning loop): d_nodes [N, node_dim] and d_edge_attr [E, edge_dim] in the CALLER's edge order, either may be NULL, both NULL
 * is gm_epd_backward.  Both are written in full, not accumulated.  The parameter gradients are bit-equal to gm_epd_backward's:
 * the encoders' chains only run one product further (dX = dz1 W1) and store.  A forward whose edge_index was flagged returns
 * exactly zero input gradients, like its parameter gradients; the rows of edges the destination sort left out are zero.
 * gm_train_backward_inputs_workspace_bytes is this entry point's workspace query (the transposed W1 images of the two encoders
 * live in the encoders' slots of the backward workspace). */
size_t gm_train_backward_inputs_workspace_bytes(const gm_model_desc* desc, int64_t n_nodes, int64_t n_edges);
int gm_epd_backward_inputs(const gm_model* m, const float* const* tensors, int n_tensors, const float* nodes,
                           const float* edge_attr, int64_t n_nodes, int64_t n_edges, const float* grad_out,
                           float* const* grads, float* d_nodes /* [N, node_dim] or NULL */,
                           float* d_edge_attr /* [E, edge_dim], caller's edge order, or NULL */, void* tape,
                           size_t tape_bytes, void* ws, size_t ws_bytes, void* stream);

/* gm_epd_backward_inputs without the parameter gradients (weights are constants of a planning loop): no `grads` argument, and none
 * of the weight-gradient work is enqueued -- no dW products (those of the factorised W_i / W_j among them), no bias sums, no
 * LayerNorm-parameter partial sums or reductions (the chain kernels skip that part of their epilogue by a launch argument).  The dz
 * chains, the segment sums they need and the input tails are the same launches on the same operands, so d_nodes / d_edge_attr are
 * bit-equal to gm_epd_backward_inputs' for the same tape.  Workspace: gm_train_backward_inputs_workspace_bytes.  d_nodes and
 * d_edge_attr both NULL is GM_ERR_INVALID_ARGUMENT (there would be nothing to compute).  A flagged edge_index gives exactly zero
 * rows, as above. */
int gm_epd_backward_inputs_only(const gm_model* m, const float* const* tensors, int n_tensors, const float* nodes,
                                const float* edge_attr, int64_t n_nodes, int64_t n_edges, const float* grad_out,
                                float* d_nodes /* [N, node_dim] or NULL */,
                                float* d_edge_attr /* [E, edge_dim], caller's edge order, or NULL */, void* tape,
                                size_t tape_bytes, void* ws, size_t ws_bytes, void* stream);

/* The two standalone blocks under autograd -- the torch_graphnet surface the reference's own
 * EncProcDecGNN wiring calls (epd_gnn.py:30-33,42-45,88,101).  *_forward_train record a tape
 * (gm_block_tape_bytes; interaction_network = 0 for GraphIndependent, 1 for InteractionNetwork);
 * *_backward accumulate parameter gradients into grads[] (full-model tensor order, only the block's own
 * entries are touched) and, for the InteractionNetwork, return the input gradients dh_in [N,H] and
 * de_in [E,H] (caller's edge order); for the GraphIndependent the input gradients dx / dedge_attr are optional
 * (NULL at the reference's call site, where the inputs are data). */
size_t gm_block_tape_bytes(const gm_model_desc* desc, int interaction_network, int64_t n_nodes, int64_t n_edges);
size_t gm_block_backward_workspace_bytes(const gm_model_desc* desc, int64_t n_nodes, int64_t n_edges);
int gm_graph_independent_forward_train(const gm_model* m, const float* x, int64_t n_nodes, const float* edge_attr,
                                       int64_t n_edges, float* h_out, float* e_out, void* tape, size_t tape_bytes,
                                       void* stream);
int gm_graph_independent_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* x,
                                  const float* edge_attr, int64_t n_nodes, int64_t n_edges, const float* dh,
                                  const float* de, float* dx /*[N,node_dim] or NULL*/,
                                  float* dedge_attr /*[E,edge_dim] or NULL*/, float* const* grads, void* tape,
                                  size_t tape_bytes, void* ws, size_t ws_bytes, void* stream);
int gm_interaction_network_forward_train(const gm_model* m, int block, const float* h, int64_t n_nodes,
                                         const float* e, const int64_t* edge_index, int64_t n_edges, float* h_out,
                                         float* e_out, void* tape, size_t tape_bytes, void* stream);
int gm_interaction_network_backward(const gm_model* m, int block, const float* const* tensors, int n_tensors,
                                    const float* h, const float* e, int64_t n_nodes, int64_t n_edges,
                                    const float* dh_out, const float* de_out, float* dh_in, float* de_in,
                                    float* const* grads, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                                    void* stream);

/* Planner loss: geomloss.SamplesLoss(loss="sinkhorn", p=2, blur) between the final
 * particle cloud x [N,3] and the desired one y [M,3], uniform weights -- traj_utils.py:69,279.  Debiased
 * Sinkhorn divergence, cost |x-y|^2/2, epsilon-scaling with ratio `scaling` (geomloss default 0.5) from the
 * bounding-box diameter down to blur.  Writes one float to loss_device.  One host synchronisation (the
 * diameter fixes the length of the epsilon schedule). */
size_t gm_sinkhorn_workspace_bytes(int64_t n, int64_t m);
int gm_sinkhorn_divergence(const float* x, int64_t n, const float* y, int64_t m, float blur, float scaling,
                           float* loss_device, void* ws, size_t ws_bytes, void* stream);
/* The losses of a whole block of candidates in one launch sequence (ABI 7) -- the loop of traj_utils.py:279 over the
 * candidates of a CMA-ES generation (traj_utils.py:247-259), `batch` clouds x [batch, N, 3] against y [M, 3]
 * (y_shared != 0: the desired cloud of the planner) or [batch, M, 3].  Pair b gets the epsilon schedule a call of
 * gm_sinkhorn_divergence on it alone would have used (its own bounding-box diameter), and loss_device[b] equals
 * that call's result bit for bit; pairs with shorter schedules idle through the tail of the longest one.
 * diameter > 0: geomloss's `diameter=` keyword -- every pair takes it and NO host synchronisation happens;
 * diameter <= 0 (geomloss default): one host synchronisation per call (the longest schedule = the launch count). */
size_t gm_sinkhorn_batched_workspace_bytes(int64_t batch, int64_t n, int64_t m);
int gm_sinkhorn_divergence_batched(const float* x, int64_t batch, int64_t n, const float* y, int64_t m, int y_shared,
                                   float blur, float scaling, float diameter, float* loss_device /*[batch]*/, void* ws,
                                   size_t ws_bytes, void* stream);
/* Gradient of gm_sinkhorn_divergence_batched (differentiable SamplesLoss): dx [batch, N, 3] and dy ([batch, M, 3], or [M, 3]
 * when y_shared: the sum over the pairs, in pair order) of sum_b grad_loss[b] * loss_b.  Either output may be NULL; both are
 * written, not accumulated.  fwd_ws is the workspace of the gm_sinkhorn_divergence_batched call with the same arguments,
 * untouched since: its plan and potentials are the backward's input (no host synchronisation, no float atomics).
 * Convention: geomloss's tensorized backend, read from its published code and UNPINNED against geomloss itself (absent), like
 * the forward.  Potentials are detached; only the last extrapolation at eps = blur^2 is differentiated, with the right-hand
 * cloud of every cost matrix detached:  dS/dx_i = (1/N) (T_xx(x_i) - T_xy(x_i)),  dS/dy_j = (1/M) (T_yy(y_j) - T_yx(y_j)),
 * T the softmax barycentres of the last extrapolation's rows.  A pair whose clouds are one point gets 0 (its loss is 0 by
 * definition), a pair with a non-finite coordinate NaN.  bwd_ws: gm_sinkhorn_batched_backward_workspace_bytes bytes
 * (0 unless y_shared, with dy requested). */
size_t gm_sinkhorn_batched_backward_workspace_bytes(int64_t batch, int64_t n, int64_t m, int y_shared);
int gm_sinkhorn_divergence_batched_backward(const float* x, int64_t batch, int64_t n, const float* y, int64_t m, int y_shared,
                                            float blur, float scaling, const float* grad_loss /*[batch], device*/,
                                            float* dx /*[batch,n,3] or NULL*/,
                                            float* dy /*[batch,m,3]; [m,3] if y_shared; or NULL*/, const void* fwd_ws,
                                            size_t fwd_ws_bytes, void* bwd_ws, size_t bwd_ws_bytes, void* stream);
/* Weighted clouds (an addition to ABI 7): geomloss's four-argument call loss(a, x, b, y).  Point i of x carries the mass
 * a[b][i] ([batch, N]), point j of y the mass b[j] ([M] when y_shared, else [batch, M]); a NULL side is uniform (1/N, 1/M),
 * and with both NULL the calls ARE gm_sinkhorn_divergence_batched and its backward, to the bit.  With la = log a, lb = log b:
 *     softmin_eps(C, h)_i = -eps log sum_j exp(h_j - C_ij / eps),   h = la + f / eps  or  lb + f / eps  (the cloud summed over)
 *     S = sum_i a_i (b_x - a_x)_i + sum_j b_j (a_y - b_y)_j
 *     dS/dx_i = a_i (T_xx(x_i) - T_xy(x_i)),  dS/dy_j = b_j (T_yy(y_j) - T_yx(y_j)),  the barycentres' softmax carrying la / lb
 * Conventions:
 *  - A weight of zero drops its point: log 0 = -inf, its term of every sum is exactly +0 and its gradient row exactly 0.0.
 *  - NO normalisation and NO mass-balance check, as in geomloss: the weights are used as given; clouds of different total mass
 *    give what the formulas above give.  (planner.density_target hands out weights that sum to 1.)
 *  - The diameter (diameter <= 0) stays geomloss's: the bounding box of ALL points of both clouds, whatever their weights.  A
 *    zero-weight point outside the others' box therefore lengthens the epsilon schedule: pad with copies of real points, or
 *    name the diameter.
 *  - The weights are constants: no gradient with respect to a or b.
 *  - A weight that is negative or not finite, or a cloud whose weights sum to 0, makes its pair's loss and gradients NaN, like
 *    a non-finite coordinate.  With diameter <= 0 -- one host synchronisation per call, as above -- the call then returns
 *    GM_ERR_DATA with a message naming the weights; with diameter > 0 no host synchronisation happens and nothing is reported:
 *    the NaN is the report.
 * ws: gm_sinkhorn_weighted_workspace_bytes bytes (the unweighted layout, then the logarithms of the weights that are given,
 * computed once per call); the backward reads it as fwd_ws and takes the same a and b; bwd_ws is sized by
 * gm_sinkhorn_batched_backward_workspace_bytes. */
size_t gm_sinkhorn_weighted_workspace_bytes(int64_t batch, int64_t n, int64_t m, int has_a, int has_b, int y_shared);
int gm_sinkhorn_divergence_weighted(const float* a /*[batch,n] or NULL: uniform*/, const float* x, int64_t batch, int64_t n,
                                    const float* b /*[m] if y_shared else [batch,m]; or NULL*/, const float* y, int64_t m,
                                    int y_shared, float blur, float scaling, float diameter, float* loss_device /*[batch]*/,
                                    void* ws, size_t ws_bytes, void* stream);
int gm_sinkhorn_divergence_weighted_backward(const float* a, const float* x, int64_t batch, int64_t n, const float* b,
                                             const float* y, int64_t m, int y_shared, float blur, float scaling,
                                             const float* grad_loss /*[batch], device*/, float* dx /*[batch,n,3] or NULL*/,
                                             float* dy /*[batch,m,3]; [m,3] if y_shared; or NULL*/, const void* fwd_ws,
                                             size_t fwd_ws_bytes, void* bwd_ws, size_t bwd_ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * One device-resident rollout step = compute_rollout's loop body, rollout_utils.py:38-61 ==
 * cma_objective's, traj_utils.py:123-152:  state_pre -> node features -> radius graph -> csr ->
 * edge features -> forward -> integrate -> state_post.  No host synchronisation.
 * ------------------------------------------------------------------------------------------ */
size_t gm_rollout_workspace_bytes(const gm_model_desc* desc, int64_t n_nodes, int max_neighbours);
int gm_rollout_step(const gm_model* m, float* obs /*[k,N,D] in/out*/, int64_t n_nodes,
                    const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                    const float* rigid_target /*[Nr,3] or NULL*/, float* pred_acc_out /*[N,3] or NULL*/,
                    void* rollout_ws, size_t rollout_ws_bytes, void* stream);
/* `steps` device-resident rollout steps without returning to the caller: compute_rollout's loop (rollout_utils.py:38-61)
 * == cma_objective's (traj_utils.py:123-152).  rigid_targets: [n_targets, n_rigid, 3] scripted poses, step i uses pose i;
 * steps beyond n_targets keep the rigid body in place (traj_utils.py:130-131); NULL / 0: no scripted poses.
 * record_last: [steps, N, D] or NULL -- the last frame of the window after the control overwrite of every step, i.e. what
 * the reference appends to `prediction` / `positions` (rollout_utils.py:49, traj_utils.py:137).  No host synchronisation.
 *
 * renumber_every > 0 (ABI 6): the loop runs on a copy of the state whose rows are in grid-cell order -- the radius graph's own
 * cell grid over the last frame, rows of a cell by index, graphs of a batch apart and in order -- re-ordered every
 * `renumber_every` steps (particles move a fraction of a cell per step; 64 is what RolloutEngine uses), so that the per-edge
 * gathers of neighbouring rows share cache lines whatever numbering the caller's simulator emits.  obs, record_last,
 * rigid_rank and rigid_targets stay in the CALLER's numbering: the result is written back through the row map, the records
 * too, and a renumbered rigid row keeps the caller's rank (ranks only index the pose arrays).  The order is computed on the
 * device (a ranking inside the graph build's cells: deterministic, no sort library, no host synchronisation).  A radius graph
 * does not depend on the numbering and every per-node / per-edge function is numbering-free: what changes is the order in
 * which a node's incoming messages are summed (float32 rounding, <= 2e-6 of the plain loop in the tests); the same state
 * gives the same bits every time.  renumber_ws: gm_rollout_renumber_workspace_bytes(fdesc, n_nodes) bytes (two copies of the
 * state + row maps); NULL / 0 with renumber_every == 0, which is the plain loop of ABI 5. */
size_t gm_rollout_renumber_workspace_bytes(const gm_feature_desc* fdesc, int64_t n_nodes);
int gm_rollout(const gm_model* m, float* obs /*[k,N,D] in/out*/, int64_t n_nodes, const gm_feature_desc* fdesc,
               int max_neighbours, const int32_t* rigid_rank, const float* rigid_targets, int64_t n_targets,
               int64_t n_rigid, int64_t steps, float* record_last, int64_t renumber_every, void* renumber_ws,
               size_t renumber_ws_bytes, void* rollout_ws, size_t rollout_ws_bytes, void* stream);
/* Error flags / edge count of the last step (synchronises). */
int gm_rollout_status(const void* rollout_ws, const gm_model_desc* desc, int64_t n_nodes,
                      int max_neighbours, int64_t* n_edges_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation against a recorded simulation: compute_rollout's ground-truth mode (rollout_utils.py:38-61 with
 * args.cma_traj None) and the sums behind the model comparison of scripts/plot_rmses.py:176-198.
 *
 * The recorded drive.  Step i, frame = frames[i] ([N,D], a recorded frame in the caller's row numbering):
 *   1. the control columns of the rigid rows (rigid_rank >= 0) of the last frame take frame's control columns
 *      (rollout_utils.py:45; control_col < 0: nothing to overwrite);
 *   2. the record is the last frame as it now stands (:48);
 *   3. the step runs as always and EVERY row, rigid ones included, takes its integrated position (:51-54);
 *   4. xyz of the rigid rows of the new last frame takes frame's xyz (:60) -- frame i again, the frame of 1: the reference's
 *      pose LAGS the window by one step, and so does this one.  The other columns of those rows are the record's.
 *
 * gm_state_recorded is 1 (what = GM_RECORDED_CONTROL) or 4 (GM_RECORDED_POSE) alone: a plain overwrite on the last frame of obs
 * [k,N,D], no shift.  row_map[j] (int32, each in [0, N)) is the row of `frame` that state row j is; NULL: the identity.
 * GM_RECORDED_CONTROL on a descriptor without control columns is refused (GM_ERR_INVALID_ARGUMENT), like gm_state_pre.
 *
 * gm_rollout_recorded runs `steps` such steps inside one call: gm_rollout's loop under the other drive, with its workspaces,
 * no host synchronisation, no allocation.  1, 2 and 4 ride in the two fused launches of the step, so a recorded step has
 * exactly the launches of a gm_rollout_step, records included.  record_pred[i] is the model's normalised acceleration of step i
 * (gm_rollout_step's pred_acc_out).  renumber_every > 0: as in gm_rollout; obs, frames, record_last and record_pred stay in the
 * caller's numbering and are reached through the row map inside the fused launches.  nodes_per_graph > 0: a batch of
 * equal-sized recorded simulations stored back to back.  frames, the records and obs must not overlap.
 *
 * gm_rollout_errors: per step i and graph g (G = N / nodes_per_graph, else 1), with gt = sim[first_frame + i],
 *   sums[i][g][0] = sum over all rows of |xyz(record_last[i]) - xyz(gt)|^2
 *   sums[i][g][1] = the same over the rows with material == 0 (gt's material column)
 *   sums[i][g][2] = sum over those rows of |record_pred[i] - a_gt|^2,  a_gt = ((p[f+1] - 2 p[f] + p[f-1]) - acc_mean) / acc_std
 *                   over xyz of sim, f = first_frame + i: the training target (collate_utils.py compute_acceleration);
 *                   0 when record_pred is NULL
 *   sums[i][g][3] = the number of rows with material == 0.
 * sim [n_frames,N,D] is read in place through the row stride D.  With record_pred: 1 <= first_frame and first_frame + steps <=
 * n_frames - 1; without: 0 <= first_frame and first_frame + steps <= n_frames; else GM_ERR_INVALID_ARGUMENT.  Every difference,
 * square, normalisation and sum is float64 from the float32 inputs.  One workgroup per (step, graph): each thread sums rows
 * t, t + 256, ... of the graph in order, the 256 partial sums go down a fixed tree -- no float atomics, no dependence on the
 * grid, the same call twice gives the same bits.  A NaN / inf coordinate makes its own (step, graph) sums non-finite only.
 * ------------------------------------------------------------------------------------------ */
#define GM_RECORDED_CONTROL 1
#define GM_RECORDED_POSE 4
int gm_state_recorded(float* obs, int64_t n_nodes, const gm_feature_desc* desc, const int32_t* rigid_rank, const float* frame,
                      const int32_t* row_map, int what, void* stream);
int gm_rollout_recorded(const gm_model* m, float* obs, int64_t n_nodes, const gm_feature_desc* fdesc,
                        int max_neighbours, const int32_t* rigid_rank, const float* frames, int64_t steps,
                        float* record_last, float* record_pred,
                        int64_t renumber_every, void* renumber_ws, size_t renumber_ws_bytes,
                        void* rollout_ws, size_t rollout_ws_bytes, void* stream);
int gm_rollout_errors(const float* record_last, const float* record_pred,
                      const float* sim, int64_t n_frames, int64_t first_frame,
                      int64_t steps, int64_t n_nodes, const gm_feature_desc* fdesc,
                      double* sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rollouts of scenes of different sizes as one ragged batch: gm_rollout_step, gm_rollout, gm_rollout_recorded and
 * gm_rollout_errors for graphs of any sizes stored back to back.  The graphs travel as in gm_radius_graph_build_ragged: graph g
 * owns rows [graph_offsets_host[g], graph_offsets_host[g + 1]) of every [.., N, ..] array, N = graph_offsets_host[n_graphs]; the
 * table is read on the host during the call and rides in the kernel arguments (no copy, no allocation, no synchronisation),
 * 1..GM_RAGGED_MAX_GRAPHS graphs.  fdesc->nodes_per_graph must be 0.  Workspace: gm_rollout_workspace_bytes(desc, N, K) -- the
 * table adds nothing to it -- and gm_rollout_status(ws, desc, N, K) reads the whole batch's flags and edge count.
 *
 * Rows and ranks.  obs [k,N,D], record_last [steps,N,D], record_pred [steps,N,3], frames [steps,N,D] and sim [n_frames,N,D] hold
 * the graphs' rows side by side along the node axis, in graph order.  rigid_rank [N] is GLOBAL: gm_rigid_rank on the assembled
 * window numbers the rigid rows of graph g behind those of the graphs before it, and rigid_target(s) [.., n_rigid, 3] hold the
 * poses in that order (n_rigid = all graphs' rigid rows; a graph may have none).
 *
 * Batch invariance.  No edge joins two graphs, every per-row and per-edge function sees its own row only, and the 32-edge block
 * tables of the processor kernels pad every graph to whole 4-block groups exactly as those of an equal-sized batch do, so a
 * graph's partial sums do not depend on what shares the launch: the rows of graph g of the state, of every record and of every
 * prediction are BIT FOR BIT what the single-scene entry point computes for scene g alone, at either precision and with any
 * gm_model_set_edge_kernel choice.  The one condition: under the automatic kernel choice at hidden 128 the processor's node path
 * is chosen by the batch's SMALLEST graph (the systolic path only if every graph would take it alone), so all graphs of a batch
 * must lie on the same side of that size (49 152 rows) -- as every batch of scenes of a few thousand to tens of thousands of rows
 * does.  A batch of equal sizes equals the nodes_per_graph form, a batch of one graph the plain call.
 *
 * There is no renumbering on a ragged batch (no renumber_* arguments).  gm_rollout_errors_ragged writes sums [steps, n_graphs, 4]:
 * still one workgroup per (step, graph), its threads over that graph's rows, the same fixed tree.
 *
 * Refused with GM_ERR_INVALID_ARGUMENT before anything is launched or written: nodes_per_graph != 0, and what
 * gm_radius_graph_build_ragged refuses of a table (n_graphs outside 1..GM_RAGGED_MAX_GRAPHS, graph_offsets_host[0] != 0, a graph
 * of fewer than 1 row, N >= 2^30, N * max_neighbours >= 2^31).  A workspace smaller than gm_rollout_workspace_bytes:
 * GM_ERR_WORKSPACE, likewise before the first launch.
 * ------------------------------------------------------------------------------------------ */
int gm_rollout_step_ragged(const gm_model* m, float* obs /*[k,N,D] in/out*/, const int64_t* graph_offsets_host /*[n_graphs+1]*/,
                           int64_t n_graphs, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                           const float* rigid_target /*[Nr,3] or NULL*/, float* pred_acc_out /*[N,3] or NULL*/,
                           void* rollout_ws, size_t rollout_ws_bytes, void* stream);
int gm_rollout_ragged(const gm_model* m, float* obs /*[k,N,D] in/out*/, const int64_t* graph_offsets_host /*[n_graphs+1]*/,
                      int64_t n_graphs, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                      const float* rigid_targets, int64_t n_targets, int64_t n_rigid, int64_t steps, float* record_last,
                      void* rollout_ws, size_t rollout_ws_bytes, void* stream);
int gm_rollout_recorded_ragged(const gm_model* m, float* obs, const int64_t* graph_offsets_host /*[n_graphs+1]*/,
                               int64_t n_graphs, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                               const float* frames, int64_t steps, float* record_last, float* record_pred,
                               void* rollout_ws, size_t rollout_ws_bytes, void* stream);
int gm_rollout_errors_ragged(const float* record_last, const float* record_pred,
                             const float* sim, int64_t n_frames, int64_t first_frame, int64_t steps,
                             const int64_t* graph_offsets_host /*[n_graphs+1]*/, int64_t n_graphs,
                             const gm_feature_desc* fdesc, double* sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * The reverse sweep of a rollout (no reference counterpart: the reference's planner is derivative-free, traj_utils.py:247-259).
 * gm_rollout_step_backward is the vector-Jacobian product of ONE gm_rollout_step with the model's parameters as constants:
 * d_obs_before [k,N,D] and d_rigid_target [N_rigid,3] (may be NULL; zeros without a rigid_target) from d_obs_after [k,N,D], the
 * gradient with respect to the window the step left.  obs_before is the window the step started from and is not written.
 *
 * The call re-runs the step's forward out of place on a copy of obs_before in the workspace, with a tape -- gm_state_pre,
 * gm_node_features, gm_radius_graph_build_batched (nodes_per_graph of the descriptor: a block-diagonal batch), gm_radius_graph_edges,
 * gm_edge_features, gm_epd_forward_train (whose destination sort opens its tape) -- and then runs, in this order,
 * gm_state_post_backward, gm_integrate_backward, gm_epd_backward_inputs_only, gm_node_features_backward and
 * gm_edge_features_backward.  The radius graph is a constant of the step (connectivity is piecewise constant in the positions).
 * Those transposes write window-sized or [N,3] contributions of their own; ONE last launch, one thread per particle row owning
 * that row in every frame, adds them in a fixed order,
 *     ((state_post's + integrator's) + node features') + edge features' (xyz of the last frame),
 * applies gm_state_pre_backward's rule to the sum where the step ran the overwrite (rigid_rank given, control columns exist) and
 * writes the row of d_rigid_target it owns as state_post's share + state_pre's share.  No float atomics: the same call twice
 * gives the same bits, and a scene of a batch gets the bits it gets alone.
 *
 * `tensors` / n_tensors: the parameter values the handle was created from (device pointers, gm_epd_backward_inputs_only's
 * argument).  Hidden sizes 64 / 128 / 256 (the training entry points).  HOST SYNCHRONISATION: the training forward takes the
 * edge count on the host, so the call reads that one number back (gm_radius_graph_num_edges) per step; n_edges_host (may be NULL)
 * returns it.  A non-finite position is reported there (GM_ERR_DATA).  The workspace depends on n_nodes and max_neighbours alone
 * (edge capacity n_nodes * max_neighbours), never on a horizon; nothing in it needs initialising.
 *
 * gm_rollout_backward is the whole sweep: windows [steps,k,N,D] are the pre-step windows a forward kept (window t = the state
 * before step t), trajectory [n_targets,N_rigid,3] or NULL the scripted poses with gm_rollout's rule (step t uses pose t, steps
 * past n_targets have none), d_final [k,N,D] the gradient with respect to the final state.  Outputs: d_obs0 [k,N,D] and
 * d_trajectory [n_targets,N_rigid,3] (may be NULL), whose rows of steps at or past `steps` are written as zeros.  steps == 0 copies
 * d_final to d_obs0.  It is a loop of gm_rollout_step_backward from the last step to the first; two [k,N,D] gradient windows take
 * turns behind the step's workspace, so the workspace is the step's plus those two, whatever `steps` is.  One host
 * synchronisation per step, as above.
 *
 * gm_rollout_step_backward_train / gm_rollout_backward_train are the same two calls with two more inputs, for a loss that trains the
 * model through the rollout and has a term on every step (both NULL: gm_rollout_step_backward / gm_rollout_backward, bit for bit --
 * those two ARE these with both NULL).
 *   grads: gm_epd_backward's argument -- one float buffer per parameter tensor, same order and shapes as `tensors` -- ACCUMULATED into
 * (the caller zeroes them); everything else these calls return is WRITTEN in full.  With grads the step's model backward is
 * gm_epd_backward_inputs, without it gm_epd_backward_inputs_only; their input gradients are bit-equal (see there), so d_obs_before,
 * d_rigid_target, d_obs0 and d_trajectory have the same bits with and without grads.  Across a sweep every step adds into the same
 * buffers, step steps-1 first and step 0 last; within a step the order is gm_epd_backward's.  No float atomics: the same call from
 * zeroed grads gives the same bits twice.  steps == 0 leaves grads untouched.
 *   d_record [N,D] / d_records [steps,N,D]: the gradient with respect to record_last[t] of gm_rollout, the last frame of window t
 * after the control overwrite of gm_state_pre -- d_records is the transpose of the record the forward offers.  It joins the last
 * frame's sum inside the one assembly launch, as the last term of the fixed order,
 *     (((state_post's + integrator's) + node features') + edge features') + record's,
 * before gm_state_pre_backward's rule is applied to that sum: no extra launch, no extra pass over a window.  Rows of d_records at or
 * past `steps` are not read; steps == 0 ignores it.  (record_last[t] is also frame k-2 of the window after step t: the window shift
 * moves it there unchanged, so a forward that keeps its windows has its records already.)
 *   Workspace: gm_train_backward_inputs_workspace_bytes is the query of both model backwards, so
 * gm_rollout_step_backward_workspace_bytes and gm_rollout_backward_workspace_bytes serve these two unchanged; one tape and one
 * backward workspace are alive whatever `steps` is.
 * ------------------------------------------------------------------------------------------ */
size_t gm_rollout_step_backward_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n_nodes,
                                                int max_neighbours);
int gm_rollout_step_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* obs_before /*[k,N,D]*/,
                             int64_t n_nodes, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                             const float* rigid_target /*[Nr,3] or NULL*/, const float* d_obs_after /*[k,N,D]*/,
                             float* d_obs_before /*[k,N,D]*/, float* d_rigid_target /*[Nr,3] or NULL*/,
                             int64_t* n_edges_host /* or NULL */, void* ws, size_t ws_bytes, void* stream);
size_t gm_rollout_backward_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n_nodes,
                                           int max_neighbours);
int gm_rollout_backward(const gm_model* m, const float* const* tensors, int n_tensors, const float* windows /*[steps,k,N,D]*/,
                        int64_t n_nodes, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                        const float* trajectory /*[n_targets,Nr,3] or NULL*/, int64_t n_targets, int64_t n_rigid, int64_t steps,
                        const float* d_final /*[k,N,D]*/, float* d_obs0 /*[k,N,D]*/, float* d_trajectory /*[n_targets,Nr,3] or NULL*/,
                        void* ws, size_t ws_bytes, void* stream);
int gm_rollout_step_backward_train(const gm_model* m, const float* const* tensors, int n_tensors, const float* obs_before /*[k,N,D]*/,
                                   int64_t n_nodes, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                                   const float* rigid_target /*[Nr,3] or NULL*/, const float* d_obs_after /*[k,N,D]*/,
                                   const float* d_record /*[N,D] or NULL*/, float* const* grads /* or NULL */,
                                   float* d_obs_before /*[k,N,D]*/, float* d_rigid_target /*[Nr,3] or NULL*/,
                                   int64_t* n_edges_host /* or NULL */, void* ws, size_t ws_bytes, void* stream);
int gm_rollout_backward_train(const gm_model* m, const float* const* tensors, int n_tensors, const float* windows /*[steps,k,N,D]*/,
                              int64_t n_nodes, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                              const float* trajectory /*[n_targets,Nr,3] or NULL*/, int64_t n_targets, int64_t n_rigid, int64_t steps,
                              const float* d_final /*[k,N,D]*/, const float* d_records /*[steps,N,D] or NULL*/,
                              float* const* grads /* or NULL */, float* d_obs0 /*[k,N,D]*/,
                              float* d_trajectory /*[n_targets,Nr,3] or NULL*/, void* ws, size_t ws_bytes, void* stream);
/* The two training sweeps on a ragged batch (see "Rollouts of scenes of different sizes as one ragged batch" above for the table,
 * the row and rank layout; fdesc->nodes_per_graph must be 0).  A step's graph is gm_radius_graph_build_ragged's; everything else is
 * per row or per edge, so the input gradients of graph g's rows are those of scene g alone and the parameter gradients are the sum
 * over the graphs, accumulated edge by edge and row by row in the batch's order.  Still ONE edge-count read per step, for the whole
 * batch.  d_record / d_records and grads both NULL: the plain vector-Jacobian product (gm_rollout_step_backward /
 * gm_rollout_backward).  Workspaces: gm_rollout_step_backward_workspace_bytes / gm_rollout_backward_workspace_bytes with N total. */
int gm_rollout_step_backward_train_ragged(const gm_model* m, const float* const* tensors, int n_tensors, const float* obs_before /*[k,N,D]*/,
                                          const int64_t* graph_offsets_host /*[n_graphs+1]*/, int64_t n_graphs, const gm_feature_desc* fdesc,
                                          int max_neighbours, const int32_t* rigid_rank, const float* rigid_target, const float* d_obs_after,
                                          const float* d_record, float* const* grads, float* d_obs_before, float* d_rigid_target,
                                          int64_t* n_edges_host, void* ws, size_t ws_bytes, void* stream);
int gm_rollout_backward_train_ragged(const gm_model* m, const float* const* tensors, int n_tensors, const float* windows /*[steps,k,N,D]*/,
                                     const int64_t* graph_offsets_host /*[n_graphs+1]*/, int64_t n_graphs, const gm_feature_desc* fdesc,
                                     int max_neighbours, const int32_t* rigid_rank, const float* trajectory, int64_t n_targets,
                                     int64_t n_rigid, int64_t steps, const float* d_final, const float* d_records, float* const* grads,
                                     float* d_obs0, float* d_trajectory, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training batches from resident recordings (an addition to ABI 7).  Replaces, for a batch of samples, CoffeeDataset's
 * stored windows (coffee_dataset.py:82-102), random_walk_noise (utils.py:96-115), _process_noisy / _process_simple
 * (collate_utils.py:169-193, 29-40) and the collate (collate_utils.py:68-87): the nodes / edge_attr / edge_index / target that
 * gm_epd_forward_train and a loss take, in two phases around the one number the host has to learn, the edge count.
 *
 * gm_train_batch_build (phase 1; no host synchronisation, no allocation).  first_frames is a HOST array of `batch` device
 * pointers; first_frames[b] points at frame t_b of a resident recording [T, N, rec_dim].  The call reads the k + 1 frames from
 * there -- the window and the frame that follows it -- and writes nothing to them; samples may come from different recordings or
 * overlap in one.  The pointers travel by value in the kernel arguments.  fdesc describes the WINDOW the features are computed
 * on: without control columns data_dim == rec_dim and control_col < 0; with them data_dim == rec_dim + 3 and
 * control_col == rec_dim (the dataset's layout: the three columns are appended).  Refused with GM_ERR_INVALID_ARGUMENT and a
 * "gm_train_batch_build: ..." message, before any device call: any other layout, k_steps < 2, batch outside
 * 1..GM_TRAIN_BATCH_MAX, nodes_per_graph < 1, the graph builder's limits (batch * N < 2^30, max_neighbours 1..160,
 * batch * N * max_neighbours < 2^31), a workspace below gm_train_batch_workspace_bytes (which is 0 for such arguments), a null
 * pointer.  k_steps above 8 is GM_ERR_UNSUPPORTED: a thread keeps its window's positions in registers, the kernel is
 * instantiated for k_steps 2..8.
 *   window   the recording's columns; the control columns of frame t are next_xyz - xyz_t where that frame's material column
 *            equals 1, else 0, from the CLEAN positions.
 *   noise    seq[0] = 0, vel_t = vel_(t-1) + n_t, seq_t = seq_(t-1) + vel_t in float32, left to right (the first term of a sum
 *            is the term itself); the window's xyz becomes xyz + seq, the position after the window next + seq[k-1].
 *            noise_sample [batch, k-1, N, 3] non-NULL gives n as it stands (already scaled, as random_walk_noise takes it);
 *            else noise_std > 0 draws n_t = z * (float)(noise_std / sqrt(k - 1)); else there is no noise (and nothing is added).
 *   the draw Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (particle index inside its graph, j,
 *            stream & 0xffffffff, stream >> 32) with stream = first_stream + b for slot b.  Normal number q = 3 (t - 1) + a
 *            (frame step t = 1..k-1, axis a) is lane q % 4 of call j = q / 4; lanes (0, 1) are the Box-Muller pair of words
 *            (0, 1), lanes (2, 3) that of words (2, 3): u1 = ((w_even >> 8) + 1) * 2^-24, u2 = (w_odd >> 8) * 2^-24,
 *            z = sqrt(-2 ln u1) * (cos, sin)(2 pi u2), every operation in float32 (2 pi = 6.2831855f), logf / sincosf the
 *            accurate ones.  A sample's noise depends on (seed, stream, particle) alone -- not on the batch it rides in, its
 *            slot, the launch shape or which workspace is used.
 *   nodes    [batch * N, F] gm_node_features of each (noisy) window;  target [batch * N, 3]
 *            (((next' - 2 p_(k-1)) + p_(k-2)) - acc_mean) / acc_std on it (compute_target's op order);  windows
 *            [batch, k, N, data_dim] or NULL: the windows themselves.  Graph b owns rows [b N, (b + 1) N).
 *   graph    gm_radius_graph_build_batched's, on the noisy last positions, nodes_per_graph = N, fdesc->conn_r.
 * The workspace begins with a 16-byte record (int32 n_edges, int32 error flags, 8 bytes reserved) that a caller may copy
 * asynchronously behind the build; gm_train_batch_status turns a HOST copy of it into E (no device access, like
 * gm_csr_header_status), or into GM_ERR_DATA where a position in one of the k + 1 recorded frames (or the noise) was not finite.
 * gm_train_batch_num_edges copies the record itself and synchronises `stream`, like gm_radius_graph_num_edges.
 *
 * gm_train_batch_edges (phase 2; the caller knows E): edge_index[0] = senders, edge_index[1] = receivers in the reference
 * order (grouped by sender ascending, distance ascending, batch offsets N * b included), edge_attr in that order.  Arguments as
 * in phase 1, on its workspace.  n_edges other than the build's count is the caller's error: nothing is written past n_edges
 * entries, and entries past the build's count are not written at all.
 * ------------------------------------------------------------------------------------------ */
#define GM_TRAIN_BATCH_MAX 64
size_t gm_train_batch_workspace_bytes(const gm_feature_desc* fdesc, int64_t batch, int64_t nodes_per_graph, int max_neighbours);
int gm_train_batch_build(const float* const* first_frames_host, int64_t batch, int64_t nodes_per_graph, int rec_dim,
                         const gm_feature_desc* fdesc, int max_neighbours, double noise_std, uint64_t seed, uint64_t first_stream,
                         const float* noise_sample, float* nodes, float* target, float* windows, void* ws, size_t ws_bytes,
                         void* stream);
int gm_train_batch_edges(const void* ws, int64_t batch, int64_t nodes_per_graph, const gm_feature_desc* fdesc, int max_neighbours,
                         int64_t n_edges, int64_t* edge_index, float* edge_attr, void* stream);
int gm_train_batch_num_edges(const void* ws, int64_t* n_edges_host, void* stream);
int gm_train_batch_status(const int32_t* record_host, int64_t* n_edges_host);

/* The same two phases for samples of DIFFERENT sizes (an addition to ABI 7): sizes_host is a HOST array, sizes_host[b] = N_b
 * the rows of sample b's recording, first_frames_host[b] points at a frame of a resident recording [T, N_b, rec_dim].  Sample b
 * owns rows [off_b, off_b + N_b) of nodes and target, off_b = N_0 + .. + N_(b-1); windows holds the samples' [k, N_b, data_dim]
 * blocks back to back, noise_sample their [k-1, N_b, 3] blocks back to back.  Everything said of gm_train_batch_build holds per
 * sample -- window, control columns from the clean positions, noise, features, target -- and the draw's counter is unchanged
 * (particle index INSIDE its graph, j, stream = first_stream + b): a sample's noise does not depend on whether it rides in a
 * ragged batch, in an equal-sized one or alone.  The graph is gm_radius_graph_build_ragged's; the record, gm_train_batch_status
 * and gm_train_batch_num_edges serve it unchanged; phase 2 emits edge_index in the reference order with the samples' row
 * offsets, and edge_attr.  With all sizes equal every output is bit-equal to gm_train_batch_build / gm_train_batch_edges.  One
 * clear launch, one row kernel (grid: the largest sample x batch), the graph build and one scan, as for an equal-sized batch;
 * the sizes travel by value in the kernel arguments.  Refusals ("gm_train_batch_build_ragged: ..." / "gm_train_batch_edges_ragged:
 * ...", GM_ERR_INVALID_ARGUMENT, before any device call) are gm_train_batch_build's, with: a size below 1, and the graph
 * builder's limits on the total of the sizes.  gm_train_batch_ragged_workspace_bytes takes that total; it is 0 for refused
 * shapes (total_rows < batch among them) and depends on the sizes through (total_rows, batch) alone. */
size_t gm_train_batch_ragged_workspace_bytes(const gm_feature_desc* fdesc, int64_t total_rows, int64_t batch, int max_neighbours);
int gm_train_batch_build_ragged(const float* const* first_frames_host, const int64_t* sizes_host, int64_t batch, int rec_dim,
                                const gm_feature_desc* fdesc, int max_neighbours, double noise_std, uint64_t seed,
                                uint64_t first_stream, const float* noise_sample, float* nodes, float* target, float* windows,
                                void* ws, size_t ws_bytes, void* stream);
int gm_train_batch_edges_ragged(const void* ws, const int64_t* sizes_host, int64_t batch, const gm_feature_desc* fdesc,
                                int max_neighbours, int64_t n_edges, int64_t* edge_index, float* edge_attr, void* stream);

/* ------------------------------------------------------------------------------------------
 * The training step in the library (examples/train_dyn.py:49-72: loss, zero_grad, backward, optimizer.step): additions to ABI 7.
 *
 * gm_l1_loss == L1Loss(reduction='sum') / rows (train_dyn.py:58-65).  mask_col < 0: every row counts.  mask_col in [0, node_dim):
 * the rows with nodes[row][mask_col] < 0.5 count (--use_updated_loss: the sand particles; a NaN there does not count).  The loss
 * is the float64 sum, in one fixed order (no atomics), of the float32 values |pred - target| over the counted rows, divided by
 * their count.  grad_out[r][c] = sign(pred - target) * (float)(1.0 / count) on counted rows, with sign(0) = 0; rows that do not
 * count get 0.  A count of 0 gives a NaN loss and an all-zero grad_out.  loss_out / rows_counted_out / grad_out are device
 * memory; rows_counted_out and grad_out may be NULL, nodes may be NULL iff mask_col < 0.  Refused before any device call
 * (GM_ERR_INVALID_ARGUMENT, "gm_l1_loss: ..."): a null pointer, n_rows or out_dim below 1, mask_col >= node_dim; a workspace
 * below gm_l1_loss_workspace_bytes is GM_ERR_WORKSPACE.  The workspace is written before it is read.
 *
 * A gm_trainer owns, for one gm_model, Adam's two moment estimates and a gradient buffer, each laid out like the model's own
 * flat copy of its tensors, and a 32-byte device record { int64 steps_applied, int64 steps_skipped, double beta1_pow, double
 * beta2_pow }.  The weights it updates ARE the model's copy: no tensor is copied in or out by a step.  The model must outlive
 * the trainer, and between gm_trainer_create and gm_trainer_destroy the trainer's calls are the only ones that change its weights.
 * Hidden 64 / 128 / 256 only, like every training entry point (GM_ERR_UNSUPPORTED).
 *
 * gm_train_step, on one stream and without a host synchronisation: clears the gradients; gm_epd_forward_train; gm_l1_loss of the
 * prediction against `target` [N, out_dim] (mask_col as above, over `nodes`); gm_epd_backward into the trainer's gradients; one
 * Adam step at learning rate lr; the model's training images re-packed, its inference images marked stale (the next inference
 * call re-packs them).  loss_out (device, may be NULL) receives the loss.  The workspace (gm_train_step_workspace_bytes) begins
 * with the forward's tape, so its first 16 bytes are the CSR header that carries the edge_index verdict (gm_csr_header_status).
 * SKIPPED STEPS: when that header flags an edge_index entry outside [0, N), or the loss is not finite, the update does not
 * happen: weights, both moments, steps_applied and the beta powers keep their bits, steps_skipped goes up by one, and loss_out
 * still receives the loss (NaN for a flagged edge_index).
 *
 * ADAM'S ARITHMETIC (no weight decay, no AMSGrad).  Scalars, in float64 on the device: beta1_pow <- beta1_pow * beta1 and
 * beta2_pow <- beta2_pow * beta2 (running products, not pow: a host loop reproduces them exactly); step = (float)(lr / (1 -
 * beta1_pow)); s2 = (float)sqrt(1 - beta2_pow).  Per element, every float32 operation rounded on its own (no fused multiply-add,
 * correctly rounded sqrt and division), with b1 = (float)beta1, o1 = (float)(1 - beta1), b2 = (float)beta2, o2 = (float)(1 -
 * beta2), e = (float)eps:
 *     m <- (b1 * m) + (o1 * g)
 *     v <- (b2 * v) + ((o2 * g) * g)
 *     p <- p - step * (m / ((sqrt(v) / s2) + e))
 * This sequence is the library's own (torch.optim.Adam uses lerp and a fused addcdiv): it agrees with float64 Adam as closely as
 * float32 torch does, not bit for bit with torch.
 *
 * gm_trainer_record copies the record into the caller's (pinned) host memory, asynchronously.  gm_trainer_export / _import copy
 * between ONE of the trainer's buffers (`what`) and caller tensors on the device, in gm_model_create's order and shapes.
 * Importing GM_TRAINER_PARAMS is gm_model_update; importing GM_TRAINER_EXP_AVG also sets steps_applied = step_count and the beta
 * powers to the running products of step_count steps; the gradients are an output and cannot be imported.  A wrong n_tensors, a
 * null tensor or an unknown `what` is GM_ERR_INVALID_ARGUMENT before any device call.
 * ------------------------------------------------------------------------------------------ */
size_t gm_l1_loss_workspace_bytes(int64_t n_rows, int out_dim);
int gm_l1_loss(const float* pred, const float* target, int64_t n_rows, int out_dim, const float* nodes /* may be NULL iff mask_col < 0 */,
               int node_dim, int mask_col, double* loss_out /* device, 1 */, int64_t* rows_counted_out /* device, may be NULL */,
               float* grad_out /* [n_rows, out_dim] device, may be NULL */, void* ws, size_t ws_bytes, void* stream);

typedef struct gm_trainer gm_trainer; /* opaque */
#define GM_TRAINER_PARAMS 1
#define GM_TRAINER_EXP_AVG 2
#define GM_TRAINER_EXP_AVG_SQ 3
#define GM_TRAINER_GRADS 4
int gm_trainer_create(gm_model* m, double beta1, double beta2, double eps, void* stream, gm_trainer** out);
void gm_trainer_destroy(gm_trainer* t);
size_t gm_train_step_workspace_bytes(const gm_model_desc* desc, int64_t n_nodes, int64_t n_edges);
int gm_train_step(gm_trainer* t, const float* nodes, int64_t n_nodes, const float* edge_attr, const int64_t* edge_index,
                  int64_t n_edges, const float* target, int mask_col, double lr, double* loss_out /* device, may be NULL */,
                  void* ws, size_t ws_bytes, void* stream);
int gm_trainer_record(const gm_trainer* t, void* record_host /* 32 bytes */, void* stream);
int gm_trainer_export(const gm_trainer* t, int what, float* const* tensors_out, int n_tensors, void* stream);
int gm_trainer_import(gm_trainer* t, int what, const float* const* tensors_in, int n_tensors, int64_t step_count /* used with EXP_AVG */,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Training on a rollout in the library (no reference counterpart: the reference trains one step ahead only): additions to ABI 7.
 *
 * gm_rollout_l1_loss is the L1 loss of a `steps`-step rollout against recorded frames, and its transpose.  windows [steps,k,N,D] are
 * the pre-step windows of a forward (gm_rollout_backward's argument), final_state [k,N,D] the state it left, frames
 * [steps,N,frame_dim] the recorded frame that follows step t, read in place from a resident recording: frame_dim is data_dim, or
 * data_dim - 3 for a recording without the three control columns a window appends.  The xyz columns are fdesc->cart_col .. + 2 in both.
 * The PREDICTED frame of step t is the last frame of windows[t + 1] for t < steps - 1 and of final_state for t = steps - 1.  A row
 * COUNTS when rigid_rank[r] < 0 (rigid_rank NULL: every row) and, with material_col >= 0 (a column of the STATE), when
 * windows[0][k-1][r][material_col] < 0.5.  s_c is the float64 sum, over the counted rows and the steps, of the float32 values
 * |pred - frame| on axis c, in one fixed order (no atomics: gm_l1_loss's two passes, a thread walking row, step, axis), and
 *     loss = ((s_0 / scale_0 + s_1 / scale_1) + s_2 / scale_2) / (steps * count)
 * with scale = pos_scale[3], HOST doubles (NULL: ones; acc_std makes a one-step rollout's loss the one-step training loss).
 * The transpose: an element is sign(pred - frame) * (float)(1.0 / ((scale_c * steps) * count)) with sign(0) = 0, written into the
 * xyz columns of d_records[t + 1] for t < steps - 1 -- gm_rollout_backward_train's argument: record t + 1 is that predicted frame --
 * and of the last frame of d_final for t = steps - 1.  d_records [steps,N,D] and d_final [k,N,D] are WRITTEN IN FULL, zeros
 * everywhere else, all of d_records[0] included: there is no memset in front.  Both NULL: the loss alone.  A count of 0 gives a
 * NaN loss and all-zero gradients.  loss_out / rows_counted_out (may be NULL) are device memory.  Refused before any device call
 * (GM_ERR_INVALID_ARGUMENT, "gm_rollout_l1_loss: ..."): a null pointer, steps outside 1..32768, n_nodes below 1, a frame_dim that is
 * neither data_dim nor data_dim - 3 or does not hold the xyz columns, material_col >= data_dim, a zero or NaN pos_scale, one of
 * d_records / d_final without the other; a workspace below gm_rollout_l1_loss_workspace_bytes is GM_ERR_WORKSPACE.  The workspace is
 * written before it is read; its size is gm_rollout_l1_loss_ragged_workspace_bytes(1): the call runs gm_rollout_l1_loss_ragged's
 * kernels on one segment [0, n_nodes), whatever fdesc->nodes_per_graph says (equal-sized graphs side by side are ONE sample).
 *
 * gm_train_rollout_step is one training step on a rollout of the trainer's model, on one stream; obs0 [k,N,D] is not written.
 *   1. one row kernel writes the scripted poses trajectory[t][rigid_rank[r]] = xyz(frames[t][r]) of the rigid rows (n_rigid of them;
 *      rigid_rank / n_rigid as gm_rigid_rank returns them; n_rigid == 0: no poses);
 *   2. the inference rollout runs from a copy of obs0 under that trajectory, a device-to-device copy of the window in front of each
 *      gm_rollout_step, so that every pre-step window stays behind; the final state is bit-equal to gm_rollout's;
 *   3. gm_rollout_l1_loss (material_col, pos_scale as above); loss_out (device, may be NULL) receives the loss;
 *   4. update != 0: the trainer's gradients are cleared, gm_rollout_backward_train runs on the windows with the loss's d_final and
 *      d_records and accumulates into them, and one Adam step at learning rate lr follows as in gm_train_step, with its rule for
 *      SKIPPED STEPS: a loss that is not finite leaves weights, both moments, steps_applied and the beta powers with their bits and
 *      raises steps_skipped by one.  update == 0 stops after the loss: a validation pass that changes nothing and never synchronises.
 * LIMITS.  The sweep reads one edge count per step back to the host (gm_rollout_backward), so an updating call synchronises `steps`
 * times.  A non-finite position reported there returns GM_ERR_DATA before Adam's launches: loss_out is written, weights, moments
 * and the record keep their bits.  Hidden sizes 64 / 128 / 256 (a gm_trainer exists for no other).  The workspace
 * (gm_train_rollout_step_workspace_bytes; 0 for refused sizes) holds the rollout's and the sweep's workspaces, steps + 1 windows,
 * d_records, two [k,N,D] gradient windows and the trajectory, and BEGINS with the windows: window t < steps at float offset
 * t k N D is the state before step t, window `steps` the final state.  Nothing in it needs initialising.  Refusals
 * ("gm_train_rollout_step: ...", before any device call): gm_rollout_l1_loss's, a null trainer, n_rigid outside [0, n_nodes], a null
 * rigid_rank with n_rigid > 0, a NaN lr, a model that does not fit the scene; a short workspace is GM_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------ */
size_t gm_rollout_l1_loss_workspace_bytes(int64_t n_nodes, int64_t steps);
int gm_rollout_l1_loss(const float* windows /*[steps,k,N,D]*/, const float* final_state /*[k,N,D]*/,
                       const float* frames /*[steps,N,frame_dim]*/, int frame_dim, int64_t steps, int64_t n_nodes,
                       const gm_feature_desc* fdesc, const int32_t* rigid_rank /* may be NULL */, int material_col,
                       const double* pos_scale /* host [3], may be NULL */, double* loss_out /* device, 1 */,
                       int64_t* rows_counted_out /* device, may be NULL */, float* d_records /*[steps,N,D] or NULL*/,
                       float* d_final /*[k,N,D] or NULL*/, void* ws, size_t ws_bytes, void* stream);
size_t gm_train_rollout_step_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n_nodes, int64_t n_rigid,
                                             int max_neighbours, int64_t steps);
int gm_train_rollout_step(gm_trainer* t, const float* obs0 /*[k,N,D]*/, int64_t n_nodes, const gm_feature_desc* fdesc, int max_neighbours,
                          const int32_t* rigid_rank, int64_t n_rigid, const float* frames /*[steps,N,frame_dim]*/, int frame_dim,
                          int64_t steps, int material_col, const double* pos_scale /* host [3], may be NULL */, double lr, int update,
                          double* loss_out /* device, may be NULL */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mini-batches and gradient clipping in the library (train_dyn.py:242 trains at batch_size = 2; clipping is
 * torch.nn.utils.clip_grad_norm_'s): additions to ABI 7.  gm_train_step and gm_train_rollout_step are one sample and one update per
 * call; the calls below split that into three phases a caller drives, on one stream:
 *
 *     gm_trainer_begin;  S >= 1 times gm_train_step_accumulate / gm_train_rollout_accumulate, in any mix;  gm_trainer_apply.
 *
 * gm_trainer_begin clears the trainer's gradient buffer and resets a second device record, the MINI-BATCH's, 48 bytes and separate
 * from the trainer's 32-byte record (whose layout does not change):
 *     { int64 samples, int64 bad, double loss_sum, double sumsq, double grad_norm, double scale }
 * (begin: 0, 0, 0.0, 0.0, NaN, NaN).  gm_trainer_accum_record copies it into the caller's (pinned) host memory, asynchronously.
 *
 * gm_train_step_accumulate takes gm_train_step's arguments without lr, gm_train_rollout_accumulate gm_train_rollout_step's without
 * lr and update; the workspaces are gm_train_step_workspace_bytes' and gm_train_rollout_step_workspace_bytes'.  Each runs exactly
 * what its parent runs up to, and not including, Adam, WITHOUT clearing the gradients: the backward entry points add the sample's
 * gradient to the buffer.  One single-thread launch then adds the sample to the record: samples += 1; loss_sum += the sample's
 * loss, in arrival order; bad += 1 when the parent would have SKIPPED its step (a flagged edge_index, a loss that is not finite).
 * loss_out (device, may be NULL) receives the sample's own loss.  The refusals are the parent's under the new name, and
 * "...: no mini-batch begun (gm_trainer_begin)".  A call that FAILS after its argument checks (GM_ERR_DATA from the sweep's edge-count
 * read, GM_ERR_HIP) leaves the mini-batch UNDEFINED: part of the sample may be in the gradients.  The handle then refuses
 * accumulate and apply until the caller calls gm_trainer_begin again.  gm_train_step and an updating gm_train_rollout_step clear
 * the gradients and so end a pending mini-batch the same way; gm_train_rollout_step(update = 0) does not touch it.
 *
 * gm_trainer_apply is ONE update from the sum of the S accumulated gradients.  One single-thread launch computes, in float64,
 *     norm  = sqrt(sumsq) / S                                  -- the norm of the MEAN gradient; sumsq: gm_grad_sumsq of the buffer
 *     coef  = clipping ? min(1.0, max_grad_norm / (norm + 1e-6)) : 1.0          -- clip_grad_norm_'s formula
 *     scale = (float)(coef / (double)S)
 * and leaves norm and (double)scale in the record.  Per element g1 = scale * g, rounded on its own, then ADAM'S ARITHMETIC above
 * on g1, no operation contracted with another.  With S = 1 and no clipping scale is exactly 1.0f and the update has gm_train_step's
 * bits.  max_grad_norm <= 0 or +inf: no clipping.  The two launches of the norm are enqueued only when clipping is in force or
 * grad_norm_out (device, may be NULL) is given -- a non-NULL grad_norm_out REQUESTS the norm and receives it; without either,
 * grad_norm in the record is NaN and sumsq stays 0.  The update is SKIPPED when bad > 0 or sumsq is not finite: weights, both
 * moments, steps_applied and the beta powers keep their bits, steps_skipped goes up by one, and loss_out (device, may be NULL)
 * receives NaN; otherwise loss_out receives loss_sum / S.  One bad sample costs its whole mini-batch: with NaN activations on the
 * tape 0 * NaN has already reached the buffer, so nothing is taken back out of the sum.  After apply the mini-batch is over:
 * the next one starts with gm_trainer_begin.  Refused before any device call ("gm_trainer_apply: ...", GM_ERR_INVALID_ARGUMENT): a
 * null trainer, a NaN lr, a NaN max_grad_norm, no mini-batch begun, no sample accumulated (the handle counts them on the host).
 *
 * gm_grad_sumsq is the reduction on its own: sumsq_out[0] (device) = the float64 sum of (double)x[i] * (double)x[i] over `count`
 * floats -- squared in float64, so that 1e-30f and 1e30f both contribute.  gm_l1_loss's two passes: at most 128 workgroups of 256
 * threads; a thread walks its 16-byte groups in a fixed stride, then its elements of the scalar tail (count % 4), adding in
 * float64; a fixed tree inside the workgroup; one partial per workgroup, summed by one workgroup; no atomics: the same bits at every
 * run.  The trainer's gradient buffer has zero gaps between its tensors, so one call over it is the whole norm.  Refused before any
 * device call: a null pointer, count < 1, x off a 16-byte or ws off an 8-byte boundary (GM_ERR_INVALID_ARGUMENT); a workspace
 * below gm_grad_sumsq_workspace_bytes (0 for count < 1) is GM_ERR_WORKSPACE.  The workspace is written before it is read.
 * ------------------------------------------------------------------------------------------ */
int gm_trainer_begin(gm_trainer* t, void* stream);
int gm_train_step_accumulate(gm_trainer* t, const float* nodes, int64_t n_nodes, const float* edge_attr, const int64_t* edge_index,
                             int64_t n_edges, const float* target, int mask_col, double* loss_out /* device, may be NULL */,
                             void* ws, size_t ws_bytes, void* stream);
int gm_train_rollout_accumulate(gm_trainer* t, const float* obs0 /*[k,N,D]*/, int64_t n_nodes, const gm_feature_desc* fdesc,
                                int max_neighbours, const int32_t* rigid_rank, int64_t n_rigid,
                                const float* frames /*[steps,N,frame_dim]*/, int frame_dim, int64_t steps, int material_col,
                                const double* pos_scale /* host [3], may be NULL */, double* loss_out /* device, may be NULL */,
                                void* ws, size_t ws_bytes, void* stream);
/* A mini-batch of rollout windows of different sizes as ONE ragged rollout (additions to ABI 7; the table, rows and ranks as in
 * gm_rollout_ragged, fdesc->nodes_per_graph == 0).
 *
 * gm_rollout_l1_loss_ragged is gm_rollout_l1_loss per graph.  frames_host [n_graphs] are HOST pointers to device arrays
 * [steps, n_g, frame_dim] -- views into the graphs' recordings -- which travel by value in the kernel arguments.  losses_out
 * [n_graphs] (device doubles) and rows_counted_out [n_graphs] (device, may be NULL) are written in full:
 *     l_g = ((s0 / scale_0 + s1 / scale_1) + s2 / scale_2) / (steps * count_g)
 * with float64 sums over graph g's counted rows in the order of the single call on graph g alone (its workgroups, its stride --
 * the same kernels: the single call is the batch of one graph): l_g is that call's loss and does not depend on what shares the batch.  The transpose in d_records [steps,N,D] / d_final [k,N,D], both
 * written in full, has on graph g's counted rows gm_rollout_l1_loss's element values with count_g in place of count.  The state it
 * leaves for the launches behind it is the mini-batch's: the sum l_0 + l_1 + ... in graph order (float64) and the number of
 * non-finite l_g.  Workspace: gm_rollout_l1_loss_ragged_workspace_bytes(n_graphs).
 *
 * gm_train_rollout_accumulate_ragged is gm_train_rollout_accumulate on such a batch: one row kernel gathers the recorded poses of
 * every graph's rigid rows into one trajectory [steps, n_rigid, 3] (global ranks), then ONE ragged rollout keeping its windows, the
 * loss above, ONE reverse sweep into the trainer's gradients (gm_rollout_backward_train_ragged: one edge-count read per step) and one
 * single-thread launch on the mini-batch's record: samples += n_graphs, bad += the number of non-finite losses, loss_sum += their
 * sum.  It needs a begun mini-batch; gm_trainer_apply is unchanged (it divides by samples and skips on bad > 0).  update == 0 stops
 * after the loss: no gradient, no record, no mini-batch needed, no synchronisation.  losses_out [n_graphs]: device doubles.
 * Workspace: gm_train_rollout_ragged_workspace_bytes.  Refusals as gm_train_rollout_accumulate's and gm_rollout_ragged's. */
size_t gm_rollout_l1_loss_ragged_workspace_bytes(int64_t n_graphs);
int gm_rollout_l1_loss_ragged(const float* windows /*[steps,k,N,D]*/, const float* final_state /*[k,N,D]*/,
                              const float* const* frames_host /*[n_graphs]*/, int frame_dim, int64_t steps,
                              const int64_t* graph_offsets_host /*[n_graphs+1]*/, int64_t n_graphs, const gm_feature_desc* fdesc,
                              const int32_t* rigid_rank, int material_col, const double* pos_scale /* host [3], may be NULL */,
                              double* losses_out /* device [n_graphs] */, int64_t* rows_counted_out /* device [n_graphs], may be NULL */,
                              float* d_records, float* d_final, void* ws, size_t ws_bytes, void* stream);
size_t gm_train_rollout_ragged_workspace_bytes(const gm_model_desc* desc, const gm_feature_desc* fdesc, int64_t n_total,
                                               int64_t n_rigid_total, int64_t n_graphs, int max_neighbours, int64_t steps);
int gm_train_rollout_accumulate_ragged(gm_trainer* t, const float* obs0 /*[k,N,D]*/, const int64_t* graph_offsets_host /*[n_graphs+1]*/,
                                       int64_t n_graphs, const gm_feature_desc* fdesc, int max_neighbours, const int32_t* rigid_rank,
                                       int64_t n_rigid, const float* const* frames_host /*[n_graphs]*/, int frame_dim, int64_t steps,
                                       int material_col, const double* pos_scale /* host [3], may be NULL */, int update,
                                       double* losses_out /* device [n_graphs] */, void* ws, size_t ws_bytes, void* stream);
int gm_trainer_apply(gm_trainer* t, double lr, double max_grad_norm, double* loss_out /* device, may be NULL */,
                     double* grad_norm_out /* device, may be NULL: non-NULL requests the norm */, void* stream);
int gm_trainer_accum_record(const gm_trainer* t, void* record_host /* 48 bytes */, void* stream);
size_t gm_grad_sumsq_workspace_bytes(int64_t count);
int gm_grad_sumsq(const float* x, int64_t count, double* sumsq_out /* device, 1 */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Data-parallel training: several processes ("ranks"), each with a trainer over the same weights, share a mini-batch (additions to
 * ABI 7; no struct changes).  Every rank runs gm_trainer_begin and accumulates ITS samples; then, between accumulate and apply,
 *
 *     gm_trainer_contribution;  the caller's all-gather of the ranks' contributions;  gm_trainer_reduce;  gm_trainer_apply.
 *
 * The library links no communication library: it writes one contiguous device buffer per rank and reads `world` of them.  Who moves
 * the bytes (RCCL, MPI, gloo through host memory) is the caller's choice.  Every rank reduces the same bytes in the same order and
 * so applies the same update, bit for bit, whatever the collective does inside.
 *
 * A CONTRIBUTION is gm_trainer_contribution_bytes(t) bytes (0 for a null trainer): the trainer's flat gradient buffer -- its floats
 * in gm_model_create's tensor order, each tensor on a 16-byte boundary with zeros in the gaps, zeros up to a multiple of 16 bytes
 * -- and behind it a 32-byte tail
 *     { int64 samples, int64 bad, double loss_sum, int64 steps_applied }
 * whose first three fields are the mini-batch record's and whose fourth is the trainer record's.  gm_trainer_contribution writes
 * it to out_dev: one device-to-device copy and one single-thread launch.  It needs a begun mini-batch and changes nothing of it;
 * zero accumulated samples are allowed (a rank that owns nothing of a short last mini-batch contributes zeros).  poisoned != 0
 * writes all-zero gradients and the tail { 0, 1, 0.0, steps_applied } instead, begun mini-batch or not: what a rank sends after one
 * of its samples failed on the host, so that no peer waits for it and every rank skips the update.  Refused before any device call
 * ("gm_trainer_contribution: ...", GM_ERR_INVALID_ARGUMENT): a null trainer or pointer, out_bytes below the contribution's, out_dev
 * off a 16-byte boundary, no mini-batch begun (unless poisoned).
 *
 * gm_trainer_reduce reads `world` contributions, rank r's at contributions_dev + r * stride_bytes, all ranks in the same order.
 * gm_rank_sum adds their gradient parts into the trainer's own gradient buffer (which the contributions must not overlap), then one
 * single-thread launch sets the mini-batch record: samples and bad are the integer sums; loss_sum is rank 0's plus rank 1's plus
 * ..., float64 adds in rank order; sumsq, grad_norm and scale are as gm_trainer_begin leaves them (0.0, NaN, NaN).  bad goes up by
 * one more when the ranks' steps_applied are not all equal (replicas out of step), and by one more when the summed samples differ
 * from samples_total_host, the global sample count the caller knows from its sharding.  samples_total_host becomes the handle's
 * host-side count, so that gm_trainer_apply accepts the mini-batch without a read-back; apply then runs unchanged on the merged
 * record -- S, the norm, the clip, the skip rule, Adam -- so a bad sample on any rank skips the update on every rank.  With
 * world == 1 the gradient and the record keep their bits: contribution, reduce, apply is apply.  Refused before any device call
 * ("gm_trainer_reduce: ...", GM_ERR_INVALID_ARGUMENT): a null trainer or pointer, world outside 1..64, stride_bytes below
 * gm_trainer_contribution_bytes or no multiple of 16, contributions_dev off a 16-byte boundary, samples_total_host < 1, no
 * mini-batch begun.
 *
 * gm_rank_sum is the reduction on its own:  dst[i] = ((src[i] + src[stride_floats + i]) + src[2 * stride_floats + i]) + ...  over
 * `world` rows of `count` floats, every add a float32 add rounded on its own, strictly in rank order; world == 1 copies the bits.
 * One thread sums an element from its first rank to its last: no atomics, nothing depends on the grid, the same bits at every run.
 * Adam's flat walk: 16-byte groups in a grid stride over at most 2048 workgroups of 256 threads, then the scalar tail (count % 4).
 * It moves world reads and one write per element.  dst must not overlap src.  Refused before any device call ("gm_rank_sum: ...",
 * GM_ERR_INVALID_ARGUMENT): a null pointer, count < 1, world outside 1..64, stride_floats below count or no multiple of 4, src or
 * dst off a 16-byte boundary.
 * ------------------------------------------------------------------------------------------ */
int gm_rank_sum(const float* src, int64_t count, int world, int64_t stride_floats, float* dst, void* stream);
size_t gm_trainer_contribution_bytes(const gm_trainer* t);
int gm_trainer_contribution(gm_trainer* t, void* out_dev, size_t out_bytes, int poisoned, void* stream);
int gm_trainer_reduce(gm_trainer* t, const void* contributions_dev, int world, size_t stride_bytes, int64_t samples_total_host,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Moments of a resident recording (an addition to ABI 7).  Replaces the reduction of simulation/generate_metadata.py:24-45
 * (np.diff over the frames, np.diff again, np.mean and np.std over all rows of all files): what vel_mean, vel_std, acc_mean and
 * acc_std of metadata.json are made of.
 *
 * rec is one recording, [n_frames, n_nodes, data_dim] float32 row-major on the device; the positions are the `dim` (1..3)
 * contiguous columns from cart0.  Velocities are p[t+1] - p[t], accelerations (p[t+2] - p[t+1]) - (p[t+1] - p[t]) in that order,
 * both in float64 from the float32 positions.  material_col >= 0: only the rows whose column material_col equals material_value
 * IN FRAME 0 are counted (sand-only statistics); material_col < 0: every row, rigid rows included, as the reference does.
 *
 * out_device receives GM_RECORDING_STATS_DOUBLES (24) doubles, 8 per axis a = 0..2 at out_device + 8 * a:
 *     [0] number of velocities   [1] their mean   [2] their M2 = sum of (v - mean)^2
 *     [3] number of accelerations [4] their mean  [5] their M2
 *     [6] smallest position      [7] largest position        (exact float32 values, over every frame of the counted rows)
 * Axes past `dim` hold zeros.  The population variance (np.std's, ddof = 0) is M2 / count; the records of several recordings merge
 * by Chan's formula:  n = na + nb, d = mb - ma, mean = ma + d * nb / n, M2 = M2a + M2b + d * d * na * nb / n.  With no row
 * counted the counts, means and M2 are 0 and the range is (+inf, -inf).  A non-finite position in a counted row makes the means,
 * M2 and range of ITS axis non-finite and changes nothing else.
 *
 * Numerics: no sumsq - n * mean^2.  Every thread runs Welford's update on its samples, taken relative to the first velocity /
 * acceleration of the first counted row (a sample of the data, so that the running means have the size of the spread whatever
 * the drift); threads, waves, workgroups and the per-workgroup partials in the workspace are merged by Chan's formula, the
 * partials by one workgroup in index order.  No floating-point atomics: the same recording gives the same bits at every call.
 * A thread walks the frames of a node and then its next node, in a grid stride over at most GM_RECORDING_STATS_MAX_WORKGROUPS
 * workgroups of 256 threads; every position is read once.  Three launches (the shifts, the partials, the finish), no host
 * synchronisation.  The workspace (gm_recording_stats_workspace_bytes: 256 bytes for the shifts and one record per workgroup;
 * 0 for n_frames < 3 or n_nodes < 1) is written before it is read.
 *
 * Refused with GM_ERR_INVALID_ARGUMENT and a "gm_recording_stats: ..." message, before any device call: a null pointer,
 * n_frames < 3 (no acceleration exists), n_nodes < 1, dim outside 1..3, cart0 < 0 or cart0 + dim > data_dim, material_col >=
 * data_dim, a workspace below the query.
 * ------------------------------------------------------------------------------------------ */
#define GM_RECORDING_STATS_DOUBLES 24
#define GM_RECORDING_STATS_MAX_WORKGROUPS 1024
size_t gm_recording_stats_workspace_bytes(int64_t n_frames, int64_t n_nodes);
int gm_recording_stats(const float* rec /*[T,N,D] device*/, int64_t n_frames, int64_t n_nodes, int data_dim, int cart0,
                       int dim /*1..3*/, int material_col /* <0: all rows */, float material_value, double* out_device, void* ws,
                       size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (no reference counterpart; the reference only wraps model.forward in
 * time.time(), examples/optimise_traj.py:99-103).  Per model handle: when enabled, launches made on behalf of THIS
 * model are bracketed with HIP events on their launch stream; other handles and streams are unaffected.
 * kind: 0 processor edge kernel, 1 processor node kernel, 2 radius-graph build of gm_rollout_step (all its kernels),
 * 3 encoder kernels, 4 the rest of gm_rollout_step (state update + node features, destination sort + block tables + edge
 * features, clears, integration + window shift: kinds 0 .. 4 add up to the step); kind_mask has bit `kind` set for every kind
 * to record (0 disables; a newly enabled kind restarts its counters).  gm_model_profile_query synchronises on the recorded
 * events.  A kind records at most 4096 scopes: once more were opened, *launches comes back NEGATIVE (minus the number opened) and
 * *total_ms covers the first 4096 only.
 * ------------------------------------------------------------------------------------------ */
int gm_model_profile(gm_model* model, int kind_mask);
int gm_model_profile_query(const gm_model* model, int kind, int64_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* GNN_MANIP_HIP_H */
