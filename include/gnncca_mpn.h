/*
 * gnncca_mpn.h -- C ABI of the MI355X-native GNN-CCA message-passing path (libgnncca_mpn.so).
 *
 * The reference (vpulab/GNN-CCA) is pure Python and has NO native/FFI layer: the
 * interface a caller binds is the Python module surface `models.mpn.MOTMPNet` (models/mpn.py:144-299).
 * This header is therefore the boundary *below* that module: every entry point states which piece of
 * the reference's Python it replaces.  The Python mirror of MOTMPNet (gnn-cca_amd/mpn.py) is the only
 * intended caller and binds these symbols with ctypes.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `gnncca_stream_t` is a hipStream_t passed as void*.
 *   - all device pointers are raw HBM addresses owned by the caller; nothing is allocated or freed here.
 *   - every function returns a gnncca_status (0 = ok).  Nothing synchronises the stream except
 *     gnncca_read_graph_flags().  All kernels are enqueued on the given stream.
 *   - row-major fp32 everywhere at the boundary; `edge_index` is int64 [2][E] exactly as
 *     torch_geometric hands it to MOTMPNet.forward (models/mpn.py:266).
 */
#ifndef GNNCCA_MPN_H
#define GNNCCA_MPN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): gnncca_frames_io gained `counters_len` -- gnncca_frames_forward writes [3 N + 1 + G] int32 through `counters` (round 5 grew
 * it from [2 N + 1] without a version change: a caller built against that header would have been overrun) and now refuses a shorter buffer. */
#define GNNCCA_ABI_VERSION 2
#define GNNCCA_MAX_LAYERS 8

#if defined(GNNCCA_BUILD)
#define GNNCCA_API __attribute__((visibility("default")))
#else
#define GNNCCA_API
#endif

typedef void* gnncca_stream_t;

typedef enum gnncca_status {
    GNNCCA_OK = 0,
    GNNCCA_ERR_INVALID_ARG = 1,     /* null pointer, negative size, inconsistent dims            */
    GNNCCA_ERR_UNSUPPORTED = 2,     /* a legal GRAPH_NET_PARAMS this build has no HIP kernel for */
    GNNCCA_ERR_WORKSPACE = 3,       /* workspace_bytes < gnncca_workspace_bytes(...)             */
    GNNCCA_ERR_HIP = 4,             /* a HIP runtime call failed; see gnncca_last_hip_error()    */
    GNNCCA_ERR_NO_DEVICE = 5        /* no gfx950 device visible                                  */
} gnncca_status;

/* Aggregators of models/mpn.py:192-202 (torch_scatter scatter_add / scatter_mean / scatter_max). */
typedef enum gnncca_agg { GNNCCA_AGG_SUM = 0, GNNCCA_AGG_MEAN = 1, GNNCCA_AGG_MAX = 2 } gnncca_agg;

/* One Linear(+BatchNorm1d eval)(+ReLU) block of models/mlp.py:10-24.  Dropout is the identity in eval. */
typedef struct gnncca_layer {
    int32_t in_dim;
    int32_t out_dim;
    int32_t has_bn;   /* models/mlp.py:14  (use_batchnorm and dim != 1) */
    int32_t relu;     /* models/mlp.py:17  (dim != 1)                   */
} gnncca_layer;

typedef struct gnncca_mlp {
    int32_t n_layers; /* 0 = MLP absent (MLPGraphIndependent passes the input through, mpn.py:133-140) */
    gnncca_layer layers[GNNCCA_MAX_LAYERS];
} gnncca_mlp;

/* Everything MOTMPNet.__init__ derives from GRAPH_NET_PARAMS (models/mpn.py:154-247). */
typedef struct gnncca_mpn_dims {
    int32_t abi_version;        /* GNNCCA_ABI_VERSION */
    int32_t node_in;            /* encoder_feats_dict.nodes[arch].node_in_dim (2048 / 512)  */
    int32_t edge_in;            /* encoder_feats_dict.edges.edge_in_dim (4; 2 for ONLY_*)   */
    int32_t node_dim;           /* node_out_dim = H (32) */
    int32_t edge_dim;           /* edge_out_dim = EF (6) */
    int32_t agg;                /* gnncca_agg */
    int32_t num_enc_steps;      /* L, mpn.py:179 */
    int32_t num_class_steps;    /* mpn.py:180 */
    int32_t reattach_nodes;     /* mpn.py:207 */
    int32_t reattach_edges;     /* mpn.py:208 */
    gnncca_mlp enc_node;        /* encoder.node_mlp                (mpn.py:173) */
    gnncca_mlp enc_edge;        /* encoder.edge_mlp                              */
    gnncca_mlp edge_mlp;        /* MPNet.edge_model.edge_mlp       (mpn.py:221) */
    gnncca_mlp node_mlp;        /* MPNet.node_model.node_mlp       (mpn.py:236) */
    gnncca_mlp cls_edge;        /* classifier.edge_mlp             (mpn.py:174) */
} gnncca_mpn_dims;

/* Optional debug taps (all nullable): the latents the golden vectors also hold.  Row-major fp32, edges
 * in the caller's (original) edge order. */
typedef struct gnncca_trace {
    float* h_enc;    /* [N][H]       encoder node output   (mpn.py:270) */
    float* e_enc;    /* [E][EF]      encoder edge output                */
    float* h_steps;  /* [L][N][H]    node latents after each step (mpn.py:288) */
    float* e_steps;  /* [L][E][EF]   edge latents after each step       */
} gnncca_trace;

/* Bits of the per-call graph flag word (device side, read back with gnncca_read_graph_flags). */
#define GNNCCA_GRAPH_UNSORTED 1u   /* `row` was not non-decreasing: the stable device sort ran     */
#define GNNCCA_GRAPH_BAD_INDEX 2u  /* an index outside [0,N): kernels skipped, logits set to NaN   */
#define GNNCCA_GRAPH_IRREGULAR 4u  /* informational: a big batch with a degree above the padded edge-state
                                      stride chosen from E/N; the step kernels used the compact layout */

GNNCCA_API int gnncca_abi_version(void);
GNNCCA_API const char* gnncca_status_string(int status);
GNNCCA_API int gnncca_last_hip_error(void); /* hipError_t of the last failed HIP call on this thread, 0 if none */

/* Number of `float*` entries gnncca_pack_weights expects, and the canonical order: for each MLP in the
 * order enc_node, enc_edge, edge_mlp, node_mlp, cls_edge, for each layer: weight[out][in], bias[out],
 * then if has_bn: bn_weight, bn_bias, bn_running_mean, bn_running_var (each [out]).
 * Replaces: nothing in the reference (it keeps nn.Parameters); this is the state_dict -> HBM layout step
 * behind MOTMPNet.load_state_dict / .cuda() (main.py:78-82). */
GNNCCA_API int gnncca_param_count(const gnncca_mpn_dims* dims);

/* Bytes of the packed weight blob. 0 on invalid dims. */
GNNCCA_API size_t gnncca_packed_weights_bytes(const gnncca_mpn_dims* dims);

/* HOST function: folds eval-mode BatchNorm into the preceding Linear, splits the MPN weights by input
 * block ([W_src|W_dst|W_edge], [W_node|W_edge], cat order of mpn.py:68 and mpn.py:97), builds the
 * per-node projection matrix, and writes the blob into `packed_host` (the caller uploads it, or
 * broadcasts it to the other ranks over RCCL).  `params` are host pointers in the canonical order. */
GNNCCA_API int gnncca_pack_weights(const gnncca_mpn_dims* dims, const float* const* params, int n_params,
                        void* packed_host, size_t packed_bytes);

/* DEVICE variant of gnncca_pack_weights for the tuned (H = 32, EF = 6) family: the same blob, byte for byte, built by
 * one kernel straight from the parameter tensors in HBM -- a training step (train.py:492-494: the optimizer has just
 * rewritten every parameter) or a load_state_dict() never moves the weights through the host.
 *   gnncca_pack_program(dims, program_host, bytes)  HOST: the copy/fold program for `dims`
 *                                                   (gnncca_pack_program_bytes() bytes); upload it once.
 *   gnncca_pack_weights_device(...)                 enqueues the packing on `stream`.  `params_dev`: a HOST array of
 *                                                   DEVICE pointers in the canonical order; `packed_dev` must have
 *                                                   been zero-filled once (padding words are not rewritten).
 * GNNCCA_ERR_UNSUPPORTED for the generic family (use the host packer). */
GNNCCA_API size_t gnncca_pack_program_bytes(void);
GNNCCA_API int gnncca_pack_program(const gnncca_mpn_dims* dims, void* program_host, size_t program_bytes);
GNNCCA_API int gnncca_pack_weights_device(const gnncca_mpn_dims* dims, const float* const* params_dev, int n_params,
                               const void* program_dev, void* packed_dev, size_t packed_bytes, gnncca_stream_t stream);

/* Bytes of device scratch one forward over a graph of N nodes / E edges needs. */
GNNCCA_API size_t gnncca_workspace_bytes(const gnncca_mpn_dims* dims, int64_t n_nodes, int64_t n_edges);

/* Whether this build has HIP kernels for `dims` (GNNCCA_OK) or not (GNNCCA_ERR_UNSUPPORTED). */
GNNCCA_API int gnncca_supported(const gnncca_mpn_dims* dims);

/* Replaces MOTMPNet.forward (models/mpn.py:250-299) in eval mode: encoder (mpn.py:270), L message
 * passing steps (MetaLayer.forward mpn.py:32-54 = EdgeModel 59-69 + NodeModel 71-101 + aggregator
 * 192-202) and the edge classifier on the last num_class_steps steps (mpn.py:290-297).
 *   x          [N][node_in]  fp32      data.x
 *   edge_index [2][E]        int64     data.edge_index (any order; row-sorted graphs take the fast path)
 *   edge_attr  [E][edge_in]  fp32      data.edge_attr
 *   logits_out [n_out][E]    fp32      n_out = gnncca_num_outputs(dims); the list 'classified_edges'
 * Inputs are read-only.  Asynchronous on `stream`. */
GNNCCA_API int gnncca_mpn_forward(const gnncca_mpn_dims* dims, const void* packed_dev, const float* x,
                       const int64_t* edge_index, const float* edge_attr, int64_t n_nodes,
                       int64_t n_edges, void* workspace, size_t workspace_bytes, float* logits_out,
                       const gnncca_trace* trace, gnncca_stream_t stream);

/* Diagnostic twin of gnncca_mpn_forward for bench.py: attaches a start and a stop hipEvent to every kernel dispatch
 * (hipExtLaunchKernelGGL), SYNCHRONISES the stream and returns each kernel's own execution time -- what
 * rocprofv3 --kernel-trace reports.  Never used on the product path. */
#define GNNCCA_PROFILE_MAX 64
enum { GNNCCA_K_PLAN_ROWS = 0, GNNCCA_K_PLAN_SORT = 1, GNNCCA_K_ENC_GEMM = 2, GNNCCA_K_ENC_REDUCE = 3,
       GNNCCA_K_ENC_TAIL = 4, GNNCCA_K_STEP = 5, GNNCCA_K_STEP_LAST = 6 };
typedef struct gnncca_profile {
    uint32_t options;                   /* in: GNNCCA_OPT_* for the profiled forward */
    int32_t count;                      /* launches recorded */
    int32_t kind[GNNCCA_PROFILE_MAX];   /* GNNCCA_K_* */
    float ms[GNNCCA_PROFILE_MAX];       /* hipEventElapsedTime(start, stop) of the dispatch's own events */
} gnncca_profile;
GNNCCA_API int gnncca_mpn_forward_profiled(const gnncca_mpn_dims* dims, const void* packed_dev, const float* x,
                                const int64_t* edge_index, const float* edge_attr, int64_t n_nodes,
                                int64_t n_edges, void* workspace, size_t workspace_bytes, float* logits_out,
                                gnncca_stream_t stream, gnncca_profile* profile);

/* Train-mode Dropout (models/mlp.py:20-21; config keys `dropout_p` of encoder_feats_dict / edge_model_feats_dict /
 * node_model_feats_dict / classifier_feats_dict).  Masks are generated on the device by a counter-based hash of
 * (*seed_dev, tensor, element) and are NOT stored: the backward evaluates the same hash, so both calls of one training
 * iteration must see the same seed word.  p = 0 switches a group off; a null pointer switches everything off. */
typedef struct gnncca_dropout {
    float p_enc;    /* encoder.node_mlp and encoder.edge_mlp */
    float p_edge;   /* MPNet.edge_model.edge_mlp             */
    float p_node;   /* MPNet.node_model.node_mlp (the messages, before aggregation) */
    float p_cls;    /* classifier.edge_mlp                   */
    const uint64_t* seed_dev;   /* DEVICE word */
} gnncca_dropout;

/* gnncca_mpn_forward with options.  GNNCCA_OPT_EDGE_STATE_BF16: keep the edge latents BETWEEN steps as bf16 in HBM
 * (round to nearest even; all arithmetic, the classifier input and every other buffer stay fp32) -- halves the
 * dominant traffic of the step kernels; honoured by the specialised kernels (shipped config shape), ignored elsewhere.
 * Measured effect on the logits: DESIGN.md section 5. */
#define GNNCCA_OPT_EDGE_STATE_BF16 1u
/* GNNCCA_OPT_ENC_SPLIT3: on batches of >= 4096 nodes the first encoder layer (models/mpn.py:131, 2048 -> 128) runs as a
 * split-bf16 MFMA GEMM; by default with the six products that give fp32-level accuracy, with this option with the three
 * leading ones (x0 w0 + x0 w1 + x1 w0): ~2^-17 relative on that layer's pre-activations (encoder output 5e-6 from fp64
 * instead of 3e-7 .. 1e-6), measured logit deviation 1.5e-7 (tolerance 1e-4), GEMM 19-28 % faster.  Off by default. */
#define GNNCCA_OPT_ENC_SPLIT3 2u
/* GNNCCA_OPT_ENC_UNSPLIT: a forward over >= 4096 nodes never splits K in that layer (for the encoder shapes named below).  By
 * default mid-size batches (a few thousand to a few ten thousand nodes) run it split-K (partial slabs + a tail launch) and the
 * largest ones un-split, so a graph's logits agree across batch sizes within rounding only (<= 2e-6 asserted, 6e-8 measured).
 * With this option the mid-size batches take an un-split 32-row kernel whose per-element arithmetic is the big un-split
 * kernel's: a graph's logits are then BIT FOR BIT independent of the batch (or the shard of a sharded batch) it is computed in,
 * as long as that batch has >= 4096 nodes.
 * This holds for fast-family node encoders of exactly two layers, the first 128 wide with node_in_dim a multiple of 256, and
 * without reattach_initial_nodes (the shipped 2048 -> 128 -> 32 among them): the un-split kernels finish the encoder in their
 * epilogue, which needs that shape.  Any other node encoder still runs its first layer split-K on mid-size batches (the option
 * only keeps it on the bf16 split GEMMs), and its logits agree across batch sizes within rounding only.
 * Price: encoder 48 instead of 44 us at 8192 nodes (plan launch included), 87 instead of 70 us at 16 384.
 * Off by default. */
#define GNNCCA_OPT_ENC_UNSPLIT 4u
/* GNNCCA_OPT_COLUMN_RANGES (forwards with >= 2 message-passing steps, specialised kernels): step 1 derives, per source node, whether
 * its target ids form at most two contiguous runs -- true for every graph the reference builds (inference.py:209-216: per camera,
 * cartesian_prod with the detections of the other cameras) and for dense graphs -- and steps 2 ... L then COMPUTE the target ids
 * instead of streaming them (4 of 56 B per edge, and the P_dst gather no longer waits for an id); a forward with any other node
 * streams them on every step, as without the option.  Results are bit for bit the same either way
 * (tests/test_gpu_column_ranges.py).  OFF by default: measured on MI355X it gains nothing -- 1 x dense256 27.6 -> 28.4 us per
 * forward, 64 x dense128 99.9 -> 101.3, 64 x dense256 / 512 x dense128 / 200 x dense256 within noise (profiles/r04_logs/ab_ranges1.log):
 * the id load and the gather behind it are not on these launches' critical path, and step 1 pays for the derivation. */
#define GNNCCA_OPT_COLUMN_RANGES 8u
GNNCCA_API int gnncca_mpn_forward_ex(const gnncca_mpn_dims* dims, const void* packed_dev, const float* x,
                                     const int64_t* edge_index, const float* edge_attr, int64_t n_nodes,
                                     int64_t n_edges, void* workspace, size_t workspace_bytes, float* logits_out,
                                     const gnncca_trace* trace, uint32_t options, gnncca_stream_t stream);

/* len(outputs['classified_edges']) for these dims (mpn.py:277-297). */
GNNCCA_API int gnncca_num_outputs(const gnncca_mpn_dims* dims);

/* ---- the step before the MPN -- graph construction + edge attributes ------------------
 * Replaces the per-frame Python of inference.py:189-279 (duplicated at train.py:257-361 and 616-692).
 * All pointers are device memory; one entry per detection (node) unless noted; frames are concatenated. */
typedef struct gnncca_frames {
    const double* xw;          /* ground-plane x  (data_df['xw'], float64 as pandas holds it)                 */
    const double* yw;          /* ground-plane y                                                              */
    const double* max_dist;    /* [G]   CONFIG['CONV_TO_M'][dataset] of each frame (inference.py:239)        */
    const int32_t* person_id;  /* data_df['id'] (any relabelling that preserves equality)                     */
    const int32_t* cam;        /* data_df['id_cam']                                                           */
    const int32_t* graph_of;   /* frame index of each node                                                    */
    const int32_t* graph_ptr;  /* [G+1] node range of each frame                                              */
    const int32_t* src_order;  /* node ids in the order the reference emits their out-edges (camera-major)     */
    const int32_t* edge_ptr;   /* [N+1] first edge of each position of src_order                              */
} gnncca_frames;
enum { GNNCCA_EDGE_ATTR_FULL = 0, GNNCCA_EDGE_ATTR_ONLY_APPEARANCE = 1, GNNCCA_EDGE_ATTR_ONLY_DIST = 2 };

/* out = x / max(||column||_2, 1e-12): F.normalize(x, p=2, dim=0) of inference.py:189-190.
 * scratch: (ceil(n_rows/64) + 1) * n_cols floats. */
GNNCCA_API int gnncca_normalize_columns(const float* x, int64_t n_rows, int64_t n_cols, float* scratch,
                                        float* out, gnncca_stream_t stream);
/* The same for up to TWO matrices of n_rows <= 4096 rows (the reid and the node embeddings of a batch of frames,
 * inference.py:189-190) in ONE launch; bit for bit gnncca_normalize_columns' results.  x1 may be NULL (n_cols1 = 0).
 * More rows: GNNCCA_ERR_UNSUPPORTED (use gnncca_normalize_columns). */
GNNCCA_API int gnncca_normalize_columns2(const float* x0, int64_t n_cols0, float* out0, const float* x1, int64_t n_cols1,
                                         float* out1, int64_t n_rows, gnncca_stream_t stream);

/* HOST side of the graph construction: the edge enumeration of a batch of frames (inference.py:207-212: per frame, cameras in
 * np.unique order, a camera's nodes in ascending id, each connected to every node of the OTHER cameras) and the staging image that
 * gnncca_build_edges reads, written into host memory `staging` (pinned memory lets the caller upload it without blocking):
 *   f64 xw[n], yw[n], max_dist[g];  i64 ids[n];  i32 person[n], cam[n], graph_of[n], graph_ptr[g+1], src_order[n], edge_ptr[n+1],
 *   edge_ptr_g[g+1]  (first edge of each frame)
 * -- the fields of gnncca_frames at those offsets once uploaded.  All inputs are host arrays, one entry per detection (frames
 * concatenated) or per frame.  Returns the number of edges E >= 0, or -status (graph_sizes that do not sum to n: INVALID_ARG;
 * 2^31 edges or more: UNSUPPORTED).  Replaces the Python list comprehensions of inference.py:199-216. */
GNNCCA_API size_t gnncca_plan_frames_bytes(int64_t n_nodes, int64_t n_frames);
GNNCCA_API int64_t gnncca_plan_frames(const double* xw, const double* yw, const int64_t* ids, const int64_t* id_cam, int64_t n_nodes,
                                      const int64_t* graph_sizes, const double* max_dist, int64_t n_frames, void* staging,
                                      size_t staging_bytes);

/* edge_index [2][E] int64, edge_attr [E][4 or 2] fp32, edge_labels [E] fp32 in the reference's edge order:
 * cartesian_prod per camera (inference.py:207-212), ground-plane L2 and L1 distance / max_dist in float64 then
 * cast (229-242), F.pairwise_distance and F.cosine_similarity of the reid rows (222-226), same-identity labels
 * (262-266); node ids are the batch-global ones Batch.from_data_list produces (269-279). */
GNNCCA_API int gnncca_build_edges(const gnncca_frames* frames, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                  int64_t n_edges, int32_t mode, int64_t* edge_index_out, float* edge_attr_out,
                                  float* edge_labels_out, gnncca_stream_t stream);

/* ---- row N1 with a capped neighbourhood: every detection keeps its k nearest cross-camera candidates -----------
 * What is kept identical to the reference (inference.py:207-266): the enumeration (sources camera-major inside a frame, a source's
 * targets in ascending node id), the four (or two) attributes and the label of every edge that is kept -- the bits gnncca_build_edges
 * writes for that edge.  THE PRUNING ITSELF HAS NO COUNTERPART IN THE REFERENCE, which only ever builds the complete cross-camera graph.
 *
 * For source i with deg_i cross-camera candidates in its own frame, the min(top_k, deg_i) candidates of smallest key are kept:
 *   GNNCCA_RANK_BY_GROUND  the ground-plane L2 distance in float64, before the division by max_dist (inference.py:229-237)
 *   GNNCCA_RANK_BY_REID    the F.pairwise_distance value of the reid rows, the fp32 number that goes into edge_attr (inference.py:222)
 * ties to the smaller destination node id.  The key need not be an emitted attribute (RANK_BY_REID with ONLY_DIST is legal and reads
 * `reid`).  The kept edges of a source stay in the dense order, so the result is a subsequence of gnncca_build_edges' edge list and, for
 * top_k >= max deg, that list bit for bit.  The graph is DIRECTED: i may keep j while j drops i (gnncca_build_edges_topk_sym_* below
 * close it under reversal, as the union or as the mutual pairs).
 *
 * gnncca_plan_frames_ex: gnncca_plan_frames with a cap -- the same staging image, edge_ptr / edge_ptr_g counting min(top_k, deg) edges
 * per source (top_k == 0: no cap, gnncca_plan_frames' image byte for byte; top_k < 0: INVALID_ARG).  Returns E = sum min(top_k, deg)
 * and writes the largest UNCAPPED deg of the batch through max_deg_out (nullable): what gnncca_build_edges_topk sizes its LDS by.
 *
 * gnncca_build_edges_topk: `frames` is the uploaded image of gnncca_plan_frames_ex(top_k), n_edges its return value, max_deg its
 * max_deg_out (any upper bound of the batch's deg will do; a source with more candidates than declared is left unwritten).  One launch,
 * no workspace, no atomics, no synchronisation, capturable.  max_deg > GNNCCA_TOPK_MAX_DEG: GNNCCA_ERR_UNSUPPORTED, nothing launched. */
#define GNNCCA_TOPK_MAX_DEG 4096
enum { GNNCCA_RANK_BY_GROUND = 0, GNNCCA_RANK_BY_REID = 1 };
GNNCCA_API int64_t gnncca_plan_frames_ex(const double* xw, const double* yw, const int64_t* ids, const int64_t* id_cam, int64_t n_nodes,
                                         const int64_t* graph_sizes, const double* max_dist, int64_t n_frames, int64_t top_k,
                                         void* staging, size_t staging_bytes, int32_t* max_deg_out);
GNNCCA_API int gnncca_build_edges_topk(const gnncca_frames* frames, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                       int64_t n_edges, int32_t mode, int32_t top_k, int32_t rank_by, int32_t max_deg,
                                       int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out, gnncca_stream_t stream);

/* ---- row N1 with a ground-plane gate: cross-camera candidates within a radius -----------------------------------------------------
 * What is kept identical to the reference (inference.py:207-266): the enumeration and the attributes / label of every kept edge -- the
 * bits gnncca_build_edges writes for that edge.  THE GATE HAS NO COUNTERPART IN THE REFERENCE'S GRAPH BUILD, which only builds the
 * complete cross-camera graph.
 *
 * Definition.  For source i and a cross-camera candidate j of its own frame g:
 *   s = dx*dx + dy*dy with dx = xw[i] - xw[j], dy = yw[i] - yw[j]: two products and one sum, each rounded once in fp64, no FMA
 *     contraction.
 *   t_g = radius for GNNCCA_RADIUS_UNIT_GROUND (the units of xw / yw, before the division by max_dist).
 *   t_g = radius * max_dist[g] (one rounded product) for GNNCCA_RADIUS_UNIT_MAX_DIST (mixed-data-set batches; a gate stated in the units
 *     of edge_attr[:, 0]).
 *   t2_g = t_g * t_g (one rounded product).  The edge is kept iff s <= t2_g.
 * The test is on the squared distance on purpose: it needs no square root on the host, s(i, j) == s(j, i) bit for bit, and the host
 * and the device evaluate the identical IEEE sequence.  A NaN anywhere compares false, so a pair involving a NaN position is dropped;
 * radius = inf keeps every pair without a NaN.  radius is a finite number >= 0 or inf; anything else (NaN, negative, an unknown unit) is
 * GNNCCA_ERR_INVALID_ARG before anything is written or launched.  The kept edges stay in the dense order: the result is a subsequence of
 * gnncca_build_edges' edge list, a kept edge carries the dense build's bits (index, attributes, label), it is closed under reversal by
 * construction, and for radius = inf on NaN-free positions it is the dense build bit for bit.  A source, a frame or a whole batch may end
 * with no edge: E == 0 is legal.
 *
 * gnncca_plan_frames_radius: gnncca_plan_frames with the gate -- the same staging image (same fields, same byte count), edge_ptr /
 * edge_ptr_g counting the kept candidates per source; returns E (radius = inf, NaN-free positions: gnncca_plan_frames' image byte for
 * byte).  Every unordered pair of a frame is evaluated once: O(sum_g n_g^2 / 2) host work.  A batch whose DENSE edge count reaches 2^31
 * is refused (UNSUPPORTED) whatever the radius would keep.
 *
 * gnncca_build_edges_radius: `frames` is the uploaded image of gnncca_plan_frames_radius for the same radius / unit, n_edges its return
 * value.  One launch, no workspace, no LDS, no atomics, no synchronisation, capturable.  The reid rows are read for the kept candidates
 * only.  A source whose kept count on the device disagrees with the plan's run is left unwritten (never written beyond its run). */
enum { GNNCCA_RADIUS_UNIT_GROUND = 0, GNNCCA_RADIUS_UNIT_MAX_DIST = 1 };
GNNCCA_API int64_t gnncca_plan_frames_radius(const double* xw, const double* yw, const int64_t* ids, const int64_t* id_cam, int64_t n_nodes,
                                             const int64_t* graph_sizes, const double* max_dist, int64_t n_frames, double radius,
                                             int32_t unit, void* staging, size_t staging_bytes);
GNNCCA_API int gnncca_build_edges_radius(const gnncca_frames* frames, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                         int64_t n_edges, int32_t mode, double radius, int32_t unit, int64_t* edge_index_out,
                                         float* edge_attr_out, float* edge_labels_out, gnncca_stream_t stream);

/* ---- the capped neighbourhood, closed under reversal ('union' / 'mutual') ------------------------------------------------------
 * With D the directed edge set of gnncca_build_edges_topk for the same top_k / rank_by (same keys, ties to the smaller destination id):
 *   GNNCCA_SYMMETRIC_UNION   keeps the dense edge (i, j) iff (i, j) in D or  (j, i) in D
 *   GNNCCA_SYMMETRIC_MUTUAL  keeps it                   iff (i, j) in D and (j, i) in D
 * Whether i is in j's list is j's own selection (the key bits j's wave ranks with: the reid key is not symmetric, F.pairwise_distance
 * adds its eps to a - b); no key is evaluated from two sides, so the result is closed under reversal by construction.  It is a
 * subsequence of gnncca_build_edges' list in its order, a kept edge carries that build's bits, mutual is a subset of D and D of union,
 * and for top_k >= max deg both are the dense build.  A frame or a source may end with no edge (E == 0 is legal).
 * LIKE THE CAP, THE CLOSURE HAS NO COUNTERPART IN THE REFERENCE, which only builds complete graphs (every pair in both directions;
 * its remove_edges_single_direction deletes an active edge whose reverse is not active -- what a directed capped list feeds it).
 *
 * E depends on the data, so the build is two calls with one host wait between them:
 *   gnncca_build_edges_topk_sym_count   three launches: every source's selection as a bit row, the closure and the per-source counts,
 *       and a scan that OVERWRITES frames->edge_ptr [N + 1] (the staging image's words; the plan's capped values) and edge_ptr_g_dev
 *       [G + 1] (the image's per-frame edge offsets, or any int32 [G + 1]) with the symmetric layout.  edge_ptr_g_dev[G] is E: the caller
 *       copies those G + 1 words to the host behind this call and waits for them.
 *   gnncca_build_edges_topk_sym_emit    one launch: edge_index / edge_attr / edge_labels [n_edges = E] from the closed rows.
 * `frames` is the uploaded image of gnncca_plan_frames_ex (any top_k; its max_deg_out is `max_deg`), graph_sizes the HOST array the plan
 * was made from (it sizes the bit matrices; sizes that do not sum to n_nodes: INVALID_ARG).  workspace: ..._sym_bytes(graph_sizes,
 * n_frames) = two bit matrices of sum_g n_g ceil(n_g / 64) 64-bit words + n_nodes int32 counts, 8-byte aligned, the SAME buffer in both
 * calls.  No atomics; bit for bit the same from run to run.  Every argument is checked before the first launch (max_deg >
 * GNNCCA_TOPK_MAX_DEG: GNNCCA_ERR_UNSUPPORTED); a source with more candidates than declared selects nothing.  Afterwards the image
 * serves gnncca_build_edges_topk_backward, the post-processing and gnncca_eval_frames unchanged (a source's run is ascending in the
 * destination, frames are contiguous). */
enum { GNNCCA_SYMMETRIC_UNION = 1, GNNCCA_SYMMETRIC_MUTUAL = 2 };
GNNCCA_API size_t gnncca_build_edges_topk_sym_bytes(const int64_t* graph_sizes, int64_t n_frames);
GNNCCA_API int gnncca_build_edges_topk_sym_count(const gnncca_frames* frames, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                                 const int64_t* graph_sizes, int64_t n_frames, int32_t top_k, int32_t rank_by,
                                                 int32_t max_deg, int32_t symmetric, void* workspace, size_t workspace_bytes,
                                                 int32_t* edge_ptr_g_dev, gnncca_stream_t stream);
GNNCCA_API int gnncca_build_edges_topk_sym_emit(const gnncca_frames* frames, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                                const int64_t* graph_sizes, int64_t n_frames, int64_t n_edges, int32_t mode,
                                                const void* workspace, size_t workspace_bytes, int64_t* edge_index_out,
                                                float* edge_attr_out, float* edge_labels_out, gnncca_stream_t stream);

/* ---- backward of row N1: gradients of the graph build reach the RAW embeddings ------------------------------
 * The reference's statements are plain torch ops, so with the torch.no_grad() around its CNN (train.py:248-253) removed autograd
 * differentiates them: F.normalize(.., p=2, dim=0) (train.py:257-259, inference.py:189-190), the gathers, F.pairwise_distance and
 * F.cosine_similarity of the reid rows (train.py:306-308, inference.py:222-226), the stack of node rows (train.py:344, 357).  The
 * ground-plane attributes go through numpy / sklearn there and carry no gradient; neither do they here.
 * Both entry points: no atomics, fp32 accumulation, bit for bit the same from run to run, everything on `stream`, no synchronisation.
 *
 * gnncca_build_edges_backward: grad_reid_out [N][R] = d loss / d (the reid table gnncca_build_edges read) from grad_edge_attr
 * [E][4 or 2] (only its emb / cos columns are read) and the FORWARD's edge_attr (its emb / cos values).  `frames` is the staged image of
 * the forward.  Overwrites grad_reid_out; detections without a cross-camera partner get a zero row.  E == 0 or
 * GNNCCA_EDGE_ATTR_ONLY_DIST: zeros (a memset, no kernel).  workspace: gnncca_build_edges_backward_bytes(n_nodes), 16-byte aligned.
 * A reid row whose norm is below F.cosine_similarity's 1e-8 clamp is outside the parity contract: its gradient is finite, not torch's. */
GNNCCA_API size_t gnncca_build_edges_backward_bytes(int64_t n_nodes);
GNNCCA_API int gnncca_build_edges_backward(const gnncca_frames* frames, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                           int64_t n_edges, int32_t mode, const float* edge_attr, const float* grad_edge_attr,
                                           void* workspace, size_t workspace_bytes, float* grad_reid_out, gnncca_stream_t stream);
/* gnncca_build_edges_topk_backward: the same for the edge list of gnncca_build_edges_topk (the selection is piecewise constant: the
 * gradient flows through the emb / cos attributes of the KEPT edges only).  `frames` is the staged image of that forward
 * (gnncca_plan_frames_ex), `edge_index` [2][E] the forward's output, edge_attr / grad_edge_attr [E][4 or 2] in its edge order.  Same
 * kernels and summation order as gnncca_build_edges_backward -- the slot of (i -> j) is searched in i's ascending destination run
 * instead of derived from the plan, an absent edge contributes zero -- so there are no atomics, the result is bit for bit the same from
 * run to run, and for top_k >= max deg it is gnncca_build_edges_backward's, bit for bit.  Workspace: ..._topk_backward_bytes(n_nodes). */
GNNCCA_API size_t gnncca_build_edges_topk_backward_bytes(int64_t n_nodes);
GNNCCA_API int gnncca_build_edges_topk_backward(const gnncca_frames* frames, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                                int64_t n_edges, int32_t mode, const int64_t* edge_index, const float* edge_attr,
                                                const float* grad_edge_attr, void* workspace, size_t workspace_bytes,
                                                float* grad_reid_out, gnncca_stream_t stream);
/* Backward of gnncca_normalize_columns (y = x / nrm_c, nrm_c = max(||x[:, c]||, 1e-12)):
 *   grad_x = (grad_out - y * sum_rows(grad_out * y)) / nrm_c
 * from the forward's INPUT x (the norms are recomputed with the forward's own ordered sums).  Any number of rows; scratch:
 * gnncca_normalize_columns_backward_bytes(n_rows, n_cols).  ...backward2: up to two matrices of n_rows <= 4096 rows in ONE launch, bit for
 * bit the same results; more rows: GNNCCA_ERR_UNSUPPORTED.  x1 may be NULL (n_cols1 = 0). */
GNNCCA_API size_t gnncca_normalize_columns_backward_bytes(int64_t n_rows, int64_t n_cols);
GNNCCA_API int gnncca_normalize_columns_backward(const float* x, const float* grad_out, int64_t n_rows, int64_t n_cols, void* scratch,
                                                 size_t scratch_bytes, float* grad_x, gnncca_stream_t stream);
GNNCCA_API int gnncca_normalize_columns_backward2(const float* x0, const float* grad_out0, int64_t n_cols0, float* grad_x0,
                                                  const float* x1, const float* grad_out1, int64_t n_cols1, float* grad_x1,
                                                  int64_t n_rows, gnncca_stream_t stream);

/* ---- the step after the MPN -- threshold, pruning, flow counts, identity clusters --------
 * probs = sigmoid(logits), predictions = (probs >= 0.5) as int64 0/1 (inference.py:286-291). */
GNNCCA_API int gnncca_post_threshold(const float* logits, int64_t n_edges, float* probs_out,
                                     int64_t* predictions_out, gnncca_stream_t stream);
/* The same at another operating point (one chosen with gnncca_eval_sweep): probs as above, predictions = ((double)probs >= at).  The
 * comparison is made in fp64 against the widened fp32 probability; with at = 0.5 both outputs are gnncca_post_threshold's bit for bit.
 * `at` must be a number (a NaN is GNNCCA_ERR_INVALID_ARG). */
GNNCCA_API int gnncca_post_threshold_at(const float* logits, int64_t n_edges, double at, float* probs_out, int64_t* predictions_out,
                                        gnncca_stream_t stream);
GNNCCA_API size_t gnncca_post_workspace_bytes(int64_t n_nodes, int64_t n_edges);
/* pruned_out[k] = predictions[k] && the reverse edge is active too (utils.remove_edges_single_direction,
 * libs/utils.py:387-404); flow_out / flow_in [N] int32 = active pruned edges leaving / entering each node
 * (scatter_add at libs/utils.py:54-55); labels_out [N] int32 = smallest node id of the node's connected component
 * over the pruned edges, *n_clusters_out = number of components incl. isolated nodes (the partition
 * utils.compute_SCC_and_Clusters, libs/utils.py:295-317, returns on the pruned graph).  edge_index may be in any
 * order.  The bridge-based rounding / splitting heuristics stay on the host. */
GNNCCA_API int gnncca_post_prune_cluster(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes,
                                         int64_t n_edges, void* workspace, size_t workspace_bytes,
                                         int64_t* pruned_out, int32_t* flow_out, int32_t* flow_in,
                                         int32_t* labels_out, int32_t* n_clusters_out, gnncca_stream_t stream);
/* The same over a batch of frame graphs laid out as Batch.from_data_list lays them out (inference.py:279): frame g owns
 * nodes [node_ptr[g], node_ptr[g+1]) and the contiguous edges [edge_ptr[g], edge_ptr[g+1]) (int32 arrays of
 * n_frames + 1 entries in DEVICE memory).  Components never cross frames, so each frame's clustering runs in its own
 * workgroup, frames-wide in parallel. */
GNNCCA_API int gnncca_post_prune_cluster_frames(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes,
                                                int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev,
                                                int32_t n_frames, void* workspace, size_t workspace_bytes,
                                                int64_t* pruned_out, int32_t* flow_out, int32_t* flow_in,
                                                int32_t* labels_out, int32_t* n_clusters_out, gnncca_stream_t stream);

/* The same with the two TRIGGER bits of the host heuristics per frame (or for the whole graph when no frame ranges are given):
 * triggers_out[g] bit 0 (GNNCCA_POST_TRIGGER_ROUNDING) = a node of frame g has flow_out or flow_in > 3 after the pruning -- the condition
 * under which utils.compute_rounding changes anything (libs/utils.py:58-62); bit 1 (GNNCCA_POST_TRIGGER_SPLITTING) = a cluster of frame g
 * has more than four members -- utils.disjoint_big_clusters' (libs/utils.py:321-322).  A frame with no bit set already has its final
 * ID_pred under ROUNDING / PRUNING / SPLITTING = True: rounding returns [], the second pruning is idempotent, splitting returns at once.
 * `sizes_scratch` [N] int32 and `triggers_out` [max(n_frames, 1)] int32 are zeroed by the call (one memset with the counters when they
 * follow n_clusters_out in memory: flow_out | flow_in | n_clusters | sizes | triggers).  Both null: the call above. */
#define GNNCCA_POST_TRIGGER_ROUNDING 1
#define GNNCCA_POST_TRIGGER_SPLITTING 2
GNNCCA_API int gnncca_post_prune_cluster_frames_ex(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes,
                                                   int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev,
                                                   int32_t n_frames, void* workspace, size_t workspace_bytes,
                                                   int64_t* pruned_out, int32_t* flow_out, int32_t* flow_in,
                                                   int32_t* labels_out, int32_t* n_clusters_out, int32_t* sizes_scratch,
                                                   int32_t* triggers_out, gnncca_stream_t stream);

/* ---- Camera-exclusive identity clusters (csrc/exclusive.cuh): a partition that is legal by construction ------------------------------
 * A connected component of the pruned edges can hold two detections of one camera, which cannot be one person.  This entry computes,
 * on the device and without a host wait, a partition of every frame in which NO cluster holds two detections of one camera, for any
 * number of cameras with ids in [0, GNNCCA_EXCLUSIVE_MAX_CAMERAS).  No counterpart in the reference (its repair, the ROUNDING /
 * SPLITTING heuristics of gnncca_post_finalize_frame_host below, is tied to four cameras and runs on the host); nothing else changes.
 * Inputs: `scores` fp32 [E] per-edge probabilities, `threshold` in (0, 1), `cam` int32 [N] camera ids in DEVICE memory, the frame ranges
 * node_ptr_dev / edge_ptr_dev (int32 [n_frames + 1], DEVICE memory) as gnncca_post_prune_cluster_frames takes them, `max_frame_nodes`
 * the largest frame as the caller's host copy of node_ptr knows it (at most GNNCCA_EXCLUSIVE_MAX_FRAME_NODES).  The rule for frame g:
 *   active      edge k is active iff (double)scores[k] >= threshold: the comparison gnncca_eval_sweep makes, in fp64 against the widened
 *               fp32 score; a NaN score is never active.
 *   candidates  the unordered pair {i, j} is a candidate iff the edges (i, j) and (j, i) both exist in the frame and both are active:
 *               exactly the pruning rule.  On a directed capped list the candidates are the mutual pairs.
 *   weight      w = min(scores[i -> j], scores[j -> i]), an exact fp32.
 *   order       candidates by descending w; ties go to the smaller lo = min(i, j), then to the smaller hi.  A strict total order.
 *   clustering  every node starts as its own cluster with camera mask 1 << cam.  Walk the candidates in that order and merge the two
 *               clusters of a candidate iff they differ and their camera masks are disjoint; the merged mask is the OR.
 *   outputs     labels_out[v] (int32 [N]) = the smallest batch-global node id of v's cluster (gnncca_post_prune_cluster's convention);
 *               predictions_out[k] (int64 [E]) = 1 iff k belongs to a candidate pair and labels[src k] == labels[dst k];
 *               *n_clusters_out (int32) = the batch total; cut_out[g] (int32 [n_frames]) = the candidate pairs of frame g whose ends
 *               lie in different clusters; flags_out[g] (uint32 [n_frames]) = 0, or one of the two refusals below.
 * Where a frame's plain connected components already hold every camera at most once, labels and predictions are
 * gnncca_post_prune_cluster_frames' labels and pruned predictions for that frame exactly, and cut_out[g] = 0.  Same-camera edges are
 * never admissible; edge lists with duplicate ordered pairs are unspecified, as in the sweep.  The kernel runs mutual-best rounds (each
 * cluster takes its first admissible candidate, pairs that chose each other merge), which give the walk's partition; every comparison
 * is an integer maximum on 64-bit keys, there are no float atomics: two runs give the same bits, and a frame's result does not depend
 * on the rest of the batch.
 * flags_out[g] = GNNCCA_EXCLUSIVE_BAD_CAMERA: a camera id of the frame lies outside [0, 64); GNNCCA_EXCLUSIVE_BAD_RANGE: the frame's
 * ranges do not fit (gnncca_eval_sweep's test; a frame larger than max_frame_nodes rounded up to a power of two included).  Either way every node of the frame is its own
 * cluster, its predictions are 0 and cut_out[g] = 0 (as far as the ranges allow writing at all); other frames are unaffected.
 * Launches: the graph plan (plan + plan finish), the prepare kernel (reverse edges; it also zeroes *n_clusters_out), one workgroup per
 * frame (candidate keys, rounds, outputs); with n_edges == 0 only the last two.  Kernels only: no memset on the stream.  LDS: 20 bytes
 * per node of the largest frame, rounded up to a power of two (80 KiB at 4096).  Workspace: gnncca_post_exclusive_workspace_bytes,
 * O(E + N).  No host synchronisation, no allocation: capturable.  GNNCCA_ERR_INVALID_ARG: a threshold outside (0, 1), max_frame_nodes above 4096 or
 * above n_nodes, a null pointer where the count is positive. */
#define GNNCCA_EXCLUSIVE_MAX_FRAME_NODES 4096
#define GNNCCA_EXCLUSIVE_MAX_CAMERAS 64
#define GNNCCA_EXCLUSIVE_BAD_CAMERA 1u
#define GNNCCA_EXCLUSIVE_BAD_RANGE 2u
GNNCCA_API size_t gnncca_post_exclusive_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames);
GNNCCA_API int gnncca_post_exclusive_frames(const int64_t* edge_index, const float* scores, int64_t n_nodes, int64_t n_edges,
                                            const int32_t* cam, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                            int32_t max_frame_nodes, double threshold, int64_t* predictions_out, int32_t* labels_out,
                                            int32_t* n_clusters_out, int32_t* cut_out, uint32_t* flags_out, void* workspace,
                                            size_t workspace_bytes, gnncca_stream_t stream);

/* ---- Identity clusters WITHOUT pruning (csrc/strong.cuh): strongly connected components on the device ---------------------------------
 * With PRUNING = False (config_inference.yaml:7; inference.py:302-304, 733-738, 904-908) the reference's utils.compute_SCC_and_Clusters
 * (libs/utils.py:295-317) clusters the digraph of ALL active edges: a directed cycle without a single mutual pair is one identity.
 * gnncca_post_prune_cluster* computes components of the pruned, symmetric edge set; this entry computes the strongly connected
 * components of the unpruned one -- also the reference's own rule for a directed capped list (gnncca_build_edges_topk), with no closure
 * and no host wait.  Frame ranges node_ptr_dev / edge_ptr_dev (int32 [n_frames + 1], DEVICE memory) as gnncca_post_prune_cluster_frames
 * takes them; both NULL with n_frames == 0: the whole graph is one frame, as gnncca_post_prune_cluster has it.  `max_frame_nodes`: the
 * largest frame as the caller's host copy of node_ptr knows it (at most GNNCCA_STRONG_MAX_FRAME_NODES).  The rule for frame g:
 *   active       edge k is active iff predictions[k] == 1 and both of its ends lie in [node_ptr[g], node_ptr[g + 1]); everything else is
 *                ignored (gnncca_post_prune_cluster_frames' rule).  The edge list may be in any order; self loops and duplicates are harmless.
 *   reachability a bit matrix in LDS, n_pad rows of n_pad / 32 words (n_pad = the frame's node count rounded up to 32), diagonal set,
 *                active edges set; closed transitively by repeated squaring in place (the owner of a word ORs in that word of every row
 *                whose bit is set in its own row; every set bit is a true fact at all times, so a row read before or after its update
 *                of the same round is sound).
 *   rounds       a COUNTED loop of ceil(log2(n_pad)) + 1 rounds at most (11 at 1024 nodes): r rounds cover every path of 2^r edges, a
 *                simple path has fewer than n_pad, and the last round only detects that nothing changes.  A round that changes nothing
 *                ends the loop early; nothing else about the run time depends on the data.
 *   outputs      labels_out[v] (int32 [N]) = the smallest batch-global node id u with v -> u and u -> v reachable (gnncca_post_prune_cluster's
 *                convention); flow_out / flow_in (int32 [N]) = active, UNPRUNED edges leaving / entering each node; *n_clusters_out
 *                (int32) = the batch total; triggers_out[g] (int32 [max(n_frames, 1)]) bit 0 (GNNCCA_POST_TRIGGER_ROUNDING) = a node of
 *                the frame has flow_out or flow_in > 3, bit 1 (GNNCCA_POST_TRIGGER_SPLITTING) = a component has more than four members;
 *                flags_out[g] (uint32 [max(n_frames, 1)]) = 0, or the refusal below.
 * ORs, integer adds and a scan in id order only: two runs give the same bits, and a frame's result does not depend on the rest of the
 * batch.  On symmetric predictions labels, counts, flows and triggers are gnncca_post_prune_cluster_frames_ex's exactly.
 * flags_out[g] = GNNCCA_STRONG_BAD_RANGE: the frame's ranges do not fit (gnncca_post_exclusive_frames' test; a frame larger than
 * max_frame_nodes rounded up to 32 included).  Every node of such a frame is its own cluster, its flows and its trigger word are 0 (as far
 * as the ranges allow writing at all); other frames are unaffected.
 * Launches: one memset of the counters when they lie back to back (flow_out | flow_in | n_clusters, as gnn_cca_amd.postprocess lays them
 * out; three memsets otherwise) and one kernel, one workgroup per frame of 64, 256 or 1024 threads by max_frame_nodes.  Dynamic LDS:
 * P * P / 8 bytes for P = max_frame_nodes rounded up to 32 (128 B at 32, 2 KiB at 128, 128 KiB at 1024).  No workspace, no allocation, no
 * host synchronisation: capturable.  GNNCCA_ERR_INVALID_ARG before any launch: max_frame_nodes outside [0, GNNCCA_STRONG_MAX_FRAME_NODES]
 * or above n_nodes, a negative size, frame ranges given half or with n_frames == 0 (or n_frames > 0 without them), a null pointer where
 * the count is positive (n_clusters_out, triggers_out and flags_out always hold one word at least).  n_edges == 0 and n_nodes == 0 are legal. */
#define GNNCCA_STRONG_MAX_FRAME_NODES 1024
#define GNNCCA_STRONG_BAD_RANGE 2u
GNNCCA_API int gnncca_post_strong_frames(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes, int64_t n_edges,
                                         const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                         int32_t max_frame_nodes, int32_t* flow_out, int32_t* flow_in, int32_t* labels_out,
                                         int32_t* n_clusters_out, int32_t* triggers_out, uint32_t* flags_out, gnncca_stream_t stream);

/* Row N2, second half, for ONE frame on the HOST ("bridges-based heuristics stay on CPU"): the reference's call sequence
 * inference.py:306-345 after the threshold -- by the three switches of config_inference.yaml:6-8 (all True as shipped):
 * utils.remove_edges_single_direction (libs/utils.py:387-404) -> utils.compute_rounding (25-173) -> remove_edges_single_direction ->
 * utils.disjoint_big_clusters (319-386) -> utils.compute_SCC_and_Clusters (295-317).  Plain host arrays: `src` / `dst` [E] the frame's
 * edges in the reference's edge order with node ids in [node_base, node_base + n_nodes), `probs` [E] the sigmoid values, `predictions`
 * [E] in: the thresholded (or already pruned) 0 / 1 predictions, out: the final ones.  labels_out [n_nodes] (optional) = smallest
 * batch-global node id of the node's final cluster, *n_clusters_out (optional) = number of final clusters, id_pred_out [n_nodes]
 * (optional) = the reference's ID_pred, its label NUMBERING included (networkx's generation order: see csrc/post_host.cpp).
 * Frames are processed one at a time as the reference does (validation batch size 1, main.py:368).  Predictions other than 0 / 1 (inference.py:291
 * thresholds to exactly those) are GNNCCA_ERR_INVALID_ARG since round 6. */
#define GNNCCA_POST_ROUNDING 1
#define GNNCCA_POST_PRUNING 2
#define GNNCCA_POST_SPLITTING 4
GNNCCA_API int gnncca_post_finalize_frame_host(const int64_t* src, const int64_t* dst, int64_t node_base, int64_t n_nodes,
                                               int64_t n_edges, const float* probs, int64_t* predictions, int32_t switches,
                                               int32_t* labels_out, int32_t* n_clusters_out, int64_t* id_pred_out);

/* The same for a list of frames of one batch, dealt to host threads (frames are independent): batch-wide arrays in Batch.from_data_list
 * layout, node_ptr / edge_ptr [G + 1] on the HOST, frames[i] the i-th frame to finalize (the ones whose trigger word is set),
 * clusters_out[i] its final cluster count; n_threads 0 = one per hardware thread, at most 16. */
GNNCCA_API int gnncca_post_finalize_frames_host(const int64_t* src, const int64_t* dst, const int32_t* node_ptr, const int32_t* edge_ptr,
                                                const int32_t* frames, int32_t n_listed, const float* probs, int64_t* predictions,
                                                int32_t switches, int32_t* labels, int32_t* clusters_out, int32_t n_threads);

/* The ASYNCHRONOUS form (round 6): a persistent pool of host threads finalizes batches while the caller enqueues the next batch's GPU
 * chain -- the reference's loop pays its heuristics between two forwards (inference.py:294-345 runs on the host while the GPU waits); here
 * batch k's host pass overlaps batch k + 1's launches.  The caller copies the batch's results to HOST memory (pinned) on a side stream
 * behind an event and submits pointers into that copy: `triggers` [G] (gnncca_post_prune_cluster_frames_ex's words), src / dst [E],
 * probs [E], `predictions` [E] in: the pruned predictions, out: the final ones, `labels` [N] in / out (the device chain's convention: a
 * component's smallest batch-global node id), `n_clusters` [1] in: the device chain's count, out: the final count.  A pool thread waits for
 * `ready_event` (a hipEvent_t recorded behind the copy; null: the data is already there) on device `device`, lists the frames whose
 * trigger word meets the switches and the pool's threads finalize them (gnncca_post_finalize_frame_host per frame; no allocation per
 * frame).  gnncca_post_pool_submit returns a ticket >= 0 (or -status); gnncca_post_pool_wait blocks until that batch is final, writes
 * the finalized frame ids to frames_out [<= G] / their number to *n_frames_out (either may be null), releases the ticket and returns
 * the first non-zero status of any frame.  The buffers must stay valid until the wait returns; `n_clusters` needs `labels` (the correction counts the
 * flagged frames' components in them).  n_threads 0 = hardware threads - 2,
 * at most 16. */
typedef struct gnncca_post_pool gnncca_post_pool;
typedef struct gnncca_post_batch {
    const int64_t* src;
    const int64_t* dst;
    const int32_t* node_ptr;       /* [G + 1] host */
    const int32_t* edge_ptr;       /* [G + 1] host */
    int32_t n_frames;
    int32_t switches;              /* GNNCCA_POST_ROUNDING | GNNCCA_POST_PRUNING | GNNCCA_POST_SPLITTING */
    const int32_t* triggers;       /* [G] */
    const float* probs;
    int64_t* predictions;
    int32_t* labels;
    int32_t* n_clusters;
    void* ready_event;             /* hipEvent_t or null */
    int32_t device;
} gnncca_post_batch;
GNNCCA_API gnncca_post_pool* gnncca_post_pool_create(int32_t n_threads);
GNNCCA_API int32_t gnncca_post_pool_threads(const gnncca_post_pool* pool);
GNNCCA_API void gnncca_post_pool_destroy(gnncca_post_pool* pool);
GNNCCA_API int64_t gnncca_post_pool_submit(gnncca_post_pool* pool, const gnncca_post_batch* batch);
/* gnncca_post_pool_submit for results that still sit in DEVICE memory: enqueues the D2H copy of `nbytes` from device_src to host_dst
 * (pinned) on `stream` -- the stream the batch's chain was enqueued on -- records the event the job waits for behind it and submits
 * `batch`, whose pointers point into host_dst.  One call, no synchronisation. */
GNNCCA_API int64_t gnncca_post_pool_submit_copy(gnncca_post_pool* pool, const gnncca_post_batch* batch, const void* device_src,
                                                void* host_dst, size_t nbytes, int32_t device, gnncca_stream_t stream);
GNNCCA_API int gnncca_post_pool_wait(gnncca_post_pool* pool, int64_t ticket, int32_t* frames_out, int32_t* n_frames_out);
/* diagnostics: gnncca_post_pool_wait plus the job's life in microseconds -- times_us_out[0..3] = submit -> picked up by a pool thread,
 * -> its event had completed, -> its last frame was final, -> this call returned (negative: the caller arrived before the job was done). */
GNNCCA_API int gnncca_post_pool_wait_timed(gnncca_post_pool* pool, int64_t ticket, int32_t* frames_out, int32_t* n_frames_out,
                                           double* times_us_out);

/* ---- rows N1 + the path + N2 in ONE call: a batch of frames from the uploaded staging image to identity clusters -------------------
 * The per-batch body of inference.py:189-345 (normalise the embeddings, build the graph, MOTMPNet.forward, sigmoid / threshold,
 * prune, flow counts, clusters) as the same launches gnncca_normalize_columns2 / gnncca_build_edges / gnncca_mpn_forward_ex /
 * gnncca_post_threshold / gnncca_post_prune_cluster_frames make, issued from one native call: what a per-batch loop pays for at this
 * size is host time per launch, and the glue between five calls is a third of it.  Every pointer is device memory; outputs are
 * caller-allocated.  `staged_dev` is the image gnncca_plan_frames wrote, uploaded as is.  Batches of more than 4096 detections:
 * GNNCCA_ERR_UNSUPPORTED (use the separate entry points). */
typedef struct gnncca_frames_io {
    const void* staged_dev;        /* gnncca_plan_frames' staging image on the device                                  */
    int64_t n_nodes, n_frames, n_edges;
    const float* node_embeds;      /* [N][node_in]  (raw; normalised into node_norm when `normalize`)                  */
    const float* reid_embeds;      /* [N][reid_dim]                                                                    */
    int32_t reid_dim, mode, normalize;
    float* node_norm;              /* [N][node_in]  out (normalize != 0): the MPN's x                                  */
    float* reid_norm;              /* [N][reid_dim] out (normalize != 0)                                               */
    int64_t* edge_index;           /* [2][E] out                                                                       */
    float* edge_attr;              /* [E][4 or 2] out                                                                  */
    float* edge_labels;            /* [E] out                                                                          */
    float* logits;                 /* [n_out][E] out                                                                   */
    float* probs;                  /* [E] out: sigmoid of the last classified step                                     */
    int64_t* predictions;          /* [E] out                                                                          */
    int64_t* pruned;               /* [E] out                                                                          */
    int32_t* counters;             /* [3 N + 1 + G] out: flow_out | flow_in | n_clusters | cluster sizes (scratch) | triggers [G] */
    int32_t* labels;               /* [N] out                                                                          */
    int64_t counters_len;          /* int32 words the caller allocated behind `counters`: < 3 N + 1 + G -> GNNCCA_ERR_INVALID_ARG  */
} gnncca_frames_io;
GNNCCA_API int gnncca_frames_forward(const gnncca_mpn_dims* dims, const void* packed_dev, const gnncca_frames_io* io,
                                     void* mpn_workspace, size_t mpn_workspace_bytes, void* post_workspace,
                                     size_t post_workspace_bytes, uint32_t options, gnncca_stream_t stream);
/* gnncca_frames_forward on a capped graph (no counterpart in the reference): the same chain and the same gnncca_frames_io, with
 * `staged_dev` the uploaded image of gnncca_plan_frames_ex(top_k) -- capped edge_ptr / edge_ptr_g -- `n_edges` its return value, `max_deg`
 * its max_deg_out, and the build gnncca_build_edges_topk's kernel (which also zeroes the counters, as the dense build does for the dense
 * chain).  The capped list is directed, so the pruning keeps an active edge only where its reverse was kept and is active too: clusters
 * come from mutual-k pairs.  Refused before any launch: top_k < 1, an unknown rank_by, max_deg < 0 (GNNCCA_ERR_INVALID_ARG);
 * max_deg > GNNCCA_TOPK_MAX_DEG (GNNCCA_ERR_UNSUPPORTED); whatever gnncca_frames_forward refuses.  GNNCCA_RANK_BY_REID reads the reid table
 * in every mode, GNNCCA_EDGE_ATTR_ONLY_DIST included. */
GNNCCA_API int gnncca_frames_forward_topk(const gnncca_mpn_dims* dims, const void* packed_dev, const gnncca_frames_io* io,
                                          void* mpn_workspace, size_t mpn_workspace_bytes, void* post_workspace,
                                          size_t post_workspace_bytes, uint32_t options, int32_t top_k, int32_t rank_by, int32_t max_deg,
                                          gnncca_stream_t stream);
/* gnncca_frames_forward on a radius-gated graph (no counterpart in the reference): the same chain and the same gnncca_frames_io, with
 * `staged_dev` the uploaded image of gnncca_plan_frames_radius(radius, unit), `n_edges` its return value and the build
 * gnncca_build_edges_radius' kernel (which also zeroes the counters).  The gated list is closed under reversal, so the pruning sees every
 * kept edge's reverse.  Refused before any launch: a radius that is not a number >= 0 or inf, an unknown unit (GNNCCA_ERR_INVALID_ARG);
 * whatever gnncca_frames_forward refuses. */
GNNCCA_API int gnncca_frames_forward_radius(const gnncca_mpn_dims* dims, const void* packed_dev, const gnncca_frames_io* io,
                                            void* mpn_workspace, size_t mpn_workspace_bytes, void* post_workspace,
                                            size_t post_workspace_bytes, uint32_t options, double radius, int32_t unit,
                                            gnncca_stream_t stream);

/* ---- backward pass (training through the HIP kernels, train.py:454-494) -----------------
 * Supported (GNNCCA_OK from gnncca_backward_supported): the MFMA family (both reattach flags, all three
 * aggregators), two-layer node encoder, L >= 1, BatchNorm nowhere or only between the classifier's two layers -- i.e.
 * both shipped config shapes (config_training.yaml:94-181, config_inference.yaml:76-163).  `saved` holds the latents written by gnncca_mpn_forward's trace taps for the same
 * inputs and weights; `params_dev` / `grads_dev` are DEVICE pointers to the raw parameters / their gradients in the
 * canonical order of gnncca_param_count (row-major, un-split, exactly the nn.Parameter layouts).  grads are
 * overwritten.  grad_logits: [n_out][E]. */
GNNCCA_API int gnncca_backward_supported(const gnncca_mpn_dims* dims);
GNNCCA_API size_t gnncca_backward_workspace_bytes(const gnncca_mpn_dims* dims, int64_t n_nodes, int64_t n_edges);
GNNCCA_API int gnncca_mpn_backward(const gnncca_mpn_dims* dims, const float* const* params_dev, int n_params,
                                   const float* x, const int64_t* edge_index, const float* edge_attr, int64_t n_nodes,
                                   int64_t n_edges, const gnncca_trace* saved, const float* cls_bn_stat,
                                   const float* grad_logits, float* const* grads_dev, void* workspace,
                                   size_t workspace_bytes, gnncca_stream_t stream);
/* gnncca_mpn_backward with options.  GNNCCA_BWD_GRADS_ZEROED: the caller has already zero-filled every buffer of
 * `grads_dev` (e.g. they are views of one flat buffer cleared by a single fill), so the per-parameter clears are
 * skipped -- sixteen fewer enqueues per training step for the shipped configs. */
#define GNNCCA_BWD_GRADS_ZEROED 1u
GNNCCA_API int gnncca_mpn_backward_ex(const gnncca_mpn_dims* dims, const float* const* params_dev, int n_params,
                                      const float* x, const int64_t* edge_index, const float* edge_attr, int64_t n_nodes,
                                      int64_t n_edges, const gnncca_trace* saved, const float* cls_bn_stat,
                                      const float* grad_logits, float* const* grads_dev, void* workspace,
                                      size_t workspace_bytes, uint32_t options, gnncca_stream_t stream);
/* Train-mode classifier when a BatchNorm1d sits between its two layers (the shipped inference config): recomputes the
 * logits of every classified step from the saved edge latents with BATCH statistics over the E edges, updates
 * running_mean / running_var in place (momentum 0.1, unbiased variance, as torch.nn.BatchNorm1d), and returns per
 * step and hidden unit (mean, 1/sqrt(var + eps)) in bn_stat_out [n_out][C1][2] for gnncca_mpn_backward (cls_bn_stat).
 * scratch: 2 * C1 doubles. */
GNNCCA_API int gnncca_classifier_train(const gnncca_mpn_dims* dims, const float* const* params_dev, int n_params,
                                       const float* e_steps, int64_t n_edges, void* scratch, float* bn_stat_out,
                                       float* logits_out, gnncca_stream_t stream);

/* Train-mode variants with Dropout (train.py:454-494 with `dropout_p` > 0 somewhere in GRAPH_NET_PARAMS): the same three
 * calls with a gnncca_dropout; `trace` is required (the post-dropout latents it receives are what the backward reads, and
 * they carry the ReLU x Dropout masks of every saved activation: y_saved > 0 <=> kept and positive).  A null `dropout`
 * makes each of them its plain counterpart. */
GNNCCA_API int gnncca_mpn_forward_train(const gnncca_mpn_dims* dims, const void* packed_dev, const float* x,
                                        const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                                        void* workspace, size_t workspace_bytes, float* logits_out, const gnncca_trace* trace,
                                        const gnncca_dropout* dropout, gnncca_stream_t stream);
GNNCCA_API int gnncca_classifier_train_dropout(const gnncca_mpn_dims* dims, const float* const* params_dev, int n_params,
                                               const float* e_steps, int64_t n_edges, void* scratch, float* bn_stat_out,
                                               float* logits_out, const gnncca_dropout* dropout, gnncca_stream_t stream);
GNNCCA_API int gnncca_mpn_backward_train(const gnncca_mpn_dims* dims, const float* const* params_dev, int n_params,
                                         const float* x, const int64_t* edge_index, const float* edge_attr, int64_t n_nodes,
                                         int64_t n_edges, const gnncca_trace* saved, const float* cls_bn_stat,
                                         const float* grad_logits, float* const* grads_dev, void* workspace,
                                         size_t workspace_bytes, uint32_t options, const gnncca_dropout* dropout,
                                         gnncca_stream_t stream);

/* Gradients of the INPUTS of a train-mode forward (the reference's module backpropagates to data.x / data.edge_attr; a ReID head or a
 * learned edge feature in front of the MPN trains through this).  dx: [N][node_in], d_edge_attr: [E][edge_in], device pointers; either
 * may be null (nothing is launched for it), and what is given is OVERWRITTEN (zero-filled when the graph has no edge: no edge, no
 * path from an input to a logit).  Each is one product with the first encoder layer's weight -- no atomics, a deterministic function
 * of the gradient that reaches the encoder; dx runs on the fp32 matrix pipe (exact fp32).  A null `input_grads` makes either call
 * its plain counterpart; neither needs more workspace / tape than that counterpart. */
typedef struct { float* dx; float* d_edge_attr; } gnncca_input_grads;
GNNCCA_API int gnncca_mpn_backward_inputs(const gnncca_mpn_dims* dims, const float* const* params_dev, int n_params,
                                          const float* x, const int64_t* edge_index, const float* edge_attr, int64_t n_nodes,
                                          int64_t n_edges, const gnncca_trace* saved, const float* cls_bn_stat,
                                          const float* grad_logits, float* const* grads_dev, void* workspace,
                                          size_t workspace_bytes, uint32_t options, const gnncca_dropout* dropout,
                                          const gnncca_input_grads* input_grads, gnncca_stream_t stream);

/* Layer-by-layer training engine (SURVEY.md 8f row N3 remainder; train.py:454-494 through models/mpn.py:250-299 and
 * models/mlp.py:4-28 op for op): EVERY legal GRAPH_NET_PARAMS in train mode -- BatchNorm1d with batch statistics in any MLP
 * (running_mean / running_var updated in place with momentum 0.1, as torch.nn.BatchNorm1d; the caller bumps num_batches_tracked),
 * Dropout behind any ReLU (masks from `dropout`, as above), any widths / depths, sum | mean | max, both reattach flags.
 * `params_dev`: the gnncca_pack_weights order (per layer: weight, bias, [BatchNorm weight, bias, running_mean, running_var]).
 * `tape` (gnncca_train_tape_bytes) receives what autograd would keep and is read back by gnncca_train_backward, which ADDS
 * d loss / d parameter into `grads_dev` (same order; entries of buffers may be null; zero them first) given
 * `grad_logits` [n_out][E].  The shipped shapes have the fused pair gnncca_mpn_forward_train / gnncca_mpn_backward_train;
 * this engine is the one that covers everything else (one launch per op, correctness first). */
GNNCCA_API size_t gnncca_train_tape_bytes(const gnncca_mpn_dims* dims, int64_t n_nodes, int64_t n_edges);
/* Where the tape of gnncca_train_forward keeps the latents a forward hook on the reference's containers would see (models/mpn.py:270,
 * 288: the outputs of `encoder` and of every `MPNet` call, train-mode values: batch-statistics BatchNorm, Dropout applied): byte
 * offsets into the tape, offsets_out[0] = encoder node output [N][node_dim], [1] = encoder edge output [E][edge_dim], then per step s
 * (0-based) [2 + 2 s] = node latents after the step [N][node_dim], [3 + 2 s] = edge latents after the step [E][edge_dim]; -1 where
 * the MLP has no layer (its input passes through).  n_offsets must be 2 + 2 * num_enc_steps.  Pure function of (dims, N, E). */
GNNCCA_API int gnncca_train_tape_latents(const gnncca_mpn_dims* dims, int64_t n_nodes, int64_t n_edges, int64_t* offsets_out,
                                         int n_offsets);
GNNCCA_API int gnncca_train_forward(const gnncca_mpn_dims* dims, float* const* params_dev, int n_params, const float* x,
                                    const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                                    void* tape, size_t tape_bytes, float* logits_out, const gnncca_dropout* dropout,
                                    gnncca_stream_t stream);
GNNCCA_API int gnncca_train_backward(const gnncca_mpn_dims* dims, float* const* params_dev, int n_params, const float* x,
                                     const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                                     void* tape, size_t tape_bytes, const float* grad_logits, float* const* grads_dev,
                                     const gnncca_dropout* dropout, gnncca_stream_t stream);
/* gnncca_train_backward that also writes the input gradients asked for in `input_grads` (see gnncca_input_grads above): any depth,
 * BatchNorm or Dropout in the two encoders; a configuration without a node / edge encoder passes the latent gradient through. */
GNNCCA_API int gnncca_train_backward_inputs(const gnncca_mpn_dims* dims, float* const* params_dev, int n_params, const float* x,
                                            const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                                            void* tape, size_t tape_bytes, const float* grad_logits, float* const* grads_dev,
                                            const gnncca_dropout* dropout, const gnncca_input_grads* input_grads,
                                            gnncca_stream_t stream);

/* Stand-alone calls of the sub-modules, which the reference allows (models/mlp.py:26-28 MLP.forward; models/mpn.py:128-142
 * MLPGraphIndependent.forward, :59-69 EdgeModel.forward, :71-101 NodeModel.forward, :32-54 MetaLayer.forward): eval semantics
 * (BatchNorm from the running statistics, Dropout = identity), one launch per op.  MOTMPNet.forward does not use them.
 *   gnncca_mlp_eval     : out[rows][out_dim] = mlp(in[rows][in_dim]); params in the order weight, bias, [BN weight, bias, mean, var]
 *   gnncca_gather_cat   : out[r] = cat(a[ia[r]], b[ib[r]], c[ic[r]]) (null ids: row r itself; width 0: segment absent) -- the
 *                         x[row], x[col] gathers and the torch.cat of mpn.py:48,68,97 without a torch kernel
 *   gnncca_aggregate    : out[i] = sum | mean | max over {k : edge_index[0][k] == i} of messages[k], empty -> 0 (mpn.py:99,192-202) */
GNNCCA_API size_t gnncca_mlp_eval_workspace_bytes(const gnncca_mlp* mlp, int64_t rows);
GNNCCA_API int gnncca_mlp_eval(const gnncca_mlp* mlp, const float* const* params_dev, int n_params, const float* in, int64_t rows,
                               float* out, void* workspace, size_t workspace_bytes, gnncca_stream_t stream);
GNNCCA_API int gnncca_gather_cat(const float* a, const int64_t* ia, int wa, int64_t rows_a, const float* b, const int64_t* ib, int wb,
                                 int64_t rows_b, const float* c, const int64_t* ic, int wc, int64_t rows_c, int64_t rows, float* out,
                                 gnncca_stream_t stream);
GNNCCA_API size_t gnncca_aggregate_workspace_bytes(int64_t n_nodes, int64_t n_edges);
GNNCCA_API int gnncca_aggregate(const float* messages, const int64_t* edge_index, int64_t n_nodes, int64_t n_edges, int width, int agg,
                                float* out, void* workspace, size_t workspace_bytes, gnncca_stream_t stream);

/* One launch that copies a frame (x [N][node_in], edge_index [2][E] int64, edge_attr [E][edge_in]) into buffers of a canonical shape
 * (x_pad [n_real_max + n_dummy][node_in], edge_index_pad [2][e_pad], edge_attr_pad [e_pad][edge_in]) and writes the padding: zero rows,
 * and e_pad - E self loops with zero attributes on the n_dummy extra nodes behind the real ones (a disjoint dummy component: the logits of
 * the frame's own edges are those of the frame alone, models/mpn.py has no cross-component term; rows stay sorted).  What lets ONE captured
 * HIP graph serve every frame of the per-frame loop of inference.py:173-283 (gnn_cca_amd.inference.GraphedForward(pad_to=...)). */
GNNCCA_API int gnncca_pad_frame(const float* x, int64_t n_nodes, const int64_t* edge_index, const float* edge_attr, int64_t n_edges,
                                float* x_pad, int64_t n_real_max, int n_dummy, int64_t* edge_index_pad, float* edge_attr_pad,
                                int64_t e_pad, int node_in, int edge_in, gnncca_stream_t stream);

/* ---- Per-frame association metrics (inference.py:349-371, the scores main.py:335-348 aggregates) ---------------------------------
 * One launch scores every frame of a batch laid out as above (node_ptr_dev / edge_ptr_dev: int32 [n_frames + 1] in DEVICE memory; edges
 * of a frame contiguous, an edge that leaves its frame is ignored).  Inputs: edge_index int64 [2][E] (batch-global ids), edge_labels fp32
 * [E] (0/1 ground truth, as gnncca_build_edges writes it), predictions int64 [E] (0/1), labels int32 [N] (the predicted partition: a
 * node's label is the smallest batch-global node id of its cluster).  ID_GT is the partition into connected components of the edges
 * with label 1 (the reference's strongly connected components of a symmetric edge set).  Output: out fp64 [n_frames][16] in the order
 * GNNCCA_EVAL_COLUMNS lists (compute_P_R_F, inference.py:23-68, and scikit-learn's adjusted_rand_score, adjusted_mutual_info_score
 * (arithmetic), homogeneity / completeness / v_measure; n_clusters_pred counts the nodes with labels[v] == v); gt_labels_out (nullable)
 * int32 [N] = ID_GT in the smallest-id convention.  Frames of at most GNNCCA_EVAL_MAX_FRAME_NODES nodes: `max_frame_nodes` (the largest
 * frame, known to the caller from its host copy of node_ptr) above that is GNNCCA_ERR_INVALID_ARG before any launch; a frame the device
 * offsets make larger than max_frame_nodes gets a NaN row.  The workspace (gnncca_eval_workspace_bytes) holds per-frame lgamma tables;
 * no host synchronisation, no allocation: capturable.
 * gnncca_eval_frames_dense scores a CAPPED batch (gnncca_build_edges_topk, ..._topk_sym_*) as the dense graph would have been scored with
 * every dropped edge predicted 0: person_id / cam are the int32 [N] arrays of the batch's staging image (gnncca_frames); per frame the
 * ordered cross-camera pairs with the same / a different person id that are NOT in the edge list are added to FN / TN (precision1 /
 * precision0 divide by the dense class counts), and ID_GT is the dense graph's: all detections of an identity seen on at least two
 * cameras form one component, every other detection its own.  Everything else -- TP, FP, the formulas, the predicted partition -- as
 * above; on a dense batch the rows are gnncca_eval_frames' bit for bit.  No counterpart in the reference (it has no capped graph). */
#define GNNCCA_EVAL_MAX_FRAME_NODES 4096
#define GNNCCA_EVAL_COLUMNS "P R F TP FP FN TN rand_index mutual_index homogeneity completeness v_measure precision0 precision1 " \
                            "n_clusters_gt n_clusters_pred"
GNNCCA_API size_t gnncca_eval_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames);
GNNCCA_API int gnncca_eval_frames(const int64_t* edge_index, const float* edge_labels, const int64_t* predictions, const int32_t* labels,
                                  int64_t n_nodes, int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev,
                                  int32_t n_frames, int32_t max_frame_nodes, int32_t* gt_labels_out, double* out, void* workspace,
                                  size_t workspace_bytes, gnncca_stream_t stream);
GNNCCA_API int gnncca_eval_frames_dense(const int64_t* edge_index, const float* edge_labels, const int64_t* predictions,
                                        const int32_t* labels, const int32_t* person_id, const int32_t* cam, int64_t n_nodes,
                                        int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                        int32_t max_frame_nodes, int32_t* gt_labels_out, double* out, void* workspace,
                                        size_t workspace_bytes, gnncca_stream_t stream);

/* ---- Threshold sweep: every operating point of a batch in one pass (csrc/eval_sweep.cuh) -------------------------------------------
 * What the reference's calibration does one threshold at a time on the host (main.py:124-319, MODE REID: 100 thresholds over a per-edge
 * score, compute_P_R_F at each, the threshold of maximal F; the OPT_TH / GEOM_TH tables of config_inference.yaml are such results).
 * `scores` fp32 [E] is ANY per-edge score (a probability, a distance: normalising it is the caller's business -- main.py:141 divides by
 * the dataset's maximum); thresholds_dev fp64 [n_thresholds] in DEVICE memory, any order, duplicates allowed.  The rule for threshold t
 * and frame g, which is exactly what gnncca_post_threshold_at -> gnncca_post_prune_cluster_frames -> gnncca_eval_frames compute one
 * threshold at a time:
 *   activity   edge k is active iff (double)scores[k] >= thresholds[t] (keep_le != 0: <=).  The comparison is made in fp64 against the
 *              widened fp32 score; a NaN score is never active.
 *   pruning    edge k is kept iff it is active and an edge (dst k, src k) of the same frame exists and is active.
 *   partition  labels_out[t] (int32 [n_thresholds][N], nullable) = the connected components of the kept edges inside the frame; a
 *              node's label is the smallest batch-global id of its component.
 *   scores     rows_out[t][g] (fp64 [n_thresholds][n_frames][16]) = the 16 columns of gnncca_eval_frames (GNNCCA_EVAL_COLUMNS) for
 *              those kept predictions and that partition, bit for bit: the scoring arithmetic is the same code.
 * Edge lists with duplicate ordered pairs are unspecified (gnncca_build_edges and its capped forms make none).  A capped batch is swept
 * against its kept edges only (no counterpart of gnncca_eval_frames_dense).  A frame whose ranges do not fit gets a NaN row, as above.
 * Four launches whatever n_thresholds is (graph plan, plan finish, reverse edges + lgamma tables, one launch of n_frames x n_thresholds
 * workgroups); no prediction vector is materialised; the workspace (gnncca_eval_sweep_workspace_bytes) is O(E + N); no host
 * synchronisation, no allocation: capturable.  GNNCCA_ERR_INVALID_ARG: n_thresholds < 1 or > GNNCCA_EVAL_SWEEP_MAX_THRESHOLDS, a null
 * pointer where the count is positive, max_frame_nodes above GNNCCA_EVAL_MAX_FRAME_NODES. */
#define GNNCCA_EVAL_SWEEP_MAX_THRESHOLDS 1024
GNNCCA_API size_t gnncca_eval_sweep_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames, int64_t n_thresholds);
GNNCCA_API int gnncca_eval_sweep(const int64_t* edge_index, const float* edge_labels, const float* scores, int64_t n_nodes,
                                 int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                 int32_t max_frame_nodes, const double* thresholds_dev, int32_t n_thresholds, int32_t keep_le,
                                 double* rows_out, int32_t* labels_out, void* workspace, size_t workspace_bytes, gnncca_stream_t stream);

/* ---- Threshold sweep over the CAMERA-EXCLUSIVE partition (csrc/eval_sweep_exclusive.cuh) --------------------------------------------
 * gnncca_eval_sweep scores the connected components of the pruned edges.  Whoever ships gnncca_post_exclusive_frames' clusters needs the
 * sweep of THAT partition: the two differ wherever a component holds a camera twice, and a threshold chosen on one says nothing about
 * the other.  Arguments: gnncca_eval_sweep's, plus `cam` int32 [N] camera ids in DEVICE memory, without keep_le (the rule needs
 * positive weights: probabilities, not distances).  The rule for threshold t (thresholds_dev[t] strictly inside (0, 1)) and frame g
 * defines nothing new:
 *   rows        rows_out[t][g] (fp64 [n_thresholds][n_frames][16]) = the 16 columns of gnncca_eval_frames for the predictions_out and
 *               labels_out of gnncca_post_exclusive_frames(..., threshold = thresholds_dev[t]), bit for bit.
 *   labels      labels_out[t] (int32 [n_thresholds][N], nullable) = that call's labels_out, exactly.
 * Activity ((double)scores[k] >= threshold, a NaN score is never active), candidates (both edges of a pair exist in the frame and are
 * active), weight (the smaller of the two scores, an exact fp32), order (descending weight, ties to the smaller lo, then the smaller hi),
 * clustering (merge iff the clusters differ and their camera masks are disjoint), labels (the smallest batch-global node id of the
 * cluster) and predictions (1 iff the edge belongs to a candidate pair inside one cluster) are the exclusive entry's, stated there in
 * full; the scoring is gnncca_eval_frames' code.
 * How one pass does it: a pair's 64-bit key -- (fp32 bits of the weight) << 24 | (4095 - lo) << 12 | (4095 - hi) -- does not depend on
 * the threshold, and the candidates at a threshold are exactly the pairs whose weight is >= it (the weight IS one of the two scores).
 * One read-only key array per batch (slot k for the edge k of a pair with src < dst, 0 elsewhere) serves all thresholds; workgroup
 * (g, t) runs the exclusive entry's mutual-best rounds over frame g's slots with the weight test in front.  Integer maxima and ORs in
 * LDS only, no float atomics: two runs give the same bits, and a frame's rows do not depend on the rest of the batch.  The partitions
 * nest: a lower threshold continues the walk of a higher one, so its clusters are unions of the higher one's.
 * Refusals as in the two parents: a frame whose ranges do not fit (gnncca_eval_sweep's test) gets a NaN row; a frame with a camera id
 * outside [0, 64) gets the row of "every node its own cluster, predictions 0"; other frames are unaffected; edge lists with duplicate
 * ordered pairs are unspecified.  Thresholds outside (0, 1) are the caller's to refuse: on the device a threshold <= 0 behaves as the
 * comparisons say -- every edge with a score >= it counts as active for the predictions, while only pairs of positive weight carry a
 * key and can merge.
 * Four launches whatever n_thresholds is (graph plan, plan finish, one prepare kernel: reverse edges + pair keys + lgamma tables, one
 * launch of n_frames x n_thresholds workgroups), kernels only (no memset on the stream); LDS 20 bytes per node of the largest frame
 * rounded up to a power of two (80 KiB at 4096); the workspace (gnncca_eval_sweep_exclusive_workspace_bytes: plan, rev int32 [E], keys
 * u64 [E], lgamma tables) is O(E + N) and does not depend on n_thresholds; no host synchronisation, no allocation: capturable.
 * GNNCCA_ERR_INVALID_ARG before any launch: n_thresholds < 1 or > GNNCCA_EVAL_SWEEP_MAX_THRESHOLDS, max_frame_nodes outside
 * [0, GNNCCA_EXCLUSIVE_MAX_FRAME_NODES] or above n_nodes, a negative size, a null thresholds_dev, a null pointer where the count is
 * positive; GNNCCA_ERR_WORKSPACE: a short workspace.  n_frames == 0 returns GNNCCA_OK and launches nothing. */
GNNCCA_API size_t gnncca_eval_sweep_exclusive_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames, int64_t n_thresholds);
GNNCCA_API int gnncca_eval_sweep_exclusive(const int64_t* edge_index, const float* edge_labels, const float* scores, const int32_t* cam,
                                           int64_t n_nodes, int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev,
                                           int32_t n_frames, int32_t max_frame_nodes, const double* thresholds_dev, int32_t n_thresholds,
                                           double* rows_out, int32_t* labels_out, void* workspace, size_t workspace_bytes,
                                           gnncca_stream_t stream);

/* ---- Joint sweep: every operating point of a CONJUNCTION of conditions in one pass (csrc/eval_sweep_joint.cuh) -----------------------
 * The reference's position baselines keep an edge iff several scores pass at once: geometrical_association iff the ground distance
 * < GEOM_TH / max_dist (inference.py:722-724), geometrical_appearance_association iff that holds AND the ReID distance < th
 * (inference.py:896); the GEOM_TH / OPT_TH tables of config_inference.yaml were swept by hand, one axis at a time.  Arguments beyond
 * gnncca_eval_sweep's: `scores` a HOST array of n_scores DEVICE pointers to fp32 scores, `score_strides` a host array of their element
 * strides (element e of score k is scores[k][e * score_strides[k]]: the columns of an edge_attr [E][4] are swept in place with stride
 * 4), `comparators` a host array of GNNCCA_CMP_* codes, one per condition (1 <= n_scores <= GNNCCA_EVAL_JOINT_MAX_SCORES);
 * points_dev fp64 [n_points][n_scores] in DEVICE memory (1 <= n_points <= GNNCCA_EVAL_JOINT_MAX_POINTS; any order, duplicates allowed);
 * frame_div_dev fp64 [n_scores][n_frames] in DEVICE memory, nullable.  The rule for point t and frame g:
 *   threshold  th[k] = points_dev[t][k] / frame_div_dev[k][g], one IEEE fp64 division; points_dev[t][k] itself when frame_div_dev is
 *              null (GEOM_TH / max_dist[g]: the table value is in metres, the attribute was divided by the frame's max_dist).
 *   activity   edge e is active iff for EVERY k: (double)scores[k][e] cmp_k th[k].  The comparison is made in fp64 against the widened
 *              fp32 score; a NaN score is never active under any comparator.
 *   pruning, partition, scores   exactly gnncca_eval_sweep's: an edge is kept iff its reverse edge of the same frame is active too;
 *              labels_out[t] (int32 [n_points][N], nullable) = the connected components of the kept edges, a node's label the smallest
 *              batch-global id of its component; rows_out[t][g] (fp64 [n_points][n_frames][16]) = the 16 columns of
 *              gnncca_eval_frames.  The workgroup body is gnncca_eval_sweep's own code with another predicate: with one score, no
 *              divisor and GNNCCA_CMP_GE / GNNCCA_CMP_LE the rows and labels are that entry's bit for bit.
 * NOT reproduced BY THIS SWEEP: the reference clusters with the strongly connected components of the digraph of active edges and does not
 * prune; with a score that is not symmetric (F.pairwise_distance adds eps to a - b) a directed cycle without a mutual pair joins nodes
 * there, here only mutual pairs join.  The reference's own rule is gnncca_eval_sweep_strong's (below), with this entry's arguments.
 * inference.py:892,896 use the last graph's labels and max_dist[0] for a whole batch; here every frame has its
 * own.  A frame whose ranges do not fit gets a NaN row; edge lists with duplicate ordered pairs are unspecified (as above).
 * Four launches whatever n_points and n_scores are (graph plan, plan finish, gnncca_eval_sweep's prepare kernel unchanged, one launch of
 * n_frames x n_points workgroups); the workspace (gnncca_eval_sweep_joint_workspace_bytes) is gnncca_eval_sweep's, O(E + N); no host
 * synchronisation, no allocation: capturable.  GNNCCA_ERR_INVALID_ARG before any launch: n_scores or n_points out of range, an unknown
 * comparator code, a stride < 1, a negative size, max_frame_nodes above GNNCCA_EVAL_MAX_FRAME_NODES or n_nodes, a null array, a null
 * pointer where its count is positive; GNNCCA_ERR_WORKSPACE: a short workspace.  n_frames == 0 returns GNNCCA_OK and launches nothing.
 *
 * gnncca_eval_rows_accumulate folds the rows fp64 [n_points][n_frames][16] of one batch into running sums fp64 [n_points][16] and a
 * frame count (int64 [1], nullable; both in DEVICE memory, zeroed by the caller before the first batch) in ONE launch:
 * sums[t][c] = ((sums[t][c] + rows[t][0][c]) + rows[t][1][c]) + ... -- the frames in ascending g, plain fp64 adds, an order that is part
 * of the contract; no atomics, no reduction tree: two runs give the same bits.  A NaN row makes its sums NaN.  *frames += n_frames. */
#define GNNCCA_EVAL_JOINT_MAX_SCORES 4
#define GNNCCA_EVAL_JOINT_MAX_POINTS 16384
#define GNNCCA_CMP_GE 0
#define GNNCCA_CMP_GT 1
#define GNNCCA_CMP_LE 2
#define GNNCCA_CMP_LT 3
GNNCCA_API size_t gnncca_eval_sweep_joint_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames);
GNNCCA_API int gnncca_eval_sweep_joint(const int64_t* edge_index, const float* edge_labels, const float* const* scores,
                                       const int64_t* score_strides, const int32_t* comparators, int32_t n_scores, int64_t n_nodes,
                                       int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                       int32_t max_frame_nodes, const double* points_dev, int32_t n_points, const double* frame_div_dev,
                                       double* rows_out, int32_t* labels_out, void* workspace, size_t workspace_bytes,
                                       gnncca_stream_t stream);
GNNCCA_API int gnncca_eval_rows_accumulate(const double* rows, int32_t n_points, int32_t n_frames, double* sums, int64_t* frames,
                                           gnncca_stream_t stream);

/* ---- Sweep over the STRONGLY CONNECTED clusters: every operating point without pruning (csrc/eval_sweep_strong.cuh) --------------------
 * With PRUNING = False, and always in geometrical_association / geometrical_appearance_association (inference.py:733-738, 904-908), the
 * reference prunes nothing and clusters a frame by the strongly connected components of the digraph of its active edges
 * (gnncca_post_strong_frames for ONE prediction vector).  This entry scores every operating point of that rule in one pass: what
 * threshold -> gnncca_post_strong_frames -> gnncca_eval_frames compute one point at a time.  The arguments are gnncca_eval_sweep_joint's
 * (K = n_scores conditions; the sweep of a single score is K = 1 with GNNCCA_CMP_GE or GNNCCA_CMP_LE).  The rule for frame g at point t:
 *   threshold    th[q] = points_dev[t][q] for condition q; with frame_div_dev, th[q] = points_dev[t][q] / frame_div_dev[q][g], one IEEE
 *                fp64 division.
 *   active edges edge k of the frame is active iff EVERY one of the K conditions holds; condition q is
 *                (double)scores[q][k * score_strides[q]] cmp_q th[q]: the fp32 score is widened and the comparison is made in fp64.  A NaN
 *                score is never active.  No reverse edge is consulted.
 *   predictions  predictions_t[k] = active ? 1 : 0 -- the UNPRUNED predictions.
 *   labels       labels_out[t][v] (int32 [n_points][N], nullable) = the smallest batch-global id u of the frame with v -> u and u -> v
 *                reachable over active edges whose two ends both lie in the frame: gnncca_post_strong_frames' rule and label
 *                convention.  An active edge that leaves its frame sets no bit; self loops and duplicates are harmless; the edge list
 *                may be in any order.
 *   row          rows_out[t][g] (fp64 [n_points][n_frames][16]) = the 16 columns of gnncca_eval_frames for predictions_t and labels_t.
 * Contract, bit for bit: with pred_t the int64 vector of `predictions` computed on the host in float64, rows_out[t] is
 * gnncca_eval_frames(pred_t, labels) and labels_out[t] is labels, for labels = gnncca_post_strong_frames(pred_t)'s.  On scores whose
 * activity is symmetric the rows and labels are gnncca_eval_sweep_joint's.
 * The closure is gnncca_post_strong_frames' own code (csrc/strong_closure.cuh): a counted loop of ceil(log2(n_pad)) + 1 rounds at most,
 * early exit after a round that changes nothing.  One workgroup per (frame, point) of 64 threads (largest frame <= 64) or 256; dynamic
 * LDS max(12 P, max(P, 32)^2 / 8) + 2 P bytes for P = the power of two >= max_frame_nodes (130 KiB at 1024 detections).
 * TWO launches whatever n_points and n_scores are: gnncca_eval_sweep's prepare kernel with no edge blocks (the lgamma tables) and the
 * sweep.  No graph plan, no CSR, no reverse-edge table, no memset, no host synchronisation, no allocation: capturable.  The workspace
 * (gnncca_eval_sweep_strong_workspace_bytes) holds the lgamma tables only, (n_nodes + n_frames) doubles.
 * A frame whose ranges do not fit (more nodes than P included) gets a NaN row and identity labels; other frames are unaffected.
 * GNNCCA_ERR_INVALID_ARG before any launch: a negative size, n_scores outside [1, GNNCCA_EVAL_JOINT_MAX_SCORES], n_points above
 * GNNCCA_EVAL_JOINT_MAX_POINTS, an unknown comparator code, a stride < 1, max_frame_nodes outside [0, GNNCCA_STRONG_MAX_FRAME_NODES] or
 * above n_nodes, a null array, a null pointer where its count is positive; GNNCCA_ERR_WORKSPACE: a short workspace (as the joint entry
 * answers it).  n_frames == 0 or n_points == 0 returns GNNCCA_OK and launches nothing. */
GNNCCA_API size_t gnncca_eval_sweep_strong_workspace_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_frames);
GNNCCA_API int gnncca_eval_sweep_strong(const int64_t* edge_index, const float* edge_labels, const float* const* scores,
                                        const int64_t* score_strides, const int32_t* comparators, int32_t n_scores, int64_t n_nodes,
                                        int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                        int32_t max_frame_nodes, const double* points_dev, int32_t n_points, const double* frame_div_dev,
                                        double* rows_out, int32_t* labels_out, void* workspace, size_t workspace_bytes,
                                        gnncca_stream_t stream);

/* ---- Ranking scores without a threshold: AUROC, average precision, best F per frame; the pooled curve (csrc/rank_metrics.cuh) --------
 * Every entry above judges a score AT a threshold.  gnncca_rank_metrics says how well a score ORDERS a frame's edges: one launch of
 * n_frames x n_scores workgroups, no workspace (a frame is sorted in LDS), no host synchronisation, no allocation: capturable.
 * `scores`, `score_strides`: as gnncca_eval_sweep_joint takes them (host arrays of n_scores device pointers and element strides,
 * 1 <= n_scores <= GNNCCA_RANK_MAX_SCORES); `positive_low`: a host array, 0 = a HIGH score speaks for label 1 (probabilities), 1 = a LOW
 * one does (distances); max_frame_edges: the batch's largest frame as the caller's host copy of edge_ptr knows it.  rows_out fp64
 * [n_scores][n_frames][8], columns GNNCCA_RANK_COLUMNS.  The rule for frame g and score k:
 *   samples    the frame's directed edges e in [edge_ptr[g], edge_ptr[g + 1]) whose label is exactly 1.0f (positive) or 0.0f (negative),
 *              the two values gnncca_eval_frames counts; an edge with any other label is no sample.  n_pos, n_neg count them (a NaN score
 *              included).  A capped batch is ranked on its kept edges.
 *   key        s = the fp32 score, exactly negated when positive_low; -0 is taken as +0; the 32 bits u of s become
 *              key = u | 0x80000000 for s >= 0 and ~u for s < 0: a larger s has a larger key, +-inf are ordinary values.  A NaN score
 *              is counted in n_nan, takes no part in the ranking, and makes the frame's four real-valued columns NaN.
 *   groups     samples with equal keys are ONE tie group; n_distinct is the number of groups.  The groups are visited from the largest
 *              key (the most positive) to the smallest with running TP, FP = the positives, negatives of the groups visited so far, the
 *              current one included; p, n = the current group's positives and negatives.
 *   AUROC      (sum over groups of p (2 neg_ranked_below + n)) / (2 n_pos n_neg), neg_ranked_below = n_neg - FP: the numerator and the
 *              denominator exact integers, converted to fp64, ONE division.  NaN if n_pos == 0 or n_neg == 0.
 *   AP         sum over groups with p > 0 of ((double)p / (double)n_pos) * ((double)TP / (double)(TP + FP)): two divisions and one
 *              multiplication per term, never fused with the additions.  Order of the additions: sort the samples by key descending; a
 *              group's term stands at the position (from 0) of the group's LAST sample, every other position holds +0; lane q of 256
 *              adds the positions q, q + 256, q + 512, ... ascending onto +0; within each block of 64 lanes six butterfly steps
 *              v[q] = v[q] + v[q ^ o], o = 32, 16, 8, 4, 2, 1 (all lanes at once); AP = ((v[0] + v[64]) + v[128]) + v[192].  Nothing in
 *              it depends on the batch, the block size or the LDS capacity.  NaN if n_pos == 0.
 *   best_F     the maximum over the n_distinct cuts (a cut predicts 1 for every group visited so far) of compute_P_R_F's F
 *              (inference.py:53-66): P = TP / (TP + FP), R = TP / (TP + FN) with FN = n_pos - TP, F = 2 * (P * R) / (P + R), 0 when
 *              P + R == 0 -- `score >= cut` (positive_low: `score <= cut`).  NaN if n_pos == 0.
 *   best_cut   the score of the FIRST cut in visiting order that reaches best_F: the key mapped back to fp32, negated back when
 *              positive_low, widened to fp64; a zero is +0.  NaN if n_pos == 0.
 *   empty      a frame without samples: the four counts 0, the four real-valued columns NaN.
 * A frame whose edge range lies outside [0, n_edges] or holds more than max_frame_edges rounded up to a power of two gets eight NaNs.
 * LDS: gnncca_rank_metrics_lds_bytes(max_frame_edges) = 8 bytes per edge of the largest frame rounded up to a power of two (at least
 * 64): 8 KiB for a Terrace frame of 768 edges, 128 KiB at GNNCCA_RANK_MAX_FRAME_EDGES; 0 for a size out of range.
 * GNNCCA_ERR_INVALID_ARG before any launch: n_scores out of range, a stride < 1, a positive_low other than 0 / 1, max_frame_edges outside
 * [0, GNNCCA_RANK_MAX_FRAME_EDGES] or above n_edges, a negative size, a null array, a null pointer where its count is positive.
 * n_frames == 0 returns GNNCCA_OK and launches nothing.
 *
 * gnncca_rank_rows_accumulate folds rows fp64 [n_scores][n_frames][8] into sums fp64 [n_scores][8] and counts int64 [n_scores][8] (DEVICE
 * memory, zeroed by the caller before the first batch) in one launch: per score and column the frames in ascending g; a NaN is skipped,
 * every other value is added onto the running sum (a plain fp64 add) and counted.  No atomics, no tree: the order is the contract.
 *
 * gnncca_rank_pool_add is the reference's own sweep (main.py:124-319, MODE REID): every raw edge distance of the data set pooled,
 * `preds = dist <= t` at each threshold, compute_P_R_F on the pooled vector -- no pruning, no clustering -- kept as two histograms, so
 * that nothing of a batch has to stay.  thresholds_dev: fp64 [n_thresholds] in DEVICE memory, strictly increasing (the caller's to
 * ensure), 1 <= n_thresholds <= GNNCCA_RANK_POOL_MAX_THRESHOLDS.  hist: int64 [2][n_thresholds + 1], row 0 the negatives (label 0.0f),
 * row 1 the positives (label 1.0f); nan_count: int64 [2] likewise; both in DEVICE memory, zeroed by the caller before the first call.
 * Sample e (scores[e * score_stride], labels[e]; any other label is no sample) adds 1 to bucket b(e) of its label's row:
 *   keep_le = 1   b = the number of thresholds <  (double)score: `score <= thresholds[t]` holds exactly for t >= b;
 *   keep_le = 0   b = the number of thresholds <= (double)score: `score >= thresholds[t]` holds exactly for t <  b;
 * compared in fp64 against the widened fp32 score, as everywhere above; +-inf are ordinary values; a NaN score adds 1 to nan_count
 * instead.  TP[t] is then the sum of row 1 over the buckets <= t (keep_le = 0: > t), FP[t] the same of row 0.  Integer atomics only: any
 * split of a data set into calls leaves the same state.  One launch, no frame size limit, no host synchronisation: capturable. */
#define GNNCCA_RANK_MAX_SCORES 4
#define GNNCCA_RANK_MAX_FRAME_EDGES 16384
#define GNNCCA_RANK_POOL_MAX_THRESHOLDS 65536
#define GNNCCA_RANK_COLUMNS "n_pos,n_neg,n_distinct,n_nan,AUROC,AP,best_F,best_cut"
GNNCCA_API size_t gnncca_rank_metrics_lds_bytes(int32_t max_frame_edges);
GNNCCA_API int gnncca_rank_metrics(const float* edge_labels, const float* const* scores, const int64_t* score_strides,
                                   const int32_t* positive_low, int32_t n_scores, int64_t n_edges, const int32_t* edge_ptr_dev,
                                   int32_t n_frames, int32_t max_frame_edges, double* rows_out, gnncca_stream_t stream);
GNNCCA_API int gnncca_rank_rows_accumulate(const double* rows, int32_t n_scores, int32_t n_frames, double* sums, int64_t* counts,
                                           gnncca_stream_t stream);
GNNCCA_API int gnncca_rank_pool_add(const float* scores, int64_t score_stride, const float* labels, int64_t n_samples,
                                    const double* thresholds_dev, int32_t n_thresholds, int32_t keep_le, int64_t* hist,
                                    int64_t* nan_count, gnncca_stream_t stream);

/* ---- Rank-R ReID baseline with k-reciprocal re-ranking (csrc/rerank.cuh) -----------------------------------------------------------
 * The reference's MODE eval_RANK (inference.py:388-511) with RERANK (libs/utils.py:578-644, Zhong et al.): the baseline the GNN has to
 * beat.  A batch's per-frame matrices lie back to back, frame g's n_g x n_g row-major fp32 matrix at element sum_{q<g} n_q^2; `total` is
 * the number of elements the caller allocated (sum_g n_g^2 by its host copy of node_ptr).  The kernels derive every offset from
 * node_ptr_dev (int32 [n_frames + 1] in DEVICE memory) and skip a frame whose matrix would not fit into `total`.  `max_frame_nodes` is
 * the largest frame as the caller's host copy of node_ptr knows it.  One launch per entry, on the caller's stream; no host
 * synchronisation, no allocation: capturable.  Deterministic: every floating-point sum has a fixed order, no float atomics.
 *
 * gnncca_frame_distances: out[g][i][j] = sqrt(sum_k (x_i[k] - x_j[k])^2) over the rows embeds fp32 [N][dim] of frame g, the sum of
 *   squared DIFFERENCES in fp32 over k ascending (torch.cdist(p=2) of inference.py:416 without the |a|^2 + |b|^2 - 2ab form).  The
 *   diagonal is exactly 0, the matrix exactly symmetric, the relative error at most (dim + 2) 2^-24.  Any dim >= 1, any frame size.
 * gnncca_rerank_frames: out = re_ranking(D, D, D, k1, k2, lam) per frame, the whole n x n matrix (the reference returns the block
 *   [:nq, nq:] of a query / gallery split, which does not depend on where the split is).  In fp32 like the reference, per frame with
 *   D = dist's matrix:
 *     1. O[i][j] = fl(D[j][i]^2) / max_k fl(D[k][i]^2), division correctly rounded; a zero maximum gives O[i][:] = 0 (the reference: NaN).
 *     2. rank[i] = the columns of O[i] ascending, ties to the smaller index (the reference's argsort is unstable).
 *     3. F_m(i) = the first min(m, n) entries of rank[i]; R_m(i) = {j in F_m(i) : i in F_m(j)}; K = k1 + 1; h = round-half-even(k1 / 2) + 1.
 *     4. X(i) = R_K(i) | OR { R_h(c) : c in R_K(i), 3 |R_h(c) & R_K(i)| > 2 |R_h(c)| }.
 *     5. V[i][j] = exp(-O[i][j]) / sum_{m in X(i)} exp(-O[i][m]) for j in X(i) (summed over m ascending), 0 elsewhere.
 *     6. k2 != 1: V'[i] = (sum of V[m] over the first min(k2, n) entries m of rank[i], in rank order) / their number; else V' = V.
 *     7. S(i, j) = sum_c min(V'[i][c], V'[j][c]) over c ascending; J = 1 - S / (2 - S).
 *     8. out[i][j] = J (1 - lam) + O[i][j] lam, with (float)(1 - lam) and (float)lam.
 *   eval_RANK passes one matrix three times, so that every distance has an exact twin and its result depends on the unstable sort's tie
 *   order: that is NOT reproduced.  One workgroup per frame, V and V' in LDS (sized by max_frame_nodes: gnncca_rerank_lds_bytes).
 *   GNNCCA_ERR_UNSUPPORTED: max_frame_nodes above GNNCCA_RERANK_MAX_FRAME_NODES.  GNNCCA_ERR_INVALID_ARG: k1 outside
 *   [1, GNNCCA_RERANK_MAX_K1], k2 outside [1, k1], lam outside [0, 1].  Debug outputs (nullable): rank_out int32 [N][rank_cols], row v =
 *   the first min(rank_cols, max(k1 + 1, k2), n) entries of v's ranking as frame-local ids, -1 after; mask_out uint64 [N][4], row v =
 *   X(v) (two words, bit j = frame-local id j) and the columns where V'[v] is not zero (two words).
 * gnncca_rank_predictions: predictions int64 [E] on the batch's edge list (edge_index int64 [2][E], edge_ptr_dev int32 [n_frames + 1]):
 *   edge (i, j) is 1 iff j is among the min(rank, deg_i) detections of i's frame on another camera (cam int32 [N]) with the smallest
 *   dist[i][.], ties to the smaller id, or i is among j's (inference.py:454-481).  Where the reference goes on to same-camera detections
 *   once rank exceeds deg_i, this stops.  An edge missing from a capped list is simply not predicted; an edge that leaves its frame is 0.
 *   Frames of at most GNNCCA_RERANK_MAX_FRAME_NODES (GNNCCA_ERR_UNSUPPORTED); rank < 1 is GNNCCA_ERR_INVALID_ARG. */
#define GNNCCA_RERANK_MAX_FRAME_NODES 128
#define GNNCCA_RERANK_MAX_K1 64
GNNCCA_API int gnncca_frame_distances(const float* embeds, int32_t dim, int64_t n_nodes, const int32_t* node_ptr_dev, int32_t n_frames,
                                      int32_t max_frame_nodes, int64_t total, float* out, gnncca_stream_t stream);
GNNCCA_API size_t gnncca_rerank_lds_bytes(int32_t max_frame_nodes, int32_t k1, int32_t k2);
GNNCCA_API int gnncca_rerank_frames(const float* dist, int64_t total, int64_t n_nodes, const int32_t* node_ptr_dev, int32_t n_frames,
                                    int32_t max_frame_nodes, int32_t k1, int32_t k2, double lam, float* out, int32_t* rank_out,
                                    int32_t rank_cols, uint64_t* mask_out, gnncca_stream_t stream);
GNNCCA_API int gnncca_rank_predictions(const float* dist, int64_t total, const int32_t* cam, int64_t n_nodes, const int64_t* edge_index,
                                       int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                       int32_t max_frame_nodes, int32_t rank, int64_t* predictions, gnncca_stream_t stream);

/* ---- Cluster summaries and frame-to-frame track ids (csrc/identities.hip) -----------------------------------------------------------
 * No counterpart in the reference, which scores single frames (inference.py:349-371) and neither fuses a cluster nor links two frames.
 * Both stages take a batch laid out as above (node_ptr_dev: int32 [n_frames + 1] in DEVICE memory) and `max_frame_nodes`, the largest
 * frame as the caller's host copy of node_ptr knows it: above GNNCCA_TRACK_MAX_FRAME_NODES it is GNNCCA_ERR_INVALID_ARG before any launch.
 * Every argument is checked before any launch; no host synchronisation, no allocation: capturable.  Deterministic: every floating-point
 * sum has a fixed order, no float atomics.
 *
 * gnncca_cluster_summaries.  Inputs: labels int32 [N] (a node's label is the smallest batch-global node id of its cluster, as
 * gnncca_post_prune_cluster_frames and the host finalisation write it), xw / yw fp64 [N], cam int32 [N] (any values), embeds fp32
 * [N][reid_dim] (NULL with reid_dim = 0).  Outputs, all of fixed shape -- nothing is compacted across frames, so nobody waits for a count:
 *   count int32 [n_frames]   clusters of frame g
 *   rank  int32 [N]          the frame-local index of the node's cluster; clusters are ordered by ascending root id
 *   cluster c of frame g is ROW node_ptr[g] + c of  size int32 [N],  n_cams int32 [N] (distinct cam values among the members),
 *   pos fp64 [N][2] (the sums of xw and of yw over the members in ascending node id, one addition per member from 0.0, then ONE division
 *   by (double)size)  and  emb fp32 [N][reid_dim] (per column the fp32 sum over the members in ascending node id, from 0.0f, then ONE
 *   division by (float)size).  Rows at or beyond count[g] of a frame are zero.
 * An empty frame gives count 0.  A frame that does not fit -- more nodes than max_frame_nodes, a node range outside [0, N], a label
 * outside the node's own frame, a label that is not a root (labels[label] != label) -- reads nothing out of bounds and gets count -1,
 * rank -1 and zero rows (where its node range lies inside [0, N]: there are no rows to speak of otherwise); its neighbours are not
 * affected.  Workspace: gnncca_cluster_summaries_bytes (every cluster's member list).
 *
 * gnncca_link_frames.  Frame t of the batch is linked to frame t - 1, frame 0 to `state_in`, which holds the last frame of the previous
 * call (NULL: nothing to link to, ids start at 0).  Frames are taken to be consecutive and in order.  For cluster a of the current and
 * cluster b of the previous frame, from their `pos` / `emb` rows:  d = sqrt(dx dx + dy dy) (fp64);  dcos = 1 - dot / (sqrt(na) sqrt(nb))
 * with dot, na, nb accumulated in fp64 (1 when a norm is 0);  cost = d / max_step + lam * dcos;  admissible iff d <= max_step and (with
 * has_max_cos) dcos <= max_cos.  With lam == 0 and no max_cos the embeddings are not read (emb may be NULL) and cost = d / max_step.
 * fwd[a] = the admissible b of smallest cost, bwd[b] = the admissible a of smallest cost, ties to the smaller index; a continues b iff
 * fwd[a] == b and bwd[b] == a (one-to-one by construction).  A matched cluster takes its partner's track id; the unmatched ones get
 * next_id, next_id + 1, ... in ascending (frame, rank) order.  A frame with count <= 0 links to nothing.  Outputs: cluster_track int64
 * [N] (row-aligned with the summaries, -1 beyond count), node_track int64 [N] (a detection's track, -1 in a refused frame), matched_prev
 * int32 [N] (the partner's rank in the previous frame, or -1), and state_out: the last frame's count, pos, emb, track ids and next_id
 * (an int64 at offset 0), gnncca_link_state_bytes(capacity, reid_dim) bytes for a capacity of at least the last frame's node count
 * (it bounds the cluster count; a frame with more clusters than state_out_capacity is carried as empty).  state_in must have been
 * written with the same reid_dim and its own capacity (<= GNNCCA_TRACK_MAX_FRAME_NODES); it is not modified.  n_frames = 0 launches
 * nothing and writes nothing.  Out of scope: re-identification after a frame in which a track was not seen (gnncca_link_frames_gap
 * below does that), an optimal assignment per frame pair in place of mutual best (gnncca_link_frames_gap_ex below does that), time
 * stamps (gnncca_link_frames_gap_timed below, with max_gap = 0, does that).  Workspace: gnncca_link_workspace_bytes. */
#define GNNCCA_TRACK_MAX_FRAME_NODES 4096
GNNCCA_API size_t gnncca_cluster_summaries_bytes(int64_t n_nodes, int64_t n_frames);
GNNCCA_API int gnncca_cluster_summaries(const int32_t* labels, const int32_t* node_ptr_dev, const double* xw, const double* yw,
                                        const int32_t* cam, const float* embeds, int32_t reid_dim, int64_t n_nodes, int32_t n_frames,
                                        int32_t max_frame_nodes, int32_t* count_out, int32_t* rank_out, int32_t* size_out,
                                        int32_t* n_cams_out, double* pos_out, float* emb_out, void* workspace, size_t workspace_bytes,
                                        gnncca_stream_t stream);
GNNCCA_API size_t gnncca_link_state_bytes(int64_t capacity, int32_t reid_dim);
GNNCCA_API size_t gnncca_link_workspace_bytes(int64_t n_nodes, int64_t n_frames);
GNNCCA_API int gnncca_link_frames(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos,
                                  const float* emb, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                  double max_step, double lam, int32_t has_max_cos, double max_cos, const void* state_in,
                                  int64_t state_in_capacity, void* state_out, int64_t state_out_capacity, int64_t* cluster_track,
                                  int64_t* node_track, int32_t* matched_prev, void* workspace, size_t workspace_bytes,
                                  gnncca_stream_t stream);

/* gnncca_link_frames_gap: gnncca_link_frames that carries a track across up to max_gap frames that miss it (0 <= max_gap <=
 * GNNCCA_TRACK_MAX_GAP; max_gap = 0 gives gnncca_link_frames' ids).  Time is the frame index over all calls since the state was NULL; a
 * frame without usable clusters (empty, count -1, a node range outside [0, N]) still counts as a frame; n_frames = 0 passes no time,
 * launches nothing and writes nothing.  Every cluster has a predecessor (none at first) and a has-a-successor flag (clear at first).
 * Levels k = 0 .. max_gap run one after the other, within a level all frames t in parallel:  A = the clusters of frame t without a
 * predecessor, B = the clusters of frame t - 1 - k (of this batch or of state_in; no such frame: nothing to do) without a successor;
 * d and dcos as above;  gate_k = max_step * (k + 1), one fp64 multiplication;  admissible iff d <= gate_k and (with has_max_cos) dcos <=
 * max_cos;  cost = d / gate_k + lam * dcos;  fwd / bwd / ties as above over A x B, ties to the smaller rank within the frame;  a continues
 * b iff each is the other's best: then a's predecessor is (frame t - 1 - k, b) and b's flag is set.  Level 0 is gnncca_link_frames' rule
 * with nothing masked; a shorter gap always wins over a longer one; a frame's links depend on earlier frames only, so the result does not
 * depend on how a sequence is cut into calls.  After the last level a cluster with a predecessor takes its id, the others get next_id,
 * next_id + 1, ... in ascending (frame, rank) order.  Outputs as above, where matched_prev is the predecessor's rank in ITS OWN frame,
 * plus matched_gap int32 [N]: the k of the level that found it (frames skipped), -1 without a predecessor.
 * The state holds the last min(max_gap + 1, frames seen) frames, oldest first:  a 64-byte header { int64 next_id (offset 0); int32
 * n_frames; int32 reid_dim; int32 count[GNNCCA_TRACK_MAX_GAP + 1]; padding },  then for C rows in all  pos fp64 [C][2], track int64 [C],
 * emb fp32 [C][R], succ int32 [C] (the final flags),  R = reid_dim if the rule reads embeddings, else 0.  Frame f owns the rows from the sum
 * of the capacities before it; the capacities are HOST arrays (state_in_frame_rows [state_in_frames], state_out_frame_rows
 * [state_out_frames]: per frame at least its node count, which bounds its cluster count, at most GNNCCA_TRACK_MAX_FRAME_NODES) passed to the
 * kernels by value: nothing is read back.  state_out_frames must be min(max_gap + 1, state_in_frames + n_frames); its newest frames are
 * the batch's, the older ones the newest of state_in copied along with the capacities they had there or larger.  state_in (NULL with
 * state_in_frames = 0: nothing seen yet, ids start at 0) must have been written by this entry with the same rule and reid_dim and at most
 * max_gap + 1 frames; it is not modified.  state_out: gnncca_link_gap_state_bytes(C, n_frames_kept, R) bytes.  GNNCCA_ERR_INVALID_ARG:
 * max_gap outside [0, GNNCCA_TRACK_MAX_GAP], a frame capacity above GNNCCA_TRACK_MAX_FRAME_NODES, the checks of gnncca_link_frames.
 * max_gap + 4 launches; deterministic (integer flags, fixed sum orders, no atomics), no host wait, no allocation: capturable.
 * Out of scope: motion prediction (a velocity term); time stamps are gnncca_link_frames_gap_timed's, below; the pairs of a (level, frame pair) table are chosen by mutual best
 * here and by a min-cost assignment in gnncca_link_frames_gap_ex below, in both cases per table, never over time.
 * Workspace: gnncca_link_gap_workspace_bytes(n_nodes, n_frames, state_rows = the sum of state_in_frame_rows). */
#define GNNCCA_TRACK_MAX_GAP 8
GNNCCA_API size_t gnncca_link_gap_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim);
GNNCCA_API size_t gnncca_link_gap_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows);
GNNCCA_API int gnncca_link_frames_gap(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos,
                                      const float* emb, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                      double max_step, double lam, int32_t has_max_cos, double max_cos, int32_t max_gap,
                                      const void* state_in, const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                                      const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track,
                                      int64_t* node_track, int32_t* matched_prev, int32_t* matched_gap, void* workspace,
                                      size_t workspace_bytes, gnncca_stream_t stream);

/* gnncca_link_frames_gap_ex: gnncca_link_frames_gap with the choice of pairs inside a (level, frame pair) table as an argument.
 * matching = 0: mutual best, gnncca_link_frames_gap itself (which calls through with 0; miss_cost is checked and not used).
 * matching = 1: the min-cost assignment of the table (csrc/identities_assign.cuh).  Levels, gates, masks, d, dcos, cost, admissibility,
 * the ids, the outputs, the state and its layout, the workspace and the launch count are gnncca_link_frames_gap's; a state written with
 * one matching is a valid state_in for the other as far as the layout goes, but the ids then follow neither rule.  At level k let A be
 * the clusters of frame t without a predecessor in ascending rank, i = 0 .. n - 1, and B those of frame t - 1 - k without a successor,
 * j = 0 .. m - 1.  A pair is an EDGE iff it is admissible and its cost is not NaN;  w[i][j] = cost - miss_cost (one fp64 subtraction).
 * Chosen is a one-to-one set of edges that minimises the sum of w, where leaving both clusters of a pair unlinked is worth 0: a pair
 * dearer than miss_cost is never worth taking.  The optimum's total is unique, its pairs need not be, so the ALGORITHM is the contract:
 * shortest augmenting paths over n rows and m + n columns, column m + i being row i's "stay unlinked" column (0 for row i, no edge for any
 * other row).  u[] = v[] = 0, p[column] = none; the rows are inserted in the order i = 0 .. n - 1; for each, minv[] = +inf, used[] =
 * false, i0 = i, j0 = none, then repeat:  (1) for every unused column j in ascending order  cur = (w[i0][j] - u[i0]) - v[j];  if cur <
 * minv[j] then minv[j] = cur, way[j] = j0;  if minv[j] < delta (strict, delta = +inf at first) then delta = minv[j], j1 = j -- a tie goes
 * to the smaller column, real columns before the unlinked ones;  (2) u[i] += delta; for every used j: u[p[j]] += delta, v[j] -= delta;
 * for every unused j: minv[j] -= delta;  (3) j1 becomes used; if p[j1] is none, p is flipped back along way[] from j1 (p[j] = p[way[j]],
 * the first column of the path takes row i) and the next row follows; otherwise i0 = p[j1], j0 = j1 and (1) again.  Every operation is
 * an elementwise fp64 one (no contraction); a row needs at most min(n, m) + 1 rounds, which bounds the kernel's loops at launch.
 * a continues b iff p[j] = i at the end.  miss_cost must be finite and > 0; FrameLinker's default is 1 + lam * (max_cos, or 2 without
 * one), the dearest an admissible pair can be.
 * The table lives in LDS (8 P^2 + 76 P + 16 bytes for frames of up to P clusters, P a power of two: 140,816 bytes at 128), so with
 * matching = 1 max_frame_nodes and every state_in_frame_rows entry are at most GNNCCA_TRACK_MAX_OPTIMAL_FRAME_NODES.
 * GNNCCA_ERR_INVALID_ARG, before any launch: a matching other than 0 or 1, a miss_cost that is not finite and > 0, a frame of the batch
 * or of the history above that limit with matching = 1, the checks of gnncca_link_frames_gap.  max_gap + 4 launches; deterministic, no
 * host wait, no allocation: capturable.  Out of scope: an assignment over time (across levels or frames), motion prediction.  Time stamps: gnncca_link_frames_gap_timed. */
#define GNNCCA_TRACK_MAX_OPTIMAL_FRAME_NODES 128
GNNCCA_API int gnncca_link_frames_gap_ex(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos,
                                         const float* emb, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                         double max_step, double lam, int32_t has_max_cos, double max_cos, int32_t max_gap,
                                         int32_t matching, double miss_cost, const void* state_in, const int32_t* state_in_frame_rows,
                                         int32_t state_in_frames, void* state_out, const int32_t* state_out_frame_rows,
                                         int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track, int32_t* matched_prev,
                                         int32_t* matched_gap, void* workspace, size_t workspace_bytes, gnncca_stream_t stream);

/* gnncca_link_frames_motion: gnncca_link_frames_gap (mutual best) that looks for a cluster where it is HEADING.  motion must be 1 (constant
 * velocity from the last link; 0 is gnncca_link_frames_gap itself and is not served here).  The levels, gates, masks, dcos, cost, mutual
 * best, ties and id numbering are gnncca_link_frames_gap's, and so are the meaning of time, of n_frames = 0 and of the host arrays of frame
 * capacities.  Two things are added, step by step:
 *   1. Every cluster has a velocity vel fp64 [2], ground-plane units per frame.  A cluster without a predecessor has vel = (0, 0).  When
 *      cluster a of frame t is linked at level k to cluster b of frame t - 1 - k:  vel(a) = (pos(a) - pos(b)) / (double)(k + 1)  per
 *      component, one subtraction and one division.  No smoothing.
 *   2. At level k the table of frame t uses, for cluster b of frame t - 1 - k,  pred(b) = pos(b) + (double)(k + 1) * vel(b)  per component,
 *      one multiplication and one addition (no FMA);  dx = pos_x(a) - pred_x(b), dy likewise, d = sqrt(dx dx + dy dy);  admissible iff
 *      d <= gate_k = max_step * (k + 1) (and dcos <= max_cos);  cost = d / gate_k + lam * dcos.  max_step is thus the largest deviation from
 *      the predicted position, per frame.  A non-finite prediction gives a NaN or infinite d, which is admissible with nobody.
 * vel(b) is known only when frame t - 1 - k has been through all its levels, so the order is frames outside, levels 0 .. max_gap inside;
 * with every velocity zero that order gives gnncca_link_frames_gap's result (a table (k, t) depends only on tables (k' < k, t' < t) and
 * (k' < k, t)).  The rule is causal: the result does not depend on how a sequence is cut into calls.
 * Outputs: those of gnncca_link_frames_gap plus velocity fp64 [N][2], row-aligned with cluster_track, zero for a cluster without a
 * predecessor and for rows at or beyond a frame's count.
 * The state is of its OWN kind (a gap state is no valid state_in, and the other way round):  the 64-byte header of the gap state, then
 * for C rows in all  pos fp64 [C][2], vel fp64 [C][2], track int64 [C], emb fp32 [C][R], succ int32 [C]  -- the 8-byte arrays first.
 * state_out: gnncca_link_motion_state_bytes(C, n_frames_kept, R) bytes;  workspace: gnncca_link_motion_workspace_bytes(n_nodes, n_frames,
 * state_rows).  Frames of up to GNNCCA_TRACK_MAX_FRAME_NODES detections: the predictions are computed on the fly, they need no LDS.
 * THREE launches whatever max_gap is: a frame-parallel clear, ONE workgroup that walks the frames in order (levels, commits between
 * barriers, ids from the running next_id; nothing waits for another workgroup), a frame-parallel launch for node_track and the new state.
 * Deterministic, no host wait, no allocation: capturable.  GNNCCA_ERR_INVALID_ARG: motion != 1, the checks of gnncca_link_frames_gap.
 * Limits: constant velocity from the LAST link only, so the prediction is wrong after a sharp turn and a track can end there and restart;
 * the min-cost assignment (gnncca_link_frames_gap_ex, matching = 1) has no motion.  Time stamps: gnncca_link_frames_motion_timed. */
GNNCCA_API size_t gnncca_link_motion_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim);
GNNCCA_API size_t gnncca_link_motion_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows);
GNNCCA_API int gnncca_link_frames_motion(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos,
                                         const float* emb, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                         double max_step, double lam, int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t motion,
                                         const void* state_in, const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                                         const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track,
                                         int64_t* node_track, int32_t* matched_prev, int32_t* matched_gap, double* velocity, void* workspace,
                                         size_t workspace_bytes, gnncca_stream_t stream);

/* gnncca_link_frames_gap_timed, gnncca_link_frames_motion_timed: gnncca_link_frames_gap_ex and gnncca_link_frames_motion with a TIME
 * STAMP per frame, so that a dropped frame is a gap and not a silent error.  The arguments are those entries', then frame_time_dev and
 * max_dt; the run is the same one (the untimed entries pass NULL, their launches and their bits are as they were); states, their
 * layouts, the workspaces and the launch counts do not change.  The rule:
 *   Time stamps.  A timed call gives one fp64 time per frame of the batch, in units of the nominal frame period: finite, strictly
 *     increasing, the first strictly greater than the last time of the previous call.  T[f] is the time of frame f over the combined
 *     list (the carried history, then the batch).
 *   Level order.  For frame t at level k the other frame is still s = t - 1 - k, counted in frames PRESENT; a shorter gap still wins, and
 *     the history still holds the last max_gap + 1 frames.
 *   Elapsed time.  dt = T[t] - T[s], one fp64 subtraction, replaces (double)(k + 1) everywhere:  gate = max_step * dt;  with motion
 *     pred(b) = pos(b) + dt * vel(b)  and  vel(a) = (pos(a) - pos(b)) / dt  -- each one operation, in the order of the untimed code, no FMA.
 *   Skipped tables.  A table with !(dt > 0 && dt <= max_dt) has no admissible pair and is skipped whole (which also makes a bad device
 *     array harmless).  max_dt is finite and > 0; FrameLinker's default is max_gap + 1, so a hole of one frame period consumes one unit
 *     of max_gap.
 *   Everything else is the mode's own rule, unchanged: masks, the cosine term, max_cos, cost = d / gate + lam * dcos, ties, mutual best
 *     or the assignment with miss_cost, the numbering of fresh ids, and matched_gap (still the level k).
 *   Consequence.  With T = 0, 1, 2, ... continuing across calls dt is exactly k + 1 and every output equals the untimed entry's bit
 *     for bit.
 * frame_time_dev is a DEVICE array, fp64 [state_in_frames + n_frames]: the times of the frames state_in holds, oldest first, then the
 * batch's.  The CALLER keeps the times of the carried frames (the state does not hold them) and checks the order on the host; the
 * kernels derive dt and the gate per (frame, level) and never loop over the array.  GNNCCA_ERR_INVALID_ARG, before any launch: max_dt
 * not finite and > 0, frame_time_dev NULL with n_frames > 0, the checks of the untimed entry.  A state written by a timed call continued
 * by an untimed one (or the reverse) is valid as far as the layout goes, but the ids then follow neither rule: FrameLinker refuses it.
 * Limit: levels count frames present, so max_gap also bounds how many PRESENT frames a track may skip. */
GNNCCA_API int gnncca_link_frames_gap_timed(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos,
                                            const float* emb, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                            double max_step, double lam, int32_t has_max_cos, double max_cos, int32_t max_gap,
                                            int32_t matching, double miss_cost, const void* state_in, const int32_t* state_in_frame_rows,
                                            int32_t state_in_frames, void* state_out, const int32_t* state_out_frame_rows,
                                            int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track, int32_t* matched_prev,
                                            int32_t* matched_gap, void* workspace, size_t workspace_bytes, gnncca_stream_t stream,
                                            const double* frame_time_dev, double max_dt);
GNNCCA_API int gnncca_link_frames_motion_timed(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos,
                                               const float* emb, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                               double max_step, double lam, int32_t has_max_cos, double max_cos, int32_t max_gap,
                                               int32_t motion, const void* state_in, const int32_t* state_in_frame_rows,
                                               int32_t state_in_frames, void* state_out, const int32_t* state_out_frame_rows,
                                               int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track, int32_t* matched_prev,
                                               int32_t* matched_gap, double* velocity, void* workspace, size_t workspace_bytes,
                                               gnncca_stream_t stream, const double* frame_time_dev, double max_dt);

/* ---- Identity-tracking scores over a sequence (csrc/track_score.cuh, included by csrc/identities.hip) --------------------------------
 * Joins ids int64 [N] (the caller's person id of every detection), cam int32 [N] and node_track int64 [N] (gnncca_link_frames*) over the
 * frames of a sequence, on the device and without a host wait.  No counterpart in the reference.  The rule:
 *   detection i is VALID iff 0 <= ids[i] < max_ids, 0 <= cam[i] < max_cams and 0 <= node_track[i] < 2^40;  it is SCORED iff it is valid
 *   and no valid detection j > i of its frame has the same (id, cam) -- the largest node id wins a duplicate;  every other detection is
 *   IGNORED (switched = -1).  A stream is a pair (person p, camera c), k = p * max_cams + c.  A scored detection with track t is a SWITCH
 *   (switched = 1, else 0) iff the latest earlier scored detection of its stream, in this call or any earlier one since the reset and
 *   however many frames back, had a track != t.  n[p][t] counts the scored detections of person p with track t.
 * The rule is causal: the result does not depend on how a sequence is cut into calls; the state holds no time, so a call without frames
 * or without detections changes nothing.
 * State, all sized by the caller from numbers it knows on the host:  `table`, ONE int64 buffer [GNNCCA_SCORE_HEADER_LEN + 2 cap] =
 * { scored, ignored, switches, pairs (non-zero cells of n), overflow, 3 unused | keys uint64 [cap] | counts int64 [cap] }, an
 * open-addressing table with linear probing: cap a power of two >= GNNCCA_SCORE_MIN_CAP, key = p << 40 | t, all ones = empty;  `last`
 * int64 [K = max_ids * max_cams], the last track of every stream, -1 for none.  gnncca_track_score_reset initialises both.  The caller
 * keeps cap >= 2 x the detections passed since the reset (pairs <= detections): gnncca_track_score_rehash fills a larger table from a
 * smaller one (table_out is overwritten, table_in is not modified; the counters carry over).  A probe gives up after cap steps, sets
 * `overflow` and drops its run, so no size can make a kernel spin; with the sizing above it cannot happen.
 * gnncca_track_score_add scores the n_frames frames whose offsets are node_ptr_dev[0 .. n_frames] - node_base (DEVICE int32; node_base is
 * the HOST copy of node_ptr_dev[0], so a run of frames inside a larger batch is passed with shifted pointers); ids, cam, node_track and
 * switched int32 [n_nodes] (output) start at the run's first detection.  `slot` is scratch: int32 [n_frames][K], at most
 * GNNCCA_SCORE_MAX_SLOTS entries -- a larger batch is cut into runs of frames by the caller, which the rule's causality allows.  One memset
 * and two launches; all atomics are integer and device scope, so every number is reproducible (only the cell a pair lands in is not).
 * No allocation, no synchronisation: capturable.  GNNCCA_ERR_INVALID_ARG before any launch: max_ids outside [1, GNNCCA_SCORE_MAX_IDS],
 * max_cams outside [1, GNNCCA_SCORE_MAX_CAMS], K above GNNCCA_SCORE_MAX_STREAMS, n_frames * K above GNNCCA_SCORE_MAX_SLOTS, n_nodes >=
 * 2^31 - 256, a cap that is no power of two >= GNNCCA_SCORE_MIN_CAP, null pointers. */
#define GNNCCA_SCORE_MAX_IDS 65536
#define GNNCCA_SCORE_MAX_CAMS 64
#define GNNCCA_SCORE_MAX_STREAMS 1048576
#define GNNCCA_SCORE_MAX_SLOTS 4194304
#define GNNCCA_SCORE_MIN_CAP 1024
#define GNNCCA_SCORE_HEADER_LEN 8
GNNCCA_API size_t gnncca_track_score_table_bytes(int64_t cap);
GNNCCA_API int gnncca_track_score_reset(void* table, int64_t cap, int64_t* last, int64_t n_streams, gnncca_stream_t stream);
GNNCCA_API int gnncca_track_score_rehash(const void* table_in, int64_t cap_in, void* table_out, int64_t cap_out, gnncca_stream_t stream);
GNNCCA_API int gnncca_track_score_add(const int64_t* ids, const int32_t* cam, const int64_t* node_track, const int32_t* node_ptr_dev,
                                      int64_t node_base, int64_t n_nodes, int32_t n_frames, int32_t max_ids, int32_t max_cams, void* table,
                                      int64_t cap, int64_t* last, int32_t* slot, int32_t* switched, gnncca_stream_t stream);

/* ---- Re-entry gallery (csrc/identities_reentry.cuh, included by csrc/identities.hip) ---------------------------------------------------
 * A second stage behind gnncca_link_frames*: a track born after an absence longer than the linker bridges gets the IDENTITY of the ended
 * track it looks like.  Track ids stay as the linker gave them; identities are what a consumer scores.  No counterpart in the reference.
 * Notation: M = max_gap (the linker's), W = window, S = W + max_batch ring slots, f = frames_seen + the frame's index in the call (the
 * caller counts the frames of all calls; an empty or refused frame counts).  A BIRTH is a usable cluster (rank < the frame's count) with
 * matched_prev == -1; b is its cluster_track.  The inputs cluster_track, matched_prev, matched_gap are the linker's outputs for the SAME
 * summaries (matched_gap of gnncca_link_frames: 0 where matched_prev >= 0, else -1).
 * State.  ring_state, gnncca_reentry_state_bytes(S, R) bytes, updated IN PLACE: owner int64 [S] (-1: empty), identity int64 [S], last
 *   int64 [S], pos fp64 [S][2], continued int32 [S], then from the next 256-byte boundary sum fp32 [S][R].  Track j lives in slot j mod S.
 *   A fresh ring has owner = -1 and everything else 0 (the caller fills it).  And the identities of the rows of the last M + 1 frames,
 *   hist_in -> hist_out int64, frame after frame, each frame with the row capacity the caller gives in hist_*_frame_rows (host arrays, as
 *   the state_*_frame_rows of gnncca_link_frames_gap: per frame its node count; hist_out_frames = min(hist_in_frames + n_frames, M + 1)).
 * Frames in order; for frame f:
 *   1. a continued cluster (matched_prev = m >= 0, matched_gap = k) takes the identity of row m of frame f - 1 - k, from this call's
 *      cluster_identity or from hist_in -- never through the ring, so a track may live longer than S births;
 *   2. track j is eligible for birth b iff  b - W <= j < b and owner[j mod S] == j;  continued[j] == 0;  f - last[j] >= M + 2;  max_age
 *      absent or f - last[j] <= max_age;  max_speed absent or d <= max_speed * (double)(f - last[j]) with d = sqrt(dx dx + dy dy) between
 *      the birth's pos and pos[j];  dcos <= max_cos, where dcos = 1 - <e, sum[j]> / (|e| |sum[j]|) in fp64 over the birth's emb row e
 *      (1 if a norm is 0; a NaN is admissible with nobody).  cost = dcos;
 *   3. mutual best among the births of the frame: b's best j has the smallest cost, ties to the smaller j; j's best birth the smallest
 *      cost, ties to the smaller rank.  Mutual: identity(b) = identity[j], continued[j] = 1, reentered_from = j.  Else identity(b) = b;
 *   4. a birth takes slot b mod S whatever it held: owner = b, sum = 0, continued = 0, identity = identity(b);
 *   5. every usable cluster whose track t has owner[t mod S] == t: sum += emb row (fp32, one addition per column, in frame order),
 *      last = f, pos = its pos.  A cluster whose slot was taken by a younger track is skipped.
 * Consequences: the result does not depend on how a sequence is cut into calls; with n_nodes <= max_batch an eligible track's slot cannot
 * have been taken by a birth of the same call; an eligible track can no longer be continued by the linker, so its sum / last / pos are
 * final -- the kernels accumulate them for the whole call first.  The dot product is a chain of fp64 fused multiply-adds in ascending
 * column order, the norms lane-strided fp64 sums: decisions equal the numpy restatement's wherever no comparison hangs on the last bits.
 * The births of a call must carry consecutive track ids in row order (every gnncca_link_frames* numbers fresh ids so); otherwise
 * nobody re-enters in that call.
 * Outputs: cluster_identity int64 [N] (row-aligned with cluster_track, -1 beyond a frame's count), node_identity int64 [N] (through
 * rank), reentered_from int64 [N] (the old TRACK id a born cluster was attached to, else -1).
 * workspace: gnncca_reentry_workspace_bytes(n_nodes, window, max_batch) bytes: the cost table fp64 [n_nodes][W] and O(n_nodes + S) more.
 * Six launches (prep, mark, accumulate, norms, the tiled cosine table, one walking workgroup); deterministic, no host wait, no
 * allocation: capturable.  n_frames = 0 launches nothing.  GNNCCA_ERR_INVALID_ARG before any launch: max_cos outside [0, 2], window
 * outside [1, GNNCCA_REENTRY_MAX_WINDOW], max_batch < 1, n_nodes > max_batch, max_age < M + 2, max_speed not finite and > 0, reid_dim < 1,
 * max_gap outside [0, GNNCCA_TRACK_MAX_GAP], a frame above GNNCCA_TRACK_MAX_FRAME_NODES, inconsistent history frames, a NULL array.
 * Limits: appearance decides (max_speed is the only use of position); chains are one-to-one, an ended track is continued once; a person
 * absent while more than W other tracks are born is forgotten; n_nodes <= max_batch per call. */
#define GNNCCA_REENTRY_MAX_WINDOW 4096
GNNCCA_API size_t gnncca_reentry_state_bytes(int64_t n_slots, int32_t reid_dim);
GNNCCA_API size_t gnncca_reentry_workspace_bytes(int64_t n_nodes, int32_t window, int32_t max_batch);
GNNCCA_API int gnncca_reentry_update(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                                     int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                     const int64_t* cluster_track, const int32_t* matched_prev, const int32_t* matched_gap, int32_t max_gap,
                                     double max_cos, int32_t window, int32_t max_batch, int32_t has_max_age, int64_t max_age,
                                     int32_t has_max_speed, double max_speed, int64_t frames_seen, void* ring_state, const int64_t* hist_in,
                                     const int32_t* hist_in_frame_rows, int32_t hist_in_frames, int64_t* hist_out,
                                     const int32_t* hist_out_frame_rows, int32_t hist_out_frames, int64_t* cluster_identity,
                                     int64_t* node_identity, int64_t* reentered_from, void* workspace, size_t workspace_bytes,
                                     gnncca_stream_t stream);

/* ---- Track smoother (csrc/identities_smooth.cuh, included by csrc/identities.hip) ------------------------------------------------------
 * A stage behind gnncca_link_frames*: a constant-velocity Kalman filter along every track, so that a consumer gets trajectories --
 * filtered position, velocity, their covariance, how far a detection lay from where its track was expected (nis) and the links since
 * birth (age).  It filters after linking and gates nothing: matched_prev / matched_gap are the linker's outputs for the SAME summaries
 * (matched_gap of gnncca_link_frames: 0 where matched_prev >= 0, else -1).  No counterpart in the reference.  The rule:
 *   The two ground-plane axes are independent and share one 2 x 2 covariance (a, b, c) = (var pos, cov pos/vel, var vel).  q: process
 *   noise intensity, finite and >= 0; r: measurement variance, finite and > 0; vel_var: initial velocity variance, finite and > 0;
 *   per_detection (0 / 1): the measurement variance of a cluster is re = r / (double)size when 1 (a cluster fused from more detections
 *   is trusted more), else re = r.  For cluster a of frame t with measurement z = pos(a):
 *   Birth (matched_gap(a) == -1):  p = z, v = (0, 0), (a, b, c) = (re, 0, vel_var), age = 0, nis = 0.
 *   Link to cluster m = matched_prev(a) of frame t - 1 - k, k = matched_gap(a):  dt = (double)(k + 1) without time stamps, with them
 *   dt = T[t] - T[t - 1 - k] (frames counted among frames PRESENT, exactly as the linker counts them); start from that cluster's
 *   filtered state (p, v, a, b, c, age).  Every line is one fp64 operation per operator as written, left to right, no FMA:
 *     dt2 = dt*dt;  dt3 = dt2*dt
 *     pp  = p + dt*v                               (per axis)
 *     a_  = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0
 *     b_  = (b + dt*c) + (q*dt2)/2.0
 *     c_  = c + q*dt
 *     s   = a_ + re
 *     k1  = a_/s;  k2 = b_/s
 *     i   = z - pp                                 (per axis)
 *     p'  = pp + k1*i;  v' = v + k2*i              (per axis)
 *     a'  = a_ - k1*a_;  b' = b_ - k1*b_;  c' = c_ - k2*b_
 *     nis = (ix*ix + iy*iy)/s
 *     age' = age + 1
 *   Non-finite inputs propagate: there is no special case.  Rows at or beyond a frame's count, and every row of a refused frame, get
 *   zeros in the fp64 outputs and age = -1.  The rule is causal along predecessor links only: the result does not depend on how a
 *   sequence is cut into calls.  A link that points at nothing (a level outside 0 .. max_gap, a rank at or beyond its frame's count, a
 *   frame before the carried history) is a birth; no linker of this library makes one.
 * State (state_in is never written, state_out is overwritten), gnncca_track_smooth_state_bytes(capacity_rows, n_frames_kept) bytes: a
 *   64-byte header (int32 n_frames, int32 count[9]: the usable cluster count per frame, zeros), then for a capacity of C rows fp64 [C][7]
 *   (px, py, vx, vy, a, b, c), then int32 age [C] (-1: not a cluster) -- the 8-byte array before the 4-byte one.  The rows are aligned with
 *   the linker's kept frames: the last max_gap + 1 frames, each with the row capacity the caller gives in state_*_frame_rows (host
 *   arrays, as the state_*_frame_rows of gnncca_link_frames_gap: per frame its node count; state_out_frames = min(state_in_frames +
 *   n_frames, max_gap + 1); a history frame that stays keeps its capacity).
 * Outputs, row-aligned with cluster_track: out_pos, out_vel fp64 [N][2], out_cov fp64 [N][3], out_nis fp64 [N], out_age int32 [N].
 * frame_time_dev: NULL (no time stamps), or the DEVICE array fp64 [state_in_frames + n_frames] the _timed linker entries take; max_dt is
 *   then checked like theirs (finite and > 0) and gates nothing: whatever the linker linked is filtered.
 * workspace: gnncca_track_smooth_workspace_bytes(n_nodes, n_frames, state_rows) bytes: a successor row int32 per combined row (the
 *   state_rows history rows, then the batch rows), and the frame and the new-state row of every batch row.
 * Three launches whatever max_gap and n_frames are, kernels only (no memset node: a captured call must replay): the workspace = -1,
 * the successor rows (frame-parallel, plain stores: links are one-to-one), then a thread per combined row, where the head of every
 * chain walks it, at most n_frames steps; every index taken from the workspace is checked against its own range.  Deterministic for one-to-one links, which is what every
 * linker gives (of two clusters that name the same predecessor, which stays on the chain and which starts as a birth is not fixed); no
 * host wait, no allocation, no cooperative launch: capturable.  n_frames = 0 launches nothing (the caller keeps its state); n_nodes = 0
 * with n_frames > 0 still passes time: the walk launch moves the history rows that stay to their new slots.
 * GNNCCA_ERR_INVALID_ARG before any launch: q, r, vel_var out of range, per_detection not 0 / 1, max_dt not finite and > 0 with
 * frame_time_dev, max_gap outside [0, GNNCCA_TRACK_MAX_GAP], a frame above GNNCCA_TRACK_MAX_FRAME_NODES, inconsistent frame-row lists, a
 * NULL array; GNNCCA_ERR_WORKSPACE: a short workspace (the status every entry of this library gives for one).
 * Limits: constant velocity, one (q, r) for every track; it follows the linker's links only -- a track the re-entry gallery re-attaches
 * starts a fresh filter. */
GNNCCA_API size_t gnncca_track_smooth_state_bytes(int64_t capacity_rows, int32_t n_frames_kept);
GNNCCA_API size_t gnncca_track_smooth_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows);
GNNCCA_API int gnncca_track_smooth(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* size, const double* pos,
                                   const int32_t* matched_prev, const int32_t* matched_gap, int64_t n_nodes, int32_t n_frames,
                                   int32_t max_frame_nodes, int32_t max_gap, double q, double r, double vel_var, int32_t per_detection,
                                   const void* state_in, const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                                   const int32_t* state_out_frame_rows, int32_t state_out_frames, double* out_pos, double* out_vel,
                                   double* out_cov, double* out_nis, int32_t* out_age, void* workspace, size_t workspace_bytes,
                                   gnncca_stream_t stream, const double* frame_time_dev, double max_dt);

/* ---- Linking by the filtered state (csrc/identities_kalman.cuh, included by csrc/identities.hip) ---------------------------------------
 * gnncca_link_frames_kalman: gnncca_link_frames_motion whose motion model is the constant-velocity Kalman filter of gnncca_track_smooth,
 * run INSIDE the linker: a track is looked for where its filtered state predicts it, every link feeds the filter, and a pair can be gated
 * by the variance of that prediction, so that a newborn track (velocity unknown: variance vel_var) is looked for widely and an established
 * one narrowly.  Mutual best only.  q, r, vel_var: the smoother's numbers (q finite and >= 0; r, vel_var finite and > 0; re = r for every
 * cluster: there is no per_detection here).  max_nis (read iff has_max_nis = 1): finite and > 0.  The rule, in full:
 *   Order.  Frames outside, levels k = 0 .. max_gap inside, exactly as in gnncca_link_frames_motion; the meaning of time, of n_frames = 0
 *     and of the host arrays of frame capacities are gnncca_link_frames_gap's.  dt = (double)(k + 1); with time stamps (frame_time_dev
 *     not NULL: the array of the _timed entries) dt = T[t] - T[t - 1 - k], one fp64 subtraction, and a table with !(dt > 0 && dt <= max_dt)
 *     is skipped whole.
 *   State.  Every cluster carries a filtered state x = (px, py, vx, vy, a, b, c), (a, b, c) = (var pos, cov pos/vel, var vel) shared by
 *     the two axes, and an age.
 *   Candidates and prediction.  At level k the clusters a of frame t without a predecessor meet the clusters b of frame t - 1 - k without
 *     a successor.  b stands at  pred(b) = p(b) + dt * v(b)  per component, one multiplication and one addition (no FMA), from the
 *     FILTERED position and velocity.
 *   Pair rule.  The shared one:  dx = pos_x(a) - pred_x(b), dy likewise, with the RAW pos(a);  d = sqrt(dx*dx + dy*dy);  gate = max_step * dt
 *     (one multiplication);  dcos and max_cos as in gnncca_link_frames;  cost = d / gate + lam * dcos;  admissible iff d <= gate (and
 *     dcos <= max_cos) and, with has_max_nis, also  (dx*dx + dy*dy) / s <= max_nis  where
 *       dt2 = dt*dt;  dt3 = dt2*dt;  a_ = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0;  s = a_ + r
 *     from b's (a, b, c): the operations of the smoother's rule in its order, one fp64 operation per operator, no FMA.  A NaN is
 *     admissible with nobody.
 *   Matching.  fwd[a] = the admissible b of smallest cost, bwd[b] = the admissible a of smallest cost, ties to the smaller rank; a
 *     continues b iff each is the other's best.  Levels go in order, so a shorter gap always wins.
 *   Commit.  For a linked at level k to b:  x(a), nis(a), age(a) = step(x(b), age(b), z = pos(a), dt, q, re = r)  where step is the link
 *     rule of gnncca_track_smooth verbatim (pp, a_, b_, c_, s, k1, k2, i, p', v', a', b', c', nis, age' = age + 1).
 *   Births.  A cluster without a predecessor after all levels:  x = (z, 0, 0, r, 0, vel_var), age = 0, nis = 0, z = pos(a).
 *   Ids.  A linked cluster takes its predecessor's id; the others get next_id, next_id + 1, ... in ascending (frame, rank) order.
 *   Consequences.  The rule is causal: the result does not depend on how a sequence is cut into calls.  And gnncca_track_smooth with the
 *     same (q, r, vel_var), per_detection = 0, fed this entry's matched_prev / matched_gap (and times) returns exactly out_pos .. out_age.
 * Outputs: cluster_track, node_track, matched_prev, matched_gap as gnncca_link_frames_motion; out_pos, out_vel fp64 [N][2] (the filtered
 * position and velocity: out_vel takes the place of that entry's velocity), out_cov fp64 [N][3], out_nis fp64 [N], out_age int32 [N], all
 * row-aligned with cluster_track; rows at or beyond a frame's count, and every row of a refused frame, are zero with age = -1.
 * The state is of its OWN kind: the 64-byte header of the gap state, then for C rows in all  pos fp64 [C][2], vel fp64 [C][2] (both
 * FILTERED), cov fp64 [C][3], track int64 [C], emb fp32 [C][R], succ int32 [C], age int32 [C]  -- the 8-byte arrays first; 28 bytes per
 * row more than the motion state.  state_out: gnncca_link_kalman_state_bytes(C, n_frames_kept, R) bytes;  workspace:
 * gnncca_link_kalman_workspace_bytes(n_nodes, n_frames, state_rows).
 * THREE launches whatever max_gap is: a frame-parallel clear, ONE workgroup of 1024 threads that walks the frames in order (with
 * has_max_nis it computes s once per level into LDS, 8 bytes per cluster beside the 12 of the motion walk: 80 KiB at 4096 rows), a
 * frame-parallel launch for node_track and the new state.  Deterministic, no host wait, no allocation: capturable.
 * GNNCCA_ERR_INVALID_ARG before any launch: q, r, vel_var out of range, has_max_nis not 0 / 1, max_nis not finite and > 0 with it, max_dt
 * not finite and > 0 with frame_time_dev, the checks of gnncca_link_frames_gap;  GNNCCA_ERR_WORKSPACE: a short workspace.
 * Limits: constant velocity, one (q, r) for every track, no per_detection, no min-cost assignment; a track the re-entry gallery
 * re-attaches starts a fresh filter. */
GNNCCA_API size_t gnncca_link_kalman_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim);
GNNCCA_API size_t gnncca_link_kalman_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows);
GNNCCA_API int gnncca_link_frames_kalman(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos,
                                         const float* emb, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                                         double max_step, double lam, int32_t has_max_cos, double max_cos, int32_t max_gap, double q,
                                         double r, double vel_var, int32_t has_max_nis, double max_nis, const void* state_in,
                                         const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                                         const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track,
                                         int64_t* node_track, int32_t* matched_prev, int32_t* matched_gap, double* out_pos,
                                         double* out_vel, double* out_cov, double* out_nis, int32_t* out_age, void* workspace,
                                         size_t workspace_bytes, gnncca_stream_t stream, const double* frame_time_dev, double max_dt);

/* ---- Training loss and its statistics (compute_loss_acc, train.py:51-208, and the mean probabilities of train.py:460-469) ---------
 * Inputs: logits fp32 [n_steps][n_edges] (step-major: the [S, E, 1] buffer of the MPN training forward), labels fp32 [n_edges] (0 / 1).
 * criterion: GNNCCA_LOSS_BCE, GNNCCA_LOSS_BCE_WEIGHTED (pos_weight > 0) or GNNCCA_LOSS_FOCAL (utils.FocalLoss_binary: focusing_param,
 * balance_param; with reduction 'mean' the focal factor applies to the step's mean BCE, with 'none' to every edge's).  validate != 0
 * uses plain BCE with logits whatever the criterion, as the reference does.  The forward writes loss_out fp32 [1] (the sum over steps of
 * the criterion) and record fp64 [GNNCCA_LOSS_REC_LEN(n_steps)]:
 *   loss, loss_class1, loss_class0 (sums over steps of the per-edge loss averaged over label 1 / label 0: NaN for an empty class),
 *   precision1, precision0, precision ((hits / count) * 100.0 on the last step with sigmoid(x) >= 0.5f, 0 without a hit), n_pos, n_neg,
 *   mean_prob [n_steps][2] (mean sigmoid over label 0, label 1; 0.5 for an empty class), coef [n_steps] (d loss / d mean BCE of step s).
 * With history != NULL the record is also written to row cursor[0] of history fp64 [capacity][REC_LEN] and cursor[0] is incremented,
 * on the device; past capacity cursor[1] is set to 1 and nothing is written.  n_edges = 0 gives NaN losses, zero precisions and mean
 * probabilities of 0.5.  The backward writes grad fp32 [n_steps][n_edges] = g * coef[s] * t(x, y) / n_edges, g = grad_loss[0] (device).
 * Deterministic (fixed-order fp64 sums, no float atomics) and capturable (workspace from the caller, no synchronisation).  Arguments are
 * checked before any launch. */
#define GNNCCA_LOSS_BCE 0
#define GNNCCA_LOSS_BCE_WEIGHTED 1
#define GNNCCA_LOSS_FOCAL 2
#define GNNCCA_LOSS_MAX_STEPS 64
#define GNNCCA_LOSS_REC_LOSS 0
#define GNNCCA_LOSS_REC_LOSS1 1
#define GNNCCA_LOSS_REC_LOSS0 2
#define GNNCCA_LOSS_REC_PREC1 3
#define GNNCCA_LOSS_REC_PREC0 4
#define GNNCCA_LOSS_REC_PREC 5
#define GNNCCA_LOSS_REC_NPOS 6
#define GNNCCA_LOSS_REC_NNEG 7
#define GNNCCA_LOSS_REC_MEAN_PROB 8
#define GNNCCA_LOSS_REC_LEN(n_steps) (8 + 3 * (n_steps))
GNNCCA_API size_t gnncca_edge_loss_workspace_bytes(int32_t n_steps, int64_t n_edges);
GNNCCA_API int gnncca_edge_loss_forward(const float* logits, const float* labels, int32_t n_steps, int64_t n_edges, int32_t criterion,
                                        int32_t validate, float pos_weight, float focusing_param, float balance_param, float* loss_out,
                                        double* record, double* history, int64_t capacity, int64_t* cursor, void* workspace,
                                        size_t workspace_bytes, gnncca_stream_t stream);
GNNCCA_API int gnncca_edge_loss_backward(const float* logits, const float* labels, int32_t n_steps, int64_t n_edges, int32_t criterion,
                                         int32_t validate, float pos_weight, const float* grad_loss, const double* record, float* grad,
                                         gnncca_stream_t stream);

/* ---- Optimizer step (train.py:492-494; the optimizers and schedules of main_training.py:220-256, 349-370) --------------------------
 * torch.optim.SGD (weight_decay, momentum, dampening, nesterov; the momentum buffer of a tensor is initialised to its gradient on the
 * tensor's first step) and torch.optim.Adam (betas, eps, L2 weight_decay, amsgrad; bias corrections in fp64 from the step count) on fp32
 * tensors, one launch per GNNCCA_OPTIM_MAX_TENSORS_PER_LAUNCH tensors.  The launches take NO hyperparameter and NO step count as an
 * argument: they read them from the "block", a zero-initialised device buffer of gnncca_optim_block_bytes(n_slots) bytes that belongs to
 * one parameter group:
 *   fp64 [8] at GNNCCA_OPTIM_BLOCK_HYPER_OFFSET   lr, weight_decay, a, b, c, flag, rule, unused (written by gnncca_optim_set_hyper:
 *                                                 SGD a = momentum, b = dampening, flag = nesterov; Adam a = beta1, b = beta2, c = eps,
 *                                                 flag = amsgrad)
 *   uint32 at GNNCCA_OPTIM_BLOCK_TICKET_OFFSET    the launch's ticket word (0 between launches)
 *   int32 [n_slots] at GNNCCA_OPTIM_BLOCK_STEPS_OFFSET   one step count per tensor slot, advanced ON THE DEVICE by the step launch itself
 *                                                 (Adam: steps taken; SGD: steps the tensor's momentum buffer has seen).  The caller may
 *                                                 read and write them between launches (checkpoints).
 * so a HIP graph that captured a step follows whatever gnncca_optim_set_hyper writes between its replays.  params / grads / state are HOST
 * arrays of n_tensors DEVICE pointers, copied into the launch arguments by value (a captured graph keeps the addresses of its capture);
 * numel[i] elements each, slots[i] in [0, n_slots) and distinct.  SGD: momentum_bufs (or single entries of it) may be NULL, the tensor
 * is then stepped without momentum.  Adam: exp_avg and exp_avg_sq are required, max_exp_avg_sq (or entries) may be NULL without amsgrad.
 * A state tensor is not read on its slot's first step (count 0), so it needs no initialisation.  16-byte accesses where every pointer
 * of a tensor is 16-byte aligned, 4-byte ones otherwise.  Every argument is checked before any launch (GNNCCA_ERR_INVALID_ARG: null
 * pointers, negative sizes, an unknown rule, lr / weight_decay / momentum / eps negative or not finite, Nesterov without momentum or with
 * dampening, a beta outside [0, 1)); capturable: no allocation, no synchronisation, nothing read back. */
#define GNNCCA_OPTIM_SGD 0
#define GNNCCA_OPTIM_ADAM 1
#define GNNCCA_OPTIM_MAX_TENSORS_PER_LAUNCH 64
#define GNNCCA_OPTIM_BLOCK_HYPER_OFFSET 0
#define GNNCCA_OPTIM_BLOCK_TICKET_OFFSET 64
#define GNNCCA_OPTIM_BLOCK_STEPS_OFFSET 80
GNNCCA_API size_t gnncca_optim_block_bytes(int32_t n_slots);
GNNCCA_API int gnncca_optim_set_hyper(void* block, int32_t rule, double lr, double weight_decay, double a, double b, double c, int32_t flag,
                                      gnncca_stream_t stream);
GNNCCA_API int gnncca_optim_sgd_step(void* block, int32_t n_slots, int32_t n_tensors, void* const* params, const void* const* grads,
                                     void* const* momentum_bufs, const int64_t* numel, const int32_t* slots, gnncca_stream_t stream);
GNNCCA_API int gnncca_optim_adam_step(void* block, int32_t n_slots, int32_t n_tensors, void* const* params, const void* const* grads,
                                      void* const* exp_avg, void* const* exp_avg_sq, void* const* max_exp_avg_sq, const int64_t* numel,
                                      const int32_t* slots, gnncca_stream_t stream);

/* Synchronises `stream` and returns the flag word of the last forward that used `workspace`. */
GNNCCA_API int gnncca_read_graph_flags(const void* workspace, uint32_t* flags_out, gnncca_stream_t stream);
/* The same plus, in flags_out[1], the column-range verdict of that forward: 0 = every node's target ids were <= 2 contiguous runs (or
 * the forward never asked: no GNNCCA_OPT_COLUMN_RANGES, L < 2, general kernels), 1 = some node's were not and every step streamed them. */
GNNCCA_API int gnncca_read_graph_flags2(const void* workspace, uint32_t flags_out[2], gnncca_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNCCA_MPN_H */
