"""ctypes binding of include/gnncca_mpn.h (libgnncca_mpn.so).  No compute here and no fallback: if the library is
missing or a call fails, the caller gets an exception."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GNNCCA_LIB") or os.path.join(HERE, "lib", "libgnncca_mpn.so")  # GNNCCA_LIB: diagnostic builds

ABI_VERSION = 2
MAX_LAYERS = 8
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_HIP, ERR_NO_DEVICE = range(6)
AGG = {"sum": 0, "mean": 1, "max": 2}
GRAPH_UNSORTED, GRAPH_BAD_INDEX = 1, 2
RANK_BY = {"ground": 0, "reid": 1}   # gnncca_build_edges_topk, gnncca_frames_forward_topk
TOPK_MAX_DEG = 4096
TRACK_MAX_GAP = 8                    # gnncca_link_frames_gap
TRACK_MAX_OPTIMAL_FRAME_NODES = 128  # gnncca_link_frames_gap_ex with matching = 1: a frame pair's table lives in LDS
MATCHING = {"mutual": 0, "optimal": 1}   # gnncca_link_frames_gap_ex
MOTION = {"none": 0, "velocity": 1}      # gnncca_link_frames_motion takes 1; "none" is the entries above
SCORE_MAX_IDS, SCORE_MAX_CAMS, SCORE_MAX_STREAMS, SCORE_MAX_SLOTS = 65536, 64, 1 << 20, 1 << 22   # gnncca_track_score_add
SCORE_MIN_CAP, SCORE_HEADER_LEN = 1024, 8
REENTRY_MAX_WINDOW = 4096            # gnncca_reentry_update: the walking workgroup keeps a frame's candidate tracks in LDS
SYMMETRIC = {"union": 1, "mutual": 2}   # gnncca_build_edges_topk_sym_count
RADIUS_UNIT = {"ground": 0, "max_dist": 1}   # GNNCCA_RADIUS_UNIT_*: gnncca_plan_frames_radius, gnncca_build_edges_radius, gnncca_frames_forward_radius
SWEEP_MAX_THRESHOLDS = 1024          # gnncca_eval_sweep
JOINT_MAX_SCORES = 4                 # gnncca_eval_sweep_joint
JOINT_MAX_POINTS = 16384
CMP = {"ge": 0, "gt": 1, "le": 2, "lt": 3}   # GNNCCA_CMP_*
RANK_MAX_SCORES, RANK_MAX_FRAME_EDGES, RANK_POOL_MAX_THRESHOLDS = 4, 16384, 65536   # gnncca_rank_metrics, gnncca_rank_pool_add
EXCLUSIVE_MAX_FRAME_NODES, EXCLUSIVE_MAX_CAMERAS = 4096, 64   # gnncca_post_exclusive_frames: 12-bit local ids, one 64-bit camera mask
EXCLUSIVE_BAD_CAMERA, EXCLUSIVE_BAD_RANGE = 1, 2              # its flags_out[g]
STRONG_MAX_FRAME_NODES, STRONG_BAD_RANGE = 1024, 2             # gnncca_post_strong_frames: a frame's reachability bit matrix lives in LDS
RERANK_MAX_FRAME_NODES, RERANK_MAX_K1 = 128, 64  # gnncca_rerank_frames, gnncca_rank_predictions: a frame's tables and masks live in LDS


class Layer(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("out_dim", C.c_int32), ("has_bn", C.c_int32), ("relu", C.c_int32)]


class Mlp(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("layers", Layer * MAX_LAYERS)]


class MpnDims(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("node_in", C.c_int32), ("edge_in", C.c_int32), ("node_dim", C.c_int32),
                ("edge_dim", C.c_int32), ("agg", C.c_int32), ("num_enc_steps", C.c_int32),
                ("num_class_steps", C.c_int32), ("reattach_nodes", C.c_int32), ("reattach_edges", C.c_int32),
                ("enc_node", Mlp), ("enc_edge", Mlp), ("edge_mlp", Mlp), ("node_mlp", Mlp), ("cls_edge", Mlp)]


class Frames(C.Structure):
    _fields_ = [("xw", C.c_void_p), ("yw", C.c_void_p), ("max_dist", C.c_void_p), ("person_id", C.c_void_p),
                ("cam", C.c_void_p), ("graph_of", C.c_void_p), ("graph_ptr", C.c_void_p), ("src_order", C.c_void_p),
                ("edge_ptr", C.c_void_p)]


class FramesIO(C.Structure):
    _fields_ = [("staged_dev", C.c_void_p), ("n_nodes", C.c_int64), ("n_frames", C.c_int64), ("n_edges", C.c_int64),
                ("node_embeds", C.c_void_p), ("reid_embeds", C.c_void_p), ("reid_dim", C.c_int32), ("mode", C.c_int32), ("normalize", C.c_int32),
                ("node_norm", C.c_void_p), ("reid_norm", C.c_void_p), ("edge_index", C.c_void_p), ("edge_attr", C.c_void_p),
                ("edge_labels", C.c_void_p), ("logits", C.c_void_p), ("probs", C.c_void_p), ("predictions", C.c_void_p), ("pruned", C.c_void_p),
                ("counters", C.c_void_p), ("labels", C.c_void_p), ("counters_len", C.c_int64)]


class PostBatch(C.Structure):
    """gnncca_post_batch (include/gnncca_mpn.h): one batch's HOST copies for the asynchronous finalizer pool."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("node_ptr", C.c_void_p), ("edge_ptr", C.c_void_p), ("n_frames", C.c_int32),
                ("switches", C.c_int32), ("triggers", C.c_void_p), ("probs", C.c_void_p), ("predictions", C.c_void_p), ("labels", C.c_void_p),
                ("n_clusters", C.c_void_p), ("ready_event", C.c_void_p), ("device", C.c_int32)]


class Trace(C.Structure):
    _fields_ = [("h_enc", C.c_void_p), ("e_enc", C.c_void_p), ("h_steps", C.c_void_p), ("e_steps", C.c_void_p)]


PROFILE_MAX = 64
KERNEL_KINDS = ["plan", "plan_sort_unused", "enc_gemm", "enc_reduce", "enc_tail", "step", "step_last"]


class Profile(C.Structure):
    _fields_ = [("options", C.c_uint32), ("count", C.c_int32), ("kind", C.c_int32 * PROFILE_MAX), ("ms", C.c_float * PROFILE_MAX)]


class Dropout(C.Structure):
    """gnncca_dropout (include/gnncca_mpn.h): Dropout probabilities per MLP group + a DEVICE seed word."""
    _fields_ = [("p_enc", C.c_float), ("p_edge", C.c_float), ("p_node", C.c_float), ("p_cls", C.c_float), ("seed_dev", C.c_void_p)]


class InputGrads(C.Structure):
    """gnncca_input_grads (include/gnncca_mpn.h): where d loss / d x and d loss / d edge_attr go; a null member is not computed."""
    _fields_ = [("dx", C.c_void_p), ("d_edge_attr", C.c_void_p)]


OPT_EDGE_STATE_BF16 = 1
OPT_ENC_SPLIT3 = 2
OPT_ENC_UNSPLIT = 4
OPT_COLUMN_RANGES = 8
BWD_GRADS_ZEROED = 1
POST_ROUNDING, POST_PRUNING, POST_SPLITTING = 1, 2, 4        # gnncca_post_finalize_frame_host switches (config_inference.yaml:6-8)
POST_TRIGGER_ROUNDING, POST_TRIGGER_SPLITTING = 1, 2         # trigger bits of gnncca_post_prune_cluster_frames_ex
OPTIM_SGD, OPTIM_ADAM = 0, 1                                 # rules of gnncca_optim_set_hyper
OPTIM_BLOCK_HYPER_OFFSET, OPTIM_BLOCK_STEPS_OFFSET = 0, 80   # byte offsets inside an optimizer block (fp64 [8]; int32 [n_slots])


_SIGNATURES = {
    "gnncca_abi_version": (C.c_int, []),
    "gnncca_status_string": (C.c_char_p, [C.c_int]),
    "gnncca_last_hip_error": (C.c_int, []),
    "gnncca_param_count": (C.c_int, [C.POINTER(MpnDims)]),
    "gnncca_packed_weights_bytes": (C.c_size_t, [C.POINTER(MpnDims)]),
    "gnncca_pack_weights": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]),
    "gnncca_pack_program_bytes": (C.c_size_t, []),
    "gnncca_pack_program": (C.c_int, [C.POINTER(MpnDims), C.c_void_p, C.c_size_t]),
    "gnncca_pack_weights_device": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_size_t, C.c_void_p]),
    "gnncca_workspace_bytes": (C.c_size_t, [C.POINTER(MpnDims), C.c_int64, C.c_int64]),
    "gnncca_supported": (C.c_int, [C.POINTER(MpnDims)]),
    "gnncca_num_outputs": (C.c_int, [C.POINTER(MpnDims)]),
    "gnncca_mpn_forward": (C.c_int, [C.POINTER(MpnDims), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Trace), C.c_void_p]),
    "gnncca_mpn_forward_ex": (C.c_int, [C.POINTER(MpnDims), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Trace), C.c_uint32, C.c_void_p]),
    "gnncca_mpn_forward_profiled": (C.c_int, [C.POINTER(MpnDims), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.POINTER(Profile)]),
    "gnncca_normalize_columns": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_build_edges": (C.c_int, [C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_build_edges_backward_bytes": (C.c_size_t, [C.c_int64]),
    "gnncca_build_edges_backward": (C.c_int, [C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gnncca_build_edges_topk": (C.c_int, [C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_build_edges_radius": (C.c_int, [C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_build_edges_topk_sym_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "gnncca_build_edges_topk_sym_count": (C.c_int, [C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gnncca_build_edges_topk_sym_emit": (C.c_int, [C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_build_edges_topk_backward_bytes": (C.c_size_t, [C.c_int64]),
    "gnncca_build_edges_topk_backward": (C.c_int, [C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gnncca_normalize_columns_backward_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnncca_normalize_columns_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p,
                                                    C.c_void_p]),
    "gnncca_normalize_columns_backward2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                     C.c_void_p, C.c_int64, C.c_void_p]),
    "gnncca_post_threshold": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_post_threshold_at": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_post_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnncca_post_prune_cluster": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_post_prune_cluster_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
    "gnncca_post_prune_cluster_frames_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_post_exclusive_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_post_exclusive_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                               C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_size_t, C.c_void_p]),
    "gnncca_post_strong_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_post_finalize_frame_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_post_finalize_frames_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]),
    "gnncca_post_pool_create": (C.c_void_p, [C.c_int32]),
    "gnncca_post_pool_threads": (C.c_int32, [C.c_void_p]),
    "gnncca_post_pool_destroy": (None, [C.c_void_p]),
    "gnncca_post_pool_submit": (C.c_int64, [C.c_void_p, C.POINTER(PostBatch)]),
    "gnncca_post_pool_submit_copy": (C.c_int64, [C.c_void_p, C.POINTER(PostBatch), C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]),
    "gnncca_post_pool_wait": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gnncca_post_pool_wait_timed": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_backward_supported": (C.c_int, [C.POINTER(MpnDims)]),
    "gnncca_backward_workspace_bytes": (C.c_size_t, [C.POINTER(MpnDims), C.c_int64, C.c_int64]),
    "gnncca_mpn_backward": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_int64, C.POINTER(Trace), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_mpn_backward_ex": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int64, C.POINTER(Trace), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                         C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "gnncca_classifier_train": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_mpn_forward_train": (C.c_int, [C.POINTER(MpnDims), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Trace), C.POINTER(Dropout),
                                           C.c_void_p]),
    "gnncca_classifier_train_dropout": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Dropout), C.c_void_p]),
    "gnncca_mpn_backward_train": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_int64, C.POINTER(Trace), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                            C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(Dropout), C.c_void_p]),
    "gnncca_mpn_backward_inputs": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_int64, C.POINTER(Trace), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                             C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(Dropout), C.POINTER(InputGrads), C.c_void_p]),
    "gnncca_mlp_eval_workspace_bytes": (C.c_size_t, [C.POINTER(Mlp), C.c_int64]),
    "gnncca_mlp_eval": (C.c_int, [C.POINTER(Mlp), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "gnncca_gather_cat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "gnncca_aggregate_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnncca_aggregate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "gnncca_train_tape_bytes": (C.c_size_t, [C.POINTER(MpnDims), C.c_int64, C.c_int64]),
    "gnncca_train_tape_latents": (C.c_int, [C.POINTER(MpnDims), C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_int]),
    "gnncca_train_forward": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Dropout), C.c_void_p]),
    "gnncca_train_backward": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                        C.POINTER(Dropout), C.c_void_p]),
    "gnncca_train_backward_inputs": (C.c_int, [C.POINTER(MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                               C.POINTER(Dropout), C.POINTER(InputGrads), C.c_void_p]),
    "gnncca_normalize_columns2": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "gnncca_frames_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "gnncca_frames_forward_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_void_p]),
    "gnncca_frames_forward_radius": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32,
                                               C.c_double, C.c_int32, C.c_void_p]),
    "gnncca_plan_frames_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnncca_plan_frames": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_size_t]),
    "gnncca_plan_frames_ex": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]),
    "gnncca_plan_frames_radius": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_double, C.c_int32, C.c_void_p, C.c_size_t]),
    "gnncca_pad_frame": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "gnncca_read_graph_flags": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "gnncca_read_graph_flags2": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "gnncca_eval_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_eval_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_eval_frames_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_eval_sweep_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_eval_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_eval_sweep_exclusive_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_eval_sweep_exclusive": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p]),
    "gnncca_eval_sweep_joint_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_eval_sweep_joint": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
                                          C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_eval_sweep_strong_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnncca_eval_sweep_strong": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
                                           C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_eval_rows_accumulate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_rank_metrics_lds_bytes": (C.c_size_t, [C.c_int32]),
    "gnncca_rank_metrics": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.c_int64,
                                      C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gnncca_rank_rows_accumulate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_rank_pool_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "gnncca_frame_distances": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "gnncca_rerank_lds_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "gnncca_rerank_frames": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gnncca_rank_predictions": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gnncca_cluster_summaries_bytes":(C.c_size_t, [C.c_int64, C.c_int64]),
    "gnncca_cluster_summaries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_link_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "gnncca_link_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnncca_link_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_double, C.c_double, C.c_int32, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_link_gap_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnncca_link_gap_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_link_frames_gap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32,
                                         C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    "gnncca_link_frames_gap_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                            C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_link_motion_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnncca_link_motion_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_link_frames_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                            C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # the two entries above plus frame_time_dev and max_dt
    "gnncca_link_frames_gap_timed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                               C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double,
                                               C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_double]),
    "gnncca_link_frames_motion_timed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                                  C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p,
                                                  C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                  C.c_void_p, C.c_double]),
    "gnncca_link_kalman_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnncca_link_kalman_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    # the motion entry's head, then q, r, vel_var, has_max_nis, max_nis; its tail with the five filter outputs; frame_time_dev (or NULL), max_dt
    "gnncca_link_frames_kalman": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double,
                                            C.c_int32, C.c_double, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_double]),
    "gnncca_track_score_table_bytes": (C.c_size_t, [C.c_int64]),
    "gnncca_track_score_reset": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "gnncca_track_score_rehash": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "gnncca_track_score_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_reentry_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "gnncca_reentry_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnncca_reentry_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                        C.c_int32, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                        C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnncca_track_smooth_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "gnncca_track_smooth_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gnncca_track_smooth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32,
                                      C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_double]),
    "gnncca_edge_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "gnncca_edge_loss_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    "gnncca_edge_loss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "gnncca_optim_block_bytes": (C.c_size_t, [C.c_int32]),
    "gnncca_optim_set_hyper": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32,
                                         C.c_void_p]),
    "gnncca_optim_sgd_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p]),
    "gnncca_optim_adam_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int32), C.c_void_p]),
}

_lib = None


class NativeError(RuntimeError):
    """A libgnncca_mpn call returned a non-zero status (the int status of SURVEY.md 8b, as a RuntimeError)."""


def exported_symbols():
    return sorted(_SIGNATURES)


def lib():
    """Load libgnncca_mpn.so (once).  Raises if it has not been built: there is no other compute path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"{LIB_PATH} is missing: build it with `python gnn-cca_amd/build.py` "
                              "(the MI355X HIP path is the only implementation; there is no CPU fallback)")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        if handle.gnncca_abi_version() != ABI_VERSION:
            raise NativeError("libgnncca_mpn.so ABI version mismatch; rebuild")
        _lib = handle
    return _lib


def check(status, what):
    if status != OK:
        l = lib()
        msg = l.gnncca_status_string(status).decode()
        if status == ERR_HIP:
            msg += f" (hipError_t {l.gnncca_last_hip_error()})"
        if status == ERR_UNSUPPORTED:
            raise NotImplementedError(f"{what}: {msg}")
        raise NativeError(f"{what}: {msg}")
