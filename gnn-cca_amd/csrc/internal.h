// internal.h -- layouts and host functions shared by the library's translation units: the host packer (pack.cpp), the node encoder's
// route (enc_route.cpp), the message steps' route (step_route.cpp), the inference kernels (mpn_forward.hip), post-processing (mpn_post.hip), training (mpn_train.hip) and the smaller
// HIP units.  Plain C++, no HIP types.
// Not part of the public ABI (include/gnncca_mpn.h is).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "gnncca_mpn.h"

namespace gnncca {

extern thread_local int g_last_hip_error;  // hipError_t of the last failed HIP call on this thread (defined in pack.cpp, set by HIP_TRY: hip_try.h)

// Diagnostic switches (the A/B experiments of DESIGN.md 5; listed in DESIGN.md 11).  They change kernel SELECTION, hence
// summation order, so the shipped library ignores every one of them unless GNNCCA_DIAG=1 is set in the same environment:
// a stray variable in one rank's environment cannot silently change its numerics.
const char* diag_env(const char* name);
int diag_env_int(const char* name, int fallback, int lo, int hi);

constexpr uint32_t kBlobMagic = 0x4D504E36u;  // "MPN6": bumped with every change of the blob layout (a blob is only
                                              // valid for the library build that packed it; load_packed_blob checks)
constexpr int kH = 32;        // node latent width the MFMA step kernel is built for (node_out_dim)
constexpr int kEF = 6;        // edge latent width (edge_out_dim): 3 k-steps of v_mfma_f32_32x32x2_f32
constexpr int kProjOut = 48;  // per-node projection slots: [0,6) P_dst, [8,14) P_src+b_e, [16,48) Q+b_n
constexpr int kPdStride = 8;  // floats per node in the P_dst gather table (32 B rows)
constexpr int kPsQStride = 40;  // floats per node in the (P_src | Q) table: slots 8..47 of the projection
constexpr int kMaxCls = 8;    // widest hidden layer of the edge classifier handled in registers
constexpr int kMaxEdgeIn = 16;

// Families of GRAPH_NET_PARAMS this build has kernels for.
enum Family : uint32_t {
    kFamilyNone = 0,
    kFamilyMfma32x6 = 1,  // H = 32, EF = 6, single-layer edge/node MLPs (both shipped configs)
    kFamilyGeneric = 2,   // any other legal GRAPH_NET_PARAMS: op-for-op kernels, correctness first
};

// Header of the packed weight blob.  All offsets are in floats from the start of the blob and are
// multiples of 4 (16-byte aligned).  BatchNorm (eval) is already folded into weight and bias.
struct BlobHeader {
    uint32_t magic, abi_version, family, total_floats;
    int32_t enc_node_layers;
    int32_t enc_node_w[GNNCCA_MAX_LAYERS];  // [out][in] row-major
    int32_t enc_node_b[GNNCCA_MAX_LAYERS];  // [out]
    int32_t enc_last_wT;                    // last encoder layer transposed: [in][32]
    int32_t enc_edge_w, enc_edge_b;         // [6][edge_in], [6]
    int32_t wee;                            // [6][ef*6]   edge-feature block of the edge MLP
    int32_t wne_b;                          // [3][64]     MFMA B operand: Wne[lane&31][2s + (lane>>5)]
    int32_t proj_wT;                        // [nf*32][48] per-node projection, transposed
    int32_t proj_b;                         // [48]        biases b_e (slots 8..13) and b_n (16..47)
    int32_t cls_layers, cls_hidden;         // 1: Linear(6,1);  2: Linear(6,C1)+ReLU, Linear(C1,1)
    int32_t cls_w1, cls_b1, cls_w2, cls_b2;
    int32_t fast_consts;                    // [kFastConsts] contiguous copy of the per-step scalars (see below), or 0
    int32_t enc_w3;                         // first encoder weight as 3 bf16 pieces, [in/32][3][out][32], or 0
    int32_t wne_bf16;                       // [9][64] dwords: W_ne as packed bf16 piece pairs, the B operands of msg_bf16.cuh
    int32_t enc_w2h;                        // first encoder weight as 2 fp16 pieces (w = w0 + w1 / 2048), the B-operand image of enc_f16.cuh:
                                            // [in/32][2 pieces][4 column tiles][2 k-steps][64 lanes][8] halfs (pack_elem.h: w2h_index); or 0
    int32_t enc_w2h_bad;                    // [kW2hBadWords] words: non-zero where a weight does not fit fp16 (|w| >= 65520): the fp16 GEMM then
                                            // hands every tile to its bf16 arm
    int32_t pad[3];
};
constexpr int kW2hBadWords = 64;            // one per pack block (pack_device_kernel's grid is 64 wide): no atomics, nothing to reset
constexpr float kF16Limit = 65520.0f;       // the smallest magnitude that fp16 round-to-nearest-even turns into infinity
constexpr float kF16Tiny = 0.0009765625f;   // 2^-10.  The fp16 pieces carry 2^-36 ABSOLUTE precision below fp16's normal range (6.1e-5): per dot product
                                            // sqrt(K) |w| 2^-36 ~ 1e-11 -- far below an fp32 ulp of the biased sum it feeds, but as RELATIVE error of
                                            // the product alone sqrt(K) 2^-36 / |x| (2.5e-6 at a largest |x| of 2^-10, 1e-5 at 1e-6).  A tile whose
                                            // LARGEST |x| is under this (and not zero) therefore takes the range arm like a tile beyond 65520 does
                                            // (ADVICE r5).  Column-normalised embeddings sit at 1 / sqrt(N): a million-node batch still has tile
                                            // maxima of 3.7e-3, so no ordinary input pays for the guard.

// Layout of the `fast_consts` block (floats): the per-step scalars mpn_step_fast_kernel reads into SGPRs.
// Present when edge_in == 4, no reattach flags and the classifier is Linear(6,4)+ReLU+Linear(4,1).
// The three matrices are stored TRANSPOSED ([in][out]) so that the weights of two adjacent outputs are one aligned
// SGPR pair, the operand form of v_pk_fma_f32.
constexpr int kFcEncW = 0;     // [4][6]  enc_edge_w^T
constexpr int kFcEncB = 24;    // [6]
constexpr int kFcWee = 32;     // [6][6]  wee^T
constexpr int kFcCw1 = 68;     // [6][4]  cls_w1^T
constexpr int kFcCb1 = 92;     // [4]
constexpr int kFcCw2 = 96;     // [4]
constexpr int kFcCb2 = 100;    // [1]
constexpr int kFcProjB = 104;  // [48]
constexpr int kFastConsts = 152;
bool fast_consts_ok(const gnncca_mpn_dims* d);

// The fast family's blob as a program: a list of strided copies out of the parameter tensors, built per GRAPH_NET_PARAMS by
// pack_program() (pack.cpp) and interpreted by gnncca_pack_weights on the host and by pack_device_kernel on the GPU
// (gnncca_pack_weights_device: the parameters never visit the host).  Both go through pack_elem.h, which has the fold, the piece
// splits and the layouts of the kinds; this is the one description of the kinds themselves.
struct PackSeg {
    int32_t kind;               // 0: weight element, 1: bias element (both: blob[dst + r * drs + c * dcs]),
                                // 2: weight element split into 3 bf16 planes, [in/32][3][out][32] (BlobHeader::enc_w3),
                                // 3: W_ne element (row = channel, column = k < 6) as bf16 pieces in the MsgB lane layout (wne_bf16),
                                // 4: weight element split into 2 fp16 pieces in the swizzled chunk image of BlobHeader::enc_w2h
                                //    (dst = enc_w2h, plane = float offset of the kW2hBadWords flag words)
                                // kinds 2 - 4 address by (r, c) alone: drs and dcs are unused and 0
    int32_t dst;                // float offset in the blob (kind 2: offset of plane 0)
    int32_t param;              // index of the Linear's weight (kind 0, 2, 3, 4) or bias (kind 1) in the parameter list
    int32_t bn;                 // index of the BatchNorm weight (gamma; beta, mean, var follow), or -1
    int32_t src_off;            // element offset inside the parameter
    int32_t rows, cols;         // rows = output units (the BatchNorm channel of element (r, c) is unit0 + r)
    int32_t unit0;
    int32_t drs, dcs, srs, scs; // destination / source strides per row and per column
    int32_t plane;              // kind 2: out * 32, the piece stride inside a 32-deep k-chunk of [in/32][3][out][32]; kind 4: see above
    int32_t pad[3];
};
constexpr int kMaxPackSegs = 96;
struct PackProgram {
    BlobHeader header;
    int32_t n_segs;
    int32_t pad[3];
    PackSeg segs[kMaxPackSegs];
};
bool pack_program(const gnncca_mpn_dims* d, PackProgram* out);
bool enc_split_ok(const gnncca_mpn_dims* d);  // first encoder layer eligible for the split-bf16 MFMA GEMM

// Blob of the generic family: every layer of every MLP as W[out][in] + b[out], BatchNorm folded.
// MLP index: 0 encoder.node, 1 encoder.edge, 2 MPNet.edge_model, 3 MPNet.node_model, 4 classifier.edge
struct GenBlobHeader {
    uint32_t magic, abi_version, family, total_floats;
    int32_t w[5][GNNCCA_MAX_LAYERS];   // transposed, padded: [in][ceil8(out)]
    int32_t b[5][GNNCCA_MAX_LAYERS];   // [ceil8(out)]
    int32_t enc0_rowmajor;             // first node-encoder weight also as [out][in] (input of the MFMA GEMM), or 0
    int32_t step_w, step_w_floats;     // the fused step's per-edge weights in the order and shape it stages them in LDS (generic_fused.cuh), or 0
    int32_t pad[1];
};
int gen_enc0_ksplit(const gnncca_mpn_dims* d, int64_t n_nodes);  // split-K factor of that GEMM (0: not used)
bool gen_blob_header(const gnncca_mpn_dims* d, GenBlobHeader* out);
const gnncca_mlp& mlp_by_index(const gnncca_mpn_dims* d, int i);

struct GenWorkspace {
    size_t flags, blockflags, seg_ptr, col32, perm, cursor, row32o, col32o;
    size_t node[3], h0, edge[4], e0, partial, tab[2], total;   // tab: per-node projection tables of the fused step (generic_fused.cuh)
    int64_t node_w, edge_w;  // floats per row of the node / edge scratch buffers
};
GenWorkspace carve_generic(const gnncca_mpn_dims* d, int64_t n, int64_t e);

// The staging image of a batch of frames: what gnncca_plan_frames writes on the host, gnn_cca_amd.frames uploads in ONE transfer and
// gnncca_frames_io::staged_dev hands to the one-call pipeline.  Eleven arrays back to back, 8-byte fields first (n detections, g frames):
//   f64 xw[n], yw[n], max_dist[g];  i64 ids[n];  i32 person[n], cam[n], graph_of[n], graph_ptr[g + 1], src_order[n], edge_ptr[n + 1],
//   edge_ptr_g[g + 1]
// The order is ABI (include/gnncca_mpn.h describes it); it is written down here and in gnn_cca_amd/frames.py (FrameLayout), nowhere else.
struct StagingImage {
    double *xw, *yw, *max_dist;
    int64_t* ids;
    int32_t *person, *cam, *graph_of, *graph_ptr, *src_order, *edge_ptr, *edge_ptr_g;
    size_t bytes;
    gnncca_frames frames() const { return gnncca_frames{xw, yw, max_dist, person, cam, graph_of, graph_ptr, src_order, edge_ptr}; }
};
inline StagingImage staging_image(const void* base, int64_t n, int64_t g) {
    uintptr_t at = reinterpret_cast<uintptr_t>(base);
    auto take = [&at](auto*& field, int64_t count) { field = reinterpret_cast<decltype(+field)>(at), at += sizeof(*field) * (size_t)count; };
    StagingImage s;
    take(s.xw, n), take(s.yw, n), take(s.max_dist, g), take(s.ids, n), take(s.person, n), take(s.cam, n), take(s.graph_of, n);
    take(s.graph_ptr, g + 1), take(s.src_order, n), take(s.edge_ptr, n + 1), take(s.edge_ptr_g, g + 1);
    s.bytes = at - reinterpret_cast<uintptr_t>(base);
    return s;
}
inline size_t staging_image_bytes(int64_t n, int64_t g) { return n < 0 || g < 0 ? 0 : staging_image(nullptr, n, g).bytes; }

// Which of a source's cross-camera candidates a graph build keeps: all of them, the top_k with the smallest key (graph_topk.cuh), or those
// within a ground-plane radius (graph_radius.cuh).  The fields of the other kinds are not looked at.
struct EdgeSelect {
    enum Kind { kDense, kCapped, kGated } kind;
    int32_t top_k, rank_by, max_deg;   // kCapped: gnncca_build_edges_topk's arguments
    double radius;                     // kGated: gnncca_build_edges_radius' arguments
    int32_t unit;
    static EdgeSelect dense() { return EdgeSelect{kDense, 0, 0, 0, 0.0, 0}; }
    static EdgeSelect capped(int32_t top_k, int32_t rank_by, int32_t max_deg) { return EdgeSelect{kCapped, top_k, rank_by, max_deg, 0.0, 0}; }
    static EdgeSelect gated(double radius, int32_t unit) { return EdgeSelect{kGated, 0, 0, 0, radius, unit}; }
};
// what the public entry points refuse of a selection's own arguments: GNNCCA_OK, GNNCCA_ERR_INVALID_ARG or GNNCCA_ERR_UNSUPPORTED (graph_build.hip)
int edge_select_refusal(const EdgeSelect& sel);

// gnncca_build_edges / _topk / _radius, by `sel`, that also zero `zero_n` int32 words at `zero_ptr` (graph_build.hip; gnncca_frames_forward*
// hand them the post stage's counters); zero_ptr == nullptr: the public entry points, bit for bit
int build_edges_zeroing(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges, int32_t mode,
                        const EdgeSelect& sel, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out, int32_t* zero_ptr,
                        int64_t zero_n, gnncca_stream_t stream);

Family classify(const gnncca_mpn_dims* d);
bool blob_header(const gnncca_mpn_dims* d, BlobHeader* out);  // false if unsupported
bool dims_valid(const gnncca_mpn_dims* d);
// The canonical parameter order (what gnncca_pack_weights, the training entry points and MOTMPNet.native_param_tensors agree on): MLP by
// MLP (mlp_by_index), layer by layer: weight, bias, then -- where has_bn -- BatchNorm weight, bias, running_mean, running_var.
struct ParamSlots {
    int w, b;   // the Linear's weight and bias
    int bn;     // the BatchNorm's gamma (beta, running mean, running var follow), or -1
};
ParamSlots mlp_param_slots(const gnncca_mlp& m, int layer);                        // counted from the MLP's own first tensor
ParamSlots param_slots(const gnncca_mpn_dims* d, int mlp_index, int layer);        // in the whole list
int mlp_param_count(const gnncca_mlp& m);
// Split-K factor of the f32 plan GEMM (enc_gemm_plan_kernel: 32-row tiles, slices at least 64 deep): enough workgroups to cover the
// chip when there are few rows.  The forward's workspace, the generic family's first layer and the backward's a1 recompute use it.
int plan_gemm_ksplit(int64_t n_rows, int K);

// Workspace carve-up (byte offsets, all multiples of 256).
struct Workspace {
    size_t flags, blockflags, seg_ptr, col32, perm, cursor, h0, act, partial, pd[2], psq[2], e, e0, rng, total;
    int ksplit;        // split-K factor of the first encoder GEMM
    int64_t e_stride;  // floats between two feature planes of the edge state
    int ell_S;         // padded edge-state layout: slots per node (multiple of 32), 0 = compact CSR order only
};
// Padded edge-state stride for big, nearly regular batches: a pure function of (dims, N, E) -- the host never reads the
// graph back; the plan kernel validates the degrees against it on the device (GNNCCA_GRAPH_IRREGULAR).
int ell_stride(const gnncca_mpn_dims* d, int64_t n, int64_t e);
// Split-K factor of the 256-row split-bf16 encoder GEMM (N >= 16 384): 1 = un-split with the fused epilogue, else 2 / 4 / 8
// partial slabs for the tail kernel.  One workgroup per CU (144 KB of LDS), so the cost is counted in ROUNDS of 256 workgroups.
int enc_lds_ksplit(int64_t n_nodes, int K);
Workspace carve(const gnncca_mpn_dims* d, int64_t n, int64_t e);

// ---- the node encoder's route (enc_route.cpp) ------------------------------------------------------------------------------------
// Which GEMM form every encoder layer but the last runs on, where the graph plan goes and which tail sums the slabs: decided ONCE
// per forward by encoder_route(), a pure host function, and carried out by launch_node_encoder (mpn_forward.hip), which compares no
// sizes.  tests/test_encoder_route.py pins the table; DESIGN.md 4.1 has it.
enum EncForm : int {
    kEncPlanGemm = 0,  // enc_gemm_plan_kernel: f32 MFMA GEMM, `slabs` k-slices of `kslice`; the plan rides on layer 0
    kEncSlices,        // enc_gemm_f16_slices{8,4,2}_kernel: fp16-split, 32-row tiles x `slabs` slices `kslice` deep; the plan rides
    kEncD128,          // enc_gemm_split_direct_kernel: split-bf16, 128-row workgroups x `slabs`; the plan rides
    kEncR32Bf16,       // enc_gemm_rows32_fused_kernel<SPLIT3, nst>: 32-row workgroups, un-split, fused epilogue
    kEncR32F16,        // enc_gemm_f16_rows32_kernel: the same on the fp16-split arithmetic
    kEncLdsBf16,       // enc_gemm_split_lds_kernel<fused, SPLIT3>: 256-row workgroups; fused epilogue or `slabs` k-slices
    kEncLdsF16,        // enc_gemm_f16_fused_kernel / enc_gemm_f16_split_kernel: the same on the fp16-split arithmetic
};
enum EncPlanPlace : int {
    kPlanNone = 0,     // E == 0: no plan
    kPlanRides,        // extra workgroups of the first GEMM launch
    kPlanBefore,       // plan_only launch in front of a fused GEMM, whose last workgroup finishes the plan
    kPlanAfter,        // plan_only launch behind the GEMM (256-row forms that are not fused); the tail finishes it
};
enum EncTail : int {
    kTailNone = 0,     // the GEMM's fused epilogue wrote h0 and the step-1 projections
    kTailFast,         // enc_tail_fast_kernel, `tail_npw` nodes per workgroup
    kTailMfma,         // enc_tail_mfma_kernel, 32 nodes per workgroup
    kTailLds,          // enc_tail_kernel with `tail_lds` bytes of dynamic LDS
    kTailRefused,      // that kernel would need more than 160 KB: GNNCCA_ERR_UNSUPPORTED where the tail would have been launched
};
constexpr int kEncSliceMaxK = 256;   // deepest k-slice of kEncSlices: a workgroup's x tile is 32 rows x 256 floats = 32 KB of LDS
// The measured thresholds of the route and the diagnostics that force an arm: the member initialisers are the defaults (the one place
// they are written), enc_tuning() is the defaults overridden by the GNNCCA_* switches of DESIGN.md 11, read once per process.
struct EncTuning {
    int split_min = 384;                       // GNNCCA_GEMM_SPLIT_MIN: first node count of the split-bf16 forms
    int lds_min = 6144;                        // GNNCCA_GEMM_LDS_MIN:   first node count of the 256-row forms
    int r32f_min = 4096, r32f_max = 8192;      // GNNCCA_GEMM_R32F_MIN / _MAX: node range of kEncR32F16
    int slices_min = 1, slices_max = 4095;     // GNNCCA_GEMM_SLICES_MIN / _MAX: node range of kEncSlices
    int slices_nks = 16, slices_wgs = 256;     // GNNCCA_GEMM_SLICES_NKS / _WGS: cap of the slice count; workgroups one round may hold
    int tail_mfma_min = 2560;                  // GNNCCA_TAIL_MFMA_MIN:  first node count of kTailMfma
    bool gemm_bf16 = false;                    // GNNCCA_GEMM_BF16:      the bf16 forms as the A/B reference of the fp16-split GEMMs
    int f16_force_arm = 0;                     // GNNCCA_GEMM_F16_ARM:   every tile / wave of the fp16-split GEMMs on its fallback arm (tests)
    int f16_x_nt = -1;                         // GNNCCA_GEMM_F16_XNT:   0 / 1 forces the non-temporal x stream off / on
};
const EncTuning& enc_tuning();
struct EncRouteIn {
    const gnncca_mpn_dims* d;
    const BlobHeader* hdr;
    const Workspace* ws;
    int N, E;
    uint32_t options;
    bool dropping;                    // train-mode Dropout active
    bool trace_h;                     // the caller asked for the encoder output (gnncca_trace::h_enc)
    bool x_aligned, ws_aligned;       // 16-byte alignment of x and of the workspace base
    int plan_blocks, plan_span;       // plan.cuh: plan_num_blocks(E), plan_span(edge_index, E)
};
struct EncGemmRoute {
    int form, K, O;
    int slabs;     // k-slices the launch writes = slabs the following reduce / tail sums (<= Workspace::ksplit)
    int kslice;    // depth of one slice
    int nst;       // kEncR32Bf16: pipeline stages, 8 or 4
    int vec_ok;    // kEncPlanGemm: rows allow 16-byte loads
};
struct EncRoute {
    int n_gemm;
    EncGemmRoute gemm[GNNCCA_MAX_LAYERS];
    bool split3, fused;               // three of the six bf16 products; layer 0's epilogue finishes the encoder (tail == kTailNone)
    int x_nt, force_arm;              // fp16-split forms: non-temporal x stream; EncTuning::f16_force_arm
    int plan_place, plan_span, plan_wgs;   // plan_wgs: workgroups the plan adds to the GEMM launch / its own launch has
    int tail, tail_npw, tail_vec;     // tail_vec: TailParams::vec_reduce
    size_t tail_lds;
};
EncRoute encoder_route(const EncRouteIn& in, const EncTuning& t);

// ---- the message steps' route (step_route.cpp) -----------------------------------------------------------------------------------
// Which instantiation of which step kernel every step launches, on what grid and into which logit slots: step_plan() decides once per
// forward what does not change from step to step, step_launch() names one step's kernel; both are pure host functions.
// launch_step_variant (mpn_forward.hip) carries a StepLaunch out and compares no sizes.  tests/test_step_route.py pins the table;
// DESIGN.md 4.2 has it.
enum StepFamily : int {
    kStepGeneral = 0,  // mpn_step_kernel<RE, MSG, MX> (step_general.cuh): any dims of the family, traces, dropout, 'max'
    kStepFast,         // mpn_step_fast_kernel<FIRST, CLS, MSG, PDL, EB, NT> (step_fast.cuh): the shipped shape, f32 message
    kStepPipe,         // mpn_step_pipe_kernel<FIRST, CLS, MSG, PDL, EB, NT, RNG, NPW, CIN> (step_pipe.cuh): the same, bf16-split message
};
#ifndef GNNCCA_NPW2_CLS
#define GNNCCA_NPW2_CLS 0         // 1: instantiate the two-nodes-per-wave form for the classifying steps as well (diagnostic builds)
#endif
// THE statement of which instantiations the library has: step_launch() never names another one, launch_step_variant instantiates
// these and no others (if constexpr).  The kernels' static_asserts are the wider, necessary conditions.
constexpr bool step_variant_exists(int family, bool FIRST, bool CLS, bool MSG, bool PDL, bool EB, int NT, bool RNG, int NPW, bool CIN) {
    if (family == kStepGeneral) return true;                    // every <RE, MSG, MX>; the other arguments are not its own
    if (NT < 0 || NT > 2 || (NT != 0 && PDL)) return false;     // non-temporal streams only without the LDS-resident gather table
    if (family == kStepFast) return !RNG && NPW == 1 && !CIN;   // no range, two-node or deferred forms
    // the nine forms that classify their input state: a message step (one or two nodes per wave), or the last step classifying both
    if (CIN) return !FIRST && !PDL && !EB && !RNG && (MSG ? !CLS && (NPW == 1 || NPW == 2) : CLS && NPW == 1);
    // column ranges: default cache policy, one node per wave (also compiled for FIRST && !MSG, where they would do nothing and the
    // route never takes them: step_launch)
    if (RNG) return NT == 0 && NPW == 1;
    // two nodes per wave: message steps without the table; the classifying ones need 143-155 VGPRs (step_pipe.cuh) and are a build option
    if (NPW == 2) return MSG && !PDL && (!CLS || GNNCCA_NPW2_CLS);
    return NPW == 1;
}
// mpn_step_pipe_kernel's eligibility: every buffer it addresses with 32-bit offsets stays below 2^31 bytes
inline bool step_pipe_fits(long long N, long long E, long long e_stride, unsigned long long ws_bytes) {
    const long long lim = 1ll << 31;
    // (the whole workspace is addressed through one descriptor: it must end below the out-of-range offset 2^31 of a dead lane, and
    // below 2^31 - 4 so that "the slot before slot 0" of DERIVE's predecessor load is out of range too)
    return 6 * e_stride * 4 <= lim && E * 16 <= lim && N * 32 <= lim && ws_bytes <= (unsigned long long)lim - 4096;
}
// The measured thresholds of the step route and the diagnostics that force a choice: the member initialisers are the defaults (the one
// place they are written), step_tuning() is the defaults overridden by the GNNCCA_* switches of DESIGN.md 11, read once per process.
// step_route.cpp has the measurements beside the rules.
struct StepTuning {
    int msg_f32_max_n = 512;                         // last node count of the f32 message (kStepFast)
    int fill_waves = 4096, fill_waves_long = 16384;  // waves that fill the chip; the same for graphs whose nodes average >= long_chunks chunks
    int long_chunks = 32;
    int npw_min_n = 16384;                           // GNNCCA_NPW_MIN_N:       first node count of two nodes per wave (steps 2 ... L)
    int npw_min_n_first = 16384;                     // GNNCCA_NPW_MIN_N_FIRST: the same for step 1
    int pd_lds_min = 0x7FFFFFFF, pd_lds_max = 1024;  // GNNCCA_PD_LDS_MIN / _MAX: node range that stages the P_dst table in LDS (default: none)
    double nt_store_bytes = 150e6;                   // edge state beyond which its stores (and the edge_attr loads) are non-temporal
    double nt_load_bytes = 256e6;                    // ... and its loads as well
    int force_wps = 0;                               // GNNCCA_WPS:     1 / 2 / 4 waves per node (capped by the chunk count)
    int force_npw = 0;                               // GNNCCA_NPW:     1 / 2 = two nodes per wave never / whenever eligible
    int force_nt = -1;                               // GNNCCA_STEP_NT: 0 / 1 / 2 = default policy / nt stores / nt loads too
};
const StepTuning& step_tuning();
struct StepRouteIn {
    const gnncca_mpn_dims* d;
    const BlobHeader* hdr;
    const Workspace* ws;
    int N, E;
    uint32_t options;
    bool dropping;                    // train-mode Dropout active
    bool traced, trace_h_steps;       // a gnncca_trace was passed; it asks for the node states of every step (so the last step sends messages)
    bool attr_aligned;                // 16-byte alignment of edge_attr
};
struct StepPlan {                     // what does not change from step to step
    int launches;                     // 0: no edges, the forward ends behind the encoder; 1 for L == 0 (classify only); else L
    int family;                       // StepFamily (kStepGeneral for L == 0)
    bool RE, MX;                      // kStepGeneral: reattach_edges, 'max' aggregation
    int N, hin;
    int msg_f32, attr_vec, wps, npw_first, npw_later, pd_lds, e_bf16;
    int nt;                           // 0 / 1 / 2: the policy (StepParams::nt_store, nt_load); the template argument where a variant has it
    bool ranges;                      // StepParams::rng is set
    int ell_S;                        // padded edge-state layout as USED (0: compact)
    bool defer;                       // deferred classification (step_pipe.cuh: CIN)
    bool trace_h_steps;
    int first_cls, L, cls_layers;
};
struct StepLaunch {
    // the instantiation: kStepGeneral <RE, MSG, MX>, kStepFast <FIRST ... NT>, kStepPipe all nine
    int family;
    bool RE, MX, FIRST, CLS, MSG, PDL, EB;
    int NT;
    bool RNG;
    int NPW;
    bool CIN;
    unsigned blocks;                  // workgroups of 256 threads
    size_t lds;                       // dynamic LDS bytes
    // the per-step scalars of StepParams (npw: the forward's choice for this step, whatever NPW the variant has)
    int first, update, store_e, npw, cls_layers, cls_no, stamp_slot;
    int slot_out, slot_in;            // logit slot this step writes / classifies from its input state; -1: none
    int buf_in, buf_out;              // index of the pd / psq table read / written; -1: none
};
StepPlan step_plan(const StepRouteIn& in, const StepTuning& t);
StepLaunch step_launch(const StepPlan& p, int step);   // step 1 ... L; 0: the L == 0 launch

// Workspace of the fused backward (gnncca_mpn_backward*, mpn_train.hip): byte offsets, all multiples of 256.  `d` must have passed
// backward_ok (a two-layer node encoder); F1 is its first layer's width.
struct BwdWorkspace {
    size_t gh0_acc, ge0_acc;   // reattach_initial_nodes / _edges: d loss / d h0, d loss / d e0 via the copies
    size_t deg, Q;
    size_t hmax;               // 'max' aggregation only: [N][32] maxima, then [N][32] tie counts
    size_t dP_all;             // one [N][44] table per step, cleared once
    size_t Hb[2], Gb[2], a1, gz1;
    size_t part;               // split-K partials of the a1 recompute: 32 slabs [N][F1]
    size_t bn_sums, bn_red;    // BatchNorm backward scratch: 2 x 64 doubles, 2 x 64 floats
    size_t total;
};
inline BwdWorkspace carve_backward(const gnncca_mpn_dims* d, int64_t n, int64_t e) {
    BwdWorkspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t N = (size_t)(n > 0 ? n : 0), E = (size_t)(e > 0 ? e : 0), F1 = (size_t)d->enc_node.layers[0].out_dim;
    const size_t L = (size_t)(d->num_enc_steps > 1 ? d->num_enc_steps : 1);
    w.gh0_acc = take(N * kH * 4), w.ge0_acc = take(E * kEF * 4), w.deg = take(N * 4), w.Q = take(N * kH * 4);
    w.hmax = take(2 * N * kH * 4), w.dP_all = take(L * N * 44 * 4);
    for (int i = 0; i < 2; ++i) w.Hb[i] = take(N * kH * 4);
    for (int i = 0; i < 2; ++i) w.Gb[i] = take(E * kEF * 4);
    w.a1 = take(N * F1 * 4), w.gz1 = take(N * F1 * 4), w.part = take(32 * N * F1 * 4);
    w.bn_sums = take(sizeof(double) * 2 * 64), w.bn_red = take(sizeof(float) * 2 * 64), w.total = off;
    return w;
}

// Workspace of the pruning / clustering stage (gnncca_post_prune_cluster*, mpn_post.hip): a graph plan of its own.
struct PostWorkspace { size_t flags, blockflags, seg_ptr, col32, perm, cursor, total; };
inline PostWorkspace carve_post(int64_t n, int64_t e) {
    PostWorkspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t N = (size_t)(n > 0 ? n : 0), E = (size_t)(e > 0 ? e : 0);
    w.flags = take(256), w.blockflags = take((E / 256 + 2) * 4), w.seg_ptr = take((N + 1) * 4), w.col32 = take(E * 4);
    w.perm = take(E * 4), w.cursor = take((N + 1) * 4), w.total = off;
    return w;
}
// The plan's six arrays inside a workspace that starts with a PostWorkspace (the post stage's, the sweeps', the exclusive clusters').
struct PostPlanPtrs {
    unsigned* flags;
    unsigned* blockflags;
    int* seg_ptr;
    int* col32;
    int* perm;
    int* cursor;
};
inline PostPlanPtrs post_plan_ptrs(void* workspace, const PostWorkspace& w) {
    char* base = static_cast<char*>(workspace);
    return PostPlanPtrs{reinterpret_cast<unsigned*>(base + w.flags), reinterpret_cast<unsigned*>(base + w.blockflags),
                        reinterpret_cast<int*>(base + w.seg_ptr),    reinterpret_cast<int*>(base + w.col32),
                        reinterpret_cast<int*>(base + w.perm),       reinterpret_cast<int*>(base + w.cursor)};
}
// Builds the plan of edge_index into those arrays: plan_only + plan finish, no padded layout to validate (mpn_post.hip defines it; the
// status is HIP_TRY's).  A graph without edges launches nothing (kSkip: the sweeps, the exclusive clusters), or the finish alone, which
// leaves a finished plan -- flag word and segment offsets -- in the workspace all the same (kFinish: gnncca_post_prune_cluster*).
enum class EmptyPlan { kSkip, kFinish };
int launch_post_plan(const long long* ei, int E, int N, const PostPlanPtrs& p, EmptyPlan when_empty, gnncca_stream_t stream);

// The frame-local kernels (one workgroup per frame, the frame in LDS): their LDS capacity in nodes is the batch's largest frame rounded
// up to a power of two, and their block is one wave while that capacity fits one (a Terrace frame has ~20 detections), 256 threads
// otherwise -- their threads stride over a frame's nodes.  launch(std::integral_constant<int, BLOCK>) makes the launch.
inline int frame_capacity(int32_t max_frame_nodes) {
    int P = 1;
    while (P < max_frame_nodes) P <<= 1;
    return P;
}
// strong_cluster_kernel's capacity is the largest frame rounded up to 32 instead: its LDS holds a bit matrix of P rows of P / 32 words,
// which a power of two would up to quadruple, and its label phase gives every node a thread of its own, hence the third rung
// (MAX_BLOCK = 1024) for frames of more than 256 nodes.
inline int strong_capacity(int32_t max_frame_nodes) { return (max_frame_nodes + 31) / 32 * 32; }
template <int MAX_BLOCK = 256, class Launch>
inline void launch_frame_block(int P, Launch&& launch) {
    if (P <= 64) launch(std::integral_constant<int, 64>{});
    else if (MAX_BLOCK <= 256 || P <= 256) launch(std::integral_constant<int, 256>{});
    else launch(std::integral_constant<int, MAX_BLOCK>{});
}

// ---- kernels of mpn_forward.hip that mpn_post.hip and mpn_train.hip launch too ---------------------------------------------------
// Every __global__ kernel is compiled in exactly one translation unit; where another unit needs one, it calls a host launcher defined
// beside the kernel (encoder.cuh, generic.cuh).  A launcher only launches -- same grid, block and LDS as a launch written in place -- and
// the caller checks hipGetLastError() as it does after launches of its own.
struct EncPlanParams {   // encoder.cuh: enc_gemm_plan_kernel, plan_only_kernel and the GEMMs the graph plan rides in
    const float* in;
    const float* W;
    float* part;
    const long long* ei;
    int* seg_ptr;
    int* col32;
    unsigned* blockflags;
    int M, K, O, kslice, vec_ok, nrt, nks, gemm_blocks, E, N;
    int ell_S;  // slots per node of the padded step layout to validate the degrees against (0: none)
    int plan_span;  // 1024-edge plan blocks per plan workgroup (plan.cuh: 1, or kPlanSpan on a plan-only launch of a big batch)
};
struct GenSeg {          // generic.cuh: one segment of a virtual concatenation
    const float* ptr;   // [rows][ld]
    const int* idx;     // optional row gather (row32 / col32 in the caller's edge order), or null
    int ld, width;
};
void launch_plan_only(const EncPlanParams& p, int blocks, gnncca_stream_t stream);
void launch_enc_gemm_plan(const EncPlanParams& p, int blocks, gnncca_stream_t stream);
void launch_reduce_bias_act(const float* part, const float* bias, float* act, int M, int O, int ks, int relu, gnncca_stream_t stream);
void launch_gen_plan_finish(const long long* ei, int E, int N, int* seg_ptr, int* col32, int* perm, int* cursor, unsigned* flags,
                            const unsigned* blockflags, gnncca_stream_t stream);
void launch_gen_index32(const long long* ei, int E, int N, int* row32, int* col32, gnncca_stream_t stream);
// one column group of a dense layer: `O` <= 2048 outputs of a layer whose padded weight rows are `ldw` floats apart
void launch_gen_dense(const GenSeg& s0, const GenSeg& s1, const GenSeg& s2, const float* Wt, const float* b, float* out, long long M, int K,
                      int O, int ldw, int ld_out, int relu, gnncca_stream_t stream);
void launch_gen_aggregate(const float* m, const int* seg_ptr, const int* perm, const unsigned* flags, float* h, int N, int H, int agg,
                          gnncca_stream_t stream);
void launch_gen_poison(float* out, long long n, const unsigned* flags, gnncca_stream_t stream);

}  // namespace gnncca
