// pack.cpp -- host side of libgnncca_mpn: dims validation, weight packing, workspace carve-up.
// Pure C++ (no HIP calls): testable on a machine without a GPU.
//
// What the packing does: the fast family's blob is stated ONCE, as the program of pack_program() below (which regions there are and how
// the edge / node MLP weights split by cat order), and gnncca_pack_weights interprets that program; what happens to one element -- the
// BatchNorm fold, the bf16 / fp16 piece splits, the operand layouts -- is in pack_elem.h, shared with the device packer.  The generic
// family has no program: pack_generic walks its layers itself, through the same fold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "internal.h"
#include "pack_elem.h"

namespace gnncca {

thread_local int g_last_hip_error = 0;  // the one definition (internal.h); every HIP translation unit sets it through HIP_TRY

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// THE walk of the canonical parameter order: weight, bias, then gamma, beta, running mean, running var where has_bn, layer by layer
ParamSlots mlp_param_slots(const gnncca_mlp& m, int layer) {
    int i = 0;
    for (int l = 0; l < layer; ++l) i += m.layers[l].has_bn ? 6 : 2;
    return ParamSlots{i, i + 1, layer < m.n_layers && m.layers[layer].has_bn ? i + 2 : -1};
}

int mlp_param_count(const gnncca_mlp& m) { return mlp_param_slots(m, m.n_layers).w; }

ParamSlots param_slots(const gnncca_mpn_dims* d, int mlp_index, int layer) {
    int base = 0;
    for (int m = 0; m < mlp_index; ++m) base += mlp_param_count(mlp_by_index(d, m));
    const ParamSlots s = mlp_param_slots(mlp_by_index(d, mlp_index), layer);
    return ParamSlots{base + s.w, base + s.b, s.bn < 0 ? -1 : base + s.bn};
}

int plan_gemm_ksplit(int64_t n_rows, int K) {
    const size_t row_tiles = ((size_t)(n_rows > 0 ? n_rows : 0) + 31) / 32;
    int ks = 1;
    while (ks < 32 && row_tiles * (size_t)ks < 512 && K / (ks * 2) >= 64) ks *= 2;
    return ks;
}

static bool mlp_chain_ok(const gnncca_mlp& m, int in_dim, int out_dim) {
    if (m.n_layers < 0 || m.n_layers > GNNCCA_MAX_LAYERS) return false;
    if (m.n_layers == 0) return in_dim == out_dim;
    int cur = in_dim;
    for (int i = 0; i < m.n_layers; ++i) {
        const gnncca_layer& l = m.layers[i];
        if (l.in_dim != cur || l.out_dim <= 0) return false;
        if ((l.relu != 0) != (l.out_dim != 1)) return false;  // models/mlp.py:17
        if (l.has_bn && l.out_dim == 1) return false;         // models/mlp.py:14
        cur = l.out_dim;
    }
    return cur == out_dim;
}

bool dims_valid(const gnncca_mpn_dims* d) {
    if (!d || d->abi_version != GNNCCA_ABI_VERSION) return false;
    if (d->node_in <= 0 || d->edge_in <= 0 || d->node_dim <= 0 || d->edge_dim <= 0) return false;
    if (d->agg < GNNCCA_AGG_SUM || d->agg > GNNCCA_AGG_MAX) return false;
    if (d->num_enc_steps < 0) return false;
    const int nf = d->reattach_nodes ? 2 : 1, ef = d->reattach_edges ? 2 : 1;
    if (!mlp_chain_ok(d->enc_node, d->node_in, d->node_dim)) return false;
    if (!mlp_chain_ok(d->enc_edge, d->edge_in, d->edge_dim)) return false;
    if (d->edge_mlp.n_layers < 1 || d->node_mlp.n_layers < 1 || d->cls_edge.n_layers < 1) return false;
    if (!mlp_chain_ok(d->edge_mlp, nf * 2 * d->node_dim + ef * d->edge_dim, d->edge_dim)) return false;  // mpn.py:213
    if (!mlp_chain_ok(d->node_mlp, nf * d->node_dim + d->edge_dim, d->node_dim)) return false;           // mpn.py:215
    if (!mlp_chain_ok(d->cls_edge, d->edge_dim, 1)) return false;
    return true;
}

Family classify(const gnncca_mpn_dims* d) {
    if (!dims_valid(d)) return kFamilyNone;
    if (d->node_dim != kH || d->edge_dim != kEF) return kFamilyGeneric;
    if (d->edge_in > kMaxEdgeIn) return kFamilyGeneric;
    if (d->enc_edge.n_layers != 1 || d->edge_mlp.n_layers != 1 || d->node_mlp.n_layers != 1) return kFamilyGeneric;
    if (d->enc_node.n_layers < 1) return kFamilyGeneric;
    for (int i = 0; i < d->enc_node.n_layers; ++i)
        if (d->enc_node.layers[i].out_dim > 1024) return kFamilyGeneric;
    if (d->cls_edge.n_layers > 2) return kFamilyGeneric;
    if (d->cls_edge.n_layers == 2 && d->cls_edge.layers[0].out_dim > kMaxCls) return kFamilyGeneric;
    // the family's classifier kernels apply ReLU after the hidden layer; a hidden layer of width 1 has none (models/mlp.py:17)
    if (d->cls_edge.n_layers == 2 && !d->cls_edge.layers[0].relu) return kFamilyGeneric;
    return kFamilyMfma32x6;
}

const gnncca_mlp& mlp_by_index(const gnncca_mpn_dims* d, int i) {
    switch (i) {
        case 0: return d->enc_node;
        case 1: return d->enc_edge;
        case 2: return d->edge_mlp;
        case 3: return d->node_mlp;
        default: return d->cls_edge;
    }
}

struct GenBlobPlan {
    GenBlobHeader h;
    size_t total_floats;
};

// layers of the fused step's weight block in stage order: fn(mlp index, layer, first row, rows, padded width)
template <typename F>
static void gen_step_block(const gnncca_mpn_dims* d, F fn) {
    const int hin = (d->reattach_nodes ? 2 : 1) * d->node_dim, ein = (d->reattach_edges ? 2 : 1) * d->edge_dim;
    const int mlps[4] = {2, 3, 4, 1};   // edge MLP, node MLP, classifier, then the edge ENCODER (step 1 runs it on the raw edge attributes)
    for (int m : mlps) {
        const gnncca_mlp& mlp = mlp_by_index(d, m);
        for (int l = 0; l < mlp.n_layers; ++l) {
            const int op = (mlp.layers[l].out_dim + 7) / 8 * 8;
            int k0 = 0, kn = mlp.layers[l].in_dim;
            if (l == 0 && m == 2) k0 = 2 * hin, kn = ein;            // cat[x[row] | x[col] | e] (models/mpn.py:68)
            if (l == 0 && m == 3) k0 = hin, kn = d->edge_dim;        // cat[x[row] | e'] (models/mpn.py:97)
            fn(m, l, k0, kn, op);
        }
    }
}

static GenBlobPlan plan_gen_blob(const gnncca_mpn_dims* d) {
    GenBlobPlan p;
    std::memset(&p, 0, sizeof(p));
    size_t off = align_up(sizeof(GenBlobHeader), 16) / 4;
    auto take = [&](size_t n) { size_t o = off; off = align_up(off + n, 4); return (int32_t)o; };
    p.h.magic = kBlobMagic;
    p.h.abi_version = GNNCCA_ABI_VERSION;
    p.h.family = kFamilyGeneric;
    for (int m = 0; m < 5; ++m) {
        const gnncca_mlp& mlp = mlp_by_index(d, m);
        for (int l = 0; l < mlp.n_layers; ++l) {
            // transposed and padded: [in][ceil8(out)] and [ceil8(out)] -- gen_dense_kernel reads 8 outputs per thread
            const size_t op = ((size_t)mlp.layers[l].out_dim + 7) / 8 * 8;
            p.h.w[m][l] = take((size_t)mlp.layers[l].in_dim * op);
            p.h.b[m][l] = take(op);
        }
    }
    // a wide first encoder layer (the 2048-d CNN embedding) runs on the MFMA family's split-K GEMM: keep its weight
    // row-major too
    if (d->enc_node.n_layers > 0 && d->enc_node.layers[0].in_dim >= 256 && d->enc_node.layers[0].in_dim % 64 == 0)
        p.h.enc0_rowmajor = take((size_t)d->enc_node.layers[0].in_dim * d->enc_node.layers[0].out_dim);
    // the fused step kernel (generic_fused.cuh) stages, per workgroup, the weights every EDGE uses: of the edge and node MLPs' first layers only
    // the rows of the e block (the x[row] / x[col] blocks became per-node projection tables), every further layer whole, the classifier,
    // each followed by its bias -- here once more, contiguous and in that order, so that the stage is ONE coalesced copy
    if (d->edge_mlp.n_layers > 0 && d->node_mlp.n_layers > 0) {
        size_t n = 0;
        gen_step_block(d, [&](int, int, int, int kn, int op) { n += (size_t)(kn + 1) * op; });
        p.h.step_w = take(n);
        p.h.step_w_floats = (int32_t)n;
    }
    p.total_floats = off;
    p.h.total_floats = (uint32_t)off;
    return p;
}

int gen_enc0_ksplit(const gnncca_mpn_dims* d, int64_t n_nodes) {
    if (classify(d) != kFamilyGeneric || plan_gen_blob(d).h.enc0_rowmajor == 0) return 0;
    return plan_gemm_ksplit(n_nodes, d->enc_node.layers[0].in_dim);
}

bool gen_blob_header(const gnncca_mpn_dims* d, GenBlobHeader* out) {
    if (classify(d) != kFamilyGeneric || !out) return false;
    *out = plan_gen_blob(d).h;
    return true;
}

bool fast_consts_ok(const gnncca_mpn_dims* d) {
    return classify(d) == kFamilyMfma32x6 && d->edge_in == 4 && !d->reattach_nodes && !d->reattach_edges &&
           d->cls_edge.n_layers == 2 && d->cls_edge.layers[0].out_dim == 4;
}

bool enc_split_ok(const gnncca_mpn_dims* d) {
    return classify(d) == kFamilyMfma32x6 && d->enc_node.n_layers >= 2 && d->enc_node.layers[0].out_dim == 128 &&
           d->enc_node.layers[0].in_dim % 32 == 0;
}

// ---------------------------------------------------------------------------------------------
struct BlobPlan {
    BlobHeader h;
    size_t total_floats;
};

static BlobPlan plan_blob(const gnncca_mpn_dims* d) {
    BlobPlan p;
    std::memset(&p, 0, sizeof(p));
    size_t off = align_up(sizeof(BlobHeader), 16) / 4;
    auto take = [&](size_t n) { size_t o = off; off = align_up(off + n, 4); return (int32_t)o; };
    const int nf = d->reattach_nodes ? 2 : 1, ef = d->reattach_edges ? 2 : 1;
    p.h.magic = kBlobMagic;
    p.h.abi_version = GNNCCA_ABI_VERSION;
    p.h.family = kFamilyMfma32x6;
    p.h.enc_node_layers = d->enc_node.n_layers;
    for (int i = 0; i < d->enc_node.n_layers; ++i) {
        const gnncca_layer& l = d->enc_node.layers[i];
        p.h.enc_node_w[i] = take((size_t)l.in_dim * l.out_dim);
        p.h.enc_node_b[i] = take(l.out_dim);
    }
    const gnncca_layer& last = d->enc_node.layers[d->enc_node.n_layers - 1];
    p.h.enc_last_wT = take((size_t)last.in_dim * kH);
    p.h.enc_edge_w = take((size_t)kEF * d->edge_in);
    p.h.enc_edge_b = take(kEF);
    p.h.wee = take((size_t)kEF * ef * kEF);
    p.h.wne_b = take(3 * 64);
    p.h.wne_bf16 = take(9 * 64);
    p.h.proj_wT = take((size_t)nf * kH * kProjOut);
    p.h.proj_b = take(kProjOut);
    p.h.cls_layers = d->cls_edge.n_layers;
    p.h.cls_hidden = d->cls_edge.n_layers == 2 ? d->cls_edge.layers[0].out_dim : 0;
    if (d->cls_edge.n_layers == 2) {
        p.h.cls_w1 = take((size_t)p.h.cls_hidden * kEF);
        p.h.cls_b1 = take(p.h.cls_hidden);
        p.h.cls_w2 = take(p.h.cls_hidden);
        p.h.cls_b2 = take(1);
    } else {
        p.h.cls_w1 = take(kEF);
        p.h.cls_b1 = take(1);
        p.h.cls_w2 = p.h.cls_b2 = 0;
    }
    p.h.fast_consts = fast_consts_ok(d) ? take(kFastConsts) : 0;
    p.h.enc_w3 = enc_split_ok(d) ? take((size_t)3 * d->enc_node.layers[0].in_dim * d->enc_node.layers[0].out_dim / 2) : 0;
    if (p.h.enc_w3) {   // (enc_split_ok: out = 128) the same weight as two fp16 pieces for enc_f16.cuh, plus its overflow words
        p.h.enc_w2h = take((size_t)d->enc_node.layers[0].in_dim * d->enc_node.layers[0].out_dim);   // 2 pieces x 2 B = 4 B per element
        p.h.enc_w2h_bad = take(kW2hBadWords);
    }
    p.total_floats = off;
    p.h.total_floats = (uint32_t)off;
    return p;
}

bool blob_header(const gnncca_mpn_dims* d, BlobHeader* out) {
    if (classify(d) != kFamilyMfma32x6 || !out) return false;
    *out = plan_blob(d).h;
    return true;
}

// ---------------------------------------------------------------------------------------------
// THE statement of the fast family's blob: every region is a strided copy out of one parameter tensor, optionally through the
// BatchNorm fold and a piece split (internal.h: PackSeg; pack_elem.h has the element rules).  gnncca_pack_weights interprets it on
// the host, pack_device_kernel on the GPU; tests/test_boundary.py holds an independent numpy interpreter and the readers' layouts
// against it.  The splits by cat order:
//   * the edge MLP weight [EF][nf*2H + ef*EF] is split by the cat order of models/mpn.py:68
//       [ x[row] | x[col] | edge_attr ]  ->  W_src, W_dst (per-node projections) and W_ee (per edge)
//   * the node MLP weight [H][nf*H + EF] is split by the cat order of models/mpn.py:97
//       [ x[row] | edge_attr ]           ->  W_nx (per-node projection Q) and W_ne (per edge, MFMA B operand)
// kMaxPackSegs cannot be reached by dims that classify() admits: at most 8 encoder layers x (weight + bias) + enc_w3 + enc_w2h +
// enc_last_wT = 19, the edge encoder 2, the edge MLP 4, the node MLP 2 + the 6 columns of wne_b + wne_bf16 = 9, the classifier 4 and
// fast_consts 9: 47 of 96.
bool pack_program(const gnncca_mpn_dims* d, PackProgram* out) {
    if (!out || classify(d) != kFamilyMfma32x6) return false;
    const BlobPlan p = plan_blob(d);
    std::memset(out, 0, sizeof(*out));
    out->header = p.h;
    int n = 0;
    bool overflow = false;
    struct Lin {
        int w, b, bn, in, out;
    };
    auto lin = [&](int mlp, int layer) {
        const ParamSlots s = param_slots(d, mlp, layer);
        const gnncca_layer& l = mlp_by_index(d, mlp).layers[layer];
        return Lin{s.w, s.b, s.bn, l.in_dim, l.out_dim};
    };
    auto weight = [&](const Lin& L, int dst, int src_off, int rows, int cols, int unit0, int drs, int dcs, int srs, int scs) {
        if (n >= kMaxPackSegs) { overflow = true; return; }
        PackSeg& g = out->segs[n++];
        g.kind = 0, g.dst = dst, g.param = L.w, g.bn = L.bn, g.src_off = src_off, g.rows = rows, g.cols = cols, g.unit0 = unit0;
        g.drs = drs, g.dcs = dcs, g.srs = srs, g.scs = scs;
    };
    auto bias = [&](const Lin& L, int dst, int rows) {
        if (n >= kMaxPackSegs) { overflow = true; return; }
        PackSeg& g = out->segs[n++];
        g.kind = 1, g.dst = dst, g.param = L.b, g.bn = L.bn, g.rows = rows, g.cols = 1, g.drs = 1, g.srs = 1;
    };
    const int nf = d->reattach_nodes ? 2 : 1, ef = d->reattach_edges ? 2 : 1;
    const int hin = nf * kH, ein = ef * kEF;
    // encoder.node_mlp
    for (int i = 0; i < d->enc_node.n_layers; ++i) {
        const Lin L = lin(0, i);
        weight(L, p.h.enc_node_w[i], 0, L.out, L.in, 0, L.in, 1, L.in, 1);
        bias(L, p.h.enc_node_b[i], L.out);
        if (i == 0 && p.h.enc_w3) {
            if (n >= kMaxPackSegs) return false;
            PackSeg& g = out->segs[n++];
            g.kind = 2, g.dst = p.h.enc_w3, g.param = L.w, g.bn = L.bn, g.rows = L.out, g.cols = L.in, g.drs = 0, g.dcs = 0;
            g.srs = L.in, g.scs = 1, g.plane = L.out * 32;  // [in/32][3 pieces][out][32]: pack_elem.h, w3_index
        }
        if (i == 0 && p.h.enc_w2h) {
            if (n >= kMaxPackSegs) return false;
            PackSeg& g = out->segs[n++];
            g.kind = 4, g.dst = p.h.enc_w2h, g.param = L.w, g.bn = L.bn, g.rows = L.out, g.cols = L.in, g.drs = 0, g.dcs = 0;
            g.srs = L.in, g.scs = 1, g.plane = p.h.enc_w2h_bad;
        }
        if (i == d->enc_node.n_layers - 1) weight(L, p.h.enc_last_wT, 0, kH, L.in, 0, 1, kH, L.in, 1);
    }
    // encoder.edge_mlp
    const Lin Le0 = lin(1, 0);
    weight(Le0, p.h.enc_edge_w, 0, kEF, d->edge_in, 0, d->edge_in, 1, d->edge_in, 1);
    bias(Le0, p.h.enc_edge_b, kEF);
    // MPNet.edge_model.edge_mlp : columns [src | dst | edge]   (mpn.py:68)
    const Lin Le = lin(2, 0);
    weight(Le, p.h.proj_wT + 8, 0, kEF, hin, 0, 1, kProjOut, Le.in, 1);        // P_src
    weight(Le, p.h.proj_wT + 0, hin, kEF, hin, 0, 1, kProjOut, Le.in, 1);      // P_dst
    weight(Le, p.h.wee, 2 * hin, kEF, ein, 0, ein, 1, Le.in, 1);
    bias(Le, p.h.proj_b + 8, kEF);
    // MPNet.node_model.node_mlp : columns [x[row] | edge]        (mpn.py:97)
    const Lin Ln = lin(3, 0);
    weight(Ln, p.h.proj_wT + 16, 0, kH, hin, 0, 1, kProjOut, Ln.in, 1);        // Q
    bias(Ln, p.h.proj_b + 16, kH);
    for (int s = 0; s < 3; ++s)
        for (int h = 0; h < 2; ++h) weight(Ln, p.h.wne_b + s * 64 + h * 32, hin + 2 * s + h, kH, 1, 0, 1, 0, Ln.in, 0);
    {   // the same six columns as bf16 pieces in the lane layout of the message MFMAs' B operands (kind 3)
        if (n >= kMaxPackSegs) return false;
        PackSeg& g = out->segs[n++];
        g.kind = 3, g.dst = p.h.wne_bf16, g.param = Ln.w, g.bn = Ln.bn, g.src_off = hin, g.rows = kH, g.cols = kEF, g.unit0 = 0;
        g.drs = 0, g.dcs = 0, g.srs = Ln.in, g.scs = 1;
    }
    // classifier.edge_mlp
    const Lin Lc1 = lin(4, 0);
    weight(Lc1, p.h.cls_w1, 0, Lc1.out, kEF, 0, kEF, 1, kEF, 1);
    bias(Lc1, p.h.cls_b1, Lc1.out);
    Lin Lc2 = Lc1;
    if (d->cls_edge.n_layers == 2) {
        Lc2 = lin(4, 1);
        weight(Lc2, p.h.cls_w2, 0, 1, Lc2.in, 0, Lc2.in, 1, Lc2.in, 1);
        bias(Lc2, p.h.cls_b2, 1);
    }
    if (p.h.fast_consts) {  // the transposed copies mpn_step_fast_kernel reads into SGPR pairs
        const int fc = p.h.fast_consts;
        weight(Le0, fc + kFcEncW, 0, kEF, 4, 0, 1, kEF, 4, 1);
        bias(Le0, fc + kFcEncB, kEF);
        weight(Le, fc + kFcWee, 2 * hin, kEF, kEF, 0, 1, kEF, Le.in, 1);
        weight(Lc1, fc + kFcCw1, 0, 4, kEF, 0, 1, 4, kEF, 1);
        bias(Lc1, fc + kFcCb1, 4);
        weight(Lc2, fc + kFcCw2, 0, 1, 4, 0, 4, 1, 4, 1);
        bias(Lc2, fc + kFcCb2, 1);
        bias(Le, fc + kFcProjB + 8, kEF);
        bias(Ln, fc + kFcProjB + 16, kH);
    }
    out->n_segs = n;
    return !overflow;
}

}  // namespace gnncca

using namespace gnncca;

extern "C" {

int gnncca_abi_version(void) { return GNNCCA_ABI_VERSION; }

const char* gnncca_status_string(int status) {
    switch (status) {
        case GNNCCA_OK: return "ok";
        case GNNCCA_ERR_INVALID_ARG: return "invalid argument";
        case GNNCCA_ERR_UNSUPPORTED: return "GRAPH_NET_PARAMS not supported by this build's HIP kernels";
        case GNNCCA_ERR_WORKSPACE: return "workspace too small";
        case GNNCCA_ERR_HIP: return "HIP runtime error";
        case GNNCCA_ERR_NO_DEVICE: return "no gfx950 device";
        default: return "unknown status";
    }
}

int gnncca_param_count(const gnncca_mpn_dims* d) {
    if (!dims_valid(d)) return -1;
    return mlp_param_count(d->enc_node) + mlp_param_count(d->enc_edge) + mlp_param_count(d->edge_mlp) +
           mlp_param_count(d->node_mlp) + mlp_param_count(d->cls_edge);
}

int gnncca_supported(const gnncca_mpn_dims* d) {
    if (!dims_valid(d)) return GNNCCA_ERR_INVALID_ARG;
    return classify(d) == kFamilyNone ? GNNCCA_ERR_UNSUPPORTED : GNNCCA_OK;
}

int gnncca_num_outputs(const gnncca_mpn_dims* d) {
    if (!dims_valid(d)) return -1;
    if (d->num_enc_steps == 0) return 1;                       // mpn.py:295-297
    const int first = d->num_enc_steps - d->num_class_steps + 1;  // mpn.py:277
    int n = 0;
    for (int s = 1; s <= d->num_enc_steps; ++s) n += (s >= first);
    return n;
}

size_t gnncca_packed_weights_bytes(const gnncca_mpn_dims* d) {
    const Family fam = classify(d);
    if (fam == kFamilyNone) return 0;
    if (fam == kFamilyGeneric) return plan_gen_blob(d).total_floats * sizeof(float);
    return plan_blob(d).total_floats * sizeof(float);
}

static int pack_generic(const gnncca_mpn_dims* d, const float* const* params, void* packed_host, size_t packed_bytes);

// The host interpreter of the pack program: the loop of pack_device_kernel (pack_device.cuh) in row order.  The fold scale is the
// row's, computed once; a row that is neither folded nor strided on either side is copied as one run.
static void run_pack_program(const PackProgram& prog, const float* const* params, float* blob) {
    for (int i = 0; i < prog.n_segs; ++i) {
        const PackSeg& g = prog.segs[i];
        const PackSrc src = pack_src(g, params);
        uint32_t* bad = reinterpret_cast<uint32_t*>(blob + g.plane);   // kind 4 only
        const bool runs = !src.gamma && g.kind <= 1 && g.scs == 1 && g.dcs == 1;
        for (int r = 0; r < g.rows; ++r) {
            if (runs) {
                std::memcpy(blob + g.dst + (size_t)r * g.drs, src.v + g.src_off + (size_t)r * g.srs, (size_t)g.cols * sizeof(float));
                continue;
            }
            const double scale = pack_scale(src, g, r);
            for (int c = 0; c < g.cols; ++c)
                if (pack_store(blob, g, r, c, pack_value(src, g, r, c, scale))) bad[(((size_t)r * g.cols + c) / 256) % kW2hBadWords] = 1u;
        }
    }
}

int gnncca_pack_weights(const gnncca_mpn_dims* d, const float* const* params, int n_params, void* packed_host,
                        size_t packed_bytes) {
    if (!dims_valid(d) || !params || !packed_host) return GNNCCA_ERR_INVALID_ARG;
    if (classify(d) == kFamilyNone) return GNNCCA_ERR_UNSUPPORTED;
    if (n_params != gnncca_param_count(d)) return GNNCCA_ERR_INVALID_ARG;
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return GNNCCA_ERR_INVALID_ARG;
    if (classify(d) == kFamilyGeneric) return pack_generic(d, params, packed_host, packed_bytes);
    if (packed_bytes < gnncca_packed_weights_bytes(d)) return GNNCCA_ERR_INVALID_ARG;
    PackProgram prog;
    if (!pack_program(d, &prog)) return GNNCCA_ERR_UNSUPPORTED;
    float* blob = static_cast<float*>(packed_host);
    std::memset(blob, 0, (size_t)prog.header.total_floats * sizeof(float));
    std::memcpy(blob, &prog.header, sizeof(BlobHeader));
    run_pack_program(prog, params, blob);
    return GNNCCA_OK;
}

static int pack_generic(const gnncca_mpn_dims* d, const float* const* params, void* packed_host, size_t packed_bytes) {
    const GenBlobPlan p = plan_gen_blob(d);
    if (packed_bytes < p.total_floats * sizeof(float)) return GNNCCA_ERR_INVALID_ARG;
    float* blob = static_cast<float*>(packed_host);
    std::memset(blob, 0, p.total_floats * sizeof(float));
    std::memcpy(blob, &p.h, sizeof(GenBlobHeader));
    for (int m = 0; m < 5; ++m) {
        const gnncca_mlp& mlp = mlp_by_index(d, m);
        for (int l = 0; l < mlp.n_layers; ++l) {
            const int in = mlp.layers[l].in_dim, out = mlp.layers[l].out_dim;
            const ParamSlots ps = param_slots(d, m, l);
            PackSeg gw = {}, gb = {};   // the layer's weight [out][in] and bias as sources of the shared fold (pack_elem.h)
            gw.kind = 0, gw.param = ps.w, gw.bn = ps.bn, gw.srs = in, gw.scs = 1;
            gb.kind = 1, gb.param = ps.b, gb.bn = ps.bn, gb.srs = 1;
            const PackSrc sw = pack_src(gw, params), sb = pack_src(gb, params);
            const size_t op = ((size_t)out + 7) / 8 * 8;  // padding stays zero
            float* rowmajor = (m == 0 && l == 0 && p.h.enc0_rowmajor) ? blob + p.h.enc0_rowmajor : nullptr;
            for (int o = 0; o < out; ++o) {
                const double s = pack_scale(sw, gw, o);
                for (int k = 0; k < in; ++k) {
                    const float v = pack_value(sw, gw, o, k, s);
                    blob[p.h.w[m][l] + (size_t)k * op + o] = v;
                    if (rowmajor) rowmajor[(size_t)o * in + k] = v;
                }
                blob[p.h.b[m][l] + o] = pack_value(sb, gb, o, 0, s);
            }
        }
    }
    if (p.h.step_w) {   // the fused step's stage image: copies of the rows above
        size_t o = (size_t)p.h.step_w;
        gen_step_block(d, [&](int m, int l, int k0, int kn, int op) {
            std::memcpy(blob + o, blob + p.h.w[m][l] + (size_t)k0 * op, (size_t)kn * op * sizeof(float));
            o += (size_t)kn * op;
            std::memcpy(blob + o, blob + p.h.b[m][l], (size_t)op * sizeof(float));
            o += (size_t)op;
        });
    }
    return GNNCCA_OK;
}

}  // extern "C"

namespace gnncca {

// (The same invariant as carve()'s: flags / seg_ptr / col32 / perm of the generic family's workspace are read by gnncca_frames_forward's post
// stage after the forward -- fused generic step, op-by-op form and L == 0 alike.)
GenWorkspace carve_generic(const gnncca_mpn_dims* d, int64_t n, int64_t e) {
    GenWorkspace w;
    std::memset(&w, 0, sizeof(w));
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t N = (size_t)(n > 0 ? n : 0), E = (size_t)(e > 0 ? e : 0);
    int64_t nw = d->node_dim, ew = d->edge_dim;
    for (int l = 0; l < d->enc_node.n_layers; ++l) nw = std::max<int64_t>(nw, d->enc_node.layers[l].out_dim);
    const int edge_side[4] = {1, 2, 3, 4};
    for (int m : edge_side) {
        const gnncca_mlp& mlp = mlp_by_index(d, m);
        for (int l = 0; l < mlp.n_layers; ++l) ew = std::max<int64_t>(ew, mlp.layers[l].out_dim);
    }
    if (d->reattach_nodes) nw = std::max<int64_t>(nw, 2 * d->node_dim);  // room for cat(initial, latent)
    if (d->reattach_edges) ew = std::max<int64_t>(ew, 2 * d->edge_dim);
    ew = std::max<int64_t>(ew, d->node_dim);  // per-edge messages [E][H]
    w.node_w = nw;
    w.edge_w = ew;
    w.flags = take(256);
    w.blockflags = take((E / 256 + 2) * 4);
    w.seg_ptr = take((N + 1) * 4);
    w.col32 = take(E * 4);
    w.perm = take(E * 4);
    w.cursor = take((N + 1) * 4);
    w.row32o = take(E * 4);
    w.col32o = take(E * 4);
    for (int i = 0; i < 3; ++i) w.node[i] = take(N * (size_t)nw * 4);
    w.h0 = take(N * (size_t)d->node_dim * 4);
    for (int i = 0; i < 4; ++i) w.edge[i] = take(E * (size_t)ew * 4);
    w.e0 = take(E * (size_t)d->edge_dim * 4);
    const int ks = gen_enc0_ksplit(d, n);
    w.partial = take(ks > 0 ? (size_t)ks * N * (size_t)d->enc_node.layers[0].out_dim * 4 : 0);
    {   // [N][2 * o1e + o1n]: P_src | P_dst | Q of the fused step kernel, ping-pong
        const size_t o1e = d->edge_mlp.n_layers > 0 ? (size_t)d->edge_mlp.layers[0].out_dim : 0;
        const size_t o1n = d->node_mlp.n_layers > 0 ? (size_t)d->node_mlp.layers[0].out_dim : 0;
        for (int i = 0; i < 2; ++i) w.tab[i] = take(N * (2 * o1e + o1n) * 4);
    }
    w.total = off;
    return w;
}

// The diagnostic switches this build reads.  With the gate open, a GNNCCA_* variable that is NOT in this list is
// reported once on stderr: a stale A/B script then says so in its log instead of comparing a build with itself.
static const char* const kDiagSwitches[] = {
    "GNNCCA_DIAG", "GNNCCA_LIB", "GNNCCA_STAMPS",
    "GNNCCA_GEMM_SPLIT_MIN", "GNNCCA_GEMM_LDS_MIN", "GNNCCA_GEMM_R32F_MIN", "GNNCCA_GEMM_R32F_MAX",
    "GNNCCA_GEMM_SLICES_MIN", "GNNCCA_GEMM_SLICES_MAX", "GNNCCA_GEMM_SLICES_NKS", "GNNCCA_GEMM_SLICES_WGS",
    "GNNCCA_GEMM_BF16", "GNNCCA_GEMM_F16_ARM", "GNNCCA_GEMM_F16_XNT", "GNNCCA_TAIL_MFMA_MIN",
    "GNNCCA_WPS", "GNNCCA_NPW", "GNNCCA_NPW_MIN_N", "GNNCCA_NPW_MIN_N_FIRST",
    "GNNCCA_STEP_NT", "GNNCCA_PD_LDS_MIN", "GNNCCA_PD_LDS_MAX", "GNNCCA_NO_PAD",
    "GNNCCA_GEN_UNFUSED", "GNNCCA_COLNORM_NOLDS", "GNNCCA_POOL_CHUNK", "GNNCCA_POOL_SPIN_US"};

extern "C" char** environ;

const char* diag_env(const char* name) {
    static const bool on = [] {
        const char* v = std::getenv("GNNCCA_DIAG");
        const bool open = v != nullptr && v[0] == '1' && v[1] == '\0';
        if (open && environ) {
            for (char** e = environ; *e; ++e) {
                if (std::strncmp(*e, "GNNCCA_", 7) != 0) continue;
                const char* eq = std::strchr(*e, '=');
                const size_t len = eq ? (size_t)(eq - *e) : std::strlen(*e);
                bool known = false;
                for (const char* k : kDiagSwitches) known = known || (std::strlen(k) == len && std::strncmp(k, *e, len) == 0);
                if (!known) {
                    std::fprintf(stderr, "[gnncca] GNNCCA_DIAG=1: '%.*s' is not a switch of this build and is ignored; recognised:", (int)len, *e);
                    for (const char* k : kDiagSwitches) std::fprintf(stderr, " %s", k);
                    std::fprintf(stderr, "\n");
                }
            }
        }
        return open;
    }();
    return on ? std::getenv(name) : nullptr;
}

// An integer-valued diagnostic switch: `fallback` when unset; a value outside [lo, hi] is reported once and ignored.
int diag_env_int(const char* name, int fallback, int lo, int hi) {
    const char* v = diag_env(name);
    if (!v) return fallback;
    char* end = nullptr;
    const long x = std::strtol(v, &end, 10);
    if (end == v || *end != '\0' || x < lo || x > hi) {
        std::fprintf(stderr, "[gnncca] GNNCCA_DIAG=1: %s=%s is outside [%d, %d] and is ignored (default %d)\n", name, v, lo, hi, fallback);
        return fallback;
    }
    return (int)x;
}

int ell_stride(const gnncca_mpn_dims* d, int64_t n, int64_t e) {
    static const bool disabled = diag_env("GNNCCA_NO_PAD") != nullptr;  // diagnostics: A/B against the compact layout
    if (disabled) return 0;
    if (!fast_consts_ok(d) || d->agg == GNNCCA_AGG_MAX || d->num_enc_steps < 1 || n <= 0) return 0;
    if (e < (1 << 19)) return 0;                           // small graphs are cache-resident and latency-bound: nothing to gain
    const int64_t avg = (e + n - 1) / n;
    const int64_t S = (avg + 31) / 32 * 32;                // whole 128-B lines per feature plane and node
    if ((double)e < 0.90 * (double)n * (double)S) return 0;  // ragged: padding would cost more traffic than the shared lines
                                                           // (200 x dense100, 77 % fill: 5 % slower padded)
    if (n * S >= (1ll << 31) - 64) return 0;
    return (int)S;
}

int enc_lds_ksplit(int64_t n_nodes, int K) {
    const int64_t b = (n_nodes + 255) / 256;               // row blocks
    // time in units of one un-split workgroup's run (~237 us): rounds of 256 workgroups / k, + the fused epilogue (un-split) or
    // the tail kernel's pass over the k slabs (measured: 14 us at N = 16 384 / k = 4, 76 us at 66 048 / k = 4).
    // N = 65 536 -> 1 (256 blocks, one round); 66 048 -> 4 (258 blocks would take two rounds un-split: 2.07 vs 1.25 + 0.33);
    // 51 200 -> 1 (200 blocks: 1.07 vs 2 / 2 + 0.15); 16 384 -> 4.
    int best = 1;
    double best_cost = (double)((b + 255) / 256) + 0.07;
    for (int k = 2; k <= 8; k *= 2) {
        if ((K / k) % 32 != 0) break;
        const double cost = (double)((b * k + 255) / 256) / k + (0.05 + 0.07 * k) * (double)b / 256.0;
        if (cost < best_cost - 1e-9) best = k, best_cost = cost;
    }
    return best;
}

// INVARIANT (gnncca_frames_forward, csrc/mpn_post.hip): the plan regions -- flags, seg_ptr, col32, perm -- stay LIVE AND FINAL from the plan's
// launch(es) until the forward returns: the post stage reads them from this workspace (found by carving it again) instead of building the
// plan a second time.  Every forward route finishes that plan (the riding plan blocks + plan_finish in a tail / fused-epilogue workgroup, the
// plan-only launch of big batches, L == 0), and no step kernel may reuse those regions.  tests/test_gpu_pipeline.py holds one pipeline call
// against the separate calls on every route.
Workspace carve(const gnncca_mpn_dims* d, int64_t n, int64_t e) {
    Workspace w;
    std::memset(&w, 0, sizeof(w));
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t N = (size_t)(n > 0 ? n : 0), E = (size_t)(e > 0 ? e : 0);
    w.e_stride = (int64_t)align_up(E > 0 ? E : 1, 64);
    w.ell_S = ell_stride(d, n, e);
    if (w.ell_S > 0) w.e_stride = std::max<int64_t>(w.e_stride, (int64_t)align_up(N * (size_t)w.ell_S, 64));
    // split-K of the first (widest) encoder GEMM: enough workgroups to cover the chip when N is small
    const int k0 = d->enc_node.layers[0].in_dim;
    int ks = plan_gemm_ksplit(n, k0);
    // from 1024 nodes on the split-bf16 GEMM runs with 128-row workgroups: room for its split-K factor too
    if (N >= 1024)
        while (ks < 8 && ((N + 127) / 128) * (size_t)ks < 512 && k0 / (ks * 2) >= 64) ks *= 2;
    if (N >= 4096) ks = std::max(ks, enc_lds_ksplit((int64_t)N, k0));  // room for the slabs of the 256-row GEMM's choice
    w.ksplit = ks;
    size_t fmax = 0;
    for (int i = 0; i < d->enc_node.n_layers; ++i)
        fmax = fmax > (size_t)d->enc_node.layers[i].out_dim ? fmax : (size_t)d->enc_node.layers[i].out_dim;
    w.flags = take(256);
    w.blockflags = take((E / 256 + 2) * 4);
    w.seg_ptr = take((N + 1) * 4);
    w.col32 = take(E * 4);
    w.perm = take(E * 4);
    w.cursor = take((N + 1) * 4);
    w.h0 = take(N * kH * 4);
    w.act = take(d->enc_node.n_layers >= 3 ? 2 * N * fmax * 4 : 0);
    w.partial = take((size_t)ks * N * fmax * 4);
    for (int i = 0; i < 2; ++i) w.pd[i] = take(N * kPdStride * 4);
    for (int i = 0; i < 2; ++i) w.psq[i] = take(N * kPsQStride * 4);
    w.e = take((size_t)kEF * w.e_stride * 4);
    w.e0 = take(d->reattach_edges ? (size_t)kEF * w.e_stride * 4 : 0);
    w.rng = take(N * 16);   // per-node column ranges (start1, len1, start2 - len1, breaks): written by step 1, read by the later steps
    w.total = off;
    return w;
}

}  // namespace gnncca

extern "C" size_t gnncca_workspace_bytes(const gnncca_mpn_dims* d, int64_t n_nodes, int64_t n_edges) {
    const Family fam = classify(d);
    if (fam == kFamilyNone || n_nodes < 0 || n_edges < 0) return 0;
    if (fam == kFamilyGeneric) return carve_generic(d, n_nodes, n_edges).total;
    return carve(d, n_nodes, n_edges).total;
}
