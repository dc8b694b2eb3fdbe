// pack_host_check.cpp -- the host packer in a stand-alone program, for a sanitizer run and for timing without Python around it.
// pack.cpp is plain C++ (no HIP call), so this needs no GPU and no ROCm:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I gnn-cca_amd/csrc \
//           tools/pack_host_check.cpp gnn-cca_amd/csrc/pack.cpp -o /tmp/pack_host_check && /tmp/pack_host_check
//
// Packs a handful of configurations of both families into heap buffers of exactly gnncca_packed_weights_bytes (so that a store past
// either end is a heap-buffer-overflow), from parameter tensors of exactly their own size (so is a read past a parameter), and prints a
// hash of every blob.  `pack_host_check N` also times N calls of the shipped shape.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "gnncca_mpn.h"

static gnncca_mlp mlp(std::vector<int> widths, bool bn) {   // widths[0] = input
    gnncca_mlp m = {};
    m.n_layers = (int)widths.size() - 1;
    for (int l = 0; l < m.n_layers; ++l) m.layers[l] = gnncca_layer{widths[l], widths[l + 1], bn && widths[l + 1] != 1, widths[l + 1] != 1};
    return m;
}

static gnncca_mpn_dims dims(std::vector<int> enc, int node_dim, int edge_in, int edge_dim, bool bn, bool re_n, bool re_e, std::vector<int> cls) {
    gnncca_mpn_dims d = {};
    d.abi_version = GNNCCA_ABI_VERSION, d.node_in = enc[0], d.edge_in = edge_in, d.node_dim = node_dim, d.edge_dim = edge_dim;
    d.agg = GNNCCA_AGG_SUM, d.num_enc_steps = 2, d.num_class_steps = 1, d.reattach_nodes = re_n, d.reattach_edges = re_e;
    const int nf = re_n ? 2 : 1, ef = re_e ? 2 : 1;
    enc.push_back(node_dim), cls.insert(cls.begin(), edge_dim), cls.push_back(1);
    d.enc_node = mlp(enc, bn), d.enc_edge = mlp({edge_in, edge_dim}, bn), d.cls_edge = mlp(cls, bn);
    d.edge_mlp = mlp({nf * 2 * node_dim + ef * edge_dim, edge_dim}, bn), d.node_mlp = mlp({nf * node_dim + edge_dim, node_dim}, bn);
    return d;
}

struct Params {
    std::vector<std::unique_ptr<float[]>> own;
    std::vector<const float*> ptr;
};
static Params make_params(const gnncca_mpn_dims& d, const std::vector<float>& planted) {
    Params p;
    uint32_t s = 12345u;
    auto tensor = [&](size_t n, float lo, float hi) {
        p.own.emplace_back(new float[n]);
        for (size_t i = 0; i < n; ++i) s = s * 1664525u + 1013904223u, p.own.back()[i] = lo + (hi - lo) * (float)(s >> 8) / 16777216.0f;
        p.ptr.push_back(p.own.back().get());
    };
    const gnncca_mlp* all[5] = {&d.enc_node, &d.enc_edge, &d.edge_mlp, &d.node_mlp, &d.cls_edge};
    for (const gnncca_mlp* m : all)
        for (int l = 0; l < m->n_layers; ++l) {
            const size_t in = m->layers[l].in_dim, out = m->layers[l].out_dim;
            tensor(in * out, -1.f, 1.f), tensor(out, -1.f, 1.f);
            if (m->layers[l].has_bn) tensor(out, 0.5f, 1.5f), tensor(out, -1.f, 1.f), tensor(out, -1.f, 1.f), tensor(out, 0.3f, 3.f);
        }
    const size_t n0 = (size_t)d.enc_node.layers[0].in_dim * d.enc_node.layers[0].out_dim;
    for (size_t i = 0; i < planted.size(); ++i) p.own[0][(i * 2087 + 300) % n0] = planted[i];
    return p;
}

static int pack(const char* name, const gnncca_mpn_dims& d, const std::vector<float>& planted, int timed_calls) {
    const Params p = make_params(d, planted);
    const size_t bytes = gnncca_packed_weights_bytes(&d);
    if ((int)p.ptr.size() != gnncca_param_count(&d) || bytes == 0) return std::printf("%s: bad configuration\n", name), 1;
    std::unique_ptr<unsigned char[]> blob(new unsigned char[bytes]);
    const int status = gnncca_pack_weights(&d, p.ptr.data(), (int)p.ptr.size(), blob.get(), bytes);
    if (status != GNNCCA_OK) return std::printf("%s: %s\n", name, gnncca_status_string(status)), 1;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ blob[i]) * 1099511628211ull;
    std::printf("%-22s %9zu bytes  fnv1a %016llx\n", name, bytes, (unsigned long long)h);
    if (timed_calls > 0) {
        std::vector<double> ms;
        for (int i = 0; i < timed_calls; ++i) {
            const auto t0 = std::chrono::steady_clock::now();
            gnncca_pack_weights(&d, p.ptr.data(), (int)p.ptr.size(), blob.get(), bytes);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("%-22s median %.3f ms, min %.3f ms over %d calls\n", name, ms[ms.size() / 2], ms[0], timed_calls);
    }
    return 0;
}

int main(int argc, char** argv) {
    const int timed = argc > 1 ? std::atoi(argv[1]) : 0;
    int bad = 0;
    bad += pack("shipped", dims({2048, 128}, 32, 4, 6, false, false, false, {4}), {}, timed);
    bad += pack("bn_everywhere", dims({2048, 128}, 32, 4, 6, true, false, false, {4}), {}, 0);
    bad += pack("enc3_bn", dims({256, 128, 64}, 32, 4, 6, true, false, false, {4}), {}, 0);
    bad += pack("enc1_edge2", dims({96}, 32, 2, 6, false, false, false, {}), {}, 0);
    bad += pack("first_in_odd", dims({100, 128}, 32, 4, 6, true, false, true, {8}), {}, 0);
    bad += pack("reattach_both_e16", dims({64, 128}, 32, 16, 6, true, true, true, {8}), {}, 0);
    bad += pack("f16_extremes", dims({64, 128}, 32, 4, 6, false, false, false, {4}), {65520.0f, -7.0e4f, 6.0e-8f, -3.0e-6f, 2.0e-8f}, 0);
    bad += pack("generic_wide", dims({512, 64}, 16, 4, 8, true, true, false, {4}), {}, 0);
    return bad != 0;
}
