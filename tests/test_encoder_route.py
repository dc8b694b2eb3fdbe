"""The node encoder's route table (csrc/enc_route.cpp: encoder_route), pinned on the CPU.

encoder_route() is a pure host function: from the dims, the blob header, the workspace carve-up, N, E, the options and a few alignment
bits it decides which GEMM form every encoder layer runs on, how many k-slabs that launch writes (the count the following reduce or tail
sums), where the graph plan goes and which tail follows; launch_node_encoder (csrc/mpn_forward.hip) carries the decision out and compares
no sizes.  Here a stand-alone host program (plain C++ against internal.h, pack.cpp and enc_route.cpp: no HIP, no GPU) prints the route of
every case with the default EncTuning, and the test holds the output against the table below -- written from the conditions of the
forward as it was before the route became a function, and confirmed there by a kernel trace.  A pull request that adds
a form or moves a threshold edits this table on purpose.

A line reads: one `FORM/slabs x kslice` per GEMM layer (R32_BF16 with its stage count), `plan=PLACE/workgroups/plan_span`,
`tail=KIND` (FAST with its nodes per workgroup, LDS with its dynamic-LDS bytes), `sums` = the slab count the tail is told, `xnt` = the
fp16-split forms' non-temporal x stream, `ksplit` = Workspace::ksplit (the slabs the workspace has room for).  The graphs are rings of
three edges per node unless E is given."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_workspace_layouts import _host_compiler

CSRC = os.path.join(ROOT, "gnn-cca_amd", "csrc")
FLAGS = {"split3": 1, "unsplit": 2, "reattach": 4, "dropping": 8, "trace_h": 16}


def C(node_in, fc, n, E=None, x_aligned=True, ei_aligned=True, **flags):
    """One case as the probe's argument: node_in:fc,fc:N:E:flag bits (32: x not 16-byte aligned, 64: edge_index not)."""
    bits = sum(FLAGS[k] for k, v in flags.items() if v) | (0 if x_aligned else 32) | (0 if ei_aligned else 64)
    return f"{node_in}:{','.join(map(str, fc))}:{n}:{3 * n if E is None else E}:{bits}"


TABLE = [
    (C(2048, [128], 1), "SLICES/16x128 plan=RIDES/1/0 tail=FAST/1 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 64), "SLICES/16x128 plan=RIDES/1/0 tail=FAST/1 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 320), "SLICES/16x128 plan=RIDES/2/0 tail=FAST/1 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 321), "SLICES/16x128 plan=RIDES/2/0 tail=FAST/2 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 512), "SLICES/16x128 plan=RIDES/3/0 tail=FAST/2 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 513), "SLICES/8x256 plan=RIDES/4/0 tail=FAST/2 sums=8 xnt=0 ksplit=32"),
    (C(2048, [128], 640), "SLICES/8x256 plan=RIDES/4/0 tail=FAST/2 sums=8 xnt=0 ksplit=32"),
    (C(2048, [128], 641), "SLICES/8x256 plan=RIDES/4/0 tail=FAST/4 sums=8 xnt=0 ksplit=32"),
    (C(2048, [128], 2559), "SLICES/8x256 plan=RIDES/15/0 tail=FAST/4 sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 2560), "SLICES/8x256 plan=RIDES/15/0 tail=MFMA sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 4095), "SLICES/8x256 plan=RIDES/24/0 tail=MFMA sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 4096), "R32_F16/1x2048 plan=BEFORE/48/0 tail=NONE sums=1 xnt=0 ksplit=8"),
    (C(2048, [128], 8192), "R32_F16/1x2048 plan=BEFORE/96/0 tail=NONE sums=1 xnt=0 ksplit=8"),
    (C(2048, [128], 8193), "LDS256_F16/4x512 plan=AFTER/97/0 tail=MFMA sums=4 xnt=0 ksplit=8"),
    (C(2048, [128], 16383), "LDS256_F16/4x512 plan=AFTER/192/0 tail=MFMA sums=4 xnt=0 ksplit=4"),
    (C(2048, [128], 16384), "LDS256_F16/4x512 plan=AFTER/192/0 tail=MFMA sums=4 xnt=1 ksplit=4"),
    (C(2048, [128], 51200), "LDS256_F16/1x2048 plan=BEFORE/600/0 tail=NONE sums=1 xnt=1 ksplit=2"),
    (C(2048, [128], 65536), "LDS256_F16/1x2048 plan=BEFORE/768/0 tail=NONE sums=1 xnt=1 ksplit=1"),
    (C(2048, [128], 66048), "LDS256_F16/4x512 plan=AFTER/774/0 tail=MFMA sums=4 xnt=1 ksplit=4"),
    (C(2048, [128], 66048, E=1056768), "LDS256_F16/4x512 plan=AFTER/1032/1 tail=MFMA sums=4 xnt=1 ksplit=4"),
    (C(2048, [128], 66048, E=1056768, ei_aligned=False), "LDS256_F16/4x512 plan=AFTER/1032/0 tail=MFMA sums=4 xnt=1 ksplit=4"),
    (C(2016, [128], 383), "PLAN/16x128 plan=RIDES/5/0 tail=FAST/2 sums=16 xnt=0 ksplit=16"),
    (C(2016, [128], 384), "D128/1x2016 plan=RIDES/5/0 tail=FAST/2 sums=1 xnt=0 ksplit=16"),
    (C(2016, [128], 6143), "D128/1x2016 plan=RIDES/72/0 tail=MFMA sums=1 xnt=0 ksplit=8"),
    (C(2016, [128], 6144), "LDS256_F16/1x2016 plan=BEFORE/72/0 tail=NONE sums=1 xnt=0 ksplit=8"),
    (C(2048, [128], 4095, unsplit=True), "D128/8x256 plan=RIDES/48/0 tail=MFMA sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 4096, unsplit=True), "R32_BF16/1x2048/nst8 plan=BEFORE/48/0 tail=NONE sums=1 xnt=0 ksplit=8"),
    (C(2048, [128], 8192, unsplit=True), "R32_BF16/1x2048/nst8 plan=BEFORE/96/0 tail=NONE sums=1 xnt=0 ksplit=8"),
    (C(2048, [128], 8193, unsplit=True), "R32_BF16/1x2048/nst4 plan=BEFORE/97/0 tail=NONE sums=1 xnt=0 ksplit=8"),
    (C(2048, [128], 51200, unsplit=True), "LDS256_BF16/1x2048 plan=BEFORE/600/0 tail=NONE sums=1 xnt=1 ksplit=2"),
    (C(2048, [128], 4099, split3=True), "D128/8x256 plan=RIDES/49/0 tail=MFMA sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 8197, split3=True), "LDS256_BF16/4x512 plan=AFTER/97/0 tail=MFMA sums=4 xnt=0 ksplit=8"),
    (C(2048, [128], 65536, split3=True), "LDS256_BF16/1x2048 plan=BEFORE/768/0 tail=NONE sums=1 xnt=1 ksplit=1"),
    (C(2048, [64], 3007), "PLAN/8x256 plan=RIDES/36/0 tail=LDS/19456 sums=8 xnt=0 ksplit=8"),
    (C(2048, [256], 8197), "PLAN/8x256 plan=RIDES/97/0 tail=LDS/47104 sums=8 xnt=0 ksplit=8"),
    (C(1000, [128], 1229), "PLAN/8x128 plan=RIDES/15/0 tail=FAST/4 sums=8 xnt=0 ksplit=8"),
    (C(2048, [], 64), "PLAN/32x64 plan=RIDES/1/0 tail=LDS/10752 sums=32 xnt=0 ksplit=32"),
    (C(2048, [], 6153), "PLAN/8x256 plan=RIDES/73/0 tail=LDS/10752 sums=8 xnt=0 ksplit=8"),
    (C(2048, [1024], 301), "PLAN/32x64 plan=RIDES/4/0 tail=LDS/157696 sums=32 xnt=0 ksplit=32"),
    (C(2048, [128, 64], 64), "SLICES/16x128 PLAN/1x128 plan=RIDES/1/0 tail=LDS/19456 sums=1 xnt=0 ksplit=32"),
    (C(2048, [128, 64], 301), "SLICES/16x128 PLAN/1x128 plan=RIDES/2/0 tail=LDS/19456 sums=1 xnt=0 ksplit=32"),
    (C(2048, [128, 64], 1229), "SLICES/8x256 PLAN/1x128 plan=RIDES/8/0 tail=LDS/19456 sums=1 xnt=0 ksplit=16"),
    (C(2048, [128, 64], 3007), "SLICES/8x256 PLAN/1x128 plan=RIDES/18/0 tail=LDS/19456 sums=1 xnt=0 ksplit=8"),
    (C(2048, [128, 64], 4099), "D128/8x256 PLAN/1x128 plan=RIDES/49/0 tail=LDS/19456 sums=1 xnt=0 ksplit=8"),
    (C(2048, [128, 64], 8197), "LDS256_F16/4x512 PLAN/1x128 plan=AFTER/97/0 tail=LDS/19456 sums=1 xnt=0 ksplit=8"),
    (C(2048, [128, 64], 51233), "LDS256_F16/1x2048 PLAN/1x128 plan=AFTER/601/0 tail=LDS/19456 sums=1 xnt=1 ksplit=2"),
    (C(2048, [128, 128, 64], 64), "SLICES/16x128 PLAN/1x128 PLAN/1x128 plan=RIDES/1/0 tail=LDS/19456 sums=1 xnt=0 ksplit=32"),
    (C(2048, [128, 128, 64], 301), "SLICES/16x128 PLAN/1x128 PLAN/1x128 plan=RIDES/2/0 tail=LDS/19456 sums=1 xnt=0 ksplit=32"),
    (C(2048, [128, 128, 64], 1229), "SLICES/8x256 PLAN/1x128 PLAN/1x128 plan=RIDES/8/0 tail=LDS/19456 sums=1 xnt=0 ksplit=16"),
    (C(2048, [128, 128, 64], 3007), "SLICES/8x256 PLAN/1x128 PLAN/1x128 plan=RIDES/18/0 tail=LDS/19456 sums=1 xnt=0 ksplit=8"),
    (C(2048, [128, 128, 64], 4099), "D128/8x256 PLAN/1x128 PLAN/1x128 plan=RIDES/49/0 tail=LDS/19456 sums=1 xnt=0 ksplit=8"),
    (C(2048, [128, 128, 64], 8197), "LDS256_F16/4x512 PLAN/1x128 PLAN/1x128 plan=AFTER/97/0 tail=LDS/19456 sums=1 xnt=0 ksplit=8"),
    (C(2048, [128, 128, 64], 51233), "LDS256_F16/1x2048 PLAN/1x128 PLAN/1x128 plan=AFTER/601/0 tail=LDS/19456 sums=1 xnt=1 ksplit=2"),
    (C(2048, [128], 301, x_aligned=False), "PLAN/32x64 plan=RIDES/4/0 tail=FAST/1 sums=32 xnt=0 ksplit=32"),
    (C(2048, [128], 4096, x_aligned=False), "PLAN/8x256 plan=RIDES/48/0 tail=MFMA sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 8193, x_aligned=False), "PLAN/8x256 plan=RIDES/97/0 tail=MFMA sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 301, E=0), "SLICES/16x128 plan=NONE tail=FAST/1 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 4096, E=0), "R32_F16/1x2048 plan=NONE tail=NONE sums=1 xnt=0 ksplit=8"),
    (C(2048, [128], 8193, E=0), "LDS256_F16/4x512 plan=NONE tail=MFMA sums=4 xnt=0 ksplit=8"),
    (C(2048, [128], 301, reattach=True), "SLICES/16x128 plan=RIDES/2/0 tail=LDS/34816 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 3007, reattach=True), "SLICES/8x256 plan=RIDES/18/0 tail=LDS/34816 sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 4096, reattach=True), "D128/8x256 plan=RIDES/48/0 tail=LDS/34816 sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 51200, reattach=True), "LDS256_F16/1x2048 plan=AFTER/600/0 tail=LDS/34816 sums=1 xnt=1 ksplit=2"),
    (C(2048, [1024], 301, reattach=True), "PLAN/32x64 plan=RIDES/4/0 tail=LDS/163840 sums=32 xnt=0 ksplit=32"),
    (C(2048, [1024, 1024], 301, reattach=True), "PLAN/32x64 PLAN/1x1024 plan=RIDES/4/0 tail=LDS/163840 sums=1 xnt=0 ksplit=32"),
    (C(2048, [128], 301, dropping=True, trace_h=True), "SLICES/16x128 plan=RIDES/2/0 tail=LDS/28672 sums=16 xnt=0 ksplit=32"),
    (C(2048, [128], 3007, dropping=True, trace_h=True), "SLICES/8x256 plan=RIDES/18/0 tail=LDS/28672 sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 4096, dropping=True, trace_h=True), "D128/8x256 plan=RIDES/48/0 tail=LDS/28672 sums=8 xnt=0 ksplit=8"),
    (C(2048, [128], 51200, dropping=True, trace_h=True), "LDS256_F16/1x2048 plan=AFTER/600/0 tail=LDS/28672 sums=1 xnt=1 ksplit=2"),
    (C(2048, [128], 301, trace_h=True), "SLICES/16x128 plan=RIDES/2/0 tail=LDS/28672 sums=16 xnt=0 ksplit=32"),
]

_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "internal.h"
using namespace gnncca;
static void layer(gnncca_mlp& m, int in, int out) {
    gnncca_layer& l = m.layers[m.n_layers++];
    l.in_dim = in, l.out_dim = out, l.has_bn = 0, l.relu = out != 1;
}
int main(int argc, char** argv) {
    static const char* forms[] = {"PLAN", "SLICES", "D128", "R32_BF16", "R32_F16", "LDS256_BF16", "LDS256_F16"};
    static const char* places[] = {"NONE", "RIDES", "BEFORE", "AFTER"};
    for (int a = 1; a < argc; ++a) {
        int K = 0, N = 0, E = 0, bits = 0;
        char fc[64] = "";
        if (std::sscanf(argv[a], "%d:%63[^:]:%d:%d:%d", &K, fc, &N, &E, &bits) != 5 && std::sscanf(argv[a], "%d::%d:%d:%d", &K, &N, &E, &bits) != 4) return 2;
        gnncca_mpn_dims d;
        std::memset(&d, 0, sizeof(d));
        d.abi_version = GNNCCA_ABI_VERSION, d.node_in = K, d.edge_in = 4, d.node_dim = kH, d.edge_dim = kEF, d.agg = GNNCCA_AGG_SUM;
        d.num_enc_steps = 4, d.num_class_steps = 2, d.reattach_nodes = (bits & 4) != 0;
        int in = K;
        for (char* tok = std::strtok(fc, ","); tok; tok = std::strtok(nullptr, ",")) layer(d.enc_node, in, std::atoi(tok)), in = std::atoi(tok);
        layer(d.enc_node, in, kH);
        const int nf = d.reattach_nodes ? 2 : 1;
        layer(d.enc_edge, 4, kEF), layer(d.edge_mlp, nf * 2 * kH + kEF, kEF), layer(d.node_mlp, nf * kH + kEF, kH);
        layer(d.cls_edge, kEF, 4), layer(d.cls_edge, 4, 1);
        BlobHeader hdr;
        if (!blob_header(&d, &hdr)) return 3;
        const Workspace ws = carve(&d, N, E);
        // plan.cuh: 1024 edges per plan block from 2^19 edges (256 below), the pair form (plan_span 1) on even, aligned edge lists
        const int per = E >= (1 << 19) ? 1024 : 256;
        const int span = (per == 1024 && E % 2 == 0 && !(bits & 64)) ? 1 : 0;
        const EncRouteIn in_{&d, &hdr, &ws, N, E, (uint32_t)((bits & 1 ? GNNCCA_OPT_ENC_SPLIT3 : 0) | (bits & 2 ? GNNCCA_OPT_ENC_UNSPLIT : 0)),
                             (bits & 8) != 0, (bits & 16) != 0, !(bits & 32), true, E > 0 ? (E + per - 1) / per : 0, E > 0 ? span : 0};
        const EncRoute r = encoder_route(in_, EncTuning{});
        for (int g = 0; g < r.n_gemm; ++g) {
            const EncGemmRoute& q = r.gemm[g];
            std::printf("%s/%dx%d", forms[q.form], q.slabs, q.kslice);
            if (q.form == kEncR32Bf16) std::printf("/nst%d", q.nst);
            std::printf(" ");
        }
        if (r.plan_place == kPlanNone) std::printf("plan=NONE ");
        else std::printf("plan=%s/%d/%d ", places[r.plan_place], r.plan_wgs, r.plan_span);
        switch (r.tail) {
            case kTailNone: std::printf("tail=NONE"); break;
            case kTailFast: std::printf("tail=FAST/%d", r.tail_npw); break;
            case kTailMfma: std::printf("tail=MFMA"); break;
            case kTailLds: std::printf("tail=LDS/%zu", r.tail_lds); break;
            default: std::printf("tail=REFUSED"); break;
        }
        std::printf(" sums=%d xnt=%d ksplit=%d fused=%d\n", r.gemm[r.n_gemm - 1].slabs, r.x_nt, ws.ksplit, (int)r.fused);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("enc_route")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(_PROBE)
    subprocess.run([_host_compiler(), "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src),
                    os.path.join(CSRC, "enc_route.cpp"), os.path.join(CSRC, "pack.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)] + [c for c, _ in TABLE], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(TABLE)
    return dict(zip((c for c, _ in TABLE), out))


@pytest.mark.parametrize("case,want", TABLE)
def test_route_is_the_table(routes, case, want):
    got = routes[case]
    assert got.rsplit(" fused=", 1)[0] == want, (case, got)


@pytest.mark.parametrize("case", [c for c, _ in TABLE])
def test_consumer_sums_the_slabs_the_producer_wrote(routes, case):
    """The invariant a stale slab count once broke: every GEMM's slab count is within the workspace's, the tail is told the last GEMM's,
    every GEMM in front of a reduce hands it its own (one field: EncGemmRoute::slabs), and a fused GEMM has no slabs and no tail."""
    got = routes[case]
    slabs = [int(s) for s in re.findall(r"[A-Z0-9_]+/(\d+)x\d+", got.split(" plan=")[0])]
    ksplit, sums, fused = (int(re.search(rf" {k}=(\d+)", got).group(1)) for k in ("ksplit", "sums", "fused"))
    assert slabs and all(1 <= s <= ksplit for s in slabs[:1]) and all(s == 1 for s in slabs[1:]), got
    assert sums == slabs[-1], got
    if fused:
        assert slabs == [1] and "tail=NONE" in got and "plan=AFTER" not in got and "plan=RIDES" not in got, got
    else:
        assert "tail=NONE" not in got and "plan=BEFORE" not in got, got
