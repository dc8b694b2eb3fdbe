"""The two workspaces whose layout used to be stated twice -- the fused backward's (gnncca_backward_workspace_bytes against the region-by-region
carve in gnncca_mpn_backward_inputs) and the post stage's (gnncca_post_workspace_bytes against post_prune_cluster_impl) -- now come from one
layout function each (csrc/internal.h: carve_backward, carve_post).  Callers size buffers from the byte counts, so both are pinned here to the
closed forms the size functions had before, to the byte; the offsets are pinned to the prefix sums of the same terms, read out of the structs by
a small stand-alone host program (the structs are not part of the exported ABI).  No GPU involved."""
import copy
import ctypes as C
import os
import shutil
import subprocess

from conftest import GOLDEN_DIR, ROOT
from oracle.mpn_oracle import load_case

NODES = (0, 1, 63, 64, 65, 255, 256, 257, 4096)
EDGES = (0, 1, 255, 256, 257, 511, 512, 100_000)
KH, KEF = 32, 6   # csrc/internal.h: kH, kEF


def up(v):
    return (v + 255) // 256 * 256


def post_terms(n, e):
    """flags | blockflags | seg_ptr | col32 | perm | cursor"""
    return [256, (e // 256 + 2) * 4, (n + 1) * 4, e * 4, e * 4, (n + 1) * 4]


def post_bytes(n, e):
    return up(256) + up((e // 256 + 2) * 4) + up((n + 1) * 4) + up(e * 4) + up(e * 4) + up((n + 1) * 4)


def bwd_terms(n, e, f1, steps):
    """gh0_acc | ge0_acc | deg | Q | hmax (+ tie counts) | dP_all | Hb[2] | Gb[2] | a1 | gz1 | part | bn_sums | bn_red"""
    L = max(steps, 1)
    return [n * KH * 4, e * KEF * 4, n * 4, n * KH * 4, 2 * n * KH * 4, L * n * 44 * 4, n * KH * 4, n * KH * 4, e * KEF * 4, e * KEF * 4,
            n * f1 * 4, n * f1 * 4, 32 * n * f1 * 4, 8 * 2 * 64, 4 * 2 * 64]


def bwd_bytes(n, e, f1, steps):
    L = max(steps, 1)
    return (up(n * KH * 4) + up(e * KEF * 4) + up(n * 4) + up(n * KH * 4) + up(2 * n * KH * 4) + up(L * n * 44 * 4) + 2 * up(n * KH * 4) +
            2 * up(e * KEF * 4) + 2 * up(n * f1 * 4) + up(32 * n * f1 * 4) + up(8 * 128) + up(4 * 128))


def prefix(terms):
    offs, off = [], 0
    for t in terms:
        offs.append(off)
        off += up(t)
    return offs + [off]


def _dims(name):
    from gnn_cca_amd import MOTMPNet
    params, arch, _, _ = load_case(os.path.join(GOLDEN_DIR, name + ".npz"))
    return MOTMPNet(copy.deepcopy(params), None, arch).native_dims()


def _backward_cases():
    """(label, dims): the shipped dims, both reattach flags, a 64-wide first encoder layer, L = 1 and L = 3"""
    shipped = _dims("terrace32")
    both = _dims("bwd_terrace32_reatt_ne_mean")
    assert both.reattach_nodes and both.reattach_edges and not shipped.reattach_nodes and not shipped.reattach_edges
    narrow = _dims("terrace32")
    narrow.enc_node.layers[0].out_dim = narrow.enc_node.layers[1].in_dim = 64
    cases = [("shipped", shipped), ("reattach_both", both), ("first_layer_64", narrow)]
    for steps in (1, 3):
        d = _dims("terrace32")
        d.num_enc_steps, d.num_class_steps = steps, 1
        cases.append(("L%d" % steps, d))
    return cases


def test_post_workspace_bytes_match_the_closed_form():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    for n in NODES:
        for e in EDGES:
            assert lib.gnncca_post_workspace_bytes(n, e) == post_bytes(n, e) == prefix(post_terms(n, e))[-1], (n, e)


def test_backward_workspace_bytes_match_the_closed_form():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    for label, d in _backward_cases():
        assert lib.gnncca_backward_supported(C.byref(d)) == nat.OK, label
        f1, steps = d.enc_node.layers[0].out_dim, d.num_enc_steps
        for n in NODES:
            for e in EDGES:
                want = bwd_bytes(n, e, f1, steps)
                assert want == prefix(bwd_terms(n, e, f1, steps))[-1]
                assert lib.gnncca_backward_workspace_bytes(C.byref(d), n, e) == want, (label, n, e)


_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "internal.h"
using namespace gnncca;
// argv: F1 L pairs.  One line per (layout, case, N, E): the offsets in region order, then the total.
int main(int argc, char** argv) {
    const long long ns[] = {%(nodes)s}, es[] = {%(edges)s};
    for (long long n : ns)
        for (long long e : es) {
            const PostWorkspace p = carve_post(n, e);
            std::printf("post 0 0 %%lld %%lld %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", n, e, p.flags, p.blockflags, p.seg_ptr, p.col32, p.perm, p.cursor, p.total);
        }
    for (int a = 1; a + 1 < argc; a += 2) {
        gnncca_mpn_dims d;
        std::memset(&d, 0, sizeof(d));
        d.enc_node.n_layers = 2;
        d.enc_node.layers[0].out_dim = std::atoi(argv[a]);
        d.num_enc_steps = std::atoi(argv[a + 1]);
        for (long long n : ns)
            for (long long e : es) {
                const BwdWorkspace w = carve_backward(&d, n, e);
                std::printf("bwd %%s %%s %%lld %%lld %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", argv[a], argv[a + 1], n, e,
                            w.gh0_acc, w.ge0_acc, w.deg, w.Q, w.hmax, w.dP_all, w.Hb[0], w.Hb[1], w.Gb[0], w.Gb[1], w.a1, w.gz1, w.part,
                            w.bn_sums, w.bn_red, w.total);
            }
    }
    return 0;
}
"""


def _host_compiler():
    from gnn_cca_amd import _native as nat
    import importlib.util
    spec = importlib.util.spec_from_file_location("gnncca_build", os.path.join(os.path.dirname(nat.__file__), "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    hipcc = os.path.realpath(build._hipcc())   # the compiler the library itself was built with ships a plain clang++
    for c in (os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "clang++"), os.path.join(os.path.dirname(hipcc), "..", "lib", "llvm", "bin", "clang++"),
              shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no host C++ compiler found")


def test_workspace_offsets_are_the_prefix_sums_of_the_closed_forms(tmp_path):
    """carve_post / carve_backward as the drivers see them: compiled into a host program (plain C++, no HIP), every offset of every region on
    the whole grid against the prefix sums of the terms above -- region order, the 256-byte alignment and every size in one comparison."""
    src = tmp_path / "probe.cpp"
    src.write_text(_PROBE % {"nodes": ", ".join(map(str, NODES)), "edges": ", ".join(map(str, EDGES))})
    exe = tmp_path / "probe"
    subprocess.run([_host_compiler(), "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gnn-cca_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    pairs = [(128, 4), (64, 4), (128, 1), (128, 3), (128, 0)]   # (F1, L); L = 0 lays out one dP table as L = 1 does
    out = subprocess.run([str(exe)] + [str(v) for p in pairs for v in p], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(NODES) * len(EDGES) * (1 + len(pairs))
    for line in out:
        kind, f1, steps, n, e, *offs = line.split()
        n, e, offs = int(n), int(e), [int(v) for v in offs]
        want = prefix(post_terms(n, e)) if kind == "post" else prefix(bwd_terms(n, e, int(f1), int(steps)))
        assert offs == want, line
        assert all(o % 256 == 0 for o in offs)
