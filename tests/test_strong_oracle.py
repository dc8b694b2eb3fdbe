"""Clusters without pruning (PRUNING: False), the parts that need no GPU.

  * the oracle (oracle/post_oracle.py: clusters = scipy's strongly connected components; finalize(pruning_on=False)) against
    tests/golden/post_unpruned.npz, produced by the reference's own functions through inference.py's own lines
    (tests/golden/make_golden_post_unpruned.py): predictions exact, partitions equal;
  * the product's host pass (csrc/post_host.cpp: gnncca_post_finalize_frame_host) WITHOUT the pruning switch against the same golden;
  * a numpy restatement of the kernel's in-place repeated squaring: the partition it gives, and the bound on its rounds;
  * the entry point declared, bound and exported; every refusal of strong_clusters / finalize / FramePipeline before a device is touched
    (host tensors stand in: a check that came too late would raise the module's "MI355X only" RuntimeError instead), and the C entry's
    GNNCCA_ERR_INVALID_ARG returns, which come before any launch."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from oracle import post_oracle as po

Z = np.load(os.path.join(GOLDEN_DIR, "post_unpruned.npz"))
NAMES = [str(n) for n in Z["names"]]
NOISY = [n for n in NAMES if re.search(r"_s\d+$", n)]


def case(name):
    g = lambda k: Z[f"{name}::{k}"]   # noqa: E731
    return int(g("n_nodes")), g("edge_index"), g("logits"), g("probs"), g


# ---- 1. the oracle against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_the_reference_without_pruning(name):
    n, ei, logits, probs, g = case(name)
    assert np.abs(po.threshold(logits)[0] - probs).max() <= 2e-7      # the sigmoid itself: an ulp of float32
    thresholded = (probs >= 0.5).astype(np.int64)
    assert np.array_equal(thresholded, g("pred_unpruned"))            # nothing is pruned
    labels, k = po.clusters(ei, thresholded, n)
    assert po.same_partition(labels, g("id_unpruned")) and k == len(set(g("id_unpruned").tolist()))
    assert all(labels[v] == min(u for u in range(n) if labels[u] == labels[v]) for v in range(n))   # the label convention
    for tag, rounding in (("unpruned", False), ("rounded", True)):
        _, pred, ids, kk = po.finalize(ei, logits, n, rounding_on=rounding, pruning_on=False, splitting_on=False, probs=probs)
        assert np.array_equal(pred, g("pred_" + tag)), (name, tag)
        assert po.same_partition(ids, g("id_" + tag)) and kk == len(set(g("id_" + tag).tolist())), (name, tag)


def test_the_golden_is_worth_having():
    assert len(NAMES) == 26 and len(NOISY) == 18
    differs = changed = 0
    for name in NOISY:
        n, ei, _, probs, g = case(name)
        thresholded = (probs >= 0.5).astype(np.int64)
        differs += not po.same_partition(po.clusters(ei, po.prune(ei, thresholded), n)[0], g("id_unpruned"))
        changed += not np.array_equal(g("pred_rounded"), g("pred_unpruned"))
    assert 2 * differs >= len(NOISY) and changed >= 1
    # the hand-made frames: what each is there for
    size = lambda nm: int(np.bincount(case(nm)[4]("id_unpruned")).max())   # noqa: E731
    assert size("cycle3_no_mutual_pair") == 3 and size("chain4") == 1 and size("two_cycles_share_a_node") == 5
    assert size("cycle_with_tails") == 3 and size("cycle5") == 5 and size("hub_four_out") == 1 and size("nothing_active") == 1
    n, ei, _, probs, g = case("mutual_pairs_only")
    pred = (probs >= 0.5).astype(np.int64)
    assert np.array_equal(po.prune(ei, pred), pred) and po.same_partition(po.clusters(ei, pred, n)[0], g("id_unpruned"))
    n, ei, _, probs, g = case("cycle3_no_mutual_pair")
    assert po.prune(ei, (probs >= 0.5).astype(np.int64)).sum() == 0        # the pruned chain sees three singletons there


# ---- 5. the native host pass without the pruning switch -------------------------------------------------------------------------------
def native_finalize(n, ei, probs, pred_in, switches, base=0):
    from gnn_cca_amd import _native as nat
    src, dst = np.ascontiguousarray(ei[0] + base), np.ascontiguousarray(ei[1] + base)
    pr = np.ascontiguousarray(probs, dtype=np.float32)
    pred = np.ascontiguousarray(pred_in, dtype=np.int64).copy()
    labels, ids, k = np.zeros(n, np.int32), np.zeros(n, np.int64), C.c_int32(0)
    st = nat.lib().gnncca_post_finalize_frame_host(src.ctypes.data, dst.ctypes.data, base, n, ei.shape[1], pr.ctypes.data, pred.ctypes.data,
                                                   switches, labels.ctypes.data, C.byref(k), ids.ctypes.data)
    assert st == 0
    return pred, ids, labels, int(k.value)


@pytest.mark.parametrize("name", NAMES)
def test_host_implementation_matches_the_reference_without_pruning(name):
    from gnn_cca_amd import _native as nat
    n, ei, _, probs, g = case(name)
    thresholded = (probs >= 0.5).astype(np.int64)
    for tag, sw in (("unpruned", 0), ("rounded", nat.POST_ROUNDING)):
        for base in (0, 1000):
            pred, ids, labels, k = native_finalize(n, ei, probs, thresholded, sw, base)
            assert np.array_equal(pred, g("pred_" + tag)), (name, tag)
            assert np.array_equal(ids, g("id_" + tag)), (name, tag)              # the reference's label numbering too
            assert k == len(set(ids.tolist())) and po.same_partition(labels, ids)
            assert all(labels[v] == base + min(u for u in range(n) if ids[u] == ids[v]) for v in range(n))


# ---- the kernel's closure, restated ---------------------------------------------------------------------------------------------------
def squaring(n, src, dst):
    """csrc/strong.cuh in numpy: the reachability matrix with the diagonal set, squared in place row by row (row i ORs in every row j
    whose bit is set in row i, reading rows that may already be this round's) under the kernel's counted loop.
    -> (labels: the smallest u with R[v][u] and R[u][v], number of rounds that changed something, rounds run, the bound)."""
    R = np.eye(n, dtype=bool)
    R[src, dst] = True
    n_pad = (n + 31) // 32 * 32
    bound = (math.ceil(math.log2(n_pad)) if n_pad > 1 else 0) + 1
    changing = run = 0
    for _ in range(bound):
        run += 1
        changed = False
        for i in range(n):
            new = R[R[i]].any(axis=0)
            if (new != R[i]).any():
                R[i], changed = new, True
        if not changed:
            break
        changing += 1
    both = R & R.T
    return both.argmax(axis=1), changing, run, bound


def test_in_place_squaring_gives_the_components_within_its_bound():
    rng = np.random.default_rng(5)
    for trial in range(120):
        n = int(rng.integers(1, 70))
        e = int(rng.integers(0, 3 * n + 1))
        src, dst = rng.integers(0, n, size=e), rng.integers(0, n, size=e)
        labels, changing, run, bound = squaring(n, src, dst)
        want, _ = po.clusters(np.stack([src, dst]), np.ones(e, np.int64), n)
        assert np.array_equal(labels, want), trial
        assert changing < bound, trial               # the last round run changed nothing, or the bound's last round was not needed
    for name in NOISY:                               # the noisy frames take at most 4 changing rounds
        n, ei, _, probs, _ = case(name)
        act = probs >= 0.5
        labels, changing, _, _ = squaring(n, ei[0][act], ei[1][act])
        assert np.array_equal(labels, po.clusters(ei, act.astype(np.int64), n)[0]) and changing <= 4, name


@pytest.mark.parametrize("n", [32, 33, 64, 256])
def test_a_directed_ring_is_the_worst_case_and_stays_inside_the_bound(n):
    """Rows are processed in ascending order and row i of a ring reads row i + 1, which this round has not touched yet: the in-place form
    gains nothing here and behaves as the two-buffer form does.  At most ceil(log2(n_pad)) rounds change something, one more detects it."""
    src = np.arange(n)
    labels, changing, run, bound = squaring(n, src, (src + 1) % n)
    assert labels.tolist() == [0] * n
    assert changing <= bound - 1 and run <= bound
    labels, changing, _, _ = squaring(n, src[:-1], src[1:])           # an ascending path: all singletons
    assert labels.tolist() == list(range(n)) and changing <= bound - 1


# ---- 2. header, binding, export -------------------------------------------------------------------------------------------------------
def _declaration(header, name, result="int"):
    m = re.search(r"GNNCCA_API\s+" + result + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_point_and_the_binding_mirrors_it():
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd import postprocess
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    lib = nat.lib()
    args = _declaration(header, "gnncca_post_strong_frames")
    res, argtypes = nat._SIGNATURES["gnncca_post_strong_frames"]
    assert len(args) == 15 == len(argtypes) and res is C.c_int
    assert "gnncca_post_strong_frames" in nat.exported_symbols() and hasattr(lib, "gnncca_post_strong_frames")
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "edge_index", "predictions", "n_nodes", "n_edges", "node_ptr_dev", "edge_ptr_dev", "n_frames", "max_frame_nodes", "flow_out", "flow_in",
        "labels_out", "n_clusters_out", "triggers_out", "flags_out", "stream"]
    assert argtypes[2] is C.c_int64 and argtypes[3] is C.c_int64 and argtypes[6] is C.c_int32 and argtypes[7] is C.c_int32
    assert "#define GNNCCA_STRONG_MAX_FRAME_NODES 1024" in header and nat.STRONG_MAX_FRAME_NODES == 1024 == postprocess.STRONG_MAX_FRAME_NODES
    assert "#define GNNCCA_STRONG_BAD_RANGE 2u" in header and nat.STRONG_BAD_RANGE == 2
    assert "#define GNNCCA_ABI_VERSION 2" in header and nat.ABI_VERSION == 2 == lib.gnncca_abi_version()
    for word in ("active", "reachability", "rounds", "ceil(log2(n_pad)) + 1", "strongly connected", "smallest batch-global node id"):
        assert word in header, word
    assert callable(postprocess.strong_clusters)


# ---- 3. every host-side refusal, no device touched ------------------------------------------------------------------------------------
def test_every_value_error_comes_before_the_gpu_is_touched():
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.postprocess import finalize, strong_clusters
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    pred = torch.ones(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="go together"):
        strong_clusters(ei, pred, 3, [0, 3], None)
    with pytest.raises(ValueError, match="go together"):
        strong_clusters(ei, pred, 3, None, [0, 4])
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        strong_clusters(ei.t(), pred, 3, [0, 3], [0, 4])
    with pytest.raises(ValueError, match="does not match"):
        strong_clusters(ei, pred[:3], 3, [0, 3], [0, 4])
    with pytest.raises(ValueError, match=r"G \+ 1"):
        strong_clusters(ei, pred, 3, [0, 1, 3], [0, 4])
    with pytest.raises(ValueError, match=r"G \+ 1"):
        strong_clusters(ei, pred, 3, [0], [0])
    with pytest.raises(ValueError, match=r"G \+ 1"):
        strong_clusters(ei, pred, 3, torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 2, 4], dtype=torch.int32))
    with pytest.raises(ValueError, match="ascend"):
        strong_clusters(ei, pred, 3, [0, 2], [0, 4])
    with pytest.raises(ValueError, match="ascend"):
        strong_clusters(ei, pred, 3, [1, 3], [0, 4])
    with pytest.raises(ValueError, match="ascend"):
        strong_clusters(ei, pred, 3, [0, 2, 1, 3], [0, 4, 4, 4])
    with pytest.raises(ValueError, match="ascend"):
        strong_clusters(ei, pred, 3, [0, 3], [0, 3])
    none = torch.zeros((2, 0), dtype=torch.int64)
    with pytest.raises(ValueError, match="at most 1024"):
        strong_clusters(none, torch.zeros(0, dtype=torch.int64), 1025, [0, 1025], [0, 0])
    with pytest.raises(ValueError, match="at most 1024"):
        strong_clusters(none, torch.zeros(0, dtype=torch.int64), 1030, [0, 5, 1030], [0, 0, 0])
    with pytest.raises(ValueError, match="at most 1024"):          # no frame ranges: the whole graph is the frame
        strong_clusters(none, torch.zeros(0, dtype=torch.int64), 1025)
    for bad in (-1, 1025):
        with pytest.raises(ValueError, match="max_frame_nodes"):
            strong_clusters(ei, pred, 3, torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32), max_frame_nodes=bad)
    # what is left is a well-formed call on host tensors: the module's usual refusal
    for args in ((ei, pred, 3, [0, 3], [0, 4]), (ei, pred.view(-1, 1), 3), (ei, pred, 3, [0, 1, 3], [0, 0, 4]),
                 (ei, pred, 3, torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32)),
                 (none, torch.zeros(0, dtype=torch.int64), 1024, [0, 1024], [0, 0])):
        with pytest.raises(RuntimeError, match="MI355X only"):
            strong_clusters(*args)
    # SPLITTING without PRUNING: the reference has no behaviour there, and the message says why
    with pytest.raises(ValueError, match="reference itself has no behaviour") as info:
        finalize(ei, None, pred, None, None, None, pruning=False, splitting=True)
    assert "disjoint_big_clusters" in str(info.value) and "reverse" in str(info.value)
    with pytest.raises(ValueError, match="reference itself has no behaviour"):
        FramePipeline(object(), pruning=False)                     # splitting defaults to True
    with pytest.raises(ValueError, match="reference itself has no behaviour"):
        FramePipeline(object(), pruning=False, splitting=True, rounding=False)
    pipe = FramePipeline(object(), pruning=False, splitting=False)  # no longer refused; nothing is touched at construction
    assert pipe.switches == (True, False, False)
    assert FramePipeline(object(), rounding=False, pruning=False, splitting=False).switches == (False, False, False)
    assert FramePipeline(object()).switches == (True, True, True)  # the default stays as it was


# ---- 4. the C entry's refusals ---------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000
    n, e, g = 10, 24, 2

    def call(max_n=6, ei=fake, pred=fake, nptr=fake, eptr=fake, fo=fake, fi=fake, lab=fake, k=fake, trig=fake, fl=fake, nn=n, ee=e, gg=g):
        return lib.gnncca_post_strong_frames(ei, pred, nn, ee, nptr, eptr, gg, max_n, fo, fi, lab, k, trig, fl, None)

    assert call(max_n=1025) == nat.ERR_INVALID_ARG and call(max_n=-1) == nat.ERR_INVALID_ARG and call(max_n=n + 1) == nat.ERR_INVALID_ARG
    for name in ("ei", "pred", "nptr", "eptr", "fo", "fi", "lab", "k", "trig", "fl"):
        assert call(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert call(nn=-1) == nat.ERR_INVALID_ARG and call(ee=-1) == nat.ERR_INVALID_ARG and call(gg=-1) == nat.ERR_INVALID_ARG
    assert call(gg=0) == nat.ERR_INVALID_ARG                        # frame ranges, but no frame
    assert call(nptr=None, eptr=None) == nat.ERR_INVALID_ARG        # frames, but no ranges
    assert call(nptr=None, eptr=None, gg=0, max_n=n + 1) == nat.ERR_INVALID_ARG   # the whole graph as one frame: the same bound
    assert call(nn=0, max_n=1) == nat.ERR_INVALID_ARG               # max_frame_nodes above n_nodes
    assert call(nn=2000, max_n=1025) == nat.ERR_INVALID_ARG
