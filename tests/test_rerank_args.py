"""gnn_cca_amd.rerank, the parts that need no GPU: every refusal comes before a device is touched (host tensors stand in for the batch: a
check that came too late would raise the module's "MI355X only" RuntimeError instead), the native entries refuse before any launch (the
pointers are never followed), the float32 oracle (tests/rerank_oracle.py) reproduces every golden of tests/golden/rerank/ (made by
tests/golden/make_golden_rerank.py from the reference's libs.utils.re_ranking) within the tolerance the GPU is held to, and the integer
form of the 2/3 test decides as the reference's float64 expression does."""
import glob
import os

import numpy as np
import pytest
import torch

import rerank_oracle as oracle
from conftest import ROOT

GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "rerank", "*.npz")))


class _Batch:
    """What the module reads of a GraphBatch, on the host."""

    def __init__(self, sizes=(3, 2), e=8, width=4):
        self.node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        n = self.node_ptr[-1]
        self.edge_ptr = [0, e // 2, e][:len(sizes) + 1]
        self.edge_index = torch.zeros((2, e), dtype=torch.int64)
        self.edge_labels = torch.zeros(e)
        self.node_ptr_dev = torch.tensor(self.node_ptr, dtype=torch.int32)
        self.edge_ptr_dev = torch.tensor(self.edge_ptr, dtype=torch.int32)
        self.cam_dev = torch.zeros(n, dtype=torch.int32)
        self.reid_embeds = torch.zeros((n, width))


def _dist(sizes=(3, 2)):
    from gnn_cca_amd.rerank import FrameMatrices
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return FrameMatrices(torch.zeros(int(sum(s * s for s in sizes))), node_ptr)


def test_every_refusal_comes_before_the_gpu_is_touched():
    from gnn_cca_amd import rerank as rr
    b, d = _Batch(), _dist()
    assert rr.MAX_FRAME_NODES == 128 and rr.MAX_K1 == 64
    assert d.mat_ptr == [0, 9, 13] and d.frame(1).shape == (2, 2) and len(d) == 2
    for k1 in (0, -1, 65, 2.0, "20", None, True):
        with pytest.raises(ValueError, match="k1"):
            rr.rerank_frames(d, k1=k1)
        with pytest.raises(ValueError, match="k1"):
            rr.rank_baseline(b, k1=k1)
    for k1, k2 in ((20, 0), (20, 21), (5, 6), (20, 1.5), (20, None)):
        with pytest.raises(ValueError, match="k2"):
            rr.rerank_frames(d, k1=k1, k2=k2)
    for lam in (-0.1, 1.0001, float("nan"), float("inf"), "0.3", None, True):
        with pytest.raises(ValueError, match="lam"):
            rr.rerank_frames(d, lam=lam)
        with pytest.raises(ValueError, match="lam"):
            rr.rank_baseline(b, lam=lam)
    for rank in (0, -1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="rank"):
            rr.rank_predictions(b, d, rank=rank)
        with pytest.raises(ValueError, match="rank"):
            rr.rank_baseline(b, rank=rank)
    big_b, big_d = _Batch(sizes=(129, 2)), _dist(sizes=(129, 2))
    with pytest.raises(NotImplementedError, match="at most 128"):
        rr.rerank_frames(big_d)
    with pytest.raises(NotImplementedError, match="at most 128"):
        rr.rank_predictions(big_b, big_d)
    with pytest.raises(NotImplementedError, match="at most 128"):
        rr.rank_baseline(big_b)
    with pytest.raises(ValueError, match="disagree"):
        rr.rank_predictions(b, _dist(sizes=(2, 3)))          # the same N, other frames
    with pytest.raises(ValueError, match="disagree"):
        rr.rank_predictions(b, _dist(sizes=(3, 2, 1)))

    class Loose:
        """Anything with the three fields is a FrameMatrices."""

    loose = Loose()
    loose.data, loose.mat_ptr, loose.node_ptr = torch.zeros(13), [0, 9, 13], [0, 3, 5]
    with pytest.raises(RuntimeError, match="MI355X only"):
        rr.rerank_frames(loose)
    loose.mat_ptr = [0, 9, 12]
    with pytest.raises(ValueError, match="mat_ptr"):
        rr.rerank_frames(loose)
    loose.mat_ptr, loose.data = [0, 9, 13], torch.zeros(12)
    with pytest.raises(ValueError, match="13 elements"):
        rr.rank_predictions(b, loose)
    with pytest.raises(ValueError, match="fields"):
        rr.rerank_frames(object())
    with pytest.raises(ValueError):
        rr.FrameMatrices(torch.zeros(12), [0, 3, 5])
    narrow = _Batch()
    narrow.reid_embeds = torch.zeros((5, 0))
    with pytest.raises(ValueError, match="reid_embeds"):
        rr.frame_distances(narrow)
    no_cam = _Batch()
    del no_cam.cam_dev
    with pytest.raises(ValueError, match="cam_dev"):
        rr.rank_predictions(no_cam, d)
    # what is left is a well-formed call on host tensors: the module's usual refusal, at the limits of every argument
    for call in (lambda: rr.frame_distances(b), lambda: rr.rerank_frames(d), lambda: rr.rerank_frames(d, k1=64, k2=64, lam=1),
                 lambda: rr.rerank_frames(d, k1=1, k2=1, lam=0), lambda: rr.rerank_frames(_dist(sizes=(128,)), debug=True),
                 lambda: rr.rank_predictions(b, d), lambda: rr.rank_predictions(b, d, rank=10 ** 12), lambda: rr.rank_baseline(b),
                 lambda: rr.rank_baseline(b, rerank=False, k1=None)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()


def test_native_entries_refuse_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000
    assert nat.RERANK_MAX_FRAME_NODES == 128 and nat.RERANK_MAX_K1 == 64
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    assert "#define GNNCCA_RERANK_MAX_FRAME_NODES 128" in header and "#define GNNCCA_RERANK_MAX_K1 64" in header
    # the largest legal configuration fits the 160 KiB a workgroup may take; a Terrace-sized frame leaves room for several per CU
    assert 0 < lib.gnncca_rerank_lds_bytes(128, 64, 64) <= 160 * 1024
    assert lib.gnncca_rerank_lds_bytes(128, 20, 6) <= lib.gnncca_rerank_lds_bytes(128, 64, 64)
    assert lib.gnncca_rerank_lds_bytes(34, 20, 6) <= 16 * 1024
    assert lib.gnncca_rerank_lds_bytes(129, 20, 6) == 0 and lib.gnncca_rerank_lds_bytes(34, 65, 6) == 0

    def rerank(k1=20, k2=6, lam=0.3, max_n=6, dist=fake, nptr=fake, out=fake, n=10, g=2, total=52, rank_out=None, cols=0):
        return lib.gnncca_rerank_frames(dist, total, n, nptr, g, max_n, k1, k2, lam, out, rank_out, cols, None, None)

    for kw in (dict(k1=0), dict(k1=65), dict(k2=0), dict(k2=21), dict(lam=-0.5), dict(lam=1.5), dict(lam=float("nan")), dict(n=-1), dict(g=-1),
               dict(total=-1), dict(max_n=-1), dict(max_n=11), dict(dist=None), dict(nptr=None), dict(out=None), dict(rank_out=fake, cols=0)):
        assert rerank(**kw) == nat.ERR_INVALID_ARG, kw
    assert rerank(max_n=129, n=200) == nat.ERR_UNSUPPORTED
    assert rerank(g=0, nptr=None, dist=None, out=None) == nat.OK      # nothing to do: nothing launched

    def distances(x=fake, dim=4, n=10, nptr=fake, g=2, max_n=6, total=52, out=fake):
        return lib.gnncca_frame_distances(x, dim, n, nptr, g, max_n, total, out, None)

    for kw in (dict(dim=0), dict(dim=-3), dict(n=-1), dict(g=-1), dict(total=-1), dict(max_n=11), dict(x=None), dict(nptr=None), dict(out=None)):
        assert distances(**kw) == nat.ERR_INVALID_ARG, kw
    assert distances(g=0, nptr=None, x=None, out=None) == nat.OK

    def predict(rank=1, max_n=6, dist=fake, cam=fake, ei=fake, nptr=fake, eptr=fake, pred=fake, n=10, e=24, g=2, total=52):
        return lib.gnncca_rank_predictions(dist, total, cam, n, ei, e, nptr, eptr, g, max_n, rank, pred, None)

    for kw in (dict(rank=0), dict(rank=-2), dict(n=-1), dict(e=-1), dict(g=-1), dict(total=-1), dict(dist=None), dict(cam=None), dict(ei=None),
               dict(nptr=None), dict(eptr=None), dict(pred=None)):
        assert predict(**kw) == nat.ERR_INVALID_ARG, kw
    assert predict(max_n=129, n=200) == nat.ERR_UNSUPPORTED
    assert predict(e=0, ei=None, pred=None) == nat.OK


def test_integer_form_of_the_two_thirds_test():
    """The reference writes len(intersection) > 2./3*len(candidate set) in float64; the kernel and the oracle test 3 a > 2 b.  The sets
    have at most k1 + 1 <= 65 members."""
    for b in range(66):
        for a in range(b + 1):
            assert (3 * a > 2 * b) == (a > 2. / 3 * b), (a, b)
    assert [oracle.half(k) for k in (1, 4, 5, 7, 20, 64)] == [1, 3, 3, 5, 11, 33]      # round half to even: 2.5 -> 2, 3.5 -> 4


def test_goldens_are_complete_and_tie_free():
    assert len(GOLDEN) >= 8
    d_ref = {float(np.load(p)["d_ref"]) for p in GOLDEN}
    assert len(d_ref) == 1 and 1e-8 < d_ref.pop() < 2e-6
    assert max(float(np.load(p)["err_ref"]) for p in GOLDEN) == float(np.load(GOLDEN[0])["d_ref"])
    eventful = 0
    for p in GOLDEN:
        z = np.load(p)
        D, k1, n = z["D"], int(z["k1"]), z["D"].shape[0]
        assert D.dtype == np.float32 and np.array_equal(D, D.T) and not D.diagonal().any() and z["ref"].dtype == np.float32
        assert z["offdiag"].sum() == n * n - n and os.path.getsize(p) < 64 * 1024
        _, dbg = oracle.rerank(D, k1, int(z["k2"]), float(z["lam"]), np.float32, debug=True)
        head = np.sort(dbg["O"], axis=1)[:, :k1 + 2]
        assert (np.diff(head, axis=1) > 0).all(), p       # no row of float32 O has a tie among its first k1 + 2 values
        assert [dbg["accepted"], dbg["rejected"], dbg["enlarged"]] == z["events"].tolist()
        eventful += int(min(z["events"]) > 0)
        assert z["rank_gaps"].min() > 8 * float(z["d_ref"])
    assert eventful >= 3


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_float32_oracle_reproduces_the_golden(path):
    """Held to the GPU's tolerance: 4 d_ref against the float64 oracle, and the float64 oracle agrees with the reference's float32 result
    to d_ref by the fixture's own record."""
    z = np.load(path)
    D, k1, k2, lam, off = z["D"], int(z["k1"]), int(z["k2"]), float(z["lam"]), z["offdiag"]
    tol = 4 * float(z["d_ref"])
    want64, d64 = oracle.rerank(D, k1, k2, lam, np.float64, debug=True)
    got32, d32 = oracle.rerank(D, k1, k2, lam, np.float32, debug=True)
    assert got32.dtype == np.float32
    err_ref = np.abs(z["ref"].astype(np.float64) - want64)[off].max()
    assert abs(err_ref - float(z["err_ref"])) <= 1e-12 and float(z["err_ref"]) <= float(z["d_ref"])   # (1e-12: another libm's fp64 exp)
    assert np.abs(got32.astype(np.float64) - want64).max() <= tol
    assert np.abs(got32.astype(np.float64) - z["ref"].astype(np.float64))[off].max() <= tol + float(z["d_ref"])
    # the discrete structure does not depend on the width
    assert np.array_equal(d32["rank"][:, :d32["prefix"]], d64["rank"][:, :d64["prefix"]])
    assert np.array_equal(d32["expansion"], d64["expansion"]) and np.array_equal(d32["support"], d64["support"])
    if lam == 1.0:
        assert np.array_equal(got32, d32["O"])
    # the rank-R selection from the reference's matrix is the oracle's
    ref = np.where(off, z["ref"], 0)
    for r in z["ranks"].tolist():
        assert np.array_equal(oracle.select(ref, z["cam"], r), oracle.select(want64, z["cam"], r))
        assert np.array_equal(oracle.select(ref, z["cam"], r), oracle.select(got32, z["cam"], r))
