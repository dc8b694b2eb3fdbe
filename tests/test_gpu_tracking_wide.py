"""The four FrameLinker modes on the GPU with WIDE appearance rows, ids exactly against the existing oracles.  A pair's cosine is summed by
a whole wave, lane k taking the columns k, k + 64, ...; the walk of motion='velocity' keeps four such loads in flight and has a remainder
loop.  The other linker tests use 4, 8 or 16 columns, where no lane ever takes a second column.  Here R is 1, 64, 65, 200, 257 and 600:
the widths at which the strided loop, the four-deep loop and its remainder each start or stop running for some lanes.  And a case made
by hand in which ONE column (the last of the row, the last a four-deep pass takes, the first the remainder takes) decides an id.
Every case first asserts, on the ORACLE's numbers, that it exercises what it is about."""
import functools

import numpy as np
import pytest
import torch

import tracking_assign_oracle as ta
import tracking_gap_oracle as tg
import tracking_motion_oracle as tm
import tracking_oracle as to

pytestmark = pytest.mark.gpu

WIDTHS = (1, 64, 65, 200, 257, 600)
MODES = ("adjacent", "gap", "optimal", "motion")
FIELDS = ("cluster_track", "node_track", "matched_prev", "matched_gap")
LAM = 1.0   # with max_cos = None: the cosine decides costs, not only admissibility


def _upload(summ):
    from gnn_cca_amd.tracking import ClusterSummaries
    ptr = np.asarray(summ["node_ptr"], np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    ones = np.ones(len(summ["rank"]), np.int32)
    return ClusterSummaries(t(summ["count"]), t(summ["rank"]), t(ones), t(ones), t(summ["pos"]), t(summ["emb"]), ptr.tolist(),
                            t(ptr.astype(np.int32)))


def _same_tracks(t, want):
    torch.cuda.synchronize()
    for k in FIELDS + ("velocity",):
        if k in want:
            got, ref = getattr(t, k).cpu(), torch.from_numpy(want[k])
            assert got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got, ref), k
    assert t.next_id.dtype == torch.int64 and int(t.next_id.item()) == want["next_id"]


def _linker(mode, max_step, max_gap):
    """The linker of a mode; max_gap: the gap of the modes that take any ('gap' itself needs one above 0)."""
    from gnn_cca_amd.tracking import FrameLinker
    if mode == "adjacent":
        return FrameLinker(max_step, lam=LAM)
    if mode == "gap":
        return FrameLinker(max_step, lam=LAM, max_gap=max_gap)
    if mode == "optimal":
        return FrameLinker(max_step, lam=LAM, max_gap=max_gap, matching="optimal")
    return FrameLinker(max_step, lam=LAM, max_gap=max_gap, motion="velocity")


def _oracle(mode, summ, max_step, max_gap):
    """-> (the oracle's tracks, the smallest margins any of its decisions hangs on)."""
    ptr = summ["node_ptr"]
    if mode == "adjacent":
        return to.link(summ, ptr, max_step, LAM, None)[0], to.margins(summ, ptr, max_step, LAM, None)
    if mode == "gap":
        return tg.link_gap(summ, ptr, max_step, LAM, None, max_gap)[0], tg.margins_gap(summ, ptr, max_step, LAM, None, max_gap)
    if mode == "optimal":   # (as in test_gpu_tracking_optimal.py: the gates; two sets of pairs with totals within 1e-9 do not occur in random data)
        gd = np.inf
        for k, t, d, dcos, cost, ok in ta.level_tables(summ, ptr, max_step, LAM, None, max_gap):
            gd = min(gd, float(np.abs(d - np.float64(max_step) * np.float64(k + 1)).min()))
        return ta.link_gap(summ, ptr, max_step, LAM, None, max_gap, matching="optimal")[0], (gd,)
    return tm.link_motion(summ, ptr, max_step, LAM, None, max_gap)[0], tm.margins_motion(summ, ptr, max_step, LAM, None, max_gap)


# ---- 1. random sequences --------------------------------------------------------------------------------------------------------------
RANDOM = dict(adjacent=(1.0, 0), gap=(1.0, 2), optimal=(1.0, 1), motion=(0.4, 2))   # mode -> max_step, max_gap


@functools.lru_cache(maxsize=None)
def random_case(mode, r):
    rng = np.random.default_rng(100 + r)
    if mode == "adjacent":
        summ = to.walk_sequence(rng, 6, 25, r, noise=0.3, p_leave=0.1, p_enter=0.5, arena=8.0)
    elif mode == "motion":
        summ = tm.cross_sequence(rng, 6, 25, r, speed=(0.3, 0.6), noise=0.05, p_hide=0.12, max_hide=3, arena=6.0)
    else:
        summ = tg.hide_sequence(rng, 6, 25, r, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=3, arena=8.0)
    max_step, max_gap = RANDOM[mode]
    want, gaps = _oracle(mode, summ, max_step, max_gap)
    print("margins:", gaps, "clusters per frame:", summ["count"].tolist())
    assert all(v > 1e-9 for v in gaps), gaps
    assert (want["matched_prev"] >= 0).sum() > 20 and (want["matched_prev"][summ["node_ptr"][1]:] < 0).any()
    return summ, want


@pytest.mark.parametrize("r", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_wide_rows_link_as_the_oracle_says(mode, r):
    summ, want = random_case(mode, r)
    _same_tracks(_linker(mode, *RANDOM[mode])(_upload(summ)), want)


# ---- 2. one column decides --------------------------------------------------------------------------------------------------------------
SENTINELS = [(65, 64, 0), (200, 199, 0), (257, 256, 3), (600, 511, 3), (600, 599, 3)]   # R, the deciding column j, a second column q


def sentinel(r, j, q, lose=False):
    """B0 = (0, 0.3) and B1 = (0, -0.3) in frame 0, A = (0.1, 0) in frame 1: the two distances are bit-equal.  emb(B0) = e_q, emb(B1) =
    emb(A) = e_j + e_q, so A continues B1 -- and if column j is lost (lose: zeroed) on either side the three cosines tie and B0 wins."""
    emb = np.zeros((3, r), np.float32)
    emb[:, q] = 1.0
    if not lose:
        emb[1:, j] = 1.0
    return dict(count=np.array([2, 1], np.int32), rank=np.array([0, 1, 0], np.int32), pos=np.array([[0.0, 0.3], [0.0, -0.3], [0.1, 0.0]]),
                emb=emb, node_ptr=np.array([0, 2, 3], np.int64))


@pytest.mark.parametrize("r,j,q", SENTINELS)
@pytest.mark.parametrize("mode", MODES)
def test_one_column_decides_an_id(mode, r, j, q):
    summ = sentinel(r, j, q)
    max_gap = 1 if mode == "gap" else 0
    want, gaps = _oracle(mode, summ, 1.0, max_gap)
    assert all(v > 1e-9 for v in gaps), gaps
    assert want["matched_prev"].tolist() == [-1, -1, 1] and want["cluster_track"].tolist() == [0, 1, 1]
    lost = sentinel(r, j, q, lose=True)
    assert to.link(lost, lost["node_ptr"], 1.0, LAM, None)[0]["matched_prev"].tolist() == [-1, -1, 0]   # what a dropped column would give
    _same_tracks(_linker(mode, 1.0, max_gap)(_upload(summ)), want)
