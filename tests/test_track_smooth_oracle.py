"""tests/track_smooth_oracle.py (the rule of gnn_cca_amd.smoothing.TrackSmoother as numpy loops) against what a constant-velocity Kalman
filter must do, and the host side of the stage, all without a GPU: a noise-free straight walk, the closed-form covariance of recursive
least squares, independence of how a sequence is cut into calls, time stamps, the error against noise-free positions on synthetic noisy
walks, the refusals of TrackSmoother and the argument checks of gnncca_track_smooth (placeholder pointers: they come before any launch)."""
import numpy as np
import pytest

import track_smooth_oracle as so
import tracking_gap_oracle as tg
import tracking_motion_oracle as tm
import tracking_time_oracle as tt

F = np.float64
KEYS = ("pos", "vel", "cov", "nis", "age")


def one_walker(points, size=None):
    """One single-cluster frame per point, linked frame to frame: the summaries and the links a linker would give."""
    n = len(points)
    summ = dict(count=np.ones(n, np.int32), rank=np.zeros(n, np.int32), size=np.ones(n, np.int32) if size is None else np.asarray(size, np.int32),
                pos=np.array(points, F).reshape(n, 2), node_ptr=np.arange(n + 1, dtype=np.int64))
    links = dict(matched_prev=np.array([-1] + [0] * (n - 1), np.int32), matched_gap=np.array([-1] + [0] * (n - 1), np.int32))
    return summ, links


def same(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def hidden_sequence(max_gap, seed):
    """12 frames of at most 12 clusters with occlusions, and the links of the linker oracle; every level 0 .. max_gap links somebody."""
    rng = np.random.default_rng(seed)
    summ = tg.hide_sequence(rng, 12, 10, 16, noise=0.3, p_leave=0.05, p_enter=0.3, p_hide=0.2 if max_gap else 0.0, max_hide=max(max_gap, 1), arena=8.0,
                            max_alive=12)
    links, _ = tt.link_timed(summ, summ["node_ptr"], np.arange(12), 0.6, lam=1.0, max_gap=max_gap)
    assert summ["count"].max() <= 12 and all((links["matched_gap"] == k).any() for k in range(max_gap + 1))
    return summ, links


def in_calls(summ, links, cuts, max_gap, times=None, **kw):
    """The oracle over the calls [cuts[i], cuts[i + 1]) -> (the outputs joined, the final state)."""
    ptr = np.asarray(summ["node_ptr"], np.int64)
    parts, state = [], None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v0, v1 = int(ptr[lo]), int(ptr[hi])
        part = {k: links[k][v0:v1] for k in ("matched_prev", "matched_gap")}
        sub = dict(tg.frames_of(summ, lo, hi))
        out, state = so.smooth(sub, sub["node_ptr"], part, max_gap=max_gap, times=None if times is None else times[lo:hi], state=state, **kw)
        parts.append(out)
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}, state


# ---- 1. a noise-free straight walk --------------------------------------------------------------------------------------------------------
def test_a_noise_free_straight_walk_gives_the_true_velocity():
    u = np.array([0.5, -0.25])
    pts = [np.array([1.0, 2.0]) + t * u for t in range(6)]   # dyadic numbers: every operation below is exact
    summ, links = one_walker(pts)
    # a measurement variance that vanishes beside vel_var (2r + V == V in fp64): the first link sets the velocity exactly
    out, _ = so.smooth(summ, summ["node_ptr"], links, q=0.0, r=2.0 ** -80, vel_var=1.0)
    assert out["age"].tolist() == [0, 1, 2, 3, 4, 5] and out["nis"][0] == 0.0
    assert np.array_equal(out["vel"][0], [0.0, 0.0]) and np.array_equal(out["vel"][1:], np.tile(u, (5, 1)))
    assert np.array_equal(out["pos"], np.array(pts)) and np.array_equal(out["nis"][2:], np.zeros(4)) and out["nis"][1] > 0
    # ordinary numbers: r / vel_var = 1e-8, so the gains differ from 1 by about 1e-8 and so do the velocity and the next prediction
    out, _ = so.smooth(summ, summ["node_ptr"], links, q=0.0, r=1e-4, vel_var=1e4)
    assert np.abs(out["vel"][1:] - u).max() < 1e-7 and out["nis"][2:].max() < 1e-10
    assert np.isclose(out["nis"][1], (u @ u) / (2e-4 + 1e4), rtol=1e-12)   # the first link: the whole step is innovation, s = (r + V) + r


# ---- 2. q = 0, equal dt: recursive least squares ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,v", [(0.0025, 1.0), (0.5, 3.0), (2.0, 0.1)])
def test_without_process_noise_the_covariance_is_least_squares(r, v):
    summ, links = one_walker(np.random.default_rng(0).normal(size=(4, 2)))
    out, _ = so.smooth(summ, summ["node_ptr"], links, q=0.0, r=r, vel_var=v)
    assert np.array_equal(out["cov"][0], [r, 0.0, v])
    for n in (1, 2, 3):   # n links: measurements at times 0 .. n of (p_n, vel), z_j = p_n - (n - j) vel + noise; the prior 1 / v on vel
        s0, s1, s2 = n + 1, n * (n + 1) / 2, n * (n + 1) * (2 * n + 1) / 6
        info = np.array([[s0 / r, -s1 / r], [-s1 / r, s2 / r + 1 / v]])
        want = np.linalg.inv(info)
        assert np.allclose(out["cov"][n], [want[0, 0], want[0, 1], want[1, 1]], rtol=1e-11, atol=0), (n, out["cov"][n], want)


# ---- 3. the result does not depend on how a sequence is cut into calls --------------------------------------------------------------------
@pytest.mark.parametrize("max_gap,seed", [(0, 1), (2, 2)])
@pytest.mark.parametrize("per_detection", [False, True])
def test_cutting_a_sequence_into_calls_changes_nothing(max_gap, seed, per_detection):
    summ, links = hidden_sequence(max_gap, seed)
    summ["size"] = (1 + np.arange(len(summ["rank"])) % 3).astype(np.int32)
    kw = dict(q=0.01, r=0.09, vel_var=1.0, per_detection=per_detection)
    whole, end = so.smooth(summ, summ["node_ptr"], links, max_gap=max_gap, **kw)
    assert whole["age"].max() >= 3 and (whole["age"] == 0).sum() > 10 and len(end["frames"]) == max_gap + 1
    for cuts in (list(range(13)), [0, 5, 10, 12], [0, 12]):
        got, state = in_calls(summ, links, cuts, max_gap, **kw)
        assert same(got, whole), cuts
        assert np.array_equal(so.state_image(state), so.state_image(end)), cuts
    image = so.state_image(end)
    rows = sum(f["rows"] for f in end["frames"])
    assert image.dtype == np.uint8 and len(image) == 64 + 60 * rows and image[:4].view(np.int32)[0] == max_gap + 1
    if per_detection:
        plain, _ = so.smooth(summ, summ["node_ptr"], links, max_gap=max_gap, **dict(kw, per_detection=False))
        assert not np.array_equal(plain["pos"], whole["pos"])
        births = whole["age"] == 0
        assert np.array_equal(whole["cov"][births, 0], F(0.09) / summ["size"][births].astype(F))


# ---- 4. time stamps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap,seed", [(0, 1), (2, 2)])
def test_times_0_1_2_equal_the_untimed_result(max_gap, seed):
    summ, links = hidden_sequence(max_gap, seed)
    kw = dict(q=0.01, r=0.09, vel_var=1.0)
    plain, _ = so.smooth(summ, summ["node_ptr"], links, max_gap=max_gap, **kw)
    for cuts in ([0, 12], [0, 5, 10, 12], list(range(13))):
        timed, state = in_calls(summ, links, cuts, max_gap, times=np.arange(12, dtype=F), **kw)
        assert same(timed, plain), cuts
        assert [f["time"] for f in state["frames"]] == [F(t) for t in range(11 - max_gap, 12)]


def test_a_dropped_frame_changes_dt_as_stated():
    pts = [(0.0, 0.0), (0.5, 0.1), (1.6, 0.2), (2.0, 0.4)]
    summ, links = one_walker(pts)
    kw = dict(q=0.02, r=0.01, vel_var=1.0)
    out, _ = so.smooth(summ, summ["node_ptr"], links, times=[0.0, 1.0, 3.0, 4.25], **kw)
    x, age = np.array([0.0, 0.0, 0.0, 0.0, 0.01, 0.0, 1.0]), 0
    for row, dt in ((1, 1.0), (2, 2.0), (3, 1.25)):   # dt = T[t] - T[t - 1]: the hole of one period makes the second link's dt 2
        x, nis, age = so.step(x, age, pts[row], dt, 0.02, 0.01)
        assert np.array_equal(np.concatenate([out["pos"][row], out["vel"][row], out["cov"][row]]), x) and out["nis"][row] == nis and out["age"][row] == age
    blind, _ = so.smooth(summ, summ["node_ptr"], links, **kw)
    assert np.array_equal(blind["pos"][:2], out["pos"][:2]) and not np.array_equal(blind["pos"][2:], out["pos"][2:])
    # a link over a missed frame (k = 1): dt = 2 without time stamps, T[t] - T[t - 2] with them
    summ2 = dict(summ, count=np.array([1, 0, 1], np.int32), pos=np.array([pts[0], pts[2]]), rank=np.zeros(2, np.int32), size=np.ones(2, np.int32),
                 node_ptr=np.array([0, 1, 1, 2], np.int64))
    links2 = dict(matched_prev=np.array([-1, 0], np.int32), matched_gap=np.array([-1, 1], np.int32))
    for times, dt in ((None, 2.0), ([0.0, 0.75, 2.5], 2.5)):
        got, _ = so.smooth(summ2, summ2["node_ptr"], links2, max_gap=1, times=times, **kw)
        want, nis, _ = so.step([0.0, 0.0, 0.0, 0.0, 0.01, 0.0, 1.0], 0, pts[2], dt, 0.02, 0.01)
        assert np.array_equal(np.concatenate([got["pos"][1], got["vel"][1], got["cov"][1]]), want) and got["nis"][1] == nis
    with pytest.raises(ValueError):
        so.smooth(summ, summ["node_ptr"], links, times=[0.0, 1.0], **kw)
    _, st = so.smooth(summ, summ["node_ptr"], links, times=[0.0, 1.0, 2.0, 3.0], **kw)
    with pytest.raises(ValueError):
        so.smooth(summ, summ["node_ptr"], links, state=st, **kw)


def test_rows_beyond_a_count_and_refused_frames_are_empty():
    summ, links = hidden_sequence(0, 1)
    ptr = summ["node_ptr"]
    summ["count"] = summ["count"].copy()
    summ["count"][3] = -1                     # a refused frame
    summ["count"][6] -= 2                     # two rows beyond the count
    links, _ = tt.link_timed(summ, ptr, np.arange(12), 0.6, lam=1.0, max_gap=0)
    out, state = so.smooth(summ, ptr, links, q=0.01, r=0.09, vel_var=1.0)
    gone = np.r_[ptr[3]:ptr[4], ptr[7] - 2:ptr[7]]
    assert (out["age"][gone] == -1).all() and not out["pos"][gone].any() and not out["cov"][gone].any() and not out["nis"][gone].any()
    live = np.setdiff1d(np.arange(ptr[-1]), gone)
    assert (out["age"][live] >= 0).all() and (out["age"][ptr[4]:ptr[5]] == 0).all()   # after a refused frame everybody is born again
    with np.errstate(all="ignore"):   # non-finite inputs propagate
        summ["pos"] = summ["pos"].copy()
        summ["pos"][0, 0] = np.nan
        bad, _ = so.smooth(summ, ptr, links, q=0.01, r=0.09, vel_var=1.0)
    assert np.isnan(bad["pos"][0, 0]) and bad["pos"][0, 1] == summ["pos"][0, 1]


# ---- 5. on noisy straight walks the filtered positions are closer to the truth --------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_filtered_positions_beat_raw_ones_on_noisy_straight_walks(seed):
    kw = dict(g=12, persons=10, r=16, speed=(0.3, 0.6), p_hide=0.1, max_hide=1, arena=8.0)
    noisy = tm.cross_sequence(np.random.default_rng(seed), noise=0.05, **kw)
    clean = tm.cross_sequence(np.random.default_rng(seed), noise=0.0, **kw)   # the same draws: the same walks, rows and order
    assert np.array_equal(noisy["person"], clean["person"]) and np.array_equal(noisy["node_ptr"], clean["node_ptr"])
    assert 0.04 < (noisy["pos"] - clean["pos"]).std() < 0.06   # the noise, 0.05 per coordinate, is all that differs
    links, _ = tt.link_timed(noisy, noisy["node_ptr"], np.arange(12), 0.8, lam=1.0, max_gap=1)
    out, _ = so.smooth(noisy, noisy["node_ptr"], links, q=1e-4, r=0.05 ** 2, vel_var=1.0, max_gap=1)
    old = out["age"] >= 3
    rmse = lambda a: float(np.sqrt(((a[old] - clean["pos"][old]) ** 2).sum(axis=1).mean()))
    raw, filtered = rmse(noisy["pos"]), rmse(out["pos"])
    print(f"seed {seed}: {int(old.sum())} rows of age >= 3, position RMSE raw {raw:.4f}, filtered {filtered:.4f}")
    assert old.sum() >= 40 and filtered < raw


# ---- 6. TrackSmoother refuses on the host -------------------------------------------------------------------------------------------------
def _cpu_batch(g=2, n_per=3):
    import torch
    from gnn_cca_amd.tracking import ClusterSummaries, Tracks
    n = g * n_per
    ptr = [n_per * i for i in range(g + 1)]
    s = ClusterSummaries(torch.full((g,), n_per, dtype=torch.int32), torch.arange(n, dtype=torch.int32) % n_per, torch.ones(n, dtype=torch.int32),
                         torch.ones(n, dtype=torch.int32), torch.zeros((n, 2), dtype=torch.float64), torch.zeros((n, 0)), ptr,
                         torch.tensor(ptr, dtype=torch.int32))
    t = Tracks(torch.arange(n), torch.arange(n), torch.full((n,), -1, dtype=torch.int32), torch.tensor([n]), None)
    return s, t


def test_track_smoother_refuses_bad_arguments():
    import torch
    from gnn_cca_amd.smoothing import TrackSmoother, Trajectories
    from gnn_cca_amd.tracking import FrameLinker, Tracks
    link = FrameLinker(0.8, max_gap=2)
    with pytest.raises(ValueError, match="linker must be the FrameLinker"):
        TrackSmoother(None, 0.01, 0.01, 1.0)
    for bad in (-1.0, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="process_noise"):
            TrackSmoother(link, bad, 0.01, 1.0)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="measurement_noise"):
            TrackSmoother(link, 0.01, bad, 1.0)
        with pytest.raises(ValueError, match="vel_var"):
            TrackSmoother(link, 0.01, 0.01, bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="per_detection"):
            TrackSmoother(link, 0.01, 0.01, 1.0, per_detection=bad)
    sm = TrackSmoother(link, 0, 0.01, 1.0, per_detection=True)   # q = 0 is allowed
    assert sm.max_gap == 2 and sm.process_noise == 0.0 and sm.per_detection is True and sm._state is None
    assert Trajectories.__slots__ == ("pos", "vel", "cov", "nis", "age")
    s, t = _cpu_batch()
    with pytest.raises(ValueError, match="takes a ClusterSummaries or a FrameResult"):
        sm(t, t)
    with pytest.raises(ValueError, match="takes the Tracks its linker returned"):
        sm(s, s)
    short = Tracks(t.cluster_track[:4], t.node_track[:4], t.matched_prev[:4], t.next_id, None)
    with pytest.raises(ValueError, match="tracks has 4 rows, the summaries 6"):
        sm(s, short)
    for bad in ([0.0], [0.0, 1.0, 2.0], [0.0, float("nan")], [0.0, "1"], [0.0, True], 3.0):
        with pytest.raises(ValueError, match="time"):
            sm(s, t, times=bad)
    sm.measurement_noise = 0.0
    with pytest.raises(ValueError, match="measurement_noise"):
        sm(s, t)
    sm.measurement_noise = 0.01
    link.max_gap = 1
    with pytest.raises(ValueError, match="max_gap changed from 2 to 1"):
        sm(s, t)
    link.max_gap = 2
    sm._state, sm._state_timed, sm._frame_rows, sm._frame_times = torch.zeros(1), True, [3], [0.0]   # as after a timed call
    with pytest.raises(ValueError, match=r"with time stamps.*reset\(\) it first"):
        sm(s, t)
    sm._state_timed, sm._frame_times = False, []
    with pytest.raises(ValueError, match=r"without time stamps.*reset\(\) it first"):
        sm(s, t, times=[1.0, 2.0])
    assert sm._frame_rows == [3] and sm._state is not None   # the refusals left the state alone
    with pytest.raises(RuntimeError, match="MI355X only"):   # every check above comes before the GPU is asked for
        sm(s, t)
    sm.reset()
    assert sm._state is None and sm._frame_rows == [] and sm._frame_times == [] and sm._state_timed is None


# ---- 7. the entry: declared, bound, and checking its arguments before any launch ----------------------------------------------------------
def test_the_binding_declares_the_smoother_entries():
    import os
    import re
    from conftest import ROOT
    from gnn_cca_amd import _native as nat
    import gnn_cca_amd.smoothing as smoothing
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    for name in ("gnncca_track_smooth_state_bytes", "gnncca_track_smooth_workspace_bytes", "gnncca_track_smooth"):
        assert name in nat.exported_symbols()
        decl = re.search(r"GNNCCA_API\s+\w+\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(nat._SIGNATURES[name][1]), name
    decl = re.search(r"GNNCCA_API\s+int\s+gnncca_track_smooth\s*\(([^;]*)\)\s*;", header).group(1).split(",")
    assert decl[-2].split()[-1] == "frame_time_dev" and decl[-1].split() == ["double", "max_dt"]
    lib = nat.lib()
    for cap, kept in ((0, 0), (1, 1), (37, 3), (4096 * 9, 9)):
        assert lib.gnncca_track_smooth_state_bytes(cap, kept) == max(256, (64 + 60 * cap + 255) // 256 * 256)
    assert lib.gnncca_track_smooth_state_bytes(-1, 1) == 0 and lib.gnncca_track_smooth_state_bytes(5, nat.TRACK_MAX_GAP + 2) == 0
    assert lib.gnncca_track_smooth_workspace_bytes(100, 4, 30) >= 4 * (30 + 2 * 100) and lib.gnncca_track_smooth_workspace_bytes(-1, 4, 30) == 0
    # the rule stands in the header, the kernel file, the module docstring and the oracle in the same words
    flat = lambda text: " ".join(text.replace("*", " ").replace("//", " ").split())
    kernels = open(os.path.join(ROOT, "gnn-cca_amd", "csrc", "identities_smooth.cuh")).read()
    for line in ("a_ = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0", "b_ = (b + dt*c) + (q*dt2)/2.0", "c_ = c + q*dt", "nis = (ix*ix + iy*iy)/s",
                 "a' = a_ - k1*a_; b' = b_ - k1*b_; c' = c_ - k2*b_"):
        for where in (header, kernels, smoothing.__doc__, so.__doc__):
            assert flat(line.replace("*", " ")) in flat(where), line


def test_the_entry_checks_its_arguments_before_any_launch():
    """No device needed: the argument checks come first and the (fake) device pointers are never followed."""
    import ctypes as C
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000

    def call(n=5, g=1, max_n=5, gap=2, q=0.01, r=0.01, vel_var=1.0, per=0, rows_in=(10, 20), rows_out=(10, 20, 5), state_in=fake, state_out=fake,
             ptr=fake, count=fake, size=fake, pos=fake, prev=fake, mgap=fake, outs=(fake,) * 5, ws=fake, ws_bytes=1 << 20, times=None, max_dt=0.0,
             n_in=None, n_out=None):
        c_in, c_out = (C.c_int32 * max(len(rows_in), 1))(*rows_in), (C.c_int32 * max(len(rows_out), 1))(*rows_out)
        return lib.gnncca_track_smooth(ptr, count, size, pos, prev, mgap, n, g, max_n, gap, q, r, vel_var, per, state_in, c_in,
                                       len(rows_in) if n_in is None else n_in, state_out, c_out, len(rows_out) if n_out is None else n_out, *outs,
                                       ws, ws_bytes, None, times, max_dt)

    assert call(g=0) == nat.OK and call(g=0, n=0, max_n=0, times=fake, max_dt=1.0) == nat.OK   # no frames: nothing is launched, nothing written
    nan, inf = float("nan"), float("inf")
    for bad in (dict(q=-1.0), dict(q=nan), dict(q=inf), dict(r=0.0), dict(r=-1.0), dict(r=nan), dict(r=inf), dict(vel_var=0.0), dict(vel_var=nan),
                dict(vel_var=inf), dict(per=2), dict(per=-1), dict(gap=-1), dict(gap=nat.TRACK_MAX_GAP + 1), dict(n=-1), dict(g=-1), dict(max_n=6),
                dict(max_n=-1), dict(n=5000, max_n=4097), dict(rows_in=(10, 4097)), dict(rows_in=(1, 2, 3, 4)), dict(n_in=-1), dict(state_in=None),
                dict(rows_out=(10, 20)), dict(rows_out=(10, 20, 5, 5)), dict(rows_out=(10, 21, 5)), dict(rows_out=(11, 20, 5)), dict(rows_out=(10, 20, -1)),
                dict(state_out=None), dict(ptr=None), dict(count=None), dict(ws=None), dict(size=None), dict(pos=None), dict(prev=None), dict(mgap=None),
                dict(times=fake, max_dt=0.0), dict(times=fake, max_dt=-1.0), dict(times=fake, max_dt=nan), dict(times=fake, max_dt=inf)):
        assert call(**bad) == nat.ERR_INVALID_ARG, bad
    for i in range(5):
        assert call(outs=tuple(None if j == i else fake for j in range(5))) == nat.ERR_INVALID_ARG, i
    assert call(g=0, q=-1.0) == nat.ERR_INVALID_ARG and call(g=0, rows_in=(10, 4097)) == nat.ERR_INVALID_ARG   # also without frames
    assert call(ws_bytes=16) == nat.ERR_WORKSPACE
