"""tests/tracking_kalman_oracle.py against itself, the hand-written variance-gate case, what the rule does to identity switches on crossing
walks, KalmanLinker's argument checks and the native entry's -- all without a GPU."""
import numpy as np
import pytest

import track_smooth_oracle as ts
import tracking_kalman_oracle as tk
import tracking_motion_oracle as tm

FIELDS = ("cluster_track", "node_track", "matched_prev", "matched_gap", "velocity", "pos", "vel", "cov", "nis", "age")
Q, R_, VV = 0.001, 0.01, 0.25


def _frames_of(summ, lo, hi):
    """Frames lo .. hi of a sequence as a sequence of its own."""
    ptr = np.asarray(summ["node_ptr"], np.int64)
    v0, v1 = int(ptr[lo]), int(ptr[hi])
    out = {k: summ[k][v0:v1] for k in ("rank", "size", "n_cams", "pos", "emb")}
    out["count"], out["node_ptr"] = summ["count"][lo:hi], ptr[lo:hi + 1] - v0
    return out


def _same(a, b):
    for k in FIELDS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["next_id"] == b["next_id"]


def _cut(summ, cuts, times=None, **kw):
    state, parts = tk.new_state(), []
    for lo, hi in cuts:
        part, state = tk.link_kalman(_frames_of(summ, lo, hi), _frames_of(summ, lo, hi)["node_ptr"], state=state,
                                     times=None if times is None else times[lo:hi], **kw)
        parts.append(part)
    out = {k: np.concatenate([p[k] for p in parts]) for k in FIELDS}
    out["next_id"] = parts[-1]["next_id"]
    return out


# ---- 1. the oracle against itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nis", [None, 9.0])
def test_the_oracle_does_not_depend_on_the_cut_and_agrees_with_the_smoother(max_nis):
    g, m = 12, 2
    summ = tm.cross_sequence(np.random.default_rng(4), g, 12, 8, noise=0.08, p_hide=0.15, max_hide=m + 1, arena=5.0)
    kw = dict(max_step=0.5, q=Q, r=R_, vel_var=VV, lam=1.0, max_cos=None, max_gap=m, max_nis=max_nis)
    whole, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    assert all((whole["matched_gap"] == k).any() for k in range(m + 1)) and (whole["age"] >= 3).any()
    for cuts in ([(i, i + 1) for i in range(g)], [(0, 5), (5, 6), (6, 12)], [(0, 3), (3, 3), (3, 12)], [(0, 1), (1, 2), (2, 12)]):
        _same(_cut(summ, cuts, **kw), whole)
    # times 0 .. G - 1 are the untimed rule, in one call and in pieces
    timed, _ = tk.link_kalman(summ, summ["node_ptr"], times=np.arange(g, dtype=np.float64), **kw)
    _same(timed, whole)
    _same(_cut(summ, [(0, 5), (5, 6), (6, 12)], times=np.arange(g, dtype=np.float64), **kw), whole)
    # the smoother fed the oracle's links gives the oracle's trajectories
    smooth, _ = ts.smooth(summ, summ["node_ptr"], whole, Q, R_, VV, False, m)
    for k in ("pos", "vel", "cov", "nis", "age"):
        assert np.array_equal(smooth[k].view(np.uint8), whole[k].view(np.uint8)), k
    linked = whole["matched_gap"] >= 0
    assert linked.sum() > 40
    if max_nis is not None:
        assert (whole["nis"][linked] <= max_nis).all()
        free, _ = tk.link_kalman(summ, summ["node_ptr"], **dict(kw, max_nis=None))
        assert not np.array_equal(free["matched_prev"], whole["matched_prev"])   # the gate refuses somebody the distance gate admits
    # a dropped frame: times 0, 1, 3, 4, ... -- the smoother identity holds with time stamps too
    times = np.array([0, 1] + list(range(3, g + 1)), np.float64)
    dropped, _ = tk.link_kalman(summ, summ["node_ptr"], times=times, **kw)
    smooth, _ = ts.smooth(summ, summ["node_ptr"], dropped, Q, R_, VV, False, m, times=times)
    for k in ("pos", "vel", "cov", "nis", "age"):
        assert np.array_equal(smooth[k].view(np.uint8), dropped[k].view(np.uint8)), k
    assert not np.array_equal(dropped["cov"], whole["cov"])
    with pytest.raises(ValueError):   # a timed state continued untimed
        _, st = tk.link_kalman(_frames_of(summ, 0, 3), _frames_of(summ, 0, 3)["node_ptr"], times=[0.0, 1.0, 2.0], **kw)
        tk.link_kalman(_frames_of(summ, 3, 5), _frames_of(summ, 3, 5)["node_ptr"], state=st, **kw)


# ---- 2. the hand-written gate case ------------------------------------------------------------------------------------------------------
def test_the_variance_gate_refuses_an_established_track_what_it_grants_a_newborn():
    s = tk.gate_case()
    out, _ = tk.link_kalman(s, s["node_ptr"], **tk.GATE)
    tk.check_gate_case(out, tk.level_tables(s, s["node_ptr"], **tk.GATE))
    # without the variance gate both are linked
    free, _ = tk.link_kalman(s, s["node_ptr"], **dict(tk.GATE, max_nis=None))
    assert free["cluster_track"].tolist() == [0, 0, 0, 0, 0, 1, 0, 1]


# ---- 3. quality -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_filtered_prediction_switches_identities_less_often_than_the_last_link_velocity(seed):
    """The issue's scratch restatement gave 363 / 363 / 366 / 391 (Kalman prediction, the same gate) against 481 / 483 / 520 / 508
    (velocity) for seeds 0 .. 3; the committed oracle's figures are in DESIGN.md section 9."""
    summ = tm.cross_sequence(np.random.default_rng(seed), 40, 25, 8, noise=0.10, p_hide=0.1, max_hide=2)
    vel, _ = tm.link_motion(summ, summ["node_ptr"], 0.35, 0.0, None, 2)
    kal, _ = tk.link_kalman(summ, summ["node_ptr"], 0.35, 0.001, 0.01, 0.25, 0.0, None, 2)
    sw = [tm.switches(summ["person"], r["cluster_track"], summ["node_ptr"]) for r in (vel, kal)]
    print("identity switches, velocity / kalman:", sw)
    assert sw[1] < sw[0], sw


# ---- 4. KalmanLinker's arguments ------------------------------------------------------------------------------------------------------
def test_the_kalman_linker_validates_its_arguments_before_the_gpu():
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd import kalman, tracking
    from gnn_cca_amd.kalman import KalmanLinker, KalmanTracks
    from gnn_cca_amd.tracking import FrameLinker, Tracks
    nan, inf = float("nan"), float("inf")
    good = dict(max_step=1.0, process_noise=0.001, measurement_noise=0.01, vel_var=0.25)
    for bad in ([dict(process_noise=v) for v in (-1e-9, nan, inf, None, "1", True)] +
                [dict(measurement_noise=v) for v in (0, 0.0, -1.0, nan, inf, None, True)] +
                [dict(vel_var=v) for v in (0, -0.5, nan, inf, None, [1.0])] +
                [dict(max_nis=v) for v in (0, -1.0, nan, inf, "9", True)] +
                [dict(max_gap=v) for v in (-1, 9, 1.0, True, None)] +
                [dict(max_dt=v) for v in (0, -1.0, nan, inf, "2")] +
                [dict(max_step=v) for v in (0, nan, inf)] + [dict(lam=-1.0), dict(max_cos=2.5)]):
        with pytest.raises(ValueError):
            KalmanLinker(**dict(good, **bad))
    for kw in (dict(matching="mutual"), dict(miss_cost=1.0), dict(motion="kalman")):   # no such arguments
        with pytest.raises(TypeError):
            KalmanLinker(**dict(good, **kw))
    link = KalmanLinker(1.0, 0.0, 0.01, 0.25, lam=0.0, max_gap=3, max_nis=13.8)
    assert isinstance(link, FrameLinker) and link.motion == "kalman" and link.matching == "mutual"
    assert (link.process_noise, link.measurement_noise, link.vel_var, link.max_nis, link.max_gap, link.max_dt) == (0.0, 0.01, 0.25, 13.8, 3, 4.0)
    assert KalmanLinker(**good).max_nis is None and not KalmanLinker(**good, lam=0.0).needs_embeddings
    assert kalman.__all__ == ["KalmanLinker", "KalmanTracks"]
    assert issubclass(KalmanTracks, Tracks) and KalmanTracks.__slots__ == ("trajectories",)
    # what the existing tests pin stays
    with pytest.raises(ValueError):
        FrameLinker(1.0, motion="kalman")
    assert nat.MOTION == {"none": 0, "velocity": 1} and len(tracking.__all__) == 10
    assert Tracks.__slots__ == ("cluster_track", "node_track", "matched_prev", "next_id", "velocity", "_state", "_matched_gap")
    # a value changed after construction is refused at the call, before the summaries' tensors are looked at
    from gnn_cca_amd.tracking import ClusterSummaries
    import torch
    z32 = torch.zeros(2, dtype=torch.int32)
    s = ClusterSummaries(torch.ones(1, dtype=torch.int32), z32, z32, z32, torch.zeros((2, 2), dtype=torch.float64), torch.zeros((2, 0)), [0, 2],
                         torch.tensor([0, 2], dtype=torch.int32))
    for name, v in (("measurement_noise", 0.0), ("process_noise", -1.0), ("vel_var", nan), ("max_nis", 0.0), ("motion", "velocity"),
                    ("matching", "optimal")):
        link = KalmanLinker(**good)
        setattr(link, name, v)
        with pytest.raises(ValueError):
            link(s)
    n = 4097
    z32 = torch.zeros(n, dtype=torch.int32)
    big = ClusterSummaries(torch.ones(1, dtype=torch.int32), z32, z32, z32, torch.zeros((n, 2), dtype=torch.float64), torch.zeros((n, 0)), [0, n],
                           torch.tensor([0, n], dtype=torch.int32))
    with pytest.raises(ValueError, match="4097 detections"):
        KalmanLinker(**good)(big)
    with pytest.raises(ValueError):
        KalmanLinker(**good)(s, times=[0.0, 1.0])   # two times for one frame


# ---- 5. the native entries -----------------------------------------------------------------------------------------------------------------
def test_the_binding_declares_the_kalman_entries():
    import os
    import re
    from conftest import ROOT
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    for name in ("gnncca_link_kalman_state_bytes", "gnncca_link_kalman_workspace_bytes", "gnncca_link_frames_kalman"):
        assert name in nat.exported_symbols() and re.search(r"GNNCCA_API[^;(]*\b" + name + r"\s*\(", header), name
        assert hasattr(nat.lib(), name)
    decl = re.search(r"GNNCCA_API\s+int\s+gnncca_link_frames_kalman\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(nat._SIGNATURES["gnncca_link_frames_kalman"][1])
    # the timed motion entry's arguments without `motion`, plus q, r, vel_var, has_max_nis, max_nis and four more outputs
    assert len(nat._SIGNATURES["gnncca_link_frames_kalman"][1]) == len(nat._SIGNATURES["gnncca_link_frames_motion_timed"][1]) - 1 + 5 + 4


def test_the_kalman_entry_checks_its_arguments_before_any_launch():
    """No device needed: the argument checks come first and the (fake) device pointers are never followed."""
    import ctypes as C
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000

    def call(n=5, g=1, max_n=5, gap=2, q=0.001, r=0.01, vv=0.25, has_nis=1, max_nis=9.0, state_in=fake, rows_in=(10, 20), rows_out=(10, 20, 5),
             frames_out=None, out_cov=fake, out_age=fake, max_step=1.0, ws_bytes=1 << 20, times=None, max_dt=0.0):
        c_in, c_out = (C.c_int32 * max(len(rows_in), 1))(*rows_in), (C.c_int32 * max(len(rows_out), 1))(*rows_out)
        return lib.gnncca_link_frames_kalman(fake, fake, fake, fake, None, 0, n, g, max_n, max_step, 0.0, 0, 0.0, gap, q, r, vv, has_nis, max_nis,
                                             state_in, c_in, len(rows_in), fake, c_out, len(rows_out) if frames_out is None else frames_out,
                                             fake, fake, fake, fake, fake, fake, out_cov, fake, out_age, fake, ws_bytes, None, times, max_dt)

    nan, inf = float("nan"), float("inf")
    assert call(g=0) == nat.OK                                                     # no frames: nothing is launched, nothing written
    assert call(g=0, has_nis=0, max_nis=nan) == nat.OK                             # max_nis is read only with has_max_nis
    for bad in (dict(q=-1.0), dict(q=nan), dict(q=inf), dict(r=0.0), dict(r=nan), dict(r=inf), dict(vv=0.0), dict(vv=-1.0), dict(vv=inf),
                dict(has_nis=2), dict(has_nis=-1), dict(max_nis=0.0), dict(max_nis=nan), dict(max_nis=inf), dict(times=fake, max_dt=0.0),
                dict(times=fake, max_dt=inf), dict(gap=-1), dict(gap=nat.TRACK_MAX_GAP + 1), dict(max_n=4097), dict(rows_in=(10, 4097)),
                dict(rows_out=(10, 4097, 5)), dict(rows_in=(1, 2, 3, 4)), dict(frames_out=2), dict(out_cov=None), dict(out_age=None),
                dict(max_step=0.0), dict(max_step=inf), dict(state_in=None, rows_in=(10, 20)), dict(n=-1)):
        assert call(**bad) == nat.ERR_INVALID_ARG, bad
        assert call(**dict(bad, g=0)) in (nat.ERR_INVALID_ARG, nat.OK), bad
    assert call(ws_bytes=16) == nat.ERR_WORKSPACE
    # the sizes: cov and age are 28 more bytes per row than the motion state, and the 8-byte arrays come first
    assert lib.gnncca_link_kalman_state_bytes(100, 3, 16) >= lib.gnncca_link_motion_state_bytes(100, 3, 16) + 2800 - 256
    assert lib.gnncca_link_kalman_state_bytes(100, 3, 16) >= 64 + 100 * (16 + 16 + 24 + 8 + 64 + 4 + 4)
    assert lib.gnncca_link_kalman_state_bytes(-1, 3, 16) == 0 and lib.gnncca_link_kalman_state_bytes(1, 10, 16) == 0
    assert lib.gnncca_link_kalman_workspace_bytes(1000, 12, 500) >= 1500 * 4 and lib.gnncca_link_kalman_workspace_bytes(-1, 1, 0) == 0
