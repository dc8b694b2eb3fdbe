"""The radius-gated graph build without a GPU: the host plan (gnncca_plan_frames_radius) against the numpy restatement of the definition
(tests/graph_radius_oracle.py), the real-geometry fixture's recall table, and the argument refusals of build_graph_batch / FramePipeline.

Fixture: tests/golden/terrace_geometry.npz (tests/golden/make_terrace_geometry.py): the ground-plane positions of the reference's
EPFL-Terrace annotations, every valid frame whose number is a multiple of 5.  RECALL records what that script printed when the committed
file was made; the test recomputes the counts from the file through the oracle's predicate."""
import math

import numpy as np
import pytest

import graph_radius_oracle as gro

RADII = (0, 40, 80, 100, math.inf)
# radius -> (kept edges, kept same-identity edges) of the committed fixture: 963 frames, 330 616 directed cross-camera edges, 49 956 of them
# same-identity, the largest same-identity distance 100.81
RECALL = {40: (55878, 42854), 60: (83788, 49060), 80: (113534, 49838), 100: (145276, 49954), 150: (223826, 49956)}
FIXTURE = dict(frames=963, edges=330616, positives=49956, mean=19.1, largest=34, farthest=100.81)


def plan(a, radius, unit, dense=False):
    """(E, staging image as uint8 numpy, layout) of gnncca_plan_frames_radius (dense=True: gnncca_plan_frames)."""
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.frames import FrameLayout
    lib = nat.lib()
    arrs = [np.ascontiguousarray(a[k], t) for k, t in (("xw", np.float64), ("yw", np.float64), ("id", np.int64), ("id_cam", np.int64))]
    sizes, md = np.ascontiguousarray(a["graph_sizes"], np.int64), np.ascontiguousarray(a["max_dist"], np.float64)
    n, g = len(arrs[3]), len(sizes)
    layout = FrameLayout(n, g)
    assert lib.gnncca_plan_frames_bytes(n, g) == layout.nbytes
    image = np.full(layout.nbytes, 0xA5, np.uint8)
    args = [x.ctypes.data for x in arrs] + [n, sizes.ctypes.data, md.ctypes.data, g]
    if dense:
        e = lib.gnncca_plan_frames(*args, image.ctypes.data, layout.nbytes)
    else:
        e = lib.gnncca_plan_frames_radius(*args, float(radius), nat.RADIUS_UNIT[unit], image.ctypes.data, layout.nbytes)
    return e, image, layout


def check_plan(a, radius, unit):
    e, image, layout = plan(a, radius, unit)
    ei, keep = gro.keep_mask(a["xw"], a["yw"], a["id_cam"], a["graph_sizes"], a["max_dist"], radius, unit)
    edge_ptr, edge_ptr_g = gro.edge_ptrs(ei, keep, a["id_cam"], a["graph_sizes"])
    assert e == int(keep.sum()), (radius, unit)
    assert np.array_equal(layout.view(image, "edge_ptr"), edge_ptr), (radius, unit)
    assert np.array_equal(layout.view(image, "edge_ptr_g"), edge_ptr_g), (radius, unit)
    return e, int(keep.size), image


@pytest.mark.parametrize("unit", gro.UNITS)
def test_plan_on_the_terrace_fixture(unit):
    """The first 64 frames at radii 0, 40, 80, 100 and inf.  In the 'max_dist' unit max_dist = 2.5 per frame, so the radii are scaled to
    the same gates (16, 32, 40 in units of max_dist) -- and checked at the plain values too."""
    a = gro.with_embeddings(gro.terrace(64), max_dist=np.full(64, 2.5))
    dense_e, dense_image, _ = plan(a, None, None, dense=True)
    counts = []
    for r in RADII:
        e, total, image = check_plan(a, r, unit)
        if unit == "max_dist":
            assert check_plan(a, r / 2.5, unit)[0] == check_plan(a, r, "ground")[0]
        assert total == dense_e
        counts.append(e)
        if r == math.inf:
            assert e == dense_e and np.array_equal(image, dense_image)      # gnncca_plan_frames' image, byte for byte
    assert counts[0] == 0 and counts == sorted(counts) and counts[-1] == dense_e
    if unit == "ground":
        assert 0 < counts[1] < counts[2] <= counts[3] <= dense_e      # the gate bites on real positions


@pytest.mark.parametrize("unit,radii,max_dist", [("ground", (5, 13), 30.0), ("max_dist", (10, 26), 0.5)])
def test_plan_on_lattice_frames(unit, radii, max_dist):
    """s == t2 occurs: 3-4-5 and 5-12-13 offsets from the anchor, kept at equality; the next lattice distance is dropped."""
    a = gro.lattice_case(max_dist=np.full(3, max_dist))
    for r, at, beyond in zip(radii, (25.0, 169.0), (26.0, 170.0)):
        e, total, _ = check_plan(a, r, unit)
        ei, keep = gro.keep_mask(a["xw"], a["yw"], a["id_cam"], a["graph_sizes"], a["max_dist"], r, unit)
        s = gro.squared_distance(a["xw"], a["yw"], ei)
        assert keep[s == at].all() and (s == at).sum() >= 6 and not keep[s == beyond].any() and (s == beyond).sum() >= 6
        assert 0 < e < total


def test_plan_on_degenerate_batches():
    """No frame, a frame of one detection, a frame on one camera, coincident points at radius 0, a NaN and an inf position."""
    from gnn_cca_amd import _native as nat
    assert plan(gro.case([], [], []), 1.0, "ground")[0] == 0
    a = gro.case([[0], [1, 1, 1], [0, 1, 0, 1]], [0, 0, 1, 2, 5, 5, 6, 5], [0, 0, 0, 0, 7, 7, 7, 7])
    assert check_plan(a, 0.0, "ground")[0] == 4      # detections 4, 5 and 7 coincide: (4, 5), (4, 7) and their reverses; 5 and 7 share camera 1
    assert check_plan(a, 1.0, "ground")[0] == 8      # ... and detection 6 (camera 0) is at distance 1 from 5 and 7: two more pairs
    b = gro.case([[0, 1, 2, 0, 1]], [0, np.nan, 1, np.inf, 2], [0, 0, 0, 0, 0])
    for r in (0.0, 1.0, 2.0, math.inf):
        check_plan(b, r, "ground")
    assert check_plan(b, math.inf, "ground")[0] == 2 * 3 + 2 * 2      # the NaN's pairs are dropped, the inf's are kept; (0, 3) share a camera
    lib = nat.lib()
    for bad_r, bad_u in ((math.nan, 0), (-1.0, 0), (-math.inf, 0), (1.0, 2), (1.0, -1)):
        assert lib.gnncca_plan_frames_radius(None, None, None, None, 0, None, None, 0, bad_r, bad_u, None, 0) == -nat.ERR_INVALID_ARG


def test_fixture_recall_table():
    a = gro.terrace()
    sizes = a["graph_sizes"]
    assert len(sizes) == FIXTURE["frames"] and int(sizes.max()) == FIXTURE["largest"] and round(float(sizes.mean()), 1) == FIXTURE["mean"]
    assert (a["frame"] % 5 == 0).all() and (np.diff(a["frame"]) > 0).all()
    assert np.isfinite(a["xw"]).all() and np.isfinite(a["yw"]).all()
    table, e, pos, far = gro.recall_table(a, sorted(RECALL))
    assert (e, pos, round(far, 2)) == (FIXTURE["edges"], FIXTURE["positives"], FIXTURE["farthest"])
    for r, kept, kept_pos in table:
        print(f"radius {r}: edges kept {kept / e:.4f}, same-identity edges kept {kept_pos / pos:.4f}")
        assert (kept, kept_pos) == RECALL[r], r
    # same order and topology as the topology fixture's frames that are here too
    import os
    topo = np.load(os.path.join(gro.GOLDEN, "terrace_topology.npz"))
    where = np.searchsorted(topo["frame"], a["frame"])
    assert np.array_equal(topo["frame"][where], a["frame"])
    for q in (0, len(where) // 2, len(where) - 1):
        t0, t1 = topo["node_ptr"][where[q]], topo["node_ptr"][where[q] + 1]
        v0, v1 = a["node_ptr"][q], a["node_ptr"][q + 1]
        assert np.array_equal(topo["cam"][t0:t1], a["id_cam"][v0:v1]) and np.array_equal(topo["person"][t0:t1], a["id"][v0:v1])


BAD_RADII = (True, False, math.nan, -1, -0.5, -math.inf, "5", [5.0], np.array([1.0, 2.0]), 1 + 2j)


@pytest.fixture
def no_native(monkeypatch):
    """Any native call (and so any device call) fails the test."""
    from gnn_cca_amd import _native as nat

    def reached():
        raise AssertionError("the native library was reached before the arguments were refused")
    monkeypatch.setattr(nat, "lib", reached)


def test_build_graph_batch_refuses_before_any_device_call(no_native):
    import torch
    from gnn_cca_amd.graph_build import build_graph_batch
    a = gro.lattice_case()
    node, reid = torch.from_numpy(a["node_embeds_raw"]), torch.from_numpy(a["reid_embeds_raw"])

    def build(**kw):
        return build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid, **kw)
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radius"):
            build(radius=bad)
    for unit in ("metres", None, 0, "GROUND"):
        with pytest.raises(ValueError, match="radius_unit"):
            build(radius=5.0, radius_unit=unit)
        with pytest.raises(ValueError, match="radius_unit"):
            build(radius_unit=unit)
    with pytest.raises(ValueError, match="radius together with top_k"):
        build(radius=5.0, top_k=3)
    with pytest.raises(ValueError, match="radius together with top_k / symmetric"):
        build(radius=5.0, top_k=3, symmetric="union")
    with pytest.raises(ValueError, match="symmetric"):
        build(radius=5.0, symmetric="mutual")
    with pytest.raises(RuntimeError, match="MI355X only"):      # good arguments get as far as the device check (host tensors here)
        build(radius=np.float32(5.0), radius_unit="max_dist")


def test_frame_pipeline_refuses_before_any_device_call(no_native):
    from gnn_cca_amd.pipeline import FramePipeline
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radius"):
            FramePipeline(None, radius=bad)
    for unit in ("metres", None, 0):
        with pytest.raises(ValueError, match="radius_unit"):
            FramePipeline(None, radius=5.0, radius_unit=unit)
    with pytest.raises(ValueError, match="radius together with top_k"):
        FramePipeline(None, radius=5.0, top_k=3)
    with pytest.raises(ValueError, match="radius together with top_k / symmetric"):
        FramePipeline(None, radius=5.0, top_k=3, symmetric="mutual")
    with pytest.raises(ValueError, match="symmetric"):
        FramePipeline(None, radius=5.0, symmetric="union")
    for good in (0, 0.0, 5, np.float64(80.0), np.int64(3), math.inf):
        p = FramePipeline(None, radius=good, radius_unit="max_dist")
        assert p.radius == float(good) and p.radius_unit == "max_dist" and p.top_k is None
    assert FramePipeline(None).radius is None


def test_native_entries_refuse_a_bad_radius():
    """gnncca_build_edges_radius / gnncca_frames_forward_radius: INVALID_ARG before anything is looked at (no device is needed for that)."""
    from gnn_cca_amd import _native as nat
    lib, fr = nat.lib(), nat.Frames()
    for bad_r, bad_u in ((math.nan, 0), (-1.0, 0), (1.0, 2)):
        assert lib.gnncca_build_edges_radius(fr, None, 4, 10, 10, 0, bad_r, bad_u, None, None, None, None) == nat.ERR_INVALID_ARG
        assert lib.gnncca_frames_forward_radius(None, None, None, None, 0, None, 0, 0, bad_r, bad_u, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_build_edges_radius(None, None, 4, 10, 10, 0, 1.0, 0, None, None, None, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_build_edges_radius(fr, None, 4, 10, 0, 0, 1.0, 0, None, None, None, None) == nat.OK      # E == 0: nothing to launch
    assert lib.gnncca_frames_forward_radius(None, None, None, None, 0, None, 0, 0, 1.0, 0, None) == nat.ERR_INVALID_ARG      # as gnncca_frames_forward
