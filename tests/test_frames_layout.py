"""gnn_cca_amd.frames on the host: FrameLayout against the staging image gnncca_plan_frames / gnncca_plan_frames_ex write (read here with
the hand-written slicing of test_graph_oracle.py: the independent statement of the layout), and check_cap's refusals.  CPU only."""
import numpy as np
import pytest
import torch

# (n, g) = (0, 0), (0, 1), (2, 1), (5, 3): an empty frame and a single-camera frame, (67, 3): a frame of more than one 64-candidate chunk
BATCHES = {
    "n0_g0": dict(sizes=[], cams=[]),
    "n0_g1": dict(sizes=[0], cams=[]),
    "n2_g1": dict(sizes=[2], cams=[0, 1]),
    "n5_g3": dict(sizes=[3, 0, 2], cams=[0, 1, 0, 4, 4]),
    "n67_g3": dict(sizes=[65, 1, 1], cams=[c % 3 for c in range(65)] + [0, 1]),
}


def make(name):
    """The six host arrays of a hand-made batch: xw, yw, ids, id_cam, graph_sizes, max_dist."""
    sizes, cams = BATCHES[name]["sizes"], BATCHES[name]["cams"]
    n = len(cams)
    assert sum(sizes) == n
    k = np.arange(n)
    return (0.5 * k, 7.0 - 0.25 * k, (k * 7) % 5 + 2 ** 33, np.asarray(cams, np.int64), np.asarray(sizes, np.int64), 10.0 + np.arange(len(sizes)))


def literal_fields(buf, n, g):
    """test_graph_oracle._native_plan's slicing, written out."""
    f64 = buf[:8 * (2 * n + g)].view(np.float64)
    i64 = buf[8 * (2 * n + g):8 * (3 * n + g)].view(np.int64)
    i32 = buf[8 * (3 * n + g):8 * (3 * n + g) + 4 * (5 * n + 2 * g + 3)].view(np.int32)
    return {"xw": f64[:n], "yw": f64[n:2 * n], "max_dist": f64[2 * n:], "ids": i64, "person": i32[:n], "cam": i32[n:2 * n],
            "graph_of": i32[2 * n:3 * n], "graph_ptr": i32[3 * n:3 * n + g + 1], "src_order": i32[3 * n + g + 1:4 * n + g + 1],
            "edge_ptr": i32[4 * n + g + 1:5 * n + g + 2], "edge_ptr_g": i32[5 * n + g + 2:5 * n + 2 * g + 3]}


@pytest.mark.parametrize("top_k", [None, 2])
@pytest.mark.parametrize("name", list(BATCHES))
def test_layout_reads_what_the_plan_wrote(name, top_k):
    import ctypes as C

    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.frames import FIELDS, INDEX, FrameLayout
    lib = nat.lib()
    xw, yw, ids, cams, sizes, md = (np.ascontiguousarray(v, t) for v, t in zip(make(name), (np.float64, np.float64, np.int64, np.int64, np.int64, np.float64)))
    n, g = len(cams), len(sizes)
    lay = FrameLayout(n, g)
    assert lay.nbytes == lib.gnncca_plan_frames_bytes(n, g) == 8 * (3 * n + g) + 4 * (5 * n + 2 * g + 3)
    buf = np.full(lay.nbytes + 16, 0xAB, np.uint8)
    args = (xw.ctypes.data, yw.ctypes.data, ids.ctypes.data, cams.ctypes.data, n, sizes.ctypes.data, md.ctypes.data, g)
    if top_k is None:
        e = lib.gnncca_plan_frames(*args, buf.ctypes.data, lay.nbytes)
    else:
        e = lib.gnncca_plan_frames_ex(*args, top_k, buf.ctypes.data, lay.nbytes, C.byref(C.c_int32(0)))
    assert e >= 0 and np.all(buf[lay.nbytes:] == 0xAB)
    want = literal_fields(buf, n, g)
    assert FIELDS == tuple(want)      # the documented order
    end = 0
    for f in FIELDS:
        got = lay.view(buf, f)
        assert got.dtype == want[f].dtype and np.array_equal(got, want[f]), f
        assert lay.cnt[INDEX[f]] == len(want[f]) and lay.off[INDEX[f]] == end, f      # contiguous, in the documented order
        assert len(got) == 0 or got.ctypes.data == buf.ctypes.data + end      # (numpy gives an empty view no address of its own)
        end += got.nbytes
    assert end == lay.nbytes == lay.off[-1]
    assert want["edge_ptr_g"][-1] == e and np.array_equal(want["ids"], ids) and np.array_equal(want["cam"], cams)
    # the native struct and the host lists come from the same offsets
    fr = lay.frames(buf.ctypes.data)
    for f, _ in nat.Frames._fields_:
        assert getattr(fr, f) == buf.ctypes.data + lay.off[INDEX["person" if f == "person_id" else f]]
    node_ptr, edge_ptr = lay.host_ptrs(torch.from_numpy(buf))
    assert node_ptr == want["graph_ptr"].tolist() and edge_ptr == want["edge_ptr_g"].tolist()


def test_check_cap_accepts_and_refuses_what_the_front_ends_do():
    from gnn_cca_amd.frames import check_cap
    for bad in (0, -1, 2.0, 2.5, "3", True):      # test_gpu_graph_topk.py::test_argument_errors_raise_before_any_launch
        with pytest.raises(ValueError, match="top_k must be"):
            check_cap(bad, "ground", None)
    for kw in (dict(top_k=2, rank_by="cosine"), dict(top_k=None, rank_by="cosine"), dict(top_k=2, rank_by=None)):
        with pytest.raises(ValueError, match="rank_by must be 'ground' or 'reid'"):
            check_cap(kw["top_k"], kw["rank_by"], None)
    # test_graph_sym_oracle.py::test_argument_refusals_come_before_the_gpu
    for sym in ("union", "mutual"):
        with pytest.raises(ValueError, match="it needs top_k"):
            check_cap(None, "ground", sym)
    for sym in ("both", True, 1, ""):
        with pytest.raises(ValueError, match="symmetric must be None, 'union' or 'mutual'"):
            check_cap(2, "ground", sym)
    with pytest.raises(ValueError, match="top_k must be >= 1"):
        check_cap(0, "ground", "union")
    with pytest.raises(ValueError, match="rank_by must be"):
        check_cap(2, "cosine", "union")
    assert check_cap(None, "ground", None) == (None, 0, 0) and check_cap(None, "reid", None) == (None, 1, 0)
    assert check_cap(np.int64(2), "ground", None) == (2, 0, 0) and type(check_cap(np.int64(2), "ground", None)[0]) is int
    assert check_cap(2, "reid", "union") == (2, 1, 1) and check_cap(3, "ground", "mutual") == (3, 0, 2)
    assert check_cap(2 ** 40, "ground", None)[0] == 2 ** 31 - 1
