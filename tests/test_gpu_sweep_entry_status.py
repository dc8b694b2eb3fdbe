"""What the four raw sweep entries answer to a call they refuse, and to a call with nothing to do (gnncca_eval_sweep, _exclusive, _joint,
_strong through nat.lib()): the status of every single bad argument, of zero frames and zero points, and the workspace sizes as literals.
Whatever the four share on the host side of csrc/evaluate.hip, this is what a caller sees of it, entry by entry.  No call here launches
anything: a refused call returns before its first launch, and so does a call without frames or points."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENTRIES = ("sweep", "exclusive", "joint", "strong")
N, E, G, T = 6, 4, 2, 2     # 2 frames x 3 nodes, 4 edges (one mutual pair per frame), 2 operating points
FILL = -7.0


def _nat():
    from gnn_cca_amd import _native as nat
    return nat


def _node_limit(entry):
    nat = _nat()
    return {"sweep": 4096, "exclusive": nat.EXCLUSIVE_MAX_FRAME_NODES, "joint": 4096, "strong": nat.STRONG_MAX_FRAME_NODES}[entry]


def _point_limit(entry):
    nat = _nat()
    return nat.SWEEP_MAX_THRESHOLDS if entry in ("sweep", "exclusive") else nat.JOINT_MAX_POINTS


def _workspace_bytes(entry, n, e, g):
    lib = _nat().lib()
    if entry == "sweep":
        return lib.gnncca_eval_sweep_workspace_bytes(n, e, g, T)
    if entry == "exclusive":
        return lib.gnncca_eval_sweep_exclusive_workspace_bytes(n, e, g, T)
    return getattr(lib, f"gnncca_eval_sweep_{entry}_workspace_bytes")(n, e, g)


class Call:
    """One good call of `entry` on the hand-made batch; `run(**changes)` makes it with some arguments replaced (a pointer by None = null)."""

    def __init__(self, entry):
        self.entry = entry
        dev = torch.device(DEV)
        self.t = {
            "ei": torch.tensor([[0, 1, 3, 4], [1, 0, 4, 3]], dtype=torch.int64, device=dev),
            "elab": torch.tensor([1, 1, 0, 0], dtype=torch.float32, device=dev),
            "scores": torch.tensor([0.9, 0.8, 0.2, 0.7], dtype=torch.float32, device=dev),
            "cam": torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32, device=dev),
            "node_ptr": torch.tensor([0, 3, 6], dtype=torch.int32, device=dev),
            "edge_ptr": torch.tensor([0, 2, 4], dtype=torch.int32, device=dev),
            "points": torch.tensor([0.5, 0.75], dtype=torch.float64, device=dev),
            "rows": torch.full((T, G, 16), FILL, dtype=torch.float64, device=dev),
            "labels": torch.full((T, N), -7, dtype=torch.int32, device=dev),
            "ws": torch.zeros(_workspace_bytes(entry, N, E, G), dtype=torch.uint8, device=dev),
        }
        self.good = {k: v.data_ptr() for k, v in self.t.items()}
        self.good.update(n=N, e=E, g=G, max_n=3, n_points=T, keep_le=0, ws_bytes=self.t["ws"].numel(), div=None,
                         score_ptrs=[self.good["scores"]], strides=[1], cmps=[0], n_scores=1, score_array=True, stride_array=True, cmp_array=True)

    def run(self, **changes):
        a = dict(self.good)
        a.update(changes)
        lib = _nat().lib()
        if self.entry == "sweep":
            return lib.gnncca_eval_sweep(a["ei"], a["elab"], a["scores"], a["n"], a["e"], a["node_ptr"], a["edge_ptr"], a["g"], a["max_n"], a["points"],
                                         a["n_points"], a["keep_le"], a["rows"], a["labels"], a["ws"], a["ws_bytes"], None)
        if self.entry == "exclusive":
            return lib.gnncca_eval_sweep_exclusive(a["ei"], a["elab"], a["scores"], a["cam"], a["n"], a["e"], a["node_ptr"], a["edge_ptr"], a["g"],
                                                   a["max_n"], a["points"], a["n_points"], a["rows"], a["labels"], a["ws"], a["ws_bytes"], None)
        k = len(a["score_ptrs"])
        ptrs = (C.c_void_p * k)(*a["score_ptrs"]) if a["score_array"] else None
        strides = (C.c_int64 * k)(*a["strides"]) if a["stride_array"] else None
        cmps = (C.c_int32 * k)(*a["cmps"]) if a["cmp_array"] else None
        fn = getattr(lib, f"gnncca_eval_sweep_{self.entry}")
        return fn(a["ei"], a["elab"], ptrs, strides, cmps, a["n_scores"], a["n"], a["e"], a["node_ptr"], a["edge_ptr"], a["g"], a["max_n"], a["points"],
                  a["n_points"], a["div"], a["rows"], a["labels"], a["ws"], a["ws_bytes"], None)

    def untouched(self):
        return bool((self.t["rows"] == FILL).all()) and bool((self.t["labels"] == -7).all())


@pytest.fixture(scope="module", params=ENTRIES)
def call(request):
    return Call(request.param)


def _joint(entry):
    return entry in ("joint", "strong")


def test_every_null_pointer_in_turn(call):
    """Every pointer an entry requires, null in turn: INVALID_ARG.  (labels_out and frame_div may be null: such a call is a good one.)"""
    nat = _nat()
    names = ["ei", "elab", "node_ptr", "edge_ptr", "points", "rows", "ws"]
    if call.entry == "exclusive":
        names += ["scores", "cam"]
    elif call.entry == "sweep":
        names += ["scores"]
    for name in names:
        assert call.run(**{name: None}) == nat.ERR_INVALID_ARG, name
    if _joint(call.entry):
        assert call.run(score_array=False) == nat.ERR_INVALID_ARG
        assert call.run(stride_array=False) == nat.ERR_INVALID_ARG
        assert call.run(cmp_array=False) == nat.ERR_INVALID_ARG
        assert call.run(score_ptrs=[None]) == nat.ERR_INVALID_ARG
    assert call.untouched()


def test_the_number_of_points(call):
    nat = _nat()
    zero = nat.OK if call.entry == "strong" else nat.ERR_INVALID_ARG     # the strong sweep takes "no points" as "nothing to do"
    assert call.run(n_points=0) == zero
    assert call.run(n_points=-1) == nat.ERR_INVALID_ARG
    assert call.run(n_points=_point_limit(call.entry) + 1) == nat.ERR_INVALID_ARG
    assert call.untouched()


def test_the_widest_frame(call):
    nat = _nat()
    limit = _node_limit(call.entry)
    assert call.run(max_n=limit + 1) == nat.ERR_INVALID_ARG
    # the entry's own limit, with enough nodes declared that `max_frame_nodes > n_nodes` is not what refuses: one above it is a bad
    # argument, the limit itself passes the size check and is stopped by the (now too small) workspace, before any launch
    assert call.run(n=limit + 1, max_n=limit + 1) == nat.ERR_INVALID_ARG
    assert call.run(n=limit, max_n=limit) == nat.ERR_WORKSPACE
    assert call.run(max_n=N + 1) == nat.ERR_INVALID_ARG
    assert call.run(max_n=-1) == nat.ERR_INVALID_ARG
    assert call.untouched()


def test_negative_sizes(call):
    nat = _nat()
    for name in ("n", "e", "g"):
        assert call.run(**{name: -1}) == nat.ERR_INVALID_ARG, name
    assert call.untouched()


@pytest.mark.parametrize("entry", ["joint", "strong"])     # (the two others take one score and no comparator array)
def test_comparators_strides_and_the_number_of_scores(entry):
    nat = _nat()
    call = Call(entry)
    assert call.run(cmps=[4]) == nat.ERR_INVALID_ARG
    assert call.run(cmps=[-1]) == nat.ERR_INVALID_ARG
    assert call.run(strides=[0]) == nat.ERR_INVALID_ARG
    assert call.run(n_scores=0) == nat.ERR_INVALID_ARG
    assert call.run(n_scores=nat.JOINT_MAX_SCORES + 1, score_ptrs=[call.good["scores"]] * 5, strides=[1] * 5, cmps=[0] * 5) == nat.ERR_INVALID_ARG
    # the second of two scores is checked like the first
    two = dict(n_scores=2, score_ptrs=[call.good["scores"]] * 2, strides=[1, 1], cmps=[0, 3])
    assert call.run(**{**two, "cmps": [0, 4]}) == nat.ERR_INVALID_ARG
    assert call.run(**{**two, "strides": [1, 0]}) == nat.ERR_INVALID_ARG
    assert call.run(**{**two, "score_ptrs": [call.good["scores"], None]}) == nat.ERR_INVALID_ARG
    assert call.untouched()


def test_a_workspace_one_byte_short(call):
    nat = _nat()
    assert call.run(ws_bytes=call.good["ws_bytes"] - 1) == nat.ERR_WORKSPACE
    assert call.run(ws_bytes=0) == nat.ERR_WORKSPACE
    assert call.untouched()


def test_no_frames_is_ok_and_writes_nothing(call):
    nat = _nat()
    assert call.run(g=0) == nat.OK
    # what comes after the "no frames" answer is not looked at ...
    later = dict(g=0, node_ptr=None, edge_ptr=None, rows=None, ws=None, ws_bytes=0, ei=None, elab=None, cam=None)
    assert call.run(**later) == nat.OK
    # ... and what comes before it is: the sizes, the points (the strong sweep asks for them only when it has frames), the scores
    assert call.run(g=0, max_n=N + 1) == nat.ERR_INVALID_ARG
    assert call.run(g=0, n_points=_point_limit(call.entry) + 1) == nat.ERR_INVALID_ARG
    assert call.run(g=0, points=None) == (nat.OK if call.entry == "strong" else nat.ERR_INVALID_ARG)
    if _joint(call.entry):
        assert call.run(g=0, cmps=[4]) == nat.ERR_INVALID_ARG
        assert call.run(g=0, score_ptrs=[None]) == nat.ERR_INVALID_ARG
    assert call.untouched()


# recorded from the tree before the four entries shared one host path: the layouts are [plan | rev | (keys) | lgamma tables]
WORKSPACE_BYTES = {
    "sweep": {(0, 0, 0): 1024, (6, 4, 2): 2048, (4096, 10000, 3): 187392},
    "exclusive": {(0, 0, 0): 1024, (6, 4, 2): 2304, (4096, 10000, 3): 267520},
    "joint": {(0, 0, 0): 1024, (6, 4, 2): 2048, (4096, 10000, 3): 187392},
    "strong": {(0, 0, 0): 256, (6, 4, 2): 256, (4096, 10000, 3): 33024},      # the lgamma tables alone
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_workspace_sizes(entry):
    for (n, e, g), want in WORKSPACE_BYTES[entry].items():
        assert _workspace_bytes(entry, n, e, g) == want, (entry, n, e, g)
    assert _workspace_bytes(entry, -1, 0, 0) == 0 and _workspace_bytes(entry, 0, -1, 0) == 0 and _workspace_bytes(entry, 0, 0, -1) == 0
