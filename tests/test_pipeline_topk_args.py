"""FramePipeline(top_k=k, rank_by=...) and gnncca_frames_forward_topk, the parts that need no GPU: the constructor validates its cap like
build_graph_batch does (before a device is touched), the header declares the entry point and the ctypes binding mirrors it, the ABI
version did not move, and the entry point's own refusals come before anything is launched (the pointers are never followed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


class _StandIn:
    """A model object the constructor only stores."""


def test_constructor_validates_the_cap_like_build_graph_batch():
    from gnn_cca_amd.pipeline import FramePipeline
    for bad in (0, -1, 2.0, 2.5, "3", True, False, np.float32(2)):
        with pytest.raises(ValueError):
            FramePipeline(_StandIn(), top_k=bad)
    with pytest.raises(ValueError):
        FramePipeline(_StandIn(), top_k=2, rank_by="cosine")
    with pytest.raises(ValueError):
        FramePipeline(_StandIn(), rank_by="cosine")
    with pytest.raises(ValueError):
        FramePipeline(_StandIn(), top_k=2, rank_by=None)
    p = FramePipeline(_StandIn())
    assert p.top_k is None and p.rank_by == "ground"
    p = FramePipeline(_StandIn(), top_k=np.int64(2))
    assert p.top_k == 2 and type(p.top_k) is int
    p = FramePipeline(_StandIn(), top_k=3, rank_by="reid")
    assert (p.top_k, p.rank_by) == (3, "reid")
    assert FramePipeline(_StandIn(), top_k=10 ** 12).top_k == 2 ** 31 - 1      # an int32 on the way down, as in build_graph_batch
    assert callable(FramePipeline._arena)


def _declaration(header, name):
    m = re.search(r"GNNCCA_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_point_and_the_binding_mirrors_it():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    args = _declaration(header, "gnncca_frames_forward_topk")
    assert len(args) == 12
    assert [a.split()[-1] for a in args[-4:]] == ["top_k", "rank_by", "max_deg", "stream"]
    dense = _declaration(header, "gnncca_frames_forward")
    assert [a.split()[-1] for a in args[:8]] == [a.split()[-1] for a in dense[:8]] and len(dense) == 9
    res, argtypes = nat._SIGNATURES["gnncca_frames_forward_topk"]
    assert res is C.c_int and len(argtypes) == 12
    assert argtypes[:8] == nat._SIGNATURES["gnncca_frames_forward"][1][:8]
    assert argtypes[8:] == [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    assert hasattr(nat.lib(), "gnncca_frames_forward_topk")


def test_abi_version_and_io_struct_did_not_move():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    assert "#define GNNCCA_ABI_VERSION 2" in header and nat.ABI_VERSION == 2 == nat.lib().gnncca_abi_version()
    assert [n for n, _ in nat.FramesIO._fields_][-3:] == ["counters", "labels", "counters_len"] and len(nat.FramesIO._fields_) == 21


def test_entry_point_refuses_bad_caps_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    d = nat.MpnDims()
    n, g, e = 10, 2, 24
    io = nat.FramesIO()
    fake = 0x10000
    for name, t in nat.FramesIO._fields_:
        if t is C.c_void_p:
            setattr(io, name, fake)
    io.n_nodes, io.n_frames, io.n_edges, io.reid_dim, io.mode, io.normalize, io.counters_len = n, g, e, 8, 0, 0, 3 * n + 1 + g

    def call(top_k, rank_by, max_deg):
        return lib.gnncca_frames_forward_topk(C.byref(d), fake, C.byref(io), None, 0, None, 0, 0, top_k, rank_by, max_deg, None)

    for top_k, rank_by, max_deg in ((0, 0, 6), (-3, 0, 6), (3, 2, 6), (3, -1, 6), (3, 0, -1)):
        assert call(top_k, rank_by, max_deg) == nat.ERR_INVALID_ARG, (top_k, rank_by, max_deg)
    assert call(3, 0, nat.TOPK_MAX_DEG + 1) == nat.ERR_UNSUPPORTED
    # what gnncca_frames_forward refuses is refused here too: a short counters buffer, too many detections, a missing staging image
    io.counters_len = 3 * n + g
    assert call(3, 0, 6) == nat.ERR_INVALID_ARG
    io.counters_len, io.n_nodes = 3 * 5000 + 1 + g, 5000
    assert call(3, 0, 6) == nat.ERR_UNSUPPORTED
    io.n_nodes, io.counters_len, io.staged_dev = n, 3 * n + 1 + g, None
    assert call(3, 0, 6) == nat.ERR_INVALID_ARG
    # ranking by the reid distance reads the table in every mode, the ground-only one included
    io.staged_dev, io.mode, io.reid_dim = fake, 2, 0
    assert call(3, nat.RANK_BY["reid"], 6) == nat.ERR_INVALID_ARG
