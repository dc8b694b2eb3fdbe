"""The threshold sweep over the camera-exclusive partition (calibration.sweep_thresholds(partition='exclusive'),
gnncca_eval_sweep_exclusive), the parts that need no GPU: the two properties of the rule the one-pass kernel rests on, checked with the
sequential walk of tests/exclusive_oracle.py -- a pair's key does not depend on the threshold, and the keys with w >= th, largest first,
ARE the walk's candidate order at th, so that the partitions nest as the threshold falls --; every refusal before a device is touched
(host tensors stand in: a check that came too late would raise the module's "MI355X only" RuntimeError instead); and the two entry
points declared, bound, exported and refusing before any launch."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

import exclusive_oracle as oracle
from conftest import ROOT

THRESHOLDS = (0.2, 0.375, 0.5, 0.625, 0.8)


def _random_frame(rng, n, cams, density, coarse):
    """n nodes on `cams` cameras, every cross-camera ordered pair an edge with probability `density`, the two directions of a pair scored
    separately: multiples of 1/8 from 0 to 1 (ties everywhere, a few zeros) or continuous, a NaN now and then."""
    cam = rng.integers(0, cams, size=n)
    src, dst = [], []
    for i in range(n):
        for j in range(n):
            if i != j and cam[i] != cam[j] and rng.random() < density:
                src.append(i), dst.append(j)
    e = len(src)
    scores = (rng.integers(0, 9, size=e) / 8.0 if coarse else rng.random(e)).astype(np.float32)
    scores[rng.random(e) < 0.03] = np.nan
    return cam, np.asarray(src, np.int64), np.asarray(dst, np.int64), scores


def _keys(src, dst, scores):
    """The kernel's key array restated: for every pair {lo, hi} whose two edges exist with scores that are not NaN and > 0,
    (float32 bits of the smaller score) << 24 | (4095 - lo) << 12 | (4095 - hi) -> {key: (w, lo, hi)}.  No threshold anywhere."""
    where = {}
    for k, (a, b) in enumerate(zip(src.tolist(), dst.tolist())):
        where.setdefault((a, b), k)
    out = {}
    for (i, j), k in where.items():
        r = where.get((j, i))
        if i < j and r is not None and scores[k] > 0 and scores[r] > 0:
            w = np.float32(min(scores[k], scores[r]))
            bits = struct.unpack("<I", struct.pack("<f", float(w)))[0]
            out[(bits << 24) | ((4095 - i) << 12) | (4095 - j)] = (w, i, j)
    return out


def _refines(fine, coarse):
    """True iff every cluster of `fine` lies inside one cluster of `coarse`."""
    seen = {}
    return all(seen.setdefault(int(f), int(c)) == int(c) for f, c in zip(fine, coarse))


def test_keys_do_not_depend_on_the_threshold_and_the_partitions_nest():
    rng = np.random.default_rng(23)
    frames = strict = 0
    for trial in range(240):
        n = int(rng.integers(2, 15))
        cams = int(rng.choice([2, 3, 4, 6]))
        cam, src, dst, scores = _random_frame(rng, n, cams, float(rng.choice([0.4, 0.7, 1.0])), coarse=trial % 2 == 0)
        ei = np.stack([src, dst]).reshape(2, -1)
        keys = _keys(src, dst, scores)
        assert len(keys) == len({(lo, hi) for _w, lo, hi in keys.values()})          # the key alone names the pair
        ranked = sorted(keys, reverse=True)                                          # the LARGEST key is the FIRST candidate
        previous = None
        for th in sorted(THRESHOLDS, reverse=True):
            want = [(int(i), int(j)) for _w, i, j, _k, _r in
                    oracle.sort_candidates(oracle.candidates(src, dst, scores, 0, len(src), 0, n, th))]
            got = [keys[key][1:] for key in ranked if float(np.float64(keys[key][0])) >= th]
            assert got == want, (trial, th)                                          # w >= th is "both edges active", the order is the keys'
            labels = oracle.exclusive_oracle(ei, scores, cam, [0, n], [0, len(src)], th)["labels"]
            if previous is not None:
                assert _refines(previous, labels), (trial, th)                       # the lower threshold continues the higher one's walk
                strict += int(not np.array_equal(previous, labels))
            previous = labels
        frames += 1
    assert frames >= 200 and strict >= 200, (frames, strict)                         # and the thresholds do change the partitions


class _Batch:
    """What sweep_thresholds(partition='exclusive') reads of a GraphBatch, on the host."""

    def __init__(self, sizes=(3, 2), e=8, cam=(0, 1, 2, 0, 1), cam_host=True):
        self.node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        self.edge_ptr = [0, e // 2, e][:len(sizes) + 1]
        self.edge_index = torch.zeros((2, e), dtype=torch.int64)
        self.edge_labels = torch.zeros(e)
        self.node_ptr_dev = torch.tensor(self.node_ptr, dtype=torch.int32)
        self.edge_ptr_dev = torch.tensor(self.edge_ptr, dtype=torch.int32)
        if cam is not None:
            self.cam_dev = torch.tensor(cam, dtype=torch.int32)
            if cam_host:
                self.cam_host = np.asarray(cam, dtype=np.int64)


def test_every_value_error_comes_before_the_gpu_is_touched():
    from gnn_cca_amd.calibration import PARTITIONS, sweep_thresholds
    from gnn_cca_amd.pipeline import FrameResult
    assert PARTITIONS == ("components", "exclusive")
    b, s = _Batch(), torch.zeros(8)
    for bad in ("exclusive ", "Exclusive", "cc", None, 1, ["exclusive"]):
        with pytest.raises(ValueError, match="partition"):
            sweep_thresholds(b, s, [0.5], partition=bad)
    with pytest.raises(ValueError, match="keep='ge' only"):
        sweep_thresholds(b, s, [0.5], keep="le", partition="exclusive")
    for ths in ([0.5, 0.0], [1.0], [0.3, -0.1], [1.5, 0.5], np.linspace(0, 1, 11)):
        with pytest.raises(ValueError, match="between 0 and 1"):
            sweep_thresholds(b, s, ths, partition="exclusive")
    for ths in ([], [float("nan")], [[0.1, 0.2]], np.full(1025, 0.5)):               # the sweep's own refusals hold as well
        with pytest.raises(ValueError):
            sweep_thresholds(b, s, ths, partition="exclusive")
    for cam in ((0, 1, 64, 0, 1), (0, -1, 2, 0, 1)):
        with pytest.raises(ValueError, match="camera ids"):                          # the batch's host copy
            sweep_thresholds(_Batch(cam=cam), s, [0.5], partition="exclusive")
        with pytest.raises(ValueError, match="camera ids"):                          # a host tensor handed over
            sweep_thresholds(_Batch(cam=None), s, [0.5], partition="exclusive", cam=torch.tensor(cam, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs camera ids"):
        sweep_thresholds(_Batch(cam=None), s, [0.5], partition="exclusive")
    with pytest.raises(ValueError, match="does not match"):
        sweep_thresholds(b, s, [0.5], partition="exclusive", cam=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="does not match"):
        sweep_thresholds(b, s, [0.5], partition="exclusive", cam=[0, 1, 2, 0, 1])
    with pytest.raises(ValueError, match="do not match"):
        sweep_thresholds(b, torch.zeros(7), [0.5], partition="exclusive")
    with pytest.raises(ValueError, match="at most 4096"):
        sweep_thresholds(_Batch(sizes=(4097, 2), cam=[0] * 4099), s, [0.5], partition="exclusive")
    # what is left is a well-formed call on host tensors: the module's usual refusal -- for the new partition (camera 63 included, with
    # and without a host copy of the cameras) and, unchanged, for the default one with thresholds the exclusive rule would refuse
    for batch, kw in ((b, {}), (_Batch(cam=(0, 63, 2, 0, 1)), {}), (_Batch(cam_host=False), {}), (_Batch(cam=None), {"cam": b.cam_dev})):
        with pytest.raises(RuntimeError, match="MI355X only"):
            sweep_thresholds(batch, s, [0.9, 0.1, 0.9], partition="exclusive", **kw)
    for kw in ({}, {"partition": "components"}, {"partition": "components", "keep": "le"}):
        with pytest.raises(RuntimeError, match="MI355X only"):
            sweep_thresholds(b, s.view(-1, 1), np.linspace(0, 1, 7), **kw)

    # FrameResult.sweep passes the keyword through and, like exclusive(), judges the batch's host camera ids first
    for batch, word in ((_Batch(cam=(0, 1, 64, 0, 1)), "camera ids"), (_Batch(cam_host=False), "host camera ids")):
        r = FrameResult()
        r.batch, r.probs = batch, s
        with pytest.raises(ValueError, match=word):
            r.sweep([0.5], partition="exclusive")
    r = FrameResult()
    r.batch, r.probs = b, s
    with pytest.raises(ValueError, match="partition"):
        r.sweep([0.5], partition="both")
    for kw in ({}, {"partition": "components"}, {"partition": "exclusive"}):
        with pytest.raises(RuntimeError, match="MI355X only"):
            r.sweep([0.25, 0.5], **kw)


def _declaration(header, name, result="int"):
    m = re.search(r"GNNCCA_API\s+" + result + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_binding_mirrors_them():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    lib = nat.lib()
    for name, result, res, count in (("gnncca_eval_sweep_exclusive_workspace_bytes", "size_t", C.c_size_t, 4),
                                     ("gnncca_eval_sweep_exclusive", "int", C.c_int, 17),
                                     ("gnncca_eval_sweep_workspace_bytes", "size_t", C.c_size_t, 4), ("gnncca_eval_sweep", "int", C.c_int, 17)):
        args = _declaration(header, name, result)
        got_res, argtypes = nat._SIGNATURES[name]
        assert len(args) == count == len(argtypes) and got_res is res, name
        assert name in nat.exported_symbols() and hasattr(lib, name)
    # gnncca_eval_sweep's arguments plus cam, without keep_le
    old = [a.split()[-1].lstrip("*") for a in _declaration(header, "gnncca_eval_sweep")]
    new = [a.split()[-1].lstrip("*") for a in _declaration(header, "gnncca_eval_sweep_exclusive")]
    assert "keep_le" in old and "keep_le" not in new and new.index("cam") == 3
    assert [a for a in new if a != "cam"] == [a for a in old if a != "keep_le"]
    assert nat._SIGNATURES["gnncca_eval_sweep_exclusive"][1][11] is C.c_int32 and nat._SIGNATURES["gnncca_eval_sweep_exclusive"][1][15] is C.c_size_t
    assert "#define GNNCCA_ABI_VERSION 2" in header and nat.ABI_VERSION == 2 == lib.gnncca_abi_version()
    # the rule is in the header in full
    section = header[header.index("Threshold sweep over the CAMERA-EXCLUSIVE partition"):header.index("gnncca_eval_sweep_exclusive_workspace_bytes(int64_t")]
    section = re.sub(r"\s*\n \* +", " ", section)                                   # (the comment's line breaks)
    for word in ("bit for bit", "does not depend on the threshold", "NaN row", "every node its own cluster", "duplicate ordered pairs",
                 "threshold <= 0", "no memset", "does not depend on n_thresholds", "partitions nest"):
        assert word in section, word


def test_entry_point_refuses_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000
    n, e, g = 10, 24, 2
    ws = lib.gnncca_eval_sweep_exclusive_workspace_bytes(n, e, g, 5)
    assert ws > 0 and ws % 256 == 0
    assert lib.gnncca_eval_sweep_exclusive_workspace_bytes(n, e, g, 1000) == ws == lib.gnncca_eval_sweep_exclusive_workspace_bytes(n, e, g, 1)
    assert ws >= lib.gnncca_eval_sweep_workspace_bytes(n, e, g, 5) + 8 * e           # the component sweep's, plus one u64 per edge
    for bad in ((-1, e, g, 5), (n, -1, g, 5), (n, e, -1, 5), (n, e, g, -1)):
        assert lib.gnncca_eval_sweep_exclusive_workspace_bytes(*bad) == 0

    def call(t=5, max_n=6, ei=fake, el=fake, sc=fake, cam=fake, nptr=fake, eptr=fake, th=fake, rows=fake, work=fake, nbytes=ws, nn=n, ee=e, gg=g):
        return lib.gnncca_eval_sweep_exclusive(ei, el, sc, cam, nn, ee, nptr, eptr, gg, max_n, th, t, rows, None, work, nbytes, None)

    for t in (0, -1, 1025, 1 << 20):
        assert call(t=t) == nat.ERR_INVALID_ARG, t
    for max_n in (4097, -1, n + 1):
        assert call(max_n=max_n) == nat.ERR_INVALID_ARG, max_n
    for name in ("ei", "el", "sc", "cam", "nptr", "eptr", "th", "rows", "work"):
        assert call(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert call(nn=-1) == nat.ERR_INVALID_ARG and call(ee=-1) == nat.ERR_INVALID_ARG and call(gg=-1) == nat.ERR_INVALID_ARG
    assert call(nbytes=ws - 1) == nat.ERR_WORKSPACE
    assert call(gg=0, nptr=None, eptr=None, rows=None, work=None, nbytes=0) == nat.OK                  # nothing to score: nothing launched
    assert call(gg=0, th=None) == nat.ERR_INVALID_ARG and call(gg=0, t=0) == nat.ERR_INVALID_ARG       # (the component sweep's order of refusals)
