"""The frame-range validation exclusive_clusters and strong_clusters share (postprocess._frame_ranges), without a GPU: it runs before
the `.is_cuda` check, so host tensors reach every ValueError, and a well-formed call on host tensors ends in the module's "MI355X only"
RuntimeError -- which shows that the validation let it through.  Both functions, the same cases, each with its own limit (4096 / 1024);
the messages are matched in full where they name the function or the limit."""
import re

import numpy as np
import pytest
import torch

from gnn_cca_amd.postprocess import MAX_FRAME_NODES, STRONG_MAX_FRAME_NODES, exclusive_clusters, strong_clusters

EI = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])           # three nodes, four edges
NONE = torch.zeros((2, 0), dtype=torch.int64)


def _exclusive(n, node_ptr, edge_ptr, ei=EI, **kw):
    e = ei.shape[1]
    return exclusive_clusters(ei, torch.full((e,), 0.9), torch.arange(n, dtype=torch.int32) % 4, n, node_ptr, edge_ptr, **kw)


def _strong(n, node_ptr=None, edge_ptr=None, ei=EI, **kw):
    return strong_clusters(ei, torch.ones(ei.shape[1], dtype=torch.int64), n, node_ptr, edge_ptr, **kw)


CALLS = [pytest.param(_exclusive, "exclusive_clusters", MAX_FRAME_NODES, id="exclusive"),
         pytest.param(_strong, "strong_clusters", STRONG_MAX_FRAME_NODES, id="strong")]


def test_the_limits_are_the_headers():
    assert MAX_FRAME_NODES == 4096 and STRONG_MAX_FRAME_NODES == 1024


def test_node_ptr_without_edge_ptr():
    with pytest.raises(ValueError, match="node_ptr and edge_ptr are required"):
        _exclusive(3, [0, 3], None)
    with pytest.raises(ValueError, match="node_ptr and edge_ptr are required"):
        _exclusive(3, None, [0, 4])
    with pytest.raises(ValueError, match="node_ptr and edge_ptr go together"):
        _strong(3, [0, 3], None)
    with pytest.raises(ValueError, match="node_ptr and edge_ptr go together"):
        _strong(3, None, [0, 4])


@pytest.mark.parametrize("call, name, limit", CALLS)
def test_offsets_that_are_no_frame_ranges(call, name, limit):
    both = re.escape("node_ptr / edge_ptr must both have G + 1 entries")
    for node_ptr, edge_ptr in (([0, 1, 3], [0, 4]), ([0, 3], [0, 2, 4]),
                               (torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 2, 4], dtype=torch.int32))):
        with pytest.raises(ValueError, match=both):
            call(3, node_ptr, edge_ptr)
    for what, bad in (("node_ptr", [[0, 3]]), ("edge_ptr", 4), ("node_ptr", [0.0, 3.0]), ("node_ptr", [0])):   # not one row of two or more integers
        with pytest.raises(ValueError, match=what + re.escape(" must hold G + 1 integer offsets")):
            call(3, bad if what == "node_ptr" else [0, 3], bad if what == "edge_ptr" else [0, 4])
    nodes = "node_ptr must ascend from 0 to n_nodes"
    for node_ptr, edge_ptr in (([1, 3], [0, 4]),                       # does not start at 0
                               ([0, 2], [0, 4]), ([0, 4], [0, 4]),     # does not end at n_nodes
                               ([0, 2, 1, 3], [0, 4, 4, 4]),           # descends
                               (torch.tensor([0, 2, 1, 3]), [0, 4, 4, 4])):
        with pytest.raises(ValueError, match=nodes):
            call(3, node_ptr, edge_ptr)
    edges = "edge_ptr must ascend from 0 to E"
    for edge_ptr in ([0, 1, 3], [0, 1, 5], [1, 2, 4], [0, 5, 4]):
        with pytest.raises(ValueError, match=edges):
            call(3, [0, 1, 3], edge_ptr)
    with pytest.raises(ValueError, match=nodes):                       # node_ptr is judged first
        call(3, [0, 2], [0, 3])


@pytest.mark.parametrize("call, name, limit", CALLS)
def test_a_frame_one_above_the_limit(call, name, limit):
    wide = limit + 1
    message = re.escape(f"a frame has {wide} detections; {name} takes frames of at most {limit}")
    with pytest.raises(ValueError, match=message):
        call(wide, [0, wide], [0, 0], ei=NONE)
    with pytest.raises(ValueError, match=message):
        call(wide + 5, [0, 5, wide + 5], [0, 0, 0], ei=NONE)
    with pytest.raises(ValueError, match=message):                     # whatever the caller says the widest frame is
        call(wide + 5, [0, 5, wide + 5], [0, 0, 0], ei=NONE, max_frame_nodes=5)
    with pytest.raises(RuntimeError, match="runs on MI355X only"):     # the limit itself is a frame like any other
        call(limit + 5, [0, 5, limit + 5], [0, 0, 0], ei=NONE)


@pytest.mark.parametrize("call, name, limit", CALLS)
def test_max_frame_nodes_outside_its_range(call, name, limit):
    for host in (True, False):                                         # sequences, and tensors as they would come from the device
        node_ptr, edge_ptr = ([0, 3], [0, 4]) if host else (torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32))
        for bad in (-1, limit + 1):
            with pytest.raises(ValueError, match=re.escape(f"max_frame_nodes must lie in [0, {limit}], not {bad}")):
                call(3, node_ptr, edge_ptr, max_frame_nodes=bad)
        for fine in (0, 2, 3, limit):                                  # (clamped to n_nodes; a frame above it is the kernel's to flag)
            with pytest.raises(RuntimeError, match="runs on MI355X only"):
                call(3, node_ptr, edge_ptr, max_frame_nodes=fine)


def test_a_whole_graph_without_ranges_must_itself_fit():
    with pytest.raises(ValueError, match=re.escape("the graph has 1025 detections; strong_clusters takes frames of at most 1024 "
                                                   "(pass node_ptr / edge_ptr for a batch of frames)")):
        _strong(1025, ei=NONE)
    with pytest.raises(ValueError, match="max_frame_nodes must lie in"):
        _strong(3, max_frame_nodes=1025)
    for n in (3, 1024):
        with pytest.raises(RuntimeError, match="runs on MI355X only"):
            _strong(n, ei=EI if n == 3 else NONE)


@pytest.mark.parametrize("call, name, limit", CALLS)
def test_valid_host_ranges_pass_the_validation(call, name, limit):
    for node_ptr, edge_ptr in (([0, 3], [0, 4]), ([0, 1, 3], [0, 0, 4]), ([0, 0, 3, 3], [0, 0, 4, 4]), ((0, 3), (0, 4)),
                               (np.array([0, 2, 3], dtype=np.int32), np.array([0, 2, 4], dtype=np.int64)),
                               (torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32)),
                               (torch.tensor([0, 3]), [np.int64(0), np.int64(4)])):
        with pytest.raises(RuntimeError, match="runs on MI355X only"):
            call(3, node_ptr, edge_ptr)
