"""The views of the staging image that a batch carries (gnn_cca_amd.frames.attach): node_ptr / node_ptr_dev, edge_ptr / edge_ptr_dev, y,
person_dev and cam_dev, from graph_build.build_graph_batch and from pipeline.FramePipeline on the same inputs -- equal to each other and to
what the host knows.  Inputs: the golden fixtures one_frame and batch3 and the hand-made (5, 3) batch of test_frames_layout.py (an empty
frame, a single-camera frame); graphs: dense, top_k=2, and top_k=2 closed under reversal (which takes the step-by-step path by design)."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from test_frames_layout import make

pytestmark = pytest.mark.gpu
VARIANTS = {"dense": {}, "top2": dict(top_k=2), "top2_union": dict(top_k=2, symmetric="union")}
NODE_DIM = 8      # of the fixtures' node embeddings

_model = []


def model():
    if not _model:
        import bench
        params = copy.deepcopy(bench.graph_net_params(L=4))
        params["encoder_feats_dict"]["nodes"]["resnet50"]["node_in_dim"] = NODE_DIM
        _model.append(bench.build_model(params, 20, seed=0).cuda().eval())
    return _model[0]


def inputs(case):
    if case == "n5_g3":
        xw, yw, ids, cams, sizes, md = make(case)
        rng = np.random.default_rng(5)
        node, reid = rng.standard_normal((len(cams), NODE_DIM)), rng.standard_normal((len(cams), 16))
    else:
        z = np.load(os.path.join(GOLDEN_DIR, f"graph_{case}.npz"))
        xw, yw, ids, cams, sizes, md, node, reid = (z[k] for k in ("xw", "yw", "id", "id_cam", "graph_sizes", "max_dist", "node_embeds_raw",
                                                                   "reid_embeds_raw"))
    return (xw, yw, ids, cams, sizes, md), torch.from_numpy(node.astype(np.float32)).cuda(), torch.from_numpy(reid.astype(np.float32)).cuda()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", ["one_frame", "batch3", "n5_g3"])
def test_both_front_ends_carry_the_hosts_frame_ranges_and_ids(case, variant):
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    host, node, reid = inputs(case)
    ids, cams, sizes = (np.asarray(host[k]) for k in (2, 3, 4))
    n, kw = len(cams), VARIANTS[variant]
    built = build_graph_batch(*host, node, reid, **kw)
    piped = FramePipeline(model(), **kw)(*host, node, reid).batch
    torch.cuda.synchronize()
    node_ptr = [0] + np.cumsum(sizes).tolist()
    # cross-camera candidates of every detection in its own frame, in node order: the dense and the capped edge counts per frame
    deg = np.concatenate([[hi - lo - np.count_nonzero(cams[lo:hi] == c) for c in cams[lo:hi]] for lo, hi in zip(node_ptr, node_ptr[1:])] + [[]])
    for b in (built, piped):
        src = b.edge_index[0].cpu().numpy()
        assert b.node_ptr == node_ptr and b.node_ptr_dev.dtype == torch.int32 and b.node_ptr_dev.cpu().tolist() == node_ptr
        assert b.edge_ptr == [int(np.count_nonzero(src < lo)) for lo in node_ptr]      # edges are emitted frame by frame
        assert b.edge_ptr_dev.dtype == torch.int32 and b.edge_ptr_dev.cpu().tolist() == b.edge_ptr
        assert b.edge_ptr[0] == 0 and b.edge_ptr[-1] == b.edge_index.shape[1]
        if "symmetric" not in kw:
            kept = np.minimum(deg, kw["top_k"]) if kw else deg
            assert b.edge_ptr == [int(kept[:lo].sum()) for lo in node_ptr]
        assert b.y.dtype == torch.int64 and np.array_equal(b.y.cpu().numpy(), ids)
        assert b.cam_dev.dtype == torch.int32 and np.array_equal(b.cam_dev.cpu().numpy(), cams)
        person = b.person_dev.cpu().numpy()
        assert b.person_dev.dtype == torch.int32 and person.shape == (n,)
        assert np.array_equal(person[:, None] == person[None, :], ids[:, None] == ids[None, :])      # a relabelling that preserves equality
    assert built.node_ptr == piped.node_ptr and built.edge_ptr == piped.edge_ptr
    for f in ("node_ptr_dev", "edge_ptr_dev", "y", "person_dev", "cam_dev", "edge_index"):
        assert torch.equal(getattr(built, f), getattr(piped, f)), f
