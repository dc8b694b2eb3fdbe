"""Every selection of the graph build -- top_k (both keys), symmetric 'union' / 'mutual', radius -- emits its edges through the one device
function the dense build uses (csrc/graph_build.hip: emit_edges), so a kept edge carries the dense build's bits.  Stated here across all
of them on ONE batch: three frames of 5, 70 and 130 detections on three cameras (one, two and three 64-candidate chunks per source, the
last one partial), in each edge-attribute mode, with a reid width the kernels read by scalar loads (6) and one they read by float4 (8).
Every edge of every variant is looked up by (src, dst) in the dense list; its attribute row and its label must be the dense ones, compared
as int32 words (a NaN or a -0.0 cannot hide a difference).  A variant that kept nothing, or everything, would pass that vacuously: in the
frames of 70 and 130 detections each one must keep an edge and drop an edge."""
import numpy as np
import pytest
import torch

import graph_radius_oracle as gro
from test_gpu_graph_radius import bits, build

pytestmark = pytest.mark.gpu

SIZES, SEED, RADIUS = (5, 70, 130), 7, 9.5      # positions are uniform in a 20 x 20 square: radius 9.5 keeps roughly half the pairs
VARIANTS = [dict(top_k=3, rank_by="ground"), dict(top_k=3, rank_by="reid"), dict(top_k=3, symmetric="union"), dict(top_k=3, symmetric="mutual"),
            dict(radius=RADIUS)]


def batch(reid_dim, **modes):
    rng = np.random.default_rng(SEED)
    cams = [rng.integers(0, 3, s) for s in SIZES]
    n = sum(SIZES)
    return gro.case(cams, rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), seed=SEED, max_dist=rng.uniform(10, 50, len(SIZES)), reid_dim=reid_dim,
                    **modes)


@pytest.mark.parametrize("reid_dim", [6, 8])
@pytest.mark.parametrize("modes", [{}, dict(only_appearance=True), dict(only_dist=True)], ids=["full", "only_appearance", "only_dist"])
def test_every_variant_carries_the_dense_bits(modes, reid_dim):
    a = batch(reid_dim, **modes)
    n = sum(SIZES)
    dense = build(a)
    dense_key = dense.edge_index[0] * n + dense.edge_index[1]      # unique: the dense list holds a pair once per direction
    sorted_key, order = torch.sort(dense_key)
    for kw in VARIANTS:
        b = build(a, **kw)
        key = b.edge_index[0] * n + b.edge_index[1]
        at = torch.searchsorted(sorted_key, key).clamp_(max=sorted_key.numel() - 1)
        assert torch.equal(sorted_key[at], key), kw      # every edge is a dense edge
        where = order[at]
        assert torch.equal(bits(b.edge_attr), bits(dense.edge_attr[where])), kw
        assert torch.equal(bits(b.edge_labels), bits(dense.edge_labels[where])), kw
        for f in (1, 2):
            kept, full = b.edge_ptr[f + 1] - b.edge_ptr[f], dense.edge_ptr[f + 1] - dense.edge_ptr[f]
            assert 0 < kept < full, (kw, f, kept, full)
