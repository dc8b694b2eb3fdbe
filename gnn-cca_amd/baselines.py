"""The reference's position baselines on the GNN's own batches: geometrical_association and geometrical_appearance_association
(inference.py:628-954, main.py:431-464) -- the other "methods the GNN has to beat", next to the ReID threshold (calibration) and the
Rank-R baseline (rerank).  Their rule is a conjunction of conditions on the edge attributes, which calibration.sweep_joint scores in
one pass (csrc/eval_sweep_joint.cuh):

    rows = geometry_baseline(batch, geom_th, max_dist)                       # MODE geometrical_association
    rows = geometry_baseline(batch, geom_th, max_dist, reid_th=th)           # MODE geometrical_appearance_association
    rows = sweep_grid(batch, [batch.edge_attr[:, 0], batch.edge_attr[:, 2]], [geom_axis, reid_axis], ['lt', 'lt'],
                      frame_div=np.stack([max_dist, np.ones_like(max_dist)]))   # the tables GEOM_TH / OPT_TH, both axes at once

    rows = geometry_baseline(batch, geom_th, max_dist, partition='strong')   # ... clustered as the reference clusters them

Which partition (include/gnncca_mpn.h has both rules in full): the reference never prunes in these modes and clusters with the strongly
connected components of the digraph of active edges (inference.py:733-738, 904-908), so with a score that is not symmetric
(F.pairwise_distance adds eps to a - b) a directed cycle without a mutual pair joins nodes there.  partition='strong' is that rule, in
geometry_baseline, sweep_joint and sweep_grid (csrc/eval_sweep_strong.cuh): rows[t] is evaluate_frames(batch, predictions,
postprocess.strong_clusters(batch.edge_index, predictions, ...)['labels']) of the unpruned predictions.  The default,
partition='components', scores mutual pairs only (the pruning rule).  Two differences from the reference stay under either partition:
inference.py:892,896 use the LAST graph's labels and max_dist[0] for a whole batch, where here every frame has its own labels and its
own max_dist; and the reference divides the ReID distance by max_dist_L2 (inference.py:845), where geometry_baseline multiplies the
threshold (see there).

What these baselines score on real features is unmeasured here, like the others: no data set and no trained ReID model exist in this
repository."""
import numpy as np

from .calibration import sweep_joint

GEOMETRY_COLUMN = 0   # edge_attr[:, 0]: the ground distance, divided by the frame's max_dist (graph_build)
REID_L2_COLUMN = 2    # edge_attr[:, 2]: the L2 distance between the ReID embeddings


def geometry_baseline(batch, geom_th, max_dist, reid_th=None, max_dist_l2=1.0, partition="components"):
    """Scores every frame of a full-mode `batch` (edge_attr [E, 4], as graph_build.build_graph_batch and FramePipeline make it) under the
    reference's geometric rule -> float64 [G, 16] on the device (columns evaluation.METRICS), one sweep_joint call at one point.

    An edge is active iff edge_attr[:, 0] < geom_th / max_dist[g] (strict, inference.py:722): `geom_th` the GEOM_TH table's value in
    metres, `max_dist` the host sequence [G] of the frames' normalisers, the ones the batch was built with.  With `reid_th` the edge must
    also have edge_attr[:, 2] < reid_th * max_dist_l2 (inference.py:896).  The reference DIVIDES the distance by max_dist_L2
    (inference.py:845) where this multiplies the threshold: the two are not the same bits, and an edge whose normalised distance lies
    within a rounding of the threshold can fall on the other side.  Whoever needs the reference's comparison passes an already
    normalised score to calibration.sweep_joint.  From there on sweep_joint's rule, by `partition`: 'components' (the default) keeps
    an edge iff the reverse edge is active too and takes the connected components of the kept edges; 'strong' prunes nothing and takes
    the strongly connected components of the active edges, which is what the reference does in these modes.

    ROUNDING / SPLITTING are not part of this call.  To reach them, run postprocess.finalize on these predictions with the geometry
    score where the probabilities stand -- that is what inference.py:742,753 pass (spatial_dist_g as preds_prob)."""
    attr = getattr(batch, "edge_attr", None)
    if attr is None or attr.dim() != 2 or attr.shape[1] != 4:
        shape = None if attr is None else list(attr.shape)
        raise ValueError(f"geometry_baseline needs a full-mode batch (edge_attr [E, 4]: ground distance, ..., ReID L2 distance, ...), not {shape}")
    g = len(batch.node_ptr) - 1
    try:
        md = np.array(max_dist, dtype=np.float64).reshape(-1)
        geom, l2 = float(geom_th), float(max_dist_l2)
        reid = None if reid_th is None else float(reid_th)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"geom_th, reid_th and max_dist_l2 must be real numbers and max_dist a sequence of them ({exc})") from None
    if md.size != g:
        raise ValueError(f"max_dist has {md.size} entries for {g} frames")
    if not (np.isfinite(md).all() and (md > 0).all()):
        raise ValueError("max_dist must be finite and > 0")
    if not np.isfinite(geom) or (reid is not None and not np.isfinite(reid)) or not (np.isfinite(l2) and l2 > 0):
        raise ValueError("geom_th and reid_th must be finite, max_dist_l2 finite and > 0")
    if reid is None:
        rows = sweep_joint(batch, [attr[:, GEOMETRY_COLUMN]], [[geom]], ["lt"], frame_div=md.reshape(1, g), partition=partition)
    else:
        rows = sweep_joint(batch, [attr[:, GEOMETRY_COLUMN], attr[:, REID_L2_COLUMN]], [[geom, reid * l2]], ["lt", "lt"],
                           frame_div=np.stack([md, np.ones(g)]), partition=partition)
    return rows[0]


__all__ = ["geometry_baseline"]
