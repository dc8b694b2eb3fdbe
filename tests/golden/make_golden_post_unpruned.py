#!/usr/bin/env python3
"""Golden vectors for PRUNING: False (config_inference.yaml:7): the reference clusters the UNPRUNED predictions by their strongly
connected components (`libs.utils.compute_SCC_and_Clusters`, libs/utils.py:295-317, at inference.py:302-304), and ROUNDING
(`compute_rounding`, libs/utils.py:25-173) then works on unpruned predictions too.  tests/golden/post2_heuristics.npz has PRUNING on in
every case; this file pins the other half: postprocess.strong_clusters, finalize(pruning=False) and the host pass without the switch.

As make_golden_post2.py does, inference.py:283-345 is read from the reference at run time and executed unmodified (that script's
`run_reference`, imported by path), under PRUNING: False, SPLITTING: False with ROUNDING False and True.  (SPLITTING without PRUNING has no
behaviour in the reference: disjoint_big_clusters looks up the reverse of an edge it removes and raises on unpruned predictions.)  Nothing
of the reference's text is stored: numbers only, per case `<name>::n_nodes`, `edge_index`, `logits`, `probs`, `pred_unpruned`, `id_unpruned`,
`pred_rounded`, `id_rounded`.  One frame per case.  Build container only:

    python tests/golden/make_golden_post_unpruned.py
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_torch_scatter_standin, cross_camera_edges  # noqa: E402
from make_golden_post2 import run_reference  # noqa: E402


def logits_from_directed(ei, active, rng, on=3.0, off=-4.0, noise=0.3):
    """Negative logits everywhere except on the listed DIRECTED edges (i, j)."""
    logit = (off + noise * rng.standard_normal(ei.shape[1])).astype(np.float32)
    pos = {(int(a), int(b)): k for k, (a, b) in enumerate(ei.T)}
    for i, j in active:
        logit[pos[(i, j)]] = on + abs(noise * rng.standard_normal())
    return logit


def partition(ids):
    _, idx, inv = np.unique(np.asarray(ids), return_index=True, return_inverse=True)
    return idx[inv]


def main():
    _install_torch_scatter_standin()
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, "/root/reference")
    from libs import utils  # the reference, unmodified

    rng = np.random.default_rng(23)
    cases = {}
    # six cameras x two detections: node v sits in camera v // 2, so any two nodes of different cameras share both edges
    n, ei = cross_camera_edges([2] * 6)

    def hand(name, active):
        cases[name] = (n, ei, logits_from_directed(ei, active, rng))

    both = lambda pairs: [e for a, b in pairs for e in ((a, b), (b, a))]   # noqa: E731
    hand("cycle3_no_mutual_pair", [(0, 2), (2, 4), (4, 0)])                 # one SCC of three; the pruned chain gives three singletons
    hand("chain4", [(0, 2), (2, 4), (4, 6)])                                # weakly connected, four SCCs
    hand("two_cycles_share_a_node", [(0, 2), (2, 4), (4, 0), (0, 6), (6, 8), (8, 0)])
    hand("cycle_with_tails", [(10, 0), (0, 2), (2, 4), (4, 0), (2, 8)])     # a tail in (10) and a tail out (8) stay outside
    hand("mutual_pairs_only", both([(0, 2), (2, 4), (1, 3)]))               # must equal the pruned chain
    hand("cycle5", [(0, 2), (2, 4), (4, 6), (6, 8), (8, 0)])                # trigger bit 1, no bit 0
    hand("hub_four_out", [(0, 2), (0, 4), (0, 6), (0, 8)])                  # bit 0, all singletons
    hand("nothing_active", [])
    noisy = []
    for name, cams, seeds in (("terrace", [8, 8, 8, 8], range(0, 6)), ("cams6", [3, 4, 2, 5, 3, 4], range(6, 12)), ("cams5x3", [3] * 5, range(12, 18))):
        for s in seeds:
            r = np.random.default_rng(200 + s)
            nn, e2 = cross_camera_edges(cams)
            ident = r.integers(0, max(nn // 4, 2), size=nn)
            same = ident[e2[0]] == ident[e2[1]]
            lg = (np.where(same, 1.0, -2.0) + r.normal(0, 1.5, size=e2.shape[1])).astype(np.float32)
            cases[f"{name}_s{s}"] = (nn, e2, lg)
            noisy.append(f"{name}_s{s}")

    out, summary, differs, rounded_changes = {}, [], 0, 0
    for name, (nn, e2, lg) in cases.items():
        p_u, id_u, probs = run_reference(utils, nn, e2, lg, False, False, False)     # threshold + SCC of the unpruned predictions
        p_r, id_r, _ = run_reference(utils, nn, e2, lg, True, False, False)          # ... with ROUNDING
        _, id_p, _ = run_reference(utils, nn, e2, lg, False, True, False)            # (for the assertion below: the pruned components)
        assert np.array_equal(p_u, (probs >= 0.5).astype(np.int64)), name            # nothing is pruned
        for k, v in (("n_nodes", np.int64(nn)), ("edge_index", e2), ("logits", lg), ("probs", probs), ("pred_unpruned", p_u),
                     ("id_unpruned", id_u), ("pred_rounded", p_r), ("id_rounded", id_r)):
            out[f"{name}::{k}"] = v
        diff = not np.array_equal(partition(id_u), partition(id_p))
        changed = not np.array_equal(p_u, p_r)
        if name in noisy:
            differs += diff
            rounded_changes += changed
        summary.append(f"{name:26s} N={nn:2d} E={e2.shape[1]:4d} active {int(p_u.sum()):3d} rounded {int(p_r.sum()):3d}  clusters: SCC "
                       f"{len(set(id_u.tolist())):2d} (max {np.bincount(id_u).max()}) pruned {len(set(id_p.tolist())):2d} rounded "
                       f"{len(set(id_r.tolist())):2d}  {'SCC != pruned' if diff else ''} {'rounding changed it' if changed else ''}")
    print("\n".join(summary))
    print(f"noisy frames whose SCC partition differs from the pruned components: {differs} of {len(noisy)}; changed by ROUNDING: {rounded_changes}")
    # the numbers come from the reference alone; these two facts make the golden worth having
    assert 2 * differs >= len(noisy), (differs, len(noisy))
    assert rounded_changes >= 1
    # the hand-made frames say what their comments say
    size = lambda nm: np.bincount(out[f"{nm}::id_unpruned"]).max()   # noqa: E731
    count = lambda nm: len(set(out[f"{nm}::id_unpruned"].tolist()))  # noqa: E731
    assert size("cycle3_no_mutual_pair") == 3 and count("cycle3_no_mutual_pair") == 10
    assert size("chain4") == 1 and size("two_cycles_share_a_node") == 5 and size("cycle_with_tails") == 3 and size("cycle5") == 5
    assert size("hub_four_out") == 1 and count("nothing_active") == 12 and count("mutual_pairs_only") == 9
    # Every tests/golden/post_*.npz is also a case of tests/test_post_oracle.py and tests/test_gpu_postprocess.py, which read ONE frame from
    # top-level keys in make_golden_post.py's format.  This file is named post_unpruned.npz, so it carries such a frame too (the first noisy
    # one), made the way that script makes its own: the reference's functions on the thresholded predictions.
    import networkx as nx
    import torch
    from torch_scatter import scatter_add
    nn, e2, lg = cases[noisy[0]]
    preds_prob = torch.nn.Sigmoid()(torch.from_numpy(lg))
    predictions = (preds_prob >= 0.5) * 1
    active = [(e2[0][pos], e2[1][pos]) for pos, p in enumerate(predictions) if p == 1]
    id_raw, n_raw = utils.compute_SCC_and_Clusters(nx.DiGraph(active), nn)
    pruned, active_p = utils.remove_edges_single_direction(active, predictions, e2)
    id_pruned, n_pruned = utils.compute_SCC_and_Clusters(nx.DiGraph(active_p), nn)
    flow_out = scatter_add(pruned, torch.from_numpy(e2[0]), dim_size=nn)
    flow_in = scatter_add(pruned, torch.from_numpy(e2[1]), dim_size=nn)
    assert np.array_equal(partition(id_raw), partition(out[f"{noisy[0]}::id_unpruned"])) and np.array_equal(preds_prob.numpy(), out[f"{noisy[0]}::probs"])
    top = dict(n_nodes=np.int64(nn), edge_index=e2, logits=lg, probs=preds_prob.numpy(), predictions=predictions.numpy(), pruned=pruned.numpy(),
               id_pruned=id_pruned, n_clusters_pruned=np.int64(n_pruned), id_raw=id_raw, n_clusters_raw=np.int64(n_raw),
               flow_out=flow_out.numpy(), flow_in=flow_in.numpy())
    np.savez_compressed(os.path.join(HERE, "post_unpruned.npz"), names=np.array(sorted(cases)), **top, **out)


if __name__ == "__main__":
    main()
