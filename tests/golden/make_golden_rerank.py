#!/usr/bin/env python3
"""Golden vectors for gnn_cca_amd.rerank: the reference's own `libs.utils.re_ranking` (libs/utils.py:578-644, imported unmodified behind
the `cv2` / `torch_scatter` stand-ins of make_golden_post.py) on synthetic frames.  Build container only:

    python tests/golden/make_golden_rerank.py

It writes tests/golden/rerank/*.npz (a sub-folder: tests/conftest.py takes every unprefixed .npz directly under tests/golden/ for a
forward case): numbers only -- D, the cameras, the parameters, the reference's result and its error against the float64 oracle.

re_ranking returns the block [:nq, nq:] of a query / gallery split.  That block does not depend on where the split is (asserted below:
difference exactly 0), so the calls nq = 1 .. n-1 give the whole upper triangle, and the same calls on the reversed node order the lower
one.  The diagonal is never returned (stored as 0, `offdiag` marks the rest).

Frames: persons x cameras, an embedding = its person's centre + noise 0.6 (16 wide), D their float32 L2 distances.  Seeds are searched
until the reference alone satisfies what the tests rely on:
  * no row of float32 O has a tie among its first k1 + 2 values (the reference's argsort is unstable, ours breaks ties by index);
  * in the cases marked `events` the 2/3 test both accepts and rejects and some accepted set enlarges X(i);
  * the gap at the rank-1 and rank-2 boundary of the reference's matrix exceeds 8 d_ref for every case (none is dropped),
    d_ref = the largest error of the reference's float32 result against the float64 oracle over all cases."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _install_torch_scatter_standin  # noqa: E402
import rerank_oracle as oracle  # noqa: E402

OUT = os.path.join(HERE, "rerank")
# name, n, cameras, k1, k2, lam, events
CASES = (("n2", 2, 2, 4, 1, 0.3, False), ("n3", 3, 3, 20, 6, 0.3, False), ("n7", 7, 3, 20, 6, 0.3, False),
         ("n21", 21, 4, 20, 6, 0.3, False), ("n22", 22, 4, 20, 6, 0.3, False), ("n34_k5", 34, 4, 5, 3, 0.3, False),
         ("n34_k7", 34, 4, 7, 1, 0.3, True), ("n34_lam0", 34, 4, 20, 6, 0.0, True), ("n34_lam1", 34, 4, 20, 6, 1.0, True),
         ("n40_k10", 40, 4, 10, 4, 0.3, True), ("n65", 65, 5, 20, 6, 0.3, True))   # (k1 = 5: h = 3, and a set of three cannot enlarge X)
RANKS = (1, 2)
GAP_FACTOR = 8.0


def frame(n, cams, seed):
    rng = np.random.default_rng(seed)
    cam = (np.arange(n) % cams).astype(np.int32)
    person = np.arange(n) // cams
    centres = rng.normal(0, 1, size=(person.max() + 1, 16))
    x = (centres[person] + 0.6 * rng.normal(0, 1, size=(n, 16))).astype(np.float32)
    D = oracle.frame_distances(x, [0, n], np.float64)[0].astype(np.float32)
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    return D, cam


def tie_free(D, k1):
    sq = D * D
    O = (sq / sq.max(axis=0)).T
    head = np.sort(O, axis=1)[:, :k1 + 2]
    return bool((np.diff(head, axis=1) > 0).all())


def reference_full(re_ranking, D, k1, k2, lam):
    n = D.shape[0]
    full = np.zeros((n, n), dtype=np.float32)
    for flip in (False, True):
        M = D[::-1, ::-1] if flip else D
        tri = np.full((n, n), np.nan, dtype=np.float32)
        for nq in range(1, n):
            block = re_ranking(M[:nq, nq:].copy(), M[:nq, :nq].copy(), M[nq:, nq:].copy(), k1=k1, k2=k2, lambda_value=lam)
            assert block.dtype == np.float32 and block.shape == (nq, n - nq)
            seen = ~np.isnan(tri[:nq, nq:])
            assert np.array_equal(tri[:nq, nq:][seen], block[seen])   # the block does not depend on the split: difference exactly 0
            tri[:nq, nq:] = block
        iu = np.triu_indices(n, 1)
        assert not np.isnan(tri[iu]).any()
        if flip:
            full[n - 1 - iu[0], n - 1 - iu[1]] = tri[iu]
        else:
            full[iu] = tri[iu]
    return full


def main():
    _install_torch_scatter_standin()
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, "/root/reference")
    from libs import utils  # the reference, unmodified

    made = []
    for idx, (name, n, cams, k1, k2, lam, events) in enumerate(CASES):
        seed = 1000 * (idx + 1)
        while True:
            D, cam = frame(n, cams, seed)
            want64, dbg = oracle.rerank(D, k1, k2, lam, np.float64, debug=True)
            ok = tie_free(D, k1)
            if ok and events:
                ok = dbg["accepted"] > 0 and dbg["rejected"] > 0 and dbg["enlarged"] > 0
            if ok:   # a provisional bound on the rank gaps; the real one (8 d_ref) is asserted once d_ref is known
                ok = all(oracle.rank_gap(want64, cam, r) > 2e-5 for r in RANKS)
            if ok:
                break
            seed += 1
        ref = reference_full(utils.re_ranking, D, k1, k2, lam)
        off = ~np.eye(n, dtype=bool)
        err = float(np.abs(ref.astype(np.float64) - want64)[off].max())
        made.append(dict(name=name, D=D, cam=cam, k1=k1, k2=k2, lam=lam, ref=ref, offdiag=off, err_ref=err, seed=seed,
                         accepted=dbg["accepted"], rejected=dbg["rejected"], enlarged=dbg["enlarged"]))
        print(f"{name:10s} n={n:3d} k1={k1:2d} k2={k2} lam={lam} seed={seed} accepted/rejected/enlarged "
              f"{dbg['accepted']}/{dbg['rejected']}/{dbg['enlarged']} |ref - fp64 oracle| {err:.3e}")
    d_ref = max(c["err_ref"] for c in made)
    assert sum(1 for c in made if c["accepted"] and c["rejected"] and c["enlarged"]) >= 3
    os.makedirs(OUT, exist_ok=True)
    for c in made:
        gaps = [oracle.rank_gap(np.where(c["offdiag"], c["ref"], 0), c["cam"], r) for r in RANKS]
        assert min(gaps) > GAP_FACTOR * d_ref, (c["name"], gaps, d_ref)   # no case is dropped for its rank gaps
        np.savez_compressed(os.path.join(OUT, c["name"] + ".npz"), D=c["D"], cam=c["cam"], k1=np.int64(c["k1"]), k2=np.int64(c["k2"]),
                            lam=np.float64(c["lam"]), ref=c["ref"], offdiag=c["offdiag"], err_ref=np.float64(c["err_ref"]),
                            d_ref=np.float64(d_ref), seed=np.int64(c["seed"]), ranks=np.asarray(RANKS, dtype=np.int64),
                            rank_gaps=np.asarray(gaps, dtype=np.float64),
                            events=np.asarray([c["accepted"], c["rejected"], c["enlarged"]], dtype=np.int64))
    print(f"d_ref = {d_ref:.3e} over {len(made)} cases")


if __name__ == "__main__":
    main()
