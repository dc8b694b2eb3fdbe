"""The re-entry gallery of gnn_cca_amd.reentry (TrackGallery) restated with numpy, for the tests: a second stage behind a FrameLinker
that gives a track born after a long absence the IDENTITY of the ended track it looks like.  Plain Python loops over frames, births and
ring slots; the cosine distance is tracking_oracle.pair_tables' (float64 products and sums, 1 if a norm is 0).

Notation: M = the linker's max_gap, W = window, S = W + max_batch ring slots, f = frames seen before this one (over all calls; an empty
or refused frame counts).  A BIRTH is a usable cluster (rank < the frame's count) with matched_prev == -1, b its track id.
State: per track j, in ring slot j mod S: owner (-1: empty), sum fp32 [R], last (frame of its latest cluster), pos fp64 [2] of that
cluster, identity, continued; and the identities of the rows of the last M + 1 frames.  Per frame, in this order:
  1. a continued cluster (matched_prev = m, matched_gap = k) takes the identity of row m of frame f - 1 - k (batch or history, never the
     ring: a track may live longer than S births);
  2. track j is eligible for birth b iff  b - W <= j < b and slot j mod S still holds j;  j is not continued;  f - last[j] >= M + 2;
     max_age is None or f - last[j] <= max_age;  max_speed is None or d <= max_speed * float64(f - last[j]) (d = sqrt(dx^2 + dy^2));
     dcos(emb[b], sum[j]) <= max_cos (a NaN is admissible with nobody).  cost = dcos;
  3. mutual best among the births of the frame: b's best j has the smallest cost (ties: the smaller track id), j's best birth the
     smallest cost (ties: the smaller rank); if mutual identity[b] = identity[j], continued[j] = 1, reentered_from = j; else identity[b] = b;
  4. a birth takes slot b mod S whatever it held: sum = 0, continued = 0, its identity;
  5. every usable cluster whose slot holds its track id: sum = sum + emb (fp32, one addition per column, in frame order), last = f, pos.
     A cluster whose slot was taken by a younger track is skipped.
Consequences (tests/test_reentry_oracle.py checks them):
  - the result does not depend on how a sequence is cut into calls (the rule is causal and the state is all it remembers);
  - with S = W + max_batch and N <= max_batch per call an eligible track's slot cannot have been overwritten by a birth of the same call
    (a younger owner of slot j mod S has an id >= j + S >= b + max_batch, and a call's births are numbered below b + N);
  - an eligible track has been absent for M + 2 frames, so the linker can no longer continue it: its sum, last and pos at frame f are
    final.  An implementation may therefore accumulate sum / last / pos for a whole call first and look at them afterwards; only
    `continued` and the identities are serial in time.
No fixture files: every case is generated from a seed or written out by hand."""
import numpy as np

import tracking_oracle as to

MAX_FRAME_NODES = 4096


def new_state(window, max_batch, r):
    s = int(window) + int(max_batch)
    return dict(seen=0, owner=np.full(s, -1, np.int64), sum=np.zeros((s, r), np.float32), last=np.zeros(s, np.int64),
                pos=np.zeros((s, 2), np.float64), identity=np.zeros(s, np.int64), continued=np.zeros(s, np.int32), ident_frames=[])


def copy_state(st):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    out["ident_frames"] = [a.copy() for a in st["ident_frames"]]
    return out


def check_args(max_gap, max_cos, window=1024, max_batch=2048, max_age=None, max_speed=None):
    """The constructor's refusals (ValueError), as TrackGallery states them."""
    def real(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

    def integer(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if not real(max_cos) or not 0 <= max_cos <= 2:
        raise ValueError(f"max_cos must be a number in [0, 2], not {max_cos!r}")
    if not integer(window) or window < 1:
        raise ValueError(f"window must be an integer >= 1, not {window!r}")
    if not integer(max_batch) or max_batch < 1:
        raise ValueError(f"max_batch must be an integer >= 1, not {max_batch!r}")
    if max_age is not None and (not integer(max_age) or max_age < max_gap + 2):
        raise ValueError(f"max_age must be None or an integer >= max_gap + 2 = {max_gap + 2}, not {max_age!r}")
    if max_speed is not None and (not real(max_speed) or not np.isfinite(max_speed) or not max_speed > 0):
        raise ValueError(f"max_speed must be None or a finite number > 0, not {max_speed!r}")


def _walk(summ, node_ptr, tracks, max_gap, max_cos, window, max_batch, max_age, max_speed, state, visit=None):
    check_args(max_gap, max_cos, window, max_batch, max_age, max_speed)
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    n, g = len(summ["rank"]), len(node_ptr) - 1
    emb = np.asarray(summ["emb"], np.float32)
    r = emb.shape[1]
    if r == 0:
        raise ValueError("the summaries have no appearance columns")
    if n > max_batch:
        raise ValueError(f"{n} rows in one call, max_batch is {max_batch}")
    if g and int(np.diff(node_ptr).max()) > MAX_FRAME_NODES:
        raise ValueError("a frame has more than 4096 detections")
    if len(tracks["cluster_track"]) != n:
        raise ValueError("tracks and summaries differ in length")
    st = copy_state(state) if state is not None else new_state(window, max_batch, r)
    if st["sum"].shape[1] != r:
        raise ValueError("R differs from the state's")
    s_slots, m_gap = int(window) + int(max_batch), int(max_gap)
    frames = list(st["ident_frames"])
    h = len(frames)
    cluster_identity, node_identity = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    reentered_from = np.full(n, -1, np.int64)
    for q in range(g):
        f = st["seen"]
        v0, v1 = int(node_ptr[q]), int(node_ptr[q + 1])
        c = int(summ["count"][q])
        c = c if 0 <= c <= v1 - v0 else 0
        ident = np.full(c, -1, np.int64)
        births = []
        for a in range(c):   # step 1
            m, k = int(tracks["matched_prev"][v0 + a]), int(tracks["matched_gap"][v0 + a])
            if m < 0:
                births.append(a)
            else:
                ident[a] = frames[h + q - 1 - k][m]
        # step 2: the table births x candidate tracks
        cand = sorted({j for a in births for j in range(max(int(tracks["cluster_track"][v0 + a]) - window, 0), int(tracks["cluster_track"][v0 + a]))
                       if st["owner"][j % s_slots] == j and not st["continued"][j % s_slots] and f - st["last"][j % s_slots] >= m_gap + 2
                       and (max_age is None or f - st["last"][j % s_slots] <= max_age)})
        cost = np.full((len(births), len(cand)), np.inf)
        if births and cand:
            slots = np.array([j % s_slots for j in cand], np.int64)
            rows = np.array([v0 + a for a in births], np.int64)
            gate = None if max_speed is None else np.float64(max_speed) * (f - st["last"][slots]).astype(np.float64)
            d, dcos, _, _ = to.pair_tables(summ["pos"][rows], emb[rows], st["pos"][slots], st["sum"][slots], np.inf, 1.0, None)
            for i, a in enumerate(births):
                b = int(tracks["cluster_track"][v0 + a])
                for x, j in enumerate(cand):
                    ok = b - window <= j < b
                    if ok and visit is not None:
                        visit(d[i, x], None if gate is None else gate[x], dcos[i, x])
                    if ok and gate is not None:
                        ok = bool(d[i, x] <= gate[x])
                    if ok and dcos[i, x] <= max_cos:
                        cost[i, x] = dcos[i, x]
        if visit is not None:
            visit(None, None, cost)
        ok = np.isfinite(cost)
        fwd, bwd = to._best(cost, ok), to._best(cost.T, ok.T)   # step 3 (births in rank order, candidates in ascending track id)
        for i, a in enumerate(births):
            b = int(tracks["cluster_track"][v0 + a])
            x = int(fwd[i])
            if x >= 0 and bwd[x] == i:
                j = cand[x]
                ident[a] = st["identity"][j % s_slots]
                st["continued"][j % s_slots] = 1
                reentered_from[v0 + a] = j
            else:
                ident[a] = b
        for a in births:   # step 4
            b = int(tracks["cluster_track"][v0 + a])
            sl = b % s_slots
            st["owner"][sl], st["sum"][sl], st["continued"][sl], st["identity"][sl] = b, 0.0, 0, ident[a]
        for a in range(c):   # step 5
            t = int(tracks["cluster_track"][v0 + a])
            sl = t % s_slots
            if t >= 0 and st["owner"][sl] == t:
                st["sum"][sl] = st["sum"][sl] + emb[v0 + a]
                st["last"][sl] = f
                st["pos"][sl] = summ["pos"][v0 + a]
        cluster_identity[v0:v0 + c] = ident
        for v in range(v0, v1):
            rk = int(summ["rank"][v])
            if 0 <= rk < c:
                node_identity[v] = ident[rk]
        frames.append(ident)
        st["seen"] = f + 1
    st["ident_frames"] = frames[-(m_gap + 1):]
    return dict(cluster_identity=cluster_identity, node_identity=node_identity, reentered_from=reentered_from), st


def gallery(summ, node_ptr, tracks, max_gap, max_cos, window=1024, max_batch=2048, max_age=None, max_speed=None, state=None):
    """-> (dict(cluster_identity [N], node_identity [N], reentered_from [N]), new state).  `tracks`: a dict with cluster_track,
    matched_prev and matched_gap, as tracking_gap_oracle.link_gap returns it for the same summaries."""
    return _walk(summ, node_ptr, tracks, max_gap, max_cos, window, max_batch, max_age, max_speed, state)


def margins(summ, node_ptr, tracks, max_gap, max_cos, window=1024, max_batch=2048, max_age=None, max_speed=None, state=None):
    """The smallest gaps of a call on the oracle's own numbers: (best versus second-best admissible cost over every row and column of a
    frame's table with at least two admissible entries, |dcos - max_cos|, |d - gate|) -- the last two over every pair that passes the
    integer tests (window, owner, continued, absence, age); inf where there is nothing to compare.  Also the number of rows or columns
    with at least two admissible entries, and the largest number of candidate tracks a frame's births saw."""
    gaps = [np.inf, np.inf, np.inf, 0, 0]

    def visit(d, gate, x):
        if d is None:
            gaps[4] = max(gaps[4], x.shape[1] if x.shape[0] else 0)
            for table in (x, x.T):
                for row in table:
                    fin = np.sort(row[np.isfinite(row)])
                    if len(fin) >= 2:
                        gaps[0] = min(gaps[0], float(fin[1] - fin[0]))
                        gaps[3] += 1
            return
        if not np.isnan(x):
            gaps[1] = min(gaps[1], float(abs(x - max_cos)))
        if gate is not None:
            gaps[2] = min(gaps[2], float(abs(d - gate)))

    _walk(summ, node_ptr, tracks, max_gap, max_cos, window, max_batch, max_age, max_speed, state, visit)
    return tuple(gaps)


def lookalike_sequence(seed, g, persons, max_hide, p_hide, r=16, empty=()):
    """The sequence the tests use: tracking_gap_oracle.hide_sequence walks whose appearances are replaced by three look-alike groups
    (look[p] = group[p mod 3] + 0.35 normal; a row = look[p] + 0.05 normal, as fp32; both from default_rng(100 + seed))."""
    import tracking_gap_oracle as tg
    seq = tg.hide_sequence(np.random.default_rng(seed), g, persons, r, p_leave=0, p_enter=0, p_hide=p_hide, max_hide=max_hide, arena=20,
                           empty=empty, max_alive=max(70, persons))
    rng = np.random.default_rng(100 + seed)
    group = rng.standard_normal((3, r))
    look = np.stack([group[p % 3] + 0.35 * rng.standard_normal(r) for p in range(persons)])
    seq["emb"] = np.stack([look[p] + 0.05 * rng.standard_normal(r) for p in seq["person"]]).astype(np.float32).reshape(-1, r)
    return seq


def link(seq, max_gap, max_step=0.8, lam=1.0, state=None):
    """The linker's oracle for any M (tracking_gap_oracle.link_gap; with M = 0 it is the adjacent-frame rule)."""
    import tracking_gap_oracle as tg
    return tg.link_gap(seq, seq["node_ptr"], max_step, lam, None, max_gap, state)
