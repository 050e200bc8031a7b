"""The rule of bridges_beam_select (include/bridges_hip.h) stated once in numpy, the probe tables the kernel is run on, defective
twins every probe set must tell from the rule, and a host restatement of the bookkeeping of VecDQN.beam_search on a scripted toy.

A *case* is a dict of numpy arrays as the entry point takes them: B (int), seg_lo / seg_hi int32 [E], q float32 [n], idx int64 [n],
cand_offset int32 [E], rep int32 [E] or None, live uint8 [E], ret / disc float64 [E]; E = G * B.  ``reference(case)`` returns the
six outputs.  Nothing here is rounded other than the rule says: the score is  ret + disc * float64(q),  two binary64 operations."""
import numpy as np

TWINS = ("row_only_ties", "score_f32", "dead_compete", "nan_as_number", "no_padding")
OUTPUTS = ("src", "sel_compact", "sel_index", "q_sel", "score", "live")


def candidates(case, g, twin=None):
    """The candidates of group g in the rule's order: a list of (S, q, env, row)."""
    B, lo, hi, q = case["B"], case["seg_lo"], case["seg_hi"], case["q"]
    live, ret, disc = case["live"], case["ret"], case["disc"]
    n_rows = len(q)
    out = []
    for e in range(g * B, (g + 1) * B):
        if not live[e] and twin != "dead_compete":
            continue
        for j in range(max(int(lo[e]), 0), min(int(hi[e]), n_rows)):
            v = np.float32(q[j])
            if twin == "nan_as_number":
                if v == -np.inf:
                    continue
            elif np.isnan(v) or v == -np.inf:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                if twin == "score_f32":
                    S = np.float64(np.float32(ret[e]) + np.float32(disc[e]) * v)
                else:
                    S = np.float64(ret[e]) + np.float64(disc[e]) * np.float64(v)
            if np.isnan(S) and twin != "nan_as_number":
                continue
            out.append((S, v, e, j))

    def before(a, b):                                            # a comes before b
        if twin == "row_only_ties":
            return (a[0] > b[0]) if a[0] != b[0] else (a[3], a[2]) < (b[3], b[2])
        if a[0] != b[0]:
            return a[0] > b[0]
        if a[1] != b[1]:
            return a[1] > b[1]
        return (a[2], a[3]) < (b[2], b[3])
    ordered = []                                                 # selection sort by the rule's comparison, nothing cleverer
    rest = list(out)
    while rest:
        best = 0
        for k in range(1, len(rest)):
            if before(rest[k], rest[best]):
                best = k
        ordered.append(rest.pop(best))
    return ordered


def reference(case, twin=None):
    B, q, idx, off, rep = case["B"], case["q"], case["idx"], case["cand_offset"], case.get("rep")
    E = len(case["seg_lo"])
    assert E % B == 0
    out = dict(src=np.arange(E, dtype=np.int32), sel_compact=np.zeros(E, np.int64), sel_index=np.zeros(E, np.int32),
               q_sel=np.zeros(E, np.float32), score=np.full(E, -np.inf), live=np.zeros(E, np.uint8))
    if twin == "no_padding":                                     # the slots beyond the candidates keep what was there
        out = sentinels(E)
    for g in range(E // B):
        for i, (S, v, e, j) in enumerate(candidates(case, g, twin)[:B]):
            s = g * B + i
            owner = e if rep is None else int(rep[e])
            out["src"][s], out["sel_compact"][s] = e, idx[j]
            out["sel_index"][s] = max(int(idx[j]) - int(off[owner]), 0)
            out["q_sel"][s], out["score"][s], out["live"][s] = v, S, 1
    return out


def sentinels(E):
    """What the output arrays hold before a call in the tests: values no call writes."""
    return dict(src=np.full(E, -7, np.int32), sel_compact=np.full(E, -7, np.int64), sel_index=np.full(E, -7, np.int32),
                q_sel=np.full(E, -7.5, np.float32), score=np.full(E, -7.5, np.float64), live=np.full(E, 9, np.uint8))


def same(a, b):
    """Two output dicts, bit for bit (a NaN equals the same NaN)."""
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in OUTPUTS)


def _case(B, segs, q, live, ret, disc, rep=None, idx=None, cand_offset=None):
    lo = np.array([s[0] for s in segs], dtype=np.int32)
    hi = np.array([s[1] for s in segs], dtype=np.int32)
    q = np.asarray(q, dtype=np.float32)
    n, E = len(q), len(segs)
    idx = np.asarray(idx if idx is not None else 10 + 3 * np.arange(n), dtype=np.int64)
    if cand_offset is None:                                      # the owner's first row's compact index, minus one
        cand_offset = [int(idx[min(max(int(l), 0), n - 1)]) - 1 for l in lo]
    return dict(B=B, seg_lo=lo, seg_hi=hi, q=q, idx=idx, cand_offset=np.asarray(cand_offset, dtype=np.int32),
                rep=None if rep is None else np.asarray(rep, dtype=np.int32), live=np.asarray(live, dtype=np.uint8),
                ret=np.asarray(ret, dtype=np.float64), disc=np.asarray(disc, dtype=np.float64))


def probe_tables():
    """name -> case: every corner the rule names, small enough to read."""
    nan, inf = np.nan, np.inf
    t = {}
    # two envs whose rows tie in S (1 + 1 * 1 == 0 + 1 * 2 == 2 + 0.5 * 0) with different q: the higher q first, whatever its row
    t["ties_in_S_different_q"] = _case(4, [(0, 2), (2, 4), (4, 6), (6, 6)], [1.0, 0.5, 2.0, 0.25, 0.0, -1.0], [1, 1, 1, 1],
                                       [1.0, 0.0, 2.0, 0.0], [1.0, 1.0, 0.5, 1.0])
    # ties in S and q: env ascending, then row ascending (env 1's rows come BEFORE env 0's in q: a row-only rule takes env 1 first)
    t["ties_in_q"] = _case(2, [(3, 6), (0, 3)], [0.5, 0.5, 0.25, 0.5, 0.5, 0.5], [1, 1], [0.0, 0.0], [1.0, 1.0])
    # NaN and -inf rows are no candidates; +inf is one
    t["nan_and_minus_inf"] = _case(4, [(0, 4), (4, 8), (8, 8), (8, 9)], [nan, 1.0, -inf, 0.5, -inf, nan, inf, -2.0, nan],
                                   [1, 1, 1, 1], [0.0, 0.5, 0.0, 0.0], [1.0, 0.5, 1.0, 1.0])
    # empty segments, and a group with fewer candidates than B: the slots are padded
    t["empty_and_short"] = _case(4, [(0, 0), (0, 2), (2, 2), (2, 2), (2, 2), (2, 2), (2, 2), (2, 2)], [0.3, 0.7],
                                 [1] * 8, [0.0] * 8, [1.0] * 8)
    # envs that share their representative's rows: distinct candidates with the representative's offsets
    t["shared_rep_rows"] = _case(4, [(0, 3), (0, 3), (3, 5), (0, 3)], [0.1, 0.9, 0.5, 0.9, 0.2], [1, 1, 1, 1], [0.0, 0.25, 0.0, -1.0],
                                 [1.0, 1.0, 1.0, 1.0], rep=[0, 0, 2, 0], cand_offset=[4, 1000, 15, 2000])
    # dead beams hold the best rows
    t["dead_beams"] = _case(2, [(0, 2), (2, 4), (4, 6), (6, 8)], [9.0, 8.0, 1.0, 0.5, 3.0, 2.0, 7.0, 6.0], [0, 1, 1, 0],
                            [5.0, 0.0, 0.0, 5.0], [1.0] * 4)
    # the score needs binary64: in float32 1e8 + 1 == 1e8 and the tie would fall to q
    t["score_needs_f64"] = _case(2, [(0, 1), (1, 2)], [1.0, 2.0], [1, 1], [1e8, 1e8 - 1.5], [1.0, 1.0])
    # B = 1, one live beam: the first maximum of q
    t["width_1"] = _case(1, [(0, 4), (4, 7), (7, 7)], [0.2, 0.8, 0.8, 0.1, -0.5, -0.25, -0.25], [1, 1, 1], [0.0, 3.0, 0.0], [1.0, 0.9, 1.0])
    return t


def random_case(G, B, seed):
    """A seeded table of G groups of B beams: segments of 0..40 rows, q from a coarse grid (ties abound), some NaN / -inf rows,
    some dead beams, returns from a coarse grid, shared rows for a part of the envs."""
    rng = np.random.default_rng(seed)
    E = G * B
    lens = rng.integers(0, 41, size=E)
    lens[rng.random(E) < 0.15] = 0
    rep = np.arange(E, dtype=np.int32)
    segs, start = [], 0
    for e in range(E):
        if e % B and rng.random() < 0.3:                         # shares the rows of an earlier env of its group
            rep[e] = rep[e - 1 - int(rng.integers(0, e % B))]
            segs.append(segs[rep[e]])
        else:
            segs.append((start, start + int(lens[e])))
            start += int(lens[e])
    n = max(start, 1)
    q = (rng.integers(-8, 9, size=n) / 4.0).astype(np.float32)
    q[rng.random(n) < 0.05] = np.nan
    q[rng.random(n) < 0.05] = -np.inf
    idx = np.cumsum(rng.integers(1, 4, size=n)).astype(np.int64)
    off = np.array([int(idx[min(s[0], n - 1)]) - int(rng.integers(0, 2)) for s in segs], dtype=np.int32)
    live = (rng.random(E) < 0.8).astype(np.uint8)
    ret = rng.integers(-4, 5, size=E) / 2.0
    disc = 0.5 ** rng.integers(0, 4, size=E)
    return _case(B, segs, q, live, ret, disc, rep=rep, idx=idx, cand_offset=off)


# ---- the bookkeeping of VecDQN.beam_search, restated on the host ---------------------------------------------------------------
def better_finished(new, old):
    """new / old: (success, ret, depth, slot) of two finished beams of a group, old may be None -> True if new replaces old:
    success first, then the higher return, then the earlier depth, then the lower slot."""
    if old is None:
        return True
    if new[0] != old[0]:
        return new[0] > old[0]
    if new[1] != old[1]:
        return new[1] > old[1]
    if new[2] != old[2]:
        return new[2] < old[2]
    return new[3] < old[3]


def toy_search(B, depths, gamma, n_targets, q_of, step_of):
    """Beam search of ONE group on a scripted toy: a state is the tuple of the actions taken so far; q_of(state) -> list of q per
    action; step_of(state, action) -> (lin_reward, reward, done).  Runs ``depths`` depths with the select rule above and the
    bookkeeping of the loop (ret += disc * lin; disc *= gamma; a beam whose step is done goes to the best-finished record and
    dies).  -> (best record or None, per depth the list of live states after it)."""
    beams = [dict(state=(), ret=0.0, ret_r=0.0, disc=1.0, live=(s == 0)) for s in range(B)]
    best, trace = None, []
    for d in range(depths):
        segs, q = [], []
        for b in beams:
            rows = list(q_of(b["state"])) if b["live"] else []
            segs.append((len(q), len(q) + len(rows)))
            q += rows
        if not q:
            break
        case = _case(B, segs, q, [b["live"] for b in beams], [b["ret"] for b in beams], [b["disc"] for b in beams],
                     idx=np.arange(len(q)), cand_offset=[s[0] for s in segs])
        out = reference(case)
        new = []
        for s in range(B):
            parent = beams[int(out["src"][s])]
            nb = dict(parent, live=bool(out["live"][s]))
            if nb["live"]:
                a = int(out["sel_index"][s])
                lin, rew, done = step_of(parent["state"], a)
                nb.update(state=parent["state"] + (a,), ret=parent["ret"] + parent["disc"] * lin,
                          ret_r=parent["ret_r"] + parent["disc"] * rew)
                nb["disc"] = parent["disc"] * gamma
                if done:
                    rec = (rew == n_targets, nb["ret"], d, s)
                    if better_finished(rec, best[0] if best else None):
                        best = (rec, nb["state"], nb["ret_r"])
                    nb["live"] = False
            new.append(nb)
        beams = new
        trace.append([b["state"] for b in beams if b["live"]])
    return best, trace
