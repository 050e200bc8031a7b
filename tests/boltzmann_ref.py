"""The rule of Boltzmann exploration (bridges_boltzmann_select, include/bridges_hip.h) stated once in float64 numpy, the probe
tables the kernel is run on and defective twins every probe set must tell from the rule.

A *case* is a dict of numpy arrays as the entry point takes them: seg_lo / seg_hi int32 [E], q float32 [n], u float32 [E],
T (python float), idx int64 [n], cand_offset int32 [E], rep int32 [E] or None.  ``reference(case)`` returns, per env, the drawn
row, sel_compact, sel_index, q_sel, explore_w, p_sel (float64, unrounded) and the *margin*  min_j |target - c_j| / total: how far,
relative to the total, the env's target lies from the nearest prefix sum.  The device's exp may differ from libm's by an ulp or
two and its prefix sums are added in another order, so a draw whose margin is below MARGIN has no single right answer; the
random tables below are seeded so that none of their draws is such a draw (tests/test_cpu_boltzmann.py asserts it), and the
exact table -- equal q, weights exactly 1, integer prefix sums -- needs no margin at all."""
import numpy as np

MARGIN = 2.0 ** -40
SEG_LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129, 300)
TEMPERATURES = (1e-6, 0.1, 1.0, 1e30)
TWINS = ("ge", "no_max", "exp_over_t", "own_offset", "lane_strided", "nan_weight_1")


def weights(q, T, twin=None):
    """float64 weights of one env's rows q (float32) at temperature T (a float64 as it stands)."""
    q = np.asarray(q, dtype=np.float32)
    T = float(T)
    qd = q.astype(np.float64)
    w = np.zeros(q.shape[0], dtype=np.float64)
    nan = np.isnan(q)
    elig = ~nan & (q != -np.inf)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if twin == "no_max":
            w[elig] = np.exp(qd[elig] / T)
        elif twin == "exp_over_t":
            w[elig] = np.exp(qd[elig]) / T
        elif elig.any():
            m = qd[elig].max()
            if m == np.inf:
                w[elig & (q == np.inf)] = 1.0
            else:
                w[elig] = np.exp((qd[elig] - m) / T)
    if twin == "nan_weight_1":
        w[nan] = 1.0
    return w, elig


def select_env(q, u, T, twin=None):
    """One env: its rows' q, its draw u, the temperature -> (row relative to the segment, p_sel, explore_w, margin)."""
    n = len(q)
    if n == 0:
        return 0, 0.0, 0.0, np.inf
    w, elig = weights(q, T, twin)
    if not elig.any() and not (w > 0).any():
        return 0, 0.0, 0.0, np.inf
    order = np.arange(n)
    if twin == "lane_strided":                               # lane l adds rows l, l + 64, ..: the order of a lane-strided loop
        order = np.lexsort((order // 64, order % 64))
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.add.accumulate(w[order])                      # sequential, in row order
        total = c[-1]
        target = float(u) * total
        hit = (c >= target) if twin == "ge" else (c > target)
    if hit.any():
        row = int(order[np.argmax(hit)])
    else:
        pos = np.flatnonzero(w > 0)
        row = int(pos.max()) if len(pos) else 0              # (none at all: a twin whose weights all underflow)
    with np.errstate(over="ignore", invalid="ignore"):
        p = float(w[row] / total)
        margin = float(np.min(np.abs(target - c)) / total)
    qe = np.where(elig, np.asarray(q, dtype=np.float32), -np.inf)
    first_max = int(np.argmax(qe)) if elig.any() else row
    return row, p, float(row != first_max), margin


def reference(case, twin=None, greedy=False):
    """Every env of a case -> dict of arrays (row, sel_compact, sel_index, q_sel, explore_w, p_sel, margin)."""
    lo, hi, q, u = case["seg_lo"], case["seg_hi"], case["q"], case["u"]
    idx, off, rep = case["idx"], case["cand_offset"], case.get("rep")
    E, n_rows = len(lo), len(q)
    T = float(np.float32(case["T"]))                         # the entry point takes the temperature as a float
    u = np.asarray(u, dtype=np.float32)
    out = dict(row=np.zeros(E, np.int64), sel_compact=np.zeros(E, np.int64), sel_index=np.zeros(E, np.int32),
               q_sel=np.zeros(E, np.float32), explore_w=np.zeros(E, np.float32), p_sel=np.zeros(E, np.float64),
               margin=np.full(E, np.inf))
    for e in range(E):
        seg = q[lo[e]:hi[e]] if hi[e] > lo[e] else q[:0]
        has = len(seg) > 0
        if greedy:                                           # the first maximum (no NaN rows: k_eps_greedy_select decides those)
            r, p, ex, mg = (int(np.argmax(seg)) if has else 0), float(has), 0.0, np.inf
        else:
            r, p, ex, mg = select_env(seg, u[e], T, twin)
        row = min(int(lo[e]) + r if has else 0, n_rows - 1)
        owner = e if (rep is None or twin == "own_offset") else int(rep[e])
        out["row"][e], out["sel_compact"][e] = row, idx[row]
        out["sel_index"][e] = max(int(idx[row]) - int(off[owner]), 0)
        out["q_sel"][e] = q[row] if has else 0.0
        out["explore_w"][e], out["p_sel"][e], out["margin"][e] = ex, p, mg
    return out


def brute_force(q, u, T):
    """The rule once more for one env, in plain Python on floats, line by line as the header states it."""
    import math
    T, u = float(T), float(u)
    q = [float(np.float32(v)) for v in q]
    if not q:
        return 0, 0.0, 0.0
    elig = [not math.isnan(v) and v != -math.inf for v in q]
    if not any(elig):
        return 0, 0.0, 0.0
    m = max(v for v, ok in zip(q, elig) if ok)
    w = []
    for v, ok in zip(q, elig):
        if not ok:
            w.append(0.0)
        elif m == math.inf:
            w.append(1.0 if v == math.inf else 0.0)
        else:
            x = (v - m) / T
            w.append(math.exp(x) if x > -746.0 else 0.0)
    total = 0.0
    for x in w:
        total += x
    target = u * total
    run, row = 0.0, None
    for j, x in enumerate(w):
        run += x
        if run > target:
            row = j
            break
    if row is None:
        row = max(j for j, x in enumerate(w) if x > 0)
    first_max = min(j for j, (v, ok) in enumerate(zip(q, elig)) if ok and v == m)
    return row, w[row] / total, float(row != first_max)


# ------------------------------------------------------------------------------------------------------------------ probe tables
def _layout(lengths, rng, shuffle_rep=False):
    """Segments of the given lengths laid end to end behind 3 rows that belong to nobody; idx and cand_offset such that every
    env's candidates are its own: cand_offset[e] = 2 lo[e] + 3 e, idx[j] = cand_offset[e] + 2 (j - lo[e]) + 1."""
    lengths = np.asarray(lengths, dtype=np.int64)
    lo = 3 + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    hi = lo + lengths
    n = int(hi[-1]) + 2
    E = len(lengths)
    off = (2 * lo + 3 * np.arange(E)).astype(np.int32)
    idx = np.zeros(n, dtype=np.int64)
    for e in range(E):
        idx[lo[e]:hi[e]] = off[e] + 2 * np.arange(lengths[e]) + 1
    return lo.astype(np.int32), hi.astype(np.int32), n, idx, off


def random_probe(T, seed=20240):
    """Segments of every length of SEG_LENGTHS, four of each, mixed within one call; q ~ 3 N(0, 1) with ties of the maximum
    planted in every fourth env; u uniform float32."""
    rng = np.random.default_rng(seed + int(1000 * np.log10(T)))
    lengths = rng.permutation(np.repeat(SEG_LENGTHS, 4))
    lo, hi, n, idx, off = _layout(lengths, rng)
    q = (3.0 * rng.standard_normal(n)).astype(np.float32)
    for e in range(0, len(lengths), 4):
        if lengths[e] >= 2:                                  # an exact tie of the maximum: T -> 0 draws among the ties
            seg = q[lo[e]:hi[e]]
            seg[rng.integers(0, lengths[e], size=min(3, lengths[e]))] = seg.max()
    u = rng.random(len(lengths), dtype=np.float32)
    return dict(seg_lo=lo, seg_hi=hi, q=q, u=u, T=float(T), idx=idx, cand_offset=off, rep=None)


def exact_probe():
    """Equal q in every segment, n = 1, 2, .. 256 rows, one env per k with u = k / n (all sharing the segment's rows through a
    (lo, hi) pair), then per n one env with u = 1 - 2^-24.  Every weight is exactly 1, every prefix sum an integer, k / n and
    (k / n) * n exact: the drawn row is lo + k, at every boundary and on both sides of the 64-row chunk edges.
    -> (case, expected rows)."""
    ns = [1, 2, 4, 8, 16, 32, 64, 128, 256]
    lo_n, _, n_rows, idx, _ = _layout(ns, None)
    q = np.full(n_rows, 0.375, dtype=np.float32)
    lo, hi, u, want, rep = [], [], [], [], []
    for i, n in enumerate(ns):
        first = len(lo)                                      # the first env of the group stands for all of them
        for k, x in zip([*range(n), n - 1], [*(k / n for k in range(n)), 1.0 - 2.0 ** -24]):
            lo.append(lo_n[i]); hi.append(lo_n[i] + n); u.append(x); want.append(lo_n[i] + k); rep.append(first)
        idx[lo_n[i]:lo_n[i] + n] = 7 * first + np.arange(n)
    off = (7 * np.arange(len(lo))).astype(np.int32)          # only the representative's offset is right for the shared rows
    return (dict(seg_lo=np.asarray(lo, np.int32), seg_hi=np.asarray(hi, np.int32), q=q, u=np.asarray(u, np.float32), T=0.1,
                 idx=idx, cand_offset=off, rep=np.asarray(rep, np.int32)), np.asarray(want, dtype=np.int64))


NAN, INF = float("nan"), float("inf")
# (q of the segment, T, the draws u) -- one env per draw
NONFINITE = [
    ([1.0, NAN, 2.0, -INF, 0.5], 1.0, [0.0, 0.1, 0.2, 0.3, 0.5, 0.9, 0.99]),
    ([NAN, NAN, 1.0, 1.0], 1.0, [0.1, 0.6]),                 # NaN rows in front: weight 1 for them would take the draw
    ([NAN, INF, 3.0, INF, -INF], 0.5, [0.1, 0.49, 0.6, 0.99]),
    ([NAN, -INF, NAN], 1.0, [0.0, 0.5]),                     # nothing eligible: the first row, p_sel 0
    ([-INF], 2.0, [0.3]),
    ([1000.0, 999.0], 1.0, [0.0, 0.1, 0.7, 0.8, 0.99]),      # exp(1000) overflows without the subtraction of the maximum
    ([0.0, 1.0], 0.1, [0.2, 0.5]),                           # exp(q) / T is not exp(q / T)
    ([NAN if j % 7 == 3 else (-INF if j % 11 == 5 else 0.25 * (j % 5)) for j in range(131)], 1.0,
     [0.0, 0.013, 0.25, 0.48, 0.5, 0.77, 0.985, 0.999]),    # across two chunk edges
]


# the same with weights that are exactly 0 or 1 and targets that are exact: a target ON a prefix sum (margin 0) is decided by
# the strict rule alone, whatever the order of the additions
NONFINITE_EXACT = [
    ([NAN, INF, 3.0, INF, -INF], 0.5, [0.0, 0.5]),           # u = 0 skips the leading row of weight 0; u = 1/2 sits on c = 1
    ([-INF, NAN, 2.0, 2.0, NAN, 2.0, 2.0], 1.0, [0.0, 0.25, 0.5, 0.75]),
]


def nonfinite_probe(table=None):
    cases = []
    for q, T, us in (NONFINITE if table is None else table):
        lo, hi, n, idx, off = _layout([len(q)], None)
        qq = np.zeros(n, dtype=np.float32)
        qq[lo[0]:hi[0]] = q
        E = len(us)
        cases.append(dict(seg_lo=np.repeat(lo, E), seg_hi=np.repeat(hi, E), q=qq, u=np.asarray(us, np.float32), T=T, idx=idx,
                          cand_offset=np.repeat(off, E), rep=np.zeros(E, np.int32)))
    return cases


def shared_probe(E=4096, n=129, seed=77):
    """E envs that all name the rows of one representative (env 5) through rep and a (lo, hi) pair, each with its own draw;
    every env has a cand_offset of its own, so an index taken against cand_offset[e] is wrong for all but the representative."""
    rng = np.random.default_rng(seed)
    lo, hi, n_rows, idx, _ = _layout([n], None)
    q = np.zeros(n_rows, dtype=np.float32)
    q[lo[0]:hi[0]] = rng.standard_normal(n)
    off = (11 * np.arange(E)).astype(np.int32)
    idx[lo[0]:hi[0]] = off[5] + 3 * np.arange(n) + 2
    return dict(seg_lo=np.repeat(lo, E), seg_hi=np.repeat(hi, E), q=q, u=rng.random(E, dtype=np.float32), T=1.0, idx=idx,
                cand_offset=off, rep=np.full(E, 5, dtype=np.int32))


def margin_cases():
    """Every table whose arithmetic is not exact: the cases the probe condition is asserted on."""
    return [random_probe(T) for T in TEMPERATURES] + nonfinite_probe() + [shared_probe()]


def all_cases():
    return margin_cases() + nonfinite_probe(NONFINITE_EXACT) + [exact_probe()[0]]


def differs(a, b):
    """Do two results differ in what the kernel is compared on?"""
    return (not np.array_equal(a["sel_compact"], b["sel_compact"]) or not np.array_equal(a["sel_index"], b["sel_index"])
            or not np.array_equal(a["explore_w"], b["explore_w"])
            or not np.allclose(a["p_sel"], b["p_sel"], rtol=2.0 ** -22, atol=0.0, equal_nan=True))
