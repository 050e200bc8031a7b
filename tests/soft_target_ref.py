"""The rule of the expected-value target operator (bridges_soft_expect, include/bridges_hip.h) stated once in float64 numpy, the
probe tables the kernel is run on, the bound every output element is held to and defective twins the bound must reject.

A *case* is a dict of numpy arrays as the entry point takes them: seg_lo / seg_hi int32 [B], select_q / next_q float32 [R] (the
same array object: the plain target), T (python float), feat float32 [F, dim] or None (dim == 0), feat_row int64 [R] or None.
The weights are tests/boltzmann_ref.weights -- one statement of them for the draw and for the expectation.

``reference(case)`` -> dict of float64 arrays value [B], feat_mean [B, dim], entropy [B], int64 argmax_row [B], bool nothing [B]
(no eligible row: every output is fixed, exact equality is asked) and the bounds value_bound, feat_mean_bound, entropy_bound.

The bound of an output y = sum_j p_j x_j (x = next_q, a column of feat, or the exponents a_j = (q_j - m) / T for the entropy):
  |device - reference| <= half an ulp of float32 at the reference  +  2 * EPS * sum_j p_j |x_j|,
  EPS = (2 n + 4  +  2 * (2 + a_max)) * 2^-52,  n = the rows of the segment, a_max = the largest |a_j| among the rows that weigh.
Derivation.  The device and this module both evaluate in float64; each is off the real-number value by at most EPS * sum p|x|,
hence the factor 2.  A weight w_j = exp(a_j): a_j takes two roundings (the difference, the quotient), so it is off by at most
|a_j| * 2^-52, which moves exp by the same RELATIVE amount (d exp(a) / exp(a) = da); the exp itself is granted 2 ulp = 2 * 2^-52.
So every w_j is off by at most (2 + a_max) * 2^-52 relative, and so is Z up to the n roundings of its sum (n * 2^-53 each way);
p_j = w_j / Z carries both: 2 * (2 + a_max) * 2^-52 + (n + 1) * 2^-53.  The products p_j x_j and the n additions add (n + 1) *
2^-53 more, whatever the order of the additions (every partial sum is at most sum p|x|).  Summed and rounded up: EPS.  a_max
is at most 745.2 (beyond it a weight is 0 and the row is skipped), so EPS stays below 2e-12 for the longest probe segment.
Rounding the float64 sum to float32 adds half a float32 ulp; taken at the reference, which is within EPS of the device's sum.
The entropy log Z - sum p a has two terms of one sign (a <= 0 <= log Z): its bound is that of sum p a plus EPS * (1 + log Z)
for the logarithm.  Where the reference is infinite, or nothing is eligible, equality is exact.
The bound is checked on every element; no share is left out."""
import numpy as np

import boltzmann_ref as B

NONE_ROW = 0x7fffffff
SEG_LENGTHS = (0, 1, 2, 63, 64, 65, 257, 1025)
TEMPERATURES = (1e-6, 0.1, 1.0, 1e30)
TWINS = ("weights_from_next_q", "hard_max", "no_max", "exp_over_t", "ineligible_in_z", "nan_weight_1", "feat_row_ignored",
         "last_row_dropped", "column_tail_dropped", "tile0_rows", "value_unmasked_empty")
TILE = 1024
NAN, INF = float("nan"), float("inf")


def temperature_of(case):
    return float(np.float32(case["T"]))                     # the entry point takes the temperature as a float


def reference(case, twin=None):
    lo, hi, sel, nq = case["seg_lo"], case["seg_hi"], case["select_q"], case["next_q"]
    feat, feat_row = case.get("feat"), case.get("feat_row")
    dim = 0 if feat is None else feat.shape[1]
    T = temperature_of(case)
    n_trans = len(lo)
    out = dict(value=np.full(n_trans, -np.inf), feat_mean=np.zeros((n_trans, dim)), entropy=np.zeros(n_trans),
               argmax_row=np.full(n_trans, NONE_ROW, dtype=np.int64), nothing=np.ones(n_trans, dtype=bool),
               value_bound=np.zeros(n_trans), feat_mean_bound=np.zeros((n_trans, dim)), entropy_bound=np.zeros(n_trans))
    if twin == "value_unmasked_empty":
        out["value"][:] = 0.0
    for i in range(n_trans):
        a, b = int(lo[i]), int(hi[i])
        if twin == "last_row_dropped":
            b -= 1
        if b <= a:
            continue
        q = (nq if twin == "weights_from_next_q" else sel)[a:b]
        w, elig = B.weights(q, T, twin if twin in ("no_max", "exp_over_t", "nan_weight_1") else None)
        if not elig.any() and not (w > 0).any():
            continue
        qd = q.astype(np.float64)
        m = qd[elig].max() if elig.any() else 0.0
        first = int(np.flatnonzero(elig & (qd == m))[0]) if elig.any() else 0
        if twin == "hard_max":
            w = np.zeros_like(w)
            w[first] = 1.0
        with np.errstate(all="ignore"):
            Z = w.sum() + (float((~elig).sum()) if twin == "ineligible_in_z" else 0.0)
            p = w / Z
            nz = np.flatnonzero(w > 0) if np.isfinite(Z) else np.arange(len(w))
            x = np.where(np.isinf(qd[nz]) & (m == np.inf), 0.0, (qd[nz] - m) / T)      # m = +inf: x = 0 on its rows
            pa = float((p[nz] * np.abs(x)).sum())
            a_max = float(np.abs(x).max()) if len(nz) else 0.0
            eps = (2 * (b - a) + 4 + 2 * (2 + min(a_max, 746.0))) * 2.0 ** -52
            v = nq[a:b].astype(np.float64)[nz]
            out["value"][i] = (p[nz] * v).sum()
            out["value_bound"][i] = 2 * eps * float((p[nz] * np.abs(v)).sum())
            out["entropy"][i] = np.log(Z) - (p[nz] * x).sum()
            out["entropy_bound"][i] = 2 * eps * (pa + 1.0 + abs(np.log(Z)))
            if dim:
                rows = a + nz
                if feat_row is not None and twin != "feat_row_ignored":
                    rows = feat_row[rows]
                f = feat[rows % feat.shape[0]].astype(np.float64)
                out["feat_mean"][i] = p[nz] @ f
                out["feat_mean_bound"][i] = 2 * eps * (p[nz] @ np.abs(f))
        out["argmax_row"][i] = a + first
        out["nothing"][i] = False
    if twin == "column_tail_dropped" and dim:
        out["feat_mean"][:, dim // 4 * 4:] = 0.0
    if twin == "tile0_rows" and dim > TILE:                  # a tile beyond the first reads the columns of tile 0
        out["feat_mean"][:, TILE:] = out["feat_mean"][:, np.arange(TILE, dim) % TILE]
    return out


def as_device(ref):
    """A reference (or a twin's) rounded as the device rounds its outputs."""
    with np.errstate(over="ignore"):
        return dict(value=ref["value"].astype(np.float32), feat_mean=ref["feat_mean"].astype(np.float32),
                    entropy=ref["entropy"].astype(np.float32), argmax_row=ref["argmax_row"].astype(np.int64))


def half_ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(over="ignore"):
        return 0.5 * np.spacing(np.minimum(x, np.finfo(np.float32).max).astype(np.float32)).astype(np.float64)


def violations(got, ref, figures=None):
    """Every element of every output against its bound -> list of (name, index, got, want, bound); [] = conforms.
    ``figures`` (a dict) receives, per output, the largest |error| / bound over the elements held to a bound."""
    bad = []
    rows = np.asarray(got["argmax_row"]).astype(np.int64)
    for i in np.flatnonzero(rows != ref["argmax_row"]):
        bad.append(("argmax_row", int(i), int(rows[i]), int(ref["argmax_row"][i]), 0))
    for name in ("value", "feat_mean", "entropy"):
        g = np.asarray(got[name]).astype(np.float64)
        want = ref[name]
        if g.shape != want.shape:
            bad.append((name, "shape", g.shape, want.shape, 0))
            continue
        nothing = ref["nothing"] if want.ndim == 1 else np.broadcast_to(ref["nothing"][:, None], want.shape)
        exact = nothing | ~np.isfinite(want)
        bound = half_ulp32(want) + ref[name + "_bound"]
        with np.errstate(invalid="ignore"):
            err = np.abs(g - want)
            ok = np.where(exact, (g == want) | (np.isnan(g) & np.isnan(want)), err <= bound)
        if figures is not None and (~exact).any():
            figures[name] = max(figures.get(name, 0.0), float(np.nanmax(np.where(exact, 0.0, err / bound))))
        for idx in np.argwhere(~ok)[:8]:
            idx = tuple(int(k) for k in idx)
            bad.append((name, idx, float(g[idx]), float(want[idx]), float(bound[idx])))
    return bad


# ------------------------------------------------------------------------------------------------------------------ probe tables
def random_probe(T, dim, n_trans=None, seed=41000, double=True, mapped=False, feat_rows=None):
    """Segments of every length of SEG_LENGTHS behind 3 rows that belong to nobody, two of each, in a shuffled order; then
    transitions that SHARE a segment and transitions whose ranges OVERLAP two neighbours.  ``n_trans`` cuts or extends the list
    (further transitions share the segments in turn).  q ~ 3 N(0, 1) with ties of the maximum planted in every third segment.
    ``double``: select_q and next_q are different vectors (else one array).  ``mapped``: a feat_row with duplicates into a feat
    of ``feat_rows`` rows."""
    rng = np.random.default_rng(seed + int(1000 * np.log10(T)) + 7 * dim)
    lengths = rng.permutation(np.repeat(SEG_LENGTHS, 2))
    lo = 3 + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    hi = lo + lengths
    R = int(hi[-1]) + 2
    seg_lo, seg_hi = list(lo), list(hi)
    for k in (1, 4, 9):                                      # shared: the very range of another transition
        seg_lo.append(lo[k]); seg_hi.append(hi[k])
    for k in (2, 6, 11):                                     # overlapping: the tail of one neighbour and the head of the next
        seg_lo.append((lo[k] + hi[k]) // 2); seg_hi.append((lo[k + 1] + hi[k + 1] + 1) // 2)
    if n_trans is not None:
        base = len(seg_lo)
        seg_lo = [seg_lo[i % base] for i in range(n_trans)]
        seg_hi = [seg_hi[i % base] for i in range(n_trans)]
    sel = (3.0 * rng.standard_normal(R)).astype(np.float32)
    for k in range(0, len(lengths), 3):
        if lengths[k] >= 2:
            seg = sel[lo[k]:hi[k]]
            seg[rng.integers(0, lengths[k], size=min(3, lengths[k]))] = seg.max()
    nq = (3.0 * rng.standard_normal(R)).astype(np.float32) if double else sel
    feat = feat_row = None
    if dim:
        F = R if not mapped else int(feat_rows or 37)
        feat = rng.standard_normal((F, dim)).astype(np.float32)
        if mapped:
            feat_row = rng.integers(0, F, size=R).astype(np.int64)
    return dict(seg_lo=np.asarray(seg_lo, np.int32), seg_hi=np.asarray(seg_hi, np.int32), select_q=sel, next_q=nq, T=float(T),
                feat=feat, feat_row=feat_row)


# (select_q of the segment, T) -- one transition each; next_q and feat hold NaN / inf at the rows marked ineligible
NONFINITE = [
    ([1.0, NAN, 2.0, -INF, 0.5], 1.0),
    ([NAN, NAN, 1.0, 1.0], 1.0),                             # NaN rows in front, a tie behind them
    ([NAN, INF, 3.0, INF, -INF], 0.5),                       # m = +inf: the two +inf rows weigh 1/2 each
    ([NAN, -INF, NAN], 1.0),                                 # nothing eligible
    ([-INF], 2.0),
    ([-INF, -INF, -INF, -INF], 1.0),                         # an all -inf segment
    ([1e4, 1e4 - 1.0, -1e4], 1.0),                           # q / T = +-1e4: exp(1e4) overflows without the subtraction
    ([1e-2, -1e-2, 0.0], 1e-6),                              # the same through a small T
    ([0.0, 1.0], 0.1),                                       # exp(q) / T is not exp(q / T)
    ([0.5, 0.25, 1.5], 1e30),                                # T -> inf: the mean
    ([NAN if j % 7 == 3 else (-INF if j % 11 == 5 else 0.25 * (j % 5)) for j in range(300)], 1.0),
]


def nonfinite_probe(dim=5):
    cases = []
    for k, (q, T) in enumerate(NONFINITE):
        rng = np.random.default_rng(900 + k)
        n = len(q)
        sel = np.zeros(n + 5, dtype=np.float32)
        sel[3:3 + n] = q
        bad = np.isnan(sel) | (sel == -np.inf)
        nq = (2.0 * rng.standard_normal(n + 5)).astype(np.float32)
        nq[bad] = np.where(rng.random(int(bad.sum())) < 0.5, np.nan, np.inf)
        feat = rng.standard_normal((n + 5, dim)).astype(np.float32)
        feat[bad] = np.nan
        feat[bad, ::2] = -np.inf
        cases.append(dict(seg_lo=np.asarray([3, 3, 3 + n], np.int32), seg_hi=np.asarray([3 + n, 3 + n, 3 + n], np.int32), select_q=sel,
                          next_q=nq, T=float(T), feat=feat, feat_row=None))
    # m = +inf with select_q the very array of next_q: the value is +inf, exactly
    sel = np.asarray([0.0, 1.0, INF, 2.0, INF, 0.0], dtype=np.float32)
    cases.append(dict(seg_lo=np.asarray([1], np.int32), seg_hi=np.asarray([5], np.int32), select_q=sel, next_q=sel, T=1.0,
                      feat=np.arange(24, dtype=np.float32).reshape(6, 4), feat_row=None))
    return cases


def cpu_cases():
    """The probe set of the CPU tests: every temperature, one- and two-vector forms, a mapped feat, a dim beyond one tile."""
    cases = [random_probe(T, 5, double=(k % 2 == 0)) for k, T in enumerate(TEMPERATURES)]
    cases.append(random_probe(1.0, 7, mapped=True))
    cases.append(random_probe(0.1, TILE + 4, n_trans=5, mapped=True, feat_rows=19))
    cases.append(random_probe(1.0, 0))
    return cases + nonfinite_probe()


def rejected(twin, cases=None):
    """Does the bound tell the twin from the rule on at least one case of the probe set?"""
    for case in (cpu_cases() if cases is None else cases):
        if violations(as_device(reference(case, twin)), reference(case)):
            return True
    return False
