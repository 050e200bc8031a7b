"""The rule of the relative-temperature operators (bridges_boltzmann_select_rel / bridges_soft_expect_rel, include/bridges_hip.h)
on top of the references of their scalar siblings: the spread of a segment, the effective temperature T_e with a derived bound,
the probe tables, and defective twins of the spread that the bound must reject.

``spread(q)`` is the population standard deviation of the finite rows of one segment, effectively exact: the mean and the sum of
squared deviations are math.fsum sums (correctly rounded), so the result carries a handful of float64 roundings, counted below.
``effective_temperature(q, temperature, floor)`` -> (T_e, bound): the device's temp_out is held to |device - T_e| <= bound.

The bound, first order in u = 2^-53, for a segment with n >= 2 finite rows, A = mean |q_j|, exact spread s:
  the device's sum of the q_j (float32 values, exact as doubles) takes n - 1 additions in an order of its own: off by at most
  (n - 1) u sum|q_j| in any order; the division by n adds u |mean|.  So its mean is off by at most d = (n - 1) u A + u |mean|
  <= n u A; this module's mean (one fsum, one division) by u |mean|.  Both fit in                 D = (n + 2) u A.
  CANCELLATION: sum_j (q_j - mean')^2 = n s^2 + n (mean - mean')^2 for ANY mean', because sum_j (q_j - mean) = 0.  A mean that
  is off by D therefore turns s into sqrt(s^2 + D^2): off by at most min(D, D^2 / (2 s)) -- D itself where all rows tie but
  for rounding (s -> 0), second order where s >> D.  This is the term that covers q - mean at a large common offset: D scales
  with |q|, not with the spread.  (Exact ties give s = 0 on both sides: k * q is exact for k < 2^29 and a float32 q, so is the
  quotient.)
  Each difference q_j - mean' is rounded once (relative u, so 2 u on its square), each square once (u), the n - 1 additions of
  non-negative terms in any order (n - 1) u, the division by n u: (n + 3) u relative on s^2, half of it on s; the square root
  u more:                                                                                          (n / 2 + 3) u s.
  This module: 2 u + u on the squares, one fsum rounding, the division, halved, and the root: 3.5 u s.  Together and rounded
  up:                                                                    s_bound = (n / 2 + 8) u s + min(D, D^2 / (2 s)).
  T_e = temperature * max(s, floor): the float32 factors are exact doubles, the product is rounded once on each side, and max
  moves by no more than its first operand:                                      bound = temperature * s_bound + 2 u T_e.
n < 2 finite rows: s = 0 and T_e = temperature * floor on both sides, one and the same product: the bound is 0.

The draw and the expectation are NOT restated here: ``select_reference`` calls boltzmann_ref.select_env and
``expect_reference`` soft_target_ref.reference at the temperatures handed in (one float64 per segment, not rounded to float32:
the device's own temp_out bits in the GPU tests)."""
import contextlib
import math

import numpy as np

import boltzmann_ref as B
import soft_target_ref as S

U = 2.0 ** -53
FLOOR = 1e-3
MULTIPLES = B.TEMPERATURES                                   # the probe tables' T, read as the multiple of the spread
TWINS = ("sample_variance", "inf_counted", "nan_counted", "ineligible_in_mean", "floor_ignored", "floor_added", "single_pass",
         "float32_accumulation")                            # and spread_of_next_q, a twin of the expectation's cases alone


def spread(q, twin=None):
    """One segment's rows (float32) -> (s, n_f, mean |q| over the finite rows)."""
    q = np.asarray(q, dtype=np.float32)
    fin = np.isfinite(q)
    if twin == "inf_counted":
        fin = ~np.isnan(q)
    elif twin == "nan_counted":
        fin = ~np.isinf(q)
    x = q[fin].astype(np.float64)
    n = len(x)
    count = n
    if twin == "ineligible_in_mean":                         # NaN and -inf rows masked to 0 but still counted
        count = n + int((np.isnan(q) | (q == -np.inf)).sum())
    if count < 2 or n == 0:
        return 0.0, n, 0.0
    A = math.fsum(np.abs(x)) / n
    with np.errstate(invalid="ignore", over="ignore"):
        if twin == "float32_accumulation":
            x32 = q[fin]
            mean32 = np.float32(0)
            for v in x32:
                mean32 = np.float32(mean32 + v)
            mean32 = np.float32(mean32 / np.float32(n))
            dev32 = np.float32(0)
            for v in x32:
                d = np.float32(v - mean32)
                dev32 = np.float32(dev32 + np.float32(d * d))
            return float(np.sqrt(np.float32(dev32 / np.float32(n)))), n, A
        if twin == "single_pass":
            mean = float(np.sum(x)) / n
            return math.sqrt(max(float(np.sum(x * x)) / n - mean * mean, 0.0)), n, A
        if not np.isfinite(x).all():                         # (a twin that lets a non-finite row in)
            return float("nan"), n, A
        mean = math.fsum(x) / count
        dev = math.fsum((x - mean) ** 2)
    return math.sqrt(dev / ((n - 1) if twin == "sample_variance" else count)), n, A


def spread_brute_force(q):
    """The spread once more in exact rational arithmetic, line by line as the header states it; one rounding and a root."""
    from fractions import Fraction
    x = [Fraction(float(v)) for v in np.asarray(q, dtype=np.float32) if math.isfinite(float(v))]
    if len(x) < 2:
        return 0.0
    mean = sum(x) / len(x)
    return math.sqrt(sum((v - mean) ** 2 for v in x) / len(x))


def effective_temperature(q, temperature, floor=FLOOR, twin=None):
    """-> (T_e, bound) of one segment; temperature and floor as the entry point takes them (floats)."""
    T, f = float(np.float32(temperature)), float(np.float32(floor))
    s, n, A = spread(q, twin)
    if twin == "floor_ignored":
        te = T * s
    elif twin == "floor_added":
        te = T * (s + f)
    else:
        te = T * max(s, f) if s == s else float("nan")
    if n < 2 or s == 0.0:
        return te, 0.0
    D = (n + 2) * U * A
    s_bound = (n / 2 + 8) * U * s + min(D, D * D / (2 * s))
    return te, T * s_bound + 2 * U * te


def temperatures(seg_lo, seg_hi, q, temperature, floor=FLOOR, twin=None):
    """Every segment of a case -> (T_e [n] float64, bound [n])."""
    out = [effective_temperature(q[lo:hi] if hi > lo else q[:0], temperature, floor, twin) for lo, hi in zip(seg_lo, seg_hi)]
    return np.asarray([t for t, _ in out], dtype=np.float64), np.asarray([b for _, b in out], dtype=np.float64)


def select_temperatures(case, floor=FLOOR, twin=None):
    return temperatures(case["seg_lo"], case["seg_hi"], case["q"], case["T"], floor, twin)


def expect_temperatures(case, floor=FLOOR, twin=None):
    q = case["next_q"] if twin == "spread_of_next_q" else case["select_q"]
    return temperatures(case["seg_lo"], case["seg_hi"], q, case["T"], floor, None if twin == "spread_of_next_q" else twin)


def select_reference(case, temps):
    """boltzmann_ref's draw of every env at ITS temperature temps[e] (float64, as it stands) -> boltzmann_ref.reference's dict."""
    lo, hi, q, idx, off, rep = case["seg_lo"], case["seg_hi"], case["q"], case["idx"], case["cand_offset"], case.get("rep")
    E, n_rows = len(lo), len(q)
    u = np.asarray(case["u"], dtype=np.float32)
    out = dict(row=np.zeros(E, np.int64), sel_compact=np.zeros(E, np.int64), sel_index=np.zeros(E, np.int32),
               q_sel=np.zeros(E, np.float32), explore_w=np.zeros(E, np.float32), p_sel=np.zeros(E, np.float64),
               margin=np.full(E, np.inf))
    for e in range(E):
        has = hi[e] > lo[e]
        r, p, ex, mg = B.select_env(q[lo[e]:hi[e]] if has else q[:0], u[e], float(temps[e]))
        row = min(int(lo[e]) + r if has else 0, n_rows - 1)
        owner = e if rep is None else int(rep[e])
        out["row"][e], out["sel_compact"][e] = row, idx[row]
        out["sel_index"][e] = max(int(idx[row]) - int(off[owner]), 0)
        out["q_sel"][e] = q[row] if has else 0.0
        out["explore_w"][e], out["p_sel"][e], out["margin"][e] = ex, p, mg
    return out


@contextlib.contextmanager
def _temperature_as_it_stands():
    """soft_target_ref.reference rounds a case's T to float32 (its entry point takes a float); here T is a float64 already."""
    keep = S.temperature_of
    S.temperature_of = lambda case: float(case["T"])
    try:
        yield
    finally:
        S.temperature_of = keep


def expect_reference(case, temps):
    """soft_target_ref.reference of every transition at ITS temperature temps[i] -> soft_target_ref.reference's dict."""
    parts = []
    with _temperature_as_it_stands():
        for i in range(len(case["seg_lo"])):
            one = dict(case, seg_lo=case["seg_lo"][i:i + 1], seg_hi=case["seg_hi"][i:i + 1], T=float(temps[i]))
            parts.append(S.reference(one))
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


# ------------------------------------------------------------------------------------------------------------------ probe tables
def _offset_values(n, rng):
    return rng.permutation(np.float32(1e4) + np.float32(1e-2) * np.arange(n, dtype=np.float32)).astype(np.float32)


def select_offset_probe(multiple=1.0, seed=5150):
    """boltzmann_ref's layout over its segment lengths, every segment 1e4 + 1e-2 k: a large common offset, a small spread."""
    rng = np.random.default_rng(seed)
    lengths = rng.permutation(np.repeat(B.SEG_LENGTHS, 2))
    lo, hi, n, idx, off = B._layout(lengths, rng)
    q = np.zeros(n, dtype=np.float32)
    for a, b in zip(lo, hi):
        q[a:b] = _offset_values(b - a, rng)
    return dict(seg_lo=lo, seg_hi=hi, q=q, u=rng.random(len(lengths), dtype=np.float32), T=float(multiple), idx=idx, cand_offset=off,
                rep=None)


def select_tied_probe(multiple=1.0, seed=5151):
    """Every segment all-tied at a value of its own (the floor binds), and segments of one finite row among NaN / inf rows."""
    case = select_offset_probe(multiple, seed)
    rng = np.random.default_rng(seed)
    for k, (a, b) in enumerate(zip(case["seg_lo"], case["seg_hi"])):
        case["q"][a:b] = np.float32(rng.standard_normal() * 100.0)
        if k % 3 == 2 and b - a >= 3:                        # one finite row: n_f = 1, s = 0
            case["q"][a + 1:b] = np.nan
            case["q"][a + 1] = -np.inf
            if k % 2:
                case["q"][b - 1] = np.inf
    return case


def select_cases():
    """Every select probe: boltzmann_ref's tables with T read as the multiple, the offset and the tied tables."""
    return B.margin_cases() + [select_offset_probe(), select_offset_probe(0.1, 5152), select_tied_probe()]


def select_exact_cases():
    return B.nonfinite_probe(B.NONFINITE_EXACT) + [B.exact_probe()[0]]


EXPECT_DIMS = (0, 5, 1027)                                   # 1027: a second column tile with a tail


def expect_offset_probe(dim, multiple=1.0, seed=6160, tied=False):
    case = S.random_probe(multiple, dim, seed=seed)
    rng = np.random.default_rng(seed)
    sel = case["select_q"]
    lengths = sorted({(int(a), int(b)) for a, b in zip(case["seg_lo"][:2 * len(S.SEG_LENGTHS)], case["seg_hi"][:2 * len(S.SEG_LENGTHS)])})
    for a, b in lengths:
        sel[a:b] = np.float32(rng.standard_normal() * 100.0) if tied else _offset_values(b - a, rng)
    return case


def expect_cases():
    """Every expectation probe: soft_target_ref's random table at every multiple and dim of EXPECT_DIMS (one and two value
    vectors, shared and overlapping segments), its non-finite tables, the offset and the tied tables."""
    cases = [S.random_probe(T, dim, double=(k + j) % 2 == 0, mapped=dim == 1027, feat_rows=19 if dim == 1027 else None)
             for k, T in enumerate(MULTIPLES) for j, dim in enumerate(EXPECT_DIMS) if dim != 1027 or T in (0.1, 1.0)]
    return cases + S.nonfinite_probe() + [expect_offset_probe(5), expect_offset_probe(0, 0.1), expect_offset_probe(5, tied=True)]


def unit_spread_rows(n, a, rng):
    """n rows (n even), half a - 1 and half a + 1 with a small integer a, shuffled: mean a and spread 1 exactly, whatever the
    order of the sums (every partial sum is a small integer)."""
    assert n % 2 == 0
    return rng.permutation(np.repeat(np.asarray([a - 1.0, a + 1.0], dtype=np.float32), n // 2))


UNIT_LENGTHS = (2, 64, 130, 1026)


def rejected(twin, select=None, expect=None):
    """Does the T_e bound tell the twin from the rule on at least one segment of the probe set?"""
    for case, temps_of in [(c, select_temperatures) for c in (select_cases() if select is None else select)] + \
                          [(c, expect_temperatures) for c in (expect_cases() if expect is None else expect)]:
        if twin == "spread_of_next_q" and temps_of is select_temperatures:
            continue
        want, bound = temps_of(case)
        got, _ = temps_of(case, twin=twin)
        with np.errstate(invalid="ignore"):
            if (~(np.abs(got - want) <= bound)).any():
                return True
    return False
