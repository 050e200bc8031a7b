"""The rule of the Munchausen operators (bridges_soft_value / bridges_action_row, include/bridges_hip.h) stated once in float64
numpy on top of boltzmann_ref.weights, the probe tables the kernels are run on, the bound every output is held to and defective
twins the probes must reject.

A *case* is a dict as the entry point takes it: seg_lo / seg_hi int32 [n], q float32 [R], T, alpha, clip_lo (python floats, taken
as float32 like the entry point's), taken_row int32 [n] or None.  ``reference(case, temps=None)`` -> float64 arrays value, tlogp,
bonus [n], uint8 miss [n], bool nothing [n] and the bounds value_bound, tlogp_bound, bonus_bound.  ``temps`` float64 [n]: a
temperature per segment as it stands (the relative form: the device's own temp_out bits), else float32(T) for all.

The bound, first order, u = 2^-53.  Device and reference both evaluate in float64, so every term below counts twice.
  A weight w_j = exp(a_j), a_j = (q_j - m) / T: soft_target_ref's allowances -- a_j carries two roundings, |a_j| 2u, which move
  exp by the same relative amount, and exp itself is granted 2 ulp = 4u -- so w_j is off by (4 + 2 |a_j|) u relative and
  Z = sum w_j by dZ = (4 + 2 sum_j p_j |a_j|) u + n u relative, the n u for the additions in any order.
  log Z: off by dZ (d log Z = dZ / Z) plus the logarithm's own 2 ulp, 4u |log Z|.
  T log Z: one more rounding.  tz_err = T (dZ + 4u |log Z|) + u T |log Z|.
  V = m + T log Z: one more rounding:                       value_bound = 2 (tz_err + u |V|).
  L = (q_a - m) - T log Z: the difference and the result are rounded once each:
                                                            tlogp_bound = 2 (u |q_a - m| + tz_err + u |L|).
  bonus = alpha * max(L, clip_lo): max moves by no more than its operand, the product is rounded once:
                                                            bonus_bound = alpha * tlogp_bound + 2u |bonus|.
Rounding to float32 adds half a float32 ulp, taken at the reference.  Where the reference is infinite, where nothing is
eligible and where the taken row misses, equality is exact (and the bonus there is +0.0, sign included).
Every element is checked; no share is left out."""
import numpy as np

import boltzmann_ref as B
import soft_target_ref as S

U = 2.0 ** -53
NONE_ROW = 0x7fffffff
SEG_LENGTHS = (0, 1, 2, 63, 64, 65, 129, 1025)
N_SEGMENTS = (1, 3, 4, 5, 9)
TEMPERATURES = (1e-3, 0.1, 1.0, 1e30)
TWINS = ("no_max", "clip_before_min", "alpha_before_clip")
ROW_TWINS = ("desc_only", "float_eq")
NAN, INF = float("nan"), float("inf")

# the record columns the action's descriptor and pose stand in (robotoddler/training/records.py)
K = 16
O_ASHAPE = 1 + 6 * K
O_APOSE = O_ASHAPE + 1
O_ATB, O_ATF, O_AFACE = O_APOSE + 4, O_APOSE + 5, O_APOSE + 6
RECORD_WIDTH = O_AFACE + 7


def f32(x):
    return float(np.float32(x))


def reference(case, temps=None, twin=None):
    lo, hi, q = case["seg_lo"], case["seg_hi"], case["q"]
    taken = case.get("taken_row")
    alpha, clip = f32(case.get("alpha", 0.0)), f32(case.get("clip_lo", -1.0))
    n = len(lo)
    out = dict(value=np.full(n, -np.inf), tlogp=np.zeros(n), bonus=np.zeros(n), miss=np.ones(n, dtype=np.uint8),
               nothing=np.ones(n, dtype=bool), value_bound=np.zeros(n), tlogp_bound=np.zeros(n), bonus_bound=np.zeros(n))
    for i in range(n):
        a, b = int(lo[i]), int(hi[i])
        T = f32(case["T"]) if temps is None else float(temps[i])
        if b <= a:
            continue
        seg = q[a:b]
        w, elig = B.weights(seg, T, "no_max" if twin == "no_max" else None)
        if not elig.any():
            continue
        out["nothing"][i] = False
        qd = seg.astype(np.float64)
        m = qd[elig].max()
        with np.errstate(all="ignore"):
            Z = w.sum()
            if twin == "no_max":
                m_used, tlz = 0.0, T * np.log(Z)
            else:
                m_used, tlz = m, T * np.log(Z)
            V = m_used + tlz
            if m == np.inf and twin != "no_max":
                V, pa = np.inf, 0.0
            else:
                nz = w > 0
                x = np.abs((qd[nz] - m) / T)
                pa = float((w[nz] / Z * x).sum()) if np.isfinite(Z) and Z > 0 else 0.0
            dZ = (4 + 2 * pa + (b - a)) * U
            tz_err = T * (dZ + 4 * U * abs(np.log(Z))) + U * abs(tlz)
        out["value"][i] = V
        out["value_bound"][i] = 2 * (tz_err + U * abs(V)) if np.isfinite(V) else 0.0
        if taken is None:
            continue
        r = int(taken[i])
        if not (a <= r < b) or not elig[r - a]:
            continue
        with np.errstate(all="ignore"):
            if m == np.inf and twin != "no_max":
                L = (0.0 - tlz) if qd[r - a] == np.inf else -np.inf
            else:
                L = (qd[r - a] - m_used) - tlz
                if twin == "clip_before_min":
                    L = min(max(L, clip), 0.0)
                else:
                    L = min(L, 0.0)
            bonus = max(alpha * L, clip) if twin == "alpha_before_clip" else alpha * max(L, clip)
            bonus = bonus + 0.0
        out["tlogp"][i], out["bonus"][i], out["miss"][i] = L, bonus, 0
        if np.isfinite(L):
            diff = 0.0 if m == np.inf else abs(qd[r - a] - m)
            out["tlogp_bound"][i] = 2 * (U * diff + tz_err + U * abs(L))
        out["bonus_bound"][i] = alpha * out["tlogp_bound"][i] + 2 * U * abs(bonus)
    return out


def as_device(ref):
    with np.errstate(over="ignore"):
        return dict(value=ref["value"].astype(np.float32), tlogp=ref["tlogp"].astype(np.float32), bonus=ref["bonus"].astype(np.float32),
                    miss=ref["miss"].copy())


def violations(got, ref, figures=None, taken=True):
    """Every element of every output against its bound -> list of (name, index, got, want, bound); [] = conforms.
    ``figures`` (a dict) receives, per output, the largest |error| / bound over the elements held to a bound."""
    bad = []
    names = ("value", "tlogp", "bonus") if taken else ("value",)
    if taken:
        miss = np.asarray(got["miss"]).astype(np.uint8)
        for i in np.flatnonzero(miss != ref["miss"]):
            bad.append(("miss", int(i), int(miss[i]), int(ref["miss"][i]), 0))
    for name in names:
        g = np.asarray(got[name]).astype(np.float64)
        want = ref[name]
        exact = ~np.isfinite(want) | (ref["nothing"] if name == "value" else ref["miss"] == 1)
        bound = S.half_ulp32(want) + ref[name + "_bound"]
        with np.errstate(invalid="ignore"):
            err = np.abs(g - want)
            ok = np.where(exact, (g == want) | (np.isnan(g) & np.isnan(want)), err <= bound)
        if name == "bonus":                                  # a zero bonus is +0.0, where it is exact and where it is not
            ok = ok & ~((g == 0.0) & np.signbit(g))
        if figures is not None and (~exact).any():
            figures[name] = max(figures.get(name, 0.0), float(np.nanmax(np.where(exact, 0.0, err / bound))))
        for i in np.flatnonzero(~ok)[:8]:
            bad.append((name, int(i), float(g[i]), float(want[i]), float(bound[i])))
    return bad


# ------------------------------------------------------------------------------------------------------------------ probe tables
def random_probe(T, n=None, seed=73000, alpha=0.9, clip_lo=-1.0, scale=3.0, offset=0.0):
    """Segments of every length of SEG_LENGTHS behind 3 rows that belong to nobody, two of each, shuffled; then segments that SHARE
    a range and segments that OVERLAP two neighbours.  ``n`` cuts or extends the list (further segments share the ranges in
    turn).  q = offset + scale N(0, 1) with ties of the maximum planted in every third segment.  The taken row of segment i is a
    row of its own, in turn the first, the last, the arg-max and a random one; every fifth is the sentinel, every seventh lies
    one past the end."""
    rng = np.random.default_rng(seed + int(1000 * np.log10(T)))
    lengths = rng.permutation(np.repeat(SEG_LENGTHS, 2))
    lo = 3 + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    hi = lo + lengths
    R = int(hi[-1]) + 2
    seg_lo, seg_hi = list(lo), list(hi)
    for k in (1, 4, 9):
        seg_lo.append(lo[k]); seg_hi.append(hi[k])
    for k in (2, 6, 11):
        seg_lo.append((lo[k] + hi[k]) // 2); seg_hi.append((lo[k + 1] + hi[k + 1] + 1) // 2)
    if n is not None:
        base = len(seg_lo)
        seg_lo = [seg_lo[i % base] for i in range(n)]
        seg_hi = [seg_hi[i % base] for i in range(n)]
    q = (np.float32(offset) + np.float32(scale) * rng.standard_normal(R).astype(np.float32)).astype(np.float32)
    for k in range(0, len(lengths), 3):
        if lengths[k] >= 2:
            seg = q[lo[k]:hi[k]]
            seg[rng.integers(0, lengths[k], size=min(3, lengths[k]))] = seg.max()
    taken = np.full(len(seg_lo), NONE_ROW, dtype=np.int32)
    for i, (a, b) in enumerate(zip(seg_lo, seg_hi)):
        if i % 5 == 4:
            continue
        if i % 7 == 6:
            taken[i] = b
        elif b > a:
            taken[i] = (a, b - 1, a + int(np.argmax(q[a:b])), int(rng.integers(a, b)))[i % 4]
        else:
            taken[i] = a
    return dict(seg_lo=np.asarray(seg_lo, np.int32), seg_hi=np.asarray(seg_hi, np.int32), q=q, T=float(T), taken_row=taken,
                alpha=float(alpha), clip_lo=float(clip_lo))


# (q of the segment, T, taken row relative to the segment)
NONFINITE = [
    ([1.0, NAN, 2.0, -INF, 0.5], 1.0, 0),
    ([1.0, NAN, 2.0, -INF, 0.5], 1.0, 1),                    # the taken row is NaN: miss
    ([1.0, NAN, 2.0, -INF, 0.5], 1.0, 3),                    # ... is -inf: miss
    ([NAN, NAN, 1.0, 1.0], 1.0, 3),
    ([NAN, INF, 3.0, INF, -INF], 0.5, 1),                    # m = +inf, a +inf row: L = -T ln 2
    ([NAN, INF, 3.0, INF, -INF], 0.5, 2),                    # m = +inf, a finite row: L = -inf, the bonus alpha * clip_lo
    ([3.0, INF], 2.0, 1),                                    # m = +inf, one +inf row: L = 0
    ([NAN, -INF, NAN], 1.0, 0),                              # nothing eligible
    ([-INF], 2.0, 0),
    ([1e4, 1e4 - 1.0, -1e4], 1.0, 1),                        # q / T = +-1e4: exp(1e4) overflows without the subtraction
    ([1e4, 1e4 - 1.0, -1e4], 1.0, 2),                        # L = -2e4: clipped
    ([800.0, 799.0, 0.0], 1.0, 0),                           # q / T beyond 709
    ([1e-2, -1e-2, 0.0], 1e-6, 1),
    ([0.5, 0.25, 1.5], 1e30, 2),
    ([NAN if j % 7 == 3 else (-INF if j % 11 == 5 else 0.25 * (j % 5)) for j in range(300)], 1.0, 4),
]


def nonfinite_probe(alpha=0.9, clip_lo=-1.0):
    cases = []
    for qs, T, r in NONFINITE:
        n = len(qs)
        q = np.zeros(n + 5, dtype=np.float32)
        q[3:3 + n] = qs
        cases.append(dict(seg_lo=np.asarray([3, 3, 3 + n], np.int32), seg_hi=np.asarray([3 + n, 3 + n, 3 + n], np.int32), q=q,
                          T=float(T), taken_row=np.asarray([3 + r, NONE_ROW, 3 + n], np.int32), alpha=alpha, clip_lo=clip_lo))
    return cases


def tied_probe(T=0.7, alpha=0.9, clip_lo=-100.0):
    """All-tied segments of every length >= 1: V = q + T ln n, L = -T ln n."""
    lengths = [k for k in SEG_LENGTHS if k >= 1]
    lo = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int32)
    hi = (lo + np.asarray(lengths)).astype(np.int32)
    q = np.zeros(int(hi[-1]), dtype=np.float32)
    for k, (a, b) in enumerate(zip(lo, hi)):
        q[a:b] = np.float32(0.5 * k - 1.25)
    return dict(seg_lo=lo, seg_hi=hi, q=q, T=T, taken_row=((lo + hi) // 2).astype(np.int32), alpha=alpha, clip_lo=clip_lo)


def single_probe(T=0.3, alpha=1.0, clip_lo=-1.0):
    """Segments of one row: V == q and the bonus +0.0, exactly."""
    q = np.asarray([0.0, -3.5, 1e4, 7.25e-3, -1e-30, 65504.0], dtype=np.float32)
    lo = np.arange(len(q), dtype=np.int32)
    return dict(seg_lo=lo, seg_hi=lo + 1, q=q, T=T, taken_row=lo.copy(), alpha=alpha, clip_lo=clip_lo)


def offset_probe(seed=73500):
    """q = 1e4 + N(0, 1) at T = 1e-3: a large common offset, exponents down to -745 and past it."""
    return random_probe(1e-3, seed=seed, scale=1.0, offset=1e4)


def cpu_cases():
    cases = [random_probe(T) for T in TEMPERATURES]
    cases += [random_probe(1.0, n=k, seed=73100 + k) for k in N_SEGMENTS]
    cases += [random_probe(0.1, alpha=0.0), random_probe(0.1, clip_lo=0.0), random_probe(1.0, alpha=0.5, clip_lo=-0.25)]
    return cases + nonfinite_probe() + [tied_probe(), single_probe(), offset_probe()]


def rejected(twin, cases=None):
    for case in (cpu_cases() if cases is None else cases):
        if violations(as_device(reference(case, twin=twin)), reference(case)):
            return True
    return False


# ------------------------------------------------------------------------------------------------------------------ the taken row
def action_row(seg_lo, seg_hi, idx, cand_desc, cand_pose, rec, twin=None):
    """bridges_action_row: int32 [n]; cand_desc int32 [C, 4] (target_block, target_face, shape, face), cand_pose float64 [C, 4],
    rec float64 [n, W]."""
    out = np.full(len(seg_lo), NONE_ROW, dtype=np.int32)
    pose_bits = np.ascontiguousarray(cand_pose).view(np.int64)
    for i, (a, b) in enumerate(zip(seg_lo, seg_hi)):
        want_desc = rec[i, [O_ATB, O_ATF, O_ASHAPE, O_AFACE]]
        want_pose = np.ascontiguousarray(rec[i, O_APOSE:O_APOSE + 4])
        for j in range(int(a), int(b)):
            c = int(idx[j])
            if not (cand_desc[c].astype(np.float64) == want_desc).all():
                continue
            if twin == "desc_only":
                same = True
            elif twin == "float_eq":
                same = bool((cand_pose[c] == want_pose).all())
            else:
                same = bool((pose_bits[c] == want_pose.view(np.int64)).all())
            if same:
                out[i] = j
                break
    return out


def action_row_table(seed=5):
    """A hand-made candidate table and records: descriptors that repeat with other poses, two candidates with one descriptor and
    one pose (the first row wins), records that match nothing, a pose that differs from its candidate in the sign of a zero only,
    rows reached through a shuffled idx, shared segments and an empty one."""
    rng = np.random.default_rng(seed)
    C = 150
    desc = np.stack([rng.integers(-1, 3, C), rng.integers(0, 4, C), rng.integers(0, 2, C), rng.integers(0, 4, C)], axis=1).astype(np.int32)
    pose = np.round(rng.standard_normal((C, 4)), 1)          # few distinct values: poses repeat among the candidates as well
    pose[:, 3] = 0.0
    desc[40], pose[40] = desc[7], pose[7]                    # one descriptor, one pose, two candidates
    desc[41] = desc[7]                                       # the descriptor again, another pose
    pose[41] = pose[7] + 1.0
    pose[90, 3] = -0.0                                       # candidate 90: a negative zero of its own
    idx = rng.permutation(C).astype(np.int64)
    seg_lo = np.asarray([0, 0, 70, 0, 149, 30, 0, 0, 60], dtype=np.int32)
    seg_hi = np.asarray([150, 150, 150, 150, 150, 30, 150, 70, 130], dtype=np.int32)
    want = [7, 41, int(idx[100]), 90, int(idx[149]), 3, 90, int(idx[5]), 12]
    rec = np.zeros((len(seg_lo), RECORD_WIDTH + 3), dtype=np.float64)
    for i, c in enumerate(want):
        rec[i, [O_ATB, O_ATF, O_ASHAPE, O_AFACE]] = desc[c]
        rec[i, O_APOSE:O_APOSE + 4] = pose[c]
    rec[6, O_APOSE + 3] = 0.0                                # candidate 90 but for the sign of its zero
    rec[8, O_APOSE] += 1e-9                                  # the descriptor of candidate 12 with a pose nobody has
    return dict(seg_lo=seg_lo, seg_hi=seg_hi, idx=idx, cand_desc=desc, cand_pose=pose, rec=rec)
