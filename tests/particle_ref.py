"""The rule of bridges_particle_select (include/bridges_hip.h) stated in float64 numpy, a brute-force second statement in plain
Python, the probe tables the kernel is run on, and defective twins every probe set must tell from the rule.

A *case* is a dict as tests/beam_ref.py makes them (B, seg_lo / seg_hi int32 [E], q float32 [n], idx int64 [n], cand_offset int32
[E], rep int32 [E] or None, live uint8 [E], ret / disc float64 [E]; E = G * B) plus u_act float32 [E], u_res float32 [G], T, Tr
(python floats, taken as float32 by the entry point) and elite (bool).  ``reference(case)`` returns the eight outputs -- p_sel as
an unrounded float64 -- and per slot the MARGINS of its two draws, min |target - C| / total for the parent and for the row: the
device's exp may differ from libm's by an ulp and its row prefix sums are added in another order, so a target within a few ulp of
a boundary has no single right answer.  A slot is DECIDED when both margins are >= boltzmann_ref.MARGIN (an elite slot and an
empty slot draw nothing: their margins are inf).  The exact probes -- equal S and equal q, weights exactly 1, integer prefix sums,
targets that are dyadic fractions -- need no margin at all.

The bounds on p_sel and ess.  u = 2^-53.  Both sides form the argument of exp by the same two exact-rounded operations, and each
exp is within 1 ulp of the truth, so two weights differ by at most 4u relatively.
  p_sel = w_row / total: a sum of n positive terms carries at most (n - 1) u of rounding in any order, so the totals differ by at
    most (4 + 2n) u, the quotients by (10 + 2n) u; two doubles that close round to float32 values at most one float32 ulp (2^-23
    relatively) apart, and a float32 subnormal adds 2^-149 absolutely:  |got - want| <= (2^-23 + (10 + 2n) u) want + 2^-149.
  ess = total^2 / sum W^2 over at most B terms added in the same order: total within (4 + 2B) u, its square within (10 + 4B) u,
    W^2 within 10u, their sum within (10 + 2B) u, the quotient within (22 + 6B) u; doubled for the second-order terms:
    |got - want| <= 2 (22 + 6B) u want.
Neither figure was taken from a device."""
import math

import numpy as np

import beam_ref as BR
import boltzmann_ref as BZ

MARGIN = BZ.MARGIN
OUTPUTS = BR.OUTPUTS + ("p_sel", "ess")
RESAMPLE_TEMPERATURES = (1e-6, 1.0, float("inf"))
TWINS = ("ge", "no_max", "own_rows", "dead_parent", "one_position", "positions_k_plus_1", "value_mean", "score_f32", "elite_ignored",
         "elite_before_resample", "score_of_slot")
CENSUS = ("resampled", "kept_place", "elite_slot", "elite_moves", "parent_twice", "parent_dropped", "dead_env", "dead_with_rows",
          "live_without_rows", "live_no_eligible", "value_nan", "value_minus_inf", "value_plus_inf", "group_without_parents",
          "shared_rows", "row_not_first_max", "tr_inf", "tr_tiny", "weight_underflows")
U = 2.0 ** -53


def p_sel_bound(want, n):
    return (2.0 ** -23 + (10 + 2 * n) * U) * np.abs(want) + 2.0 ** -149


def ess_bound(want, B):
    return 2 * (22 + 6 * B) * U * np.abs(want)


def sentinels(E, G):
    s = BR.sentinels(E)
    s.update(p_sel=np.full(E, -7.5, np.float32), ess=np.full(G, -7.5, np.float64))
    return s


def _rows(case, e):
    n = len(case["q"])
    lo, hi = max(int(case["seg_lo"][e]), 0), min(int(case["seg_hi"][e]), n)
    return lo, max(hi, lo)


def env_value(case, e, twin=None):
    """(is a parent, S, the largest eligible q as float64) of env e."""
    lo, hi = _rows(case, e)
    seg = case["q"][lo:hi]
    elig = ~np.isnan(seg) & (seg != -np.inf)
    if not (case["live"][e] or twin == "dead_parent") or not elig.any():
        return False, np.nan, -np.inf
    v = np.float32(seg[elig].max())
    with np.errstate(invalid="ignore", over="ignore"):
        if twin == "value_mean":
            v = np.float32(seg[elig].astype(np.float64).mean())
        if twin == "score_f32":
            S = np.float64(np.float32(case["ret"][e]) + np.float32(case["disc"][e]) * v)
        else:
            S = np.float64(case["ret"][e]) + np.float64(case["disc"][e]) * np.float64(v)
    return bool(not np.isnan(S) and S != -np.inf), S, np.float64(seg[elig].max())


def resample_weights(S, Tr, twin=None):
    """S float64 [P] of the parents in env order -> their weights."""
    S = np.asarray(S, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if twin == "no_max":
            return np.exp(S / Tr)
        M = S.max()
        if Tr == np.inf:
            return np.ones(len(S))
        if M == np.inf:
            return (S == np.inf).astype(np.float64)
        return np.exp((S - M) / Tr)


def reference(case, twin=None):
    B, q, idx, off, rep = case["B"], case["q"], case["idx"], case["cand_offset"], case.get("rep")
    E = len(case["seg_lo"])
    G = E // B
    T, Tr = float(np.float32(case["T"])), float(np.float32(case["Tr"]))
    elite = bool(case["elite"]) and twin != "elite_ignored"
    u_act, u_res = np.asarray(case["u_act"], np.float32), np.asarray(case["u_res"], np.float32)
    out = dict(src=np.arange(E, dtype=np.int32), sel_compact=np.zeros(E, np.int64), sel_index=np.zeros(E, np.int32),
               q_sel=np.zeros(E, np.float32), score=np.full(E, -np.inf), live=np.zeros(E, np.uint8), p_sel=np.zeros(E, np.float64),
               ess=np.zeros(G, np.float64), margin_parent=np.full(E, np.inf), margin_row=np.full(E, np.inf),
               row=np.full(E, -1, np.int64), n_rows=np.zeros(E, np.int64), W=np.zeros(E, np.float64))
    for g in range(G):
        vals = [env_value(case, e, twin) for e in range(g * B, (g + 1) * B)]
        par = np.array([b for b in range(B) if vals[b][0]], dtype=np.int64)
        if len(par) == 0:
            continue
        S = np.array([vals[b][1] for b in par])
        W = resample_weights(S, Tr, twin)
        out["W"][g * B + par] = W
        with np.errstate(invalid="ignore", over="ignore"):
            C = np.add.accumulate(W)                             # sequential, in env order
            total = C[-1]
            out["ess"][g] = total * total / np.sum(W * W)
        best = int(par[np.argmax(S)])                            # the first parent of maximal S
        for k in range(B):
            s = g * B + k
            pos = k
            if twin == "positions_k_plus_1":
                pos = k + 1
            if twin == "elite_before_resample" and elite:        # the elite takes slot 0 first, the rule's slots follow it
                pos = k - 1
            with np.errstate(invalid="ignore", over="ignore"):
                t = (np.float64(u_res[g]) + np.float64(pos)) / np.float64(B) * total
                if twin == "one_position":
                    t = np.float64(u_res[g]) * total
                hit = (C >= t) if twin == "ge" else (C > t)
                hit &= W > 0
                mp = float(np.min(np.abs(t - C)) / total)
            if hit.any():
                p = int(par[np.argmax(hit)])
            else:
                p = int(par[np.flatnonzero(W > 0).max()]) if (W > 0).any() else int(par[-1])
            if elite and k == 0:
                p, mp = best, np.inf
            pe = g * B + p
            lo, hi = _rows(case, (s if twin == "own_rows" else pe))
            seg = q[lo:hi]
            if elite and k == 0:
                elig = ~np.isnan(seg) & (seg != -np.inf)
                r, pr, mr = int(np.argmax(np.where(elig, seg, -np.inf))), 1.0, np.inf
            else:
                r, pr, _ex, mr = BZ.select_env(seg, u_act[s], T, "ge" if twin == "ge" else ("no_max" if twin == "no_max" else None))
            if hi <= lo:                                         # (a twin only: the slot's own env has no rows)
                continue
            row = lo + r
            owner = pe if rep is None else int(rep[pe])
            sc = s if twin == "score_of_slot" else pe
            out["src"][s], out["sel_compact"][s] = pe, idx[row]
            out["sel_index"][s] = max(int(idx[row]) - int(off[owner]), 0)
            out["q_sel"][s], out["live"][s], out["p_sel"][s] = q[row], 1, pr
            with np.errstate(invalid="ignore", over="ignore"):
                out["score"][s] = np.float64(case["ret"][sc]) + np.float64(case["disc"][sc]) * np.float64(q[row])
            out["margin_parent"][s], out["margin_row"][s], out["row"][s], out["n_rows"][s] = mp, mr, row, hi - lo
    with np.errstate(invalid="ignore"):
        out["decided"] = (out["margin_parent"] >= MARGIN) & (out["margin_row"] >= MARGIN)
    return out


def brute_force(case):
    """The rule once more, in plain Python on floats, line by line as the header states it -> list per slot of
    (src, row or None, live, p_sel), and the list of ess per group."""
    B, E = case["B"], len(case["seg_lo"])
    n = len(case["q"])
    T, Tr = float(np.float32(case["T"])), float(np.float32(case["Tr"]))
    q = [float(np.float32(v)) for v in case["q"]]
    slots, esses = [], []
    for g in range(E // B):
        parents = []                                             # (b, S, lo, hi, m)
        for b in range(B):
            e = g * B + b
            lo, hi = max(int(case["seg_lo"][e]), 0), min(int(case["seg_hi"][e]), n)
            good = [q[j] for j in range(lo, hi) if not math.isnan(q[j]) and q[j] != -math.inf]
            if not case["live"][e] or not good:
                continue
            m = max(good)
            r, d = float(case["ret"][e]), float(case["disc"][e])
            prod = float(np.float64(d) * np.float64(m)) if not (d == 0.0 and math.isinf(m)) else math.nan
            S = float(np.float64(r) + np.float64(prod))
            if math.isnan(S) or S == -math.inf:
                continue
            parents.append((b, S, lo, hi, m))
        if not parents:
            slots += [(g * B + k, None, 0, 0.0) for k in range(B)]
            esses.append(0.0)
            continue
        M = max(p[1] for p in parents)
        W = []
        for p in parents:
            if Tr == math.inf:
                W.append(1.0)
            elif M == math.inf:
                W.append(1.0 if p[1] == math.inf else 0.0)
            else:
                x = (p[1] - M) / Tr
                W.append(math.exp(x) if x > -746.0 else 0.0)
        total, sq, C = 0.0, 0.0, []
        for w in W:
            total += w
            sq += w * w
            C.append(total)
        esses.append(total * total / sq)
        for k in range(B):
            t = (float(np.float32(case["u_res"][g])) + k) / B * total
            chosen = None
            for i in range(len(parents)):
                if C[i] > t:
                    chosen = i
                    break
            if chosen is None:
                chosen = max(i for i, w in enumerate(W) if w > 0)
            if case["elite"] and k == 0:
                chosen = min(i for i, p in enumerate(parents) if p[1] == M)
                b, S, lo, hi, m = parents[chosen]
                row = min(j for j in range(lo, hi) if q[j] == m)
                slots.append((g * B + b, row, 1, 1.0))
                continue
            b, S, lo, hi, m = parents[chosen]
            r, pr, _ex = BZ.brute_force(q[lo:hi], float(np.float32(case["u_act"][g * B + k])), T)
            slots.append((g * B + b, lo + r, 1, pr))
    return slots, esses


def agrees_with_brute_force(case):
    ref = reference(case)
    slots, esses = brute_force(case)
    for s, (src, row, live, pr) in enumerate(slots):
        if not ref["decided"][s] and not case.get("exact"):
            continue
        if (int(ref["src"][s]), int(ref["live"][s])) != (src, live):
            return False
        if live and (int(ref["row"][s]) != row or not math.isclose(ref["p_sel"][s], pr, rel_tol=1e-12, abs_tol=0.0)):
            return False
    return bool(np.allclose(ref["ess"], esses, rtol=1e-12, atol=0.0))


def differs(a, b, case):
    """Do two results differ on a slot that the rule (a) decides, or in ess?"""
    d = a["decided"] if not case.get("exact") else np.ones(len(a["src"]), bool)
    for k in ("src", "sel_compact", "sel_index", "live"):
        if not np.array_equal(a[k][d], b[k][d]):
            return True
    for k in ("q_sel", "score"):
        if a[k][d].tobytes() != b[k][d].tobytes():
            return True
    if not np.allclose(a["p_sel"][d], b["p_sel"][d], rtol=2.0 ** -22, atol=0.0, equal_nan=True):
        return True
    return not np.allclose(a["ess"], b["ess"], rtol=2.0 ** -40, atol=0.0, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ probe tables
def _with(case, u_act, u_res, T, Tr, elite, **extra):
    case = dict(case)
    case.update(u_act=np.asarray(u_act, np.float32), u_res=np.asarray(u_res, np.float32), T=float(T), Tr=float(Tr), elite=bool(elite))
    case.update(extra)
    return case


def random_probe(G, B, T, Tr, elite, seed, lengths=BZ.SEG_LENGTHS, all_parents=False):
    """G groups of B envs with segments of the lengths of boltzmann_ref.SEG_LENGTHS mixed within one call (a length 0 makes a live
    env without rows), q ~ 3 N(0, 1) with planted ties of the maximum, some dead envs (with rows), some envs that share an earlier
    env's rows, returns on a coarse grid (values tie across envs), discounts 0.5^d."""
    rng = np.random.default_rng(seed)
    E = G * B
    lens = rng.choice(np.asarray([v for v in lengths if v or not all_parents]), size=E)
    rep = np.arange(E, dtype=np.int32)
    segs, start = [], 3                                          # three rows in front that belong to nobody
    for e in range(E):
        if e % B and rng.random() < 0.2 and not all_parents:
            rep[e] = rep[e - 1 - int(rng.integers(0, e % B))]
            segs.append(segs[rep[e]])
        else:
            segs.append((start, start + int(lens[e])))
            start += int(lens[e])
    n = start + 2
    q = (3.0 * rng.standard_normal(n)).astype(np.float32)
    for e in range(0, E, 4):
        lo, hi = segs[e]
        if hi - lo >= 2:
            q[lo + rng.integers(0, hi - lo, size=min(3, hi - lo))] = q[lo:hi].max()
    idx = np.cumsum(rng.integers(1, 4, size=n)).astype(np.int64)
    off = np.array([int(idx[min(s[0], n - 1)]) - int(rng.integers(0, 2)) for s in segs], dtype=np.int32)
    live = np.ones(E, np.uint8) if all_parents else (rng.random(E) < 0.85).astype(np.uint8)
    ret = rng.integers(-4, 5, size=E) / 2.0
    disc = 0.5 ** rng.integers(0, 4, size=E)
    case = BR._case(B, segs, q, live, ret, disc, rep=rep, idx=idx, cand_offset=off)
    return _with(case, rng.random(E, dtype=np.float32), rng.random(G, dtype=np.float32), T, Tr, elite)


def random_probes():
    """name -> case: every width, temperature and resampling temperature of the lists, with and without the elite."""
    t = {}
    for i, B in enumerate((1, 2, 3, 16)):
        for j, T in enumerate(BZ.TEMPERATURES):
            for k, Tr in enumerate(RESAMPLE_TEMPERATURES):
                elite = (i + j + k) % 2 == 0
                t[f"B{B}_T{T:g}_Tr{Tr:g}_{'elite' if elite else 'plain'}"] = random_probe(5, B, T, Tr, elite, seed=9000 + 100 * i + 10 * j + k)
    return t


def exact_probes():
    """name -> case with exact=True: equal q everywhere and ret / disc such that every parent has the same S, so every weight is
    exactly 1 and every prefix sum an integer; B a power of two, u_res and u_act dyadic (k / n and k / n +- 2^-24), so the targets
    are exact and lie on and one float32 step beside every boundary.  The strict rule alone decides them, whatever the order of the additions."""
    t = {}
    for B in (1, 2, 4, 8, 16):
        for dead in ((), (0,), tuple(range(1, B, 2))):
            if len(dead) >= B:
                continue
            n_seg = 8
            us = [0.0, 0.125, 0.5, 0.875, 1.0 - 2.0 ** -24]
            G = len(us)
            segs = [(3 + e * n_seg, 3 + (e + 1) * n_seg) for e in range(G * B)]
            q = np.full(3 + G * B * n_seg + 2, 0.375, np.float32)
            live = np.array([0 if (e % B) in dead else 1 for e in range(G * B)], np.uint8)
            case = BR._case(B, segs, q, live, [0.5] * (G * B), [0.25] * (G * B))
            # k / n on every boundary, and one float32 step beside it on either side (2^-24: exact in float32 below 1, and
            # (k / 8 +- 2^-24) * 8 is exact in binary64)
            u_act = [((3 * e) % n_seg) / n_seg + (0.0, 2.0 ** -24, -(2.0 ** -24) if (3 * e) % n_seg else 2.0 ** -24)[e % 3]
                     for e in range(G * B)]
            for elite in (False, True):
                t[f"B{B}_dead{len(dead)}_{'elite' if elite else 'plain'}"] = _with(case, u_act, us, 0.1, 1.0, elite, exact=True)
    return t


NAN, INF = float("nan"), float("inf")


def nonfinite_probes():
    """name -> case: NaN / +-inf in q, ret and disc, all-dead groups, a live env without rows, a dead env with rows."""
    t = {}
    # B = 4 throughout; rows: env 0 (0,3) env 1 (3,6) env 2 (6,6) env 3 (6,9)
    segs = [(0, 3), (3, 6), (6, 6), (6, 9)]
    base_q = [1.0, 2.0, 0.5, 0.25, 1.5, 1.75, 3.0, -1.0, 0.0]

    def mk(q=base_q, live=(1, 1, 1, 1), ret=(0.0, 0.5, 9.0, -1.0), disc=(1.0, 0.5, 1.0, 0.25), Tr=1.0, T=1.0, elite=False,
           u_res=0.3, u_act=(0.1, 0.4, 0.6, 0.9)):
        return _with(BR._case(4, segs, q, live, ret, disc), u_act, [u_res], T, Tr, elite)
    t["live_env_without_rows"] = mk()
    t["dead_env_with_rows"] = mk(live=(1, 0, 1, 1), ret=(0.0, 50.0, 9.0, -1.0))
    t["all_dead"] = mk(live=(0, 0, 0, 0))
    t["q_nan_and_minus_inf"] = mk(q=[NAN, 2.0, -INF, -INF, NAN, -INF, 3.0, NAN, 0.0])
    t["q_plus_inf"] = mk(q=[1.0, INF, 0.5, 0.25, 1.5, 1.75, INF, -1.0, INF], u_act=(0.1, 0.4, 0.6, 0.7))
    t["q_plus_inf_disc_zero"] = mk(q=[1.0, INF, 0.5, 0.25, 1.5, 1.75, 3.0, -1.0, 0.0], disc=(0.0, 0.5, 1.0, 0.25))   # S NaN: no parent
    t["ret_nan"] = mk(ret=(NAN, 0.5, 9.0, -1.0))
    t["ret_minus_inf"] = mk(ret=(0.0, -INF, 9.0, -1.0))
    t["ret_plus_inf"] = mk(ret=(0.0, INF, 9.0, INF), u_res=0.6)
    t["ret_plus_inf_tr_inf"] = mk(ret=(0.0, INF, 9.0, -1.0), Tr=INF)
    t["disc_nan"] = mk(disc=(1.0, NAN, 1.0, 0.25))
    t["disc_minus_inf"] = mk(disc=(1.0, 0.5, 1.0, -INF))         # S = -1 + -inf * 3 = -inf: no parent
    t["nothing_eligible_anywhere"] = mk(q=[NAN] * 3 + [-INF] * 3 + [NAN, -INF, NAN])
    t["elite_on_nonfinite"] = mk(q=[NAN, 2.0, 2.0, -INF, NAN, 1.0, 3.0, NAN, 3.0], ret=(1.0, 0.5, 9.0, 0.0), disc=(1.0, 1.0, 1.0, 1.0),
                                 elite=True)
    return t


def named_probes():
    """name -> case: one small table per defect the twins make, small enough to read."""
    t = {}
    segs = [(0, 3), (3, 6), (6, 9), (9, 12)]
    q = [1.0, 2.0, 0.5, 0.25, 1.5, 1.75, 3.0, -1.0, 0.0, 0.5, 0.5, 4.0]
    # four parents, moderate weights, a draw in every quarter
    t["plain"] = _with(BR._case(4, segs, q, [1, 1, 1, 1], [0.0, 0.5, -1.0, -2.5], [1.0, 0.5, 1.0, 0.25]), [0.1, 0.4, 0.6, 0.9], [0.3],
                       1.0, 1.0, False)
    t["plain_elite"] = dict(t["plain"], elite=True)
    # a dead env holds the best value by far
    t["dead_best"] = _with(BR._case(4, segs, q, [1, 0, 1, 1], [0.0, 50.0, -1.0, -2.5], [1.0, 0.5, 1.0, 0.25]), [0.1, 0.4, 0.6, 0.9],
                           [0.3], 1.0, 1.0, False)
    # values near 1000 at T_r = 1 and q near 1000 at T = 1: exp overflows without the maximum
    t["large_values"] = _with(BR._case(2, [(0, 2), (2, 4)], [1000.0, 999.0, 999.5, 998.0], [1, 1], [900.0, 900.5], [1.0, 1.0]),
                              [0.5, 0.9], [0.4], 1.0, 1.0, False)
    # the values need binary64: in float32 1e8 + 1 == 1e8 + 2.5 and the weights would tie
    t["value_needs_f64"] = _with(BR._case(2, [(0, 1), (1, 2)], [1.0, 2.5], [1, 1], [1e8, 1e8], [1.0, 1.0]), [0.5, 0.5], [0.3], 1.0, 1.0, False)
    # equal weights, integer prefix sums, targets ON the boundaries: the strict rule alone decides
    t["on_boundaries"] = _with(BR._case(4, segs, [0.5] * 12, [1, 1, 1, 1], [1.0] * 4, [1.0] * 4), [0.0, 1.0 / 3, 2.0 / 3, 0.0], [0.0],
                               1.0, 1.0, False, exact=True)
    # the best parent is the last env: the elite moves it to slot 0, and only after the assignment
    t["elite_last_env"] = _with(BR._case(4, segs, q, [1, 1, 1, 1], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]), [0.1, 0.4, 0.6, 0.9],
                                [0.5], 1.0, 2.0, True)
    # the mean of q and its maximum order the parents differently
    t["mean_and_max"] = _with(BR._case(2, [(0, 3), (3, 6)], [5.0, -9.0, -9.0, 2.0, 2.0, 2.0], [1, 1], [0.0, 0.0], [1.0, 1.0]),
                              [0.5, 0.5], [0.25], 1.0, 0.5, False)
    # every weight but the best underflows: T_r tiny
    t["tr_tiny"] = dict(t["plain"], Tr=1e-6)
    t["tr_inf"] = dict(t["plain"], Tr=INF)
    # envs that share rows through rep, with offsets of their own
    t["shared_rows"] = _with(BR._case(4, [(0, 3), (0, 3), (3, 5), (0, 3)], [0.1, 0.9, 0.5, 0.9, 0.2], [1, 1, 1, 1], [0.0, 0.25, 0.0, -1.0],
                                      [1.0] * 4, rep=[0, 0, 2, 0], cand_offset=[4, 1000, 15, 2000]), [0.2, 0.5, 0.7, 0.95], [0.6],
                             0.5, 1.0, False)
    return t


def all_probes():
    t = {}
    for make in (named_probes, nonfinite_probes, exact_probes, random_probes):
        for k, v in make().items():
            t[f"{make.__name__}:{k}"] = v
    return t


def census(case):
    """The names of CENSUS that a case shows."""
    ref = reference(case)
    B, E = case["B"], len(case["seg_lo"])
    seen = set()
    Tr = float(np.float32(case["Tr"]))
    if Tr == np.inf:
        seen.add("tr_inf")
    if Tr <= 1e-5:
        seen.add("tr_tiny")
    for e in range(E):
        lo, hi = _rows(case, e)
        seg = case["q"][lo:hi]
        elig = ~np.isnan(seg) & (seg != -np.inf)
        if not case["live"][e]:
            seen.add("dead_env")
            if hi > lo:
                seen.add("dead_with_rows")
            continue
        if hi <= lo:
            seen.add("live_without_rows")
        elif not elig.any():
            seen.add("live_no_eligible")
        else:
            _ok, S, _m = env_value(case, e)
            if np.isnan(S):
                seen.add("value_nan")
            elif S == -np.inf:
                seen.add("value_minus_inf")
            elif S == np.inf:
                seen.add("value_plus_inf")
        if case.get("rep") is not None and case["rep"][e] != e:
            seen.add("shared_rows")
    for g in range(E // B):
        sl = slice(g * B, (g + 1) * B)
        if not ref["live"][sl].any():
            seen.add("group_without_parents")
            continue
        src = ref["src"][sl] - g * B
        parents = [b for b in range(B) if env_value(case, g * B + b)[0]]
        counts = np.bincount(src, minlength=B)
        if (counts > 1).any():
            seen.add("parent_twice")
        if any(counts[b] == 0 for b in parents):
            seen.add("parent_dropped")
        if ((ref["W"][sl] == 0) & np.isin(np.arange(B), parents)).any():
            seen.add("weight_underflows")
        for k in range(B):
            s = g * B + k
            if case["elite"] and k == 0:
                seen.add("elite_slot")
                if src[k] != 0:
                    seen.add("elite_moves")
                continue
            seen.add("kept_place" if src[k] == k else "resampled")
            lo, hi = _rows(case, int(ref["src"][s]))
            seg = case["q"][lo:hi]
            elig = ~np.isnan(seg) & (seg != -np.inf)
            if int(ref["row"][s]) != lo + int(np.argmax(np.where(elig, seg, -np.inf))):
                seen.add("row_not_first_max")
    return seen
