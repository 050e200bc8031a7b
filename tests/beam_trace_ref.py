"""The rule of bridges_beam_trace (include/bridges_hip.h) stated once in numpy, the probe tables the kernel is run on, seeded tables
and deliberately defective twins of the rule.  Test infrastructure, not a test module: nothing here needs a GPU, so
tests/test_cpu_beam_trace.py holds the reference against the n-step window of tests/nstep_ref.py and against the twins, and
tests/test_gpu_beam_trace.py applies the same rule to the kernel.

A case is a dict: B, n_step, gamma, priority, rec float64 [D, E, 111], valid uint8 [D, E], parent int32 [D, E], end_env and
end_depth int32 [G], tail float64 [E, n_tail] or None.  Copies are of BITS: every comparison goes through the uint64 view."""
import math

import numpy as np

from robotoddler.training import records as R

W = R.RECORD_WIDTH
TWINS = ("by_slot", "parent_of_wrong_depth", "no_clamp_at_the_tail", "stable_of_last_step", "undiscounted", "tail_of_first_slot",
         "broken_emitted", "offsets_count_broken")
OUTPUTS = ("rows", "offset", "status")
ROW_SENTINEL = np.uint64(0x7FF8DEADBEEF0001)                 # a NaN with a payload no computation produces
INT_SENTINEL = -77
U64 = 2.0 ** -53


def dims(case):
    D, E = case["parent"].shape
    B = case["B"]
    n_tail = 0 if case["tail"] is None else case["tail"].shape[1]
    return dict(D=D, E=E, B=B, G=E // B, n_tail=n_tail, W_out=W + n_tail + (1 if case["n_step"] > 1 else 0))


def sentinels(case):
    d = dims(case)
    return dict(rows=np.full((d["G"] * d["D"], d["W_out"]), ROW_SENTINEL, dtype=np.uint64).view(np.float64),
                offset=np.full(d["G"] + 1, INT_SENTINEL, dtype=np.int32), status=np.full(d["G"], INT_SENTINEL, dtype=np.int32))


def same(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in OUTPUTS)


def chain(case, g, twin=None):
    """-> (envs e_0 .. e_{L-1} or None, status).  None with status 0: nothing ended; None with status 1: a broken chain."""
    d = dims(case)
    D, B = d["D"], d["B"]
    lo, hi = g * B, g * B + B
    ed = int(case["end_depth"][g])
    if ed < 0:
        return None, 0
    if ed >= D:
        return None, 1
    lenient = twin == "broken_emitted"
    e = int(case["end_env"][g])
    if not lo <= e < hi:
        if not lenient:
            return None, 1
        e = lo + e % B
    envs = [0] * (ed + 1)
    for t in range(ed, -1, -1):
        if not lo <= e < hi:
            if not lenient:
                return None, 1
            e = lo + e % B
        if not case["valid"][t, e] and not lenient:
            return None, 1
        envs[t] = e
        if t > 0:
            if twin == "by_slot":
                pass
            elif twin == "parent_of_wrong_depth":
                e = int(case["parent"][t - 1, e])
            else:
                e = int(case["parent"][t, e])
    return envs, 0


def returns(lins, gamma, twin=None):
    """The h-step return in the fixed order of the rule: binary64, every product and sum rounded once."""
    acc, disc = np.float64(0.0), np.float64(1.0)
    with np.errstate(all="ignore"):
        for lin in lins:
            acc = acc + disc * np.float64(lin)
            if twin != "undiscounted":
                disc = disc * np.float64(gamma)
    return acc


def reference(case, twin=None):
    """-> dict(rows [G * D, W_out] float64 -- the sentinel where nothing is written --, offset int32 [G + 1], status int32 [G]) and,
    under the keys g_exact / g_bound [G * D], the direct sum of every row's return (math.fsum) and the bound of
    tests/nstep_ref.py on the distance of the rule's summation order from it."""
    d = dims(case)
    D, B, G, n_tail, Wo = d["D"], d["B"], d["G"], d["n_tail"], d["W_out"]
    n, gamma = case["n_step"], float(case["gamma"])
    rec_bits = case["rec"].view(np.uint64)
    out = sentinels(case)
    rows = out["rows"].view(np.uint64)
    g_exact, g_bound = np.zeros(G * D), np.zeros(G * D)
    at = 0
    for g in range(G):
        out["offset"][g] = at
        envs, status = chain(case, g, twin)
        out["status"][g] = status
        if envs is None:
            if twin == "offsets_count_broken" and status == 1:
                at += min(int(case["end_depth"][g]) + 1, D)
            continue
        L = len(envs)
        for t in range(L):
            h = n if twin == "no_clamp_at_the_tail" else min(n, L - t)
            last = min(t + h - 1, L - 1)
            row = rows[at + t]
            row[:W] = rec_bits[last, envs[last]]
            if twin != "stable_of_last_step":
                row[R.O_STABLE_S] = rec_bits[t, envs[t], R.O_STABLE_S]
            row[R.O_TD] = np.float64(case["priority"]).view(np.uint64)
            lins = [case["rec"][k, envs[k], R.O_LIN] for k in range(t, last + 1)]
            if h > 1:
                row[R.O_LIN] = returns(lins, gamma, twin).view(np.uint64)
            with np.errstate(all="ignore"):
                terms = [gamma ** k * float(l) for k, l in enumerate(lins)]
            if all(math.isfinite(v) for v in terms):
                g_exact[at + t] = math.fsum(terms)
                g_bound[at + t] = 2 * len(terms) * U64 * math.fsum(abs(v) for v in terms)
            else:
                g_exact[at + t] = g_bound[at + t] = math.nan
            if n_tail:
                src = g * B if twin == "tail_of_first_slot" else int(case["end_env"][g])
                src = src if g * B <= src < g * B + B else g * B + src % B             # (broken_emitted only)
                row[W:W + n_tail] = case["tail"].view(np.uint64)[src]
            if n > 1:
                row[W + n_tail] = np.float64(h).view(np.uint64)
        at += L
    out["offset"][G] = at
    out["g_exact"], out["g_bound"] = g_exact, g_bound
    return out


def emitted(case, ref):
    """The rows of ``ref`` that a call writes: a bool mask over its G * D rows."""
    m = np.zeros(ref["rows"].shape[0], dtype=bool)
    m[:int(ref["offset"][-1])] = True
    return m


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def _records(rng, D, E):
    """Records as a search leaves them: NB = the depth, plausible scalars, DONE nowhere (the caller sets it at the ends)."""
    rec = rng.standard_normal((D, E, W))
    rec[:, :, R.O_NB] = np.arange(D)[:, None]
    rec[:, :, R.O_REWARD] = rng.integers(0, 3, (D, E))
    rec[:, :, R.O_DONE] = 0.0
    rec[:, :, R.O_STABLE_S] = rng.integers(0, 2, (D, E))
    rec[:, :, R.O_STABLE_N] = rng.integers(0, 2, (D, E))
    return np.ascontiguousarray(rec)


def _permuting_parents(rng, D, G, B):
    """Every depth permutes the slots of every group (a derangement where B > 1); row 0 holds what must never be read."""
    parent = np.zeros((D, G * B), dtype=np.int32)
    for t in range(D):
        for g in range(G):
            p = rng.permutation(B)
            if B > 1:
                while np.any(p == np.arange(B)):
                    p = rng.permutation(B)
            parent[t, g * B:(g + 1) * B] = g * B + p
    parent[0] = np.int32(0x7FFFFFF0)
    return parent


def make_case(G, B, D, n_step, n_tail, seed, ends=None, gamma=0.95, priority=0.0):
    """Permuting parents, every step valid, group g ending at depth ends[g] (default: seeded, some groups with nothing ended) in a
    seeded slot, DONE set at the ends."""
    rng = np.random.default_rng(seed)
    E = G * B
    rec, parent = _records(rng, D, E), _permuting_parents(rng, D, G, B)
    valid = np.ones((D, E), dtype=np.uint8)
    if ends is None:
        ends = [int(rng.integers(0, D)) if rng.random() > 0.2 else -1 for _ in range(G)]
    end_depth = np.asarray(ends, dtype=np.int32)
    end_env = (np.arange(G) * B + rng.integers(0, B, G)).astype(np.int32)
    for g in range(G):
        if 0 <= end_depth[g] < D:
            rec[end_depth[g], end_env[g], R.O_DONE] = 1.0
    tail = np.ascontiguousarray(rng.standard_normal((E, n_tail))) if n_tail else None
    return dict(B=B, n_step=n_step, gamma=gamma, priority=priority, rec=rec, valid=valid, parent=parent, end_env=end_env,
                end_depth=end_depth, tail=tail)


def random_case(G, B, D, n_step, n_tail, seed):
    """A seeded table: as make_case, then off-chain steps made invalid at random and about a sixth of the ended groups broken (an
    invalid step on the chain, or a parent outside the group)."""
    case = make_case(G, B, D, n_step, n_tail, seed, priority=float(seed % 3))
    rng = np.random.default_rng(seed + 7919)
    on_chain = np.zeros(case["valid"].shape, dtype=bool)
    chains = {}
    for g in range(G):
        envs, _ = chain(case, g)
        if envs is not None:
            chains[g] = envs
            on_chain[np.arange(len(envs)), envs] = True
    case["valid"][(rng.random(on_chain.shape) < 0.3) & ~on_chain] = 0
    for g, envs in chains.items():
        if rng.random() < 1 / 6:
            t = int(rng.integers(0, len(envs)))
            if t > 0 and rng.random() < 0.5:
                case["parent"][t, envs[t]] = (g * B - 1) if rng.random() < 0.5 else (g * B + B)
            else:
                case["valid"][t, envs[t]] = 0
    return case


def _set_bits(rng, rec, lin_finite):
    """Every column of every record a random 64-bit pattern, NaN payloads, infinities and -0.0 planted on top.  lin_finite: O_LIN
    holds finite doubles of moderate exponent instead -- where a return is SUMMED from it, the payload of a NaN result is the
    platform's and not the rule's."""
    bits = rng.integers(0, 2 ** 64, rec.shape, dtype=np.uint64)
    flat = bits.reshape(-1)
    plant = np.array([0x7FF8000000000001, 0xFFF8000000ABCDEF, 0x7FF0000000000000, 0x8000000000000000, 0x7FF4000000000123,
                      0x0000000000000001], dtype=np.uint64)
    where = rng.choice(flat.size, size=32 * len(plant), replace=False)
    flat[where] = np.tile(plant, 32)
    rec[...] = bits.view(np.float64)
    for col in (R.O_STABLE_S, R.O_TD, R.O_NB):                # the columns the rule replaces or that tell rows apart: bits as well
        rec[:, :, col] = rng.integers(0, 2 ** 64, rec.shape[:2], dtype=np.uint64).view(np.float64)
    rec[0, 0, R.O_STABLE_S] = np.uint64(0xFFF8000000000777).view(np.float64)
    rec[0, 0, R.O_LIN] = -0.0
    if lin_finite:
        rec[:, :, R.O_LIN] = np.ldexp(rng.uniform(-1, 1, rec.shape[:2]), rng.integers(-40, 40, rec.shape[:2]))
        rec[0, :, R.O_LIN] = -0.0


def probe_tables():
    """Name -> case.  Every probe the issue of the operator lists; every defective twin differs from the rule on at least one."""
    P = {}
    n = 3
    # L = 1, D, n_step, n_step + 1 and a group with nothing ended, through parents that permute the slots at every depth
    P["lengths"] = make_case(5, 4, 6, n, 5, seed=11, ends=[0, 5, n - 1, n, -1], priority=1.0)
    P["lengths_one_step"] = make_case(5, 4, 6, 1, 5, seed=12, ends=[0, 5, 2, 3, -1])
    P["nothing_ended_anywhere"] = make_case(3, 2, 4, n, 0, seed=13, ends=[-1, -1, -1])
    # a chain through an invalid step: at its end, in its middle, at depth 0; the groups beside it are intact
    c = make_case(5, 4, 6, n, 5, seed=14, ends=[4, 4, 4, 4, 2])
    for g, t in ((0, 4), (1, 2), (2, 0)):
        envs, _ = chain(c, g)
        c["valid"][t, envs[t]] = 0
    P["invalid_step"] = c
    # a parent outside its group: below gB, at gB + B, far outside on both sides; an end_env outside the group
    c = make_case(6, 4, 6, n, 5, seed=15, ends=[3, 3, 3, 3, 3, 3])
    for g, p in ((1, 1 * 4 - 1), (2, 2 * 4 + 4), (3, -5), (4, 2 ** 31 - 1)):
        envs, _ = chain(c, g)
        c["parent"][2, envs[2]] = p
    c["end_env"][5] = 5 * 4 + 4
    P["parent_outside"] = c
    c = make_case(3, 4, 6, n, 5, seed=16, ends=[2, 2, 2])
    c["end_env"][:] = [-1, 4 * 1 - 1, 2 ** 31 - 1]
    P["end_env_outside"] = c
    # end_depth >= D, and far beyond
    P["end_depth_beyond"] = make_case(4, 2, 5, n, 2, seed=17, ends=[5, 4, 2 ** 31 - 1, 0])
    # the copy is of bits
    c = make_case(3, 4, 6, 1, 4, seed=18, ends=[5, 3, 0])
    _set_bits(np.random.default_rng(181), c["rec"], lin_finite=False)
    c["tail"][...] = np.random.default_rng(182).integers(0, 2 ** 64, c["tail"].shape, dtype=np.uint64).view(np.float64)
    P["bits_one_step"] = c
    c = make_case(3, 4, 6, n, 4, seed=19, ends=[5, 3, 0], priority=-0.0)
    _set_bits(np.random.default_rng(191), c["rec"], lin_finite=True)
    P["bits_three_step"] = c
    # the widest and the narrowest the operator admits
    P["widest"] = make_case(2, 16, 16, 8, 9, seed=20, ends=[15, 8])
    P["single_beam"] = make_case(3, 1, 1, 1, 0, seed=21, ends=[0, -1, 0])
    return P
