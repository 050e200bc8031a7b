"""Reference of prioritised replay on the device (not a test module): the masses, the exact CDF, the acceptance rule of the
sampler (bridges_priority_sample) and the reference of the refresh (bridges_priority_update), in numpy, with the defective
twins the rule must reject.  tests/test_cpu_priority_replay.py checks all of it without a GPU; tests/test_gpu_priority_replay.py
holds the kernels to it.

The rule.  A draw u_j names the first row k whose inclusive prefix sum exceeds u_j * total (searchsorted(right=True), clamped to
the last row).  The device sums in an order of its own, so where u_j * total lies within TOL * total of a prefix sum the row
before or after is as good: for each draw the reference returns its own index and the index range [lo, hi] that
u_j * total -/+ TOL * total allows.  lo == hi: the draw is DECIDED and the device must return exactly that row.  Otherwise
anything in [lo, hi] passes, and at most CAP of a case's draws may be undecided (the probe's cases leave none).
TOL = 1e-9: at most 2^20 terms, each addition off by at most 2^-52 of the running sum, times a small constant for the summation
order and the ulps of pow -- about 2.3e-10, rounded up.
Exact cases.  Where every mass is an integer (alpha = 0: all ones) every partial sum below 2^53 is exact in ANY order, so no
tolerance is due: sample_ref(..., tol=0.0) decides every draw, ties included."""
import functools
import math

import numpy as np

TOL = 1e-9
CAP = 0.01
FLOOR = 1e-5
CEIL = 1e30
CHUNK = 256                                          # rows per chunk of the device's two-level search (csrc/replay_kernels.hip)

PROBE_N = (1, 2, 255, 256, 257, 1023, 1025, 4099, 65539)
PROBE_ALPHA = (1.0, 0.6, 0.0)
PROBE_DRAWS = (1, 63, 64, 65, 800)
PROBE_CASES = [(N, a, n) for N in PROBE_N for a in PROBE_ALPHA for n in PROBE_DRAWS]


def probe(N, n):
    """(td [N], u [n]) float64: exponential(1) priorities by default_rng(1000 N + n), 20 % of the rows 0; for N > 3 row N // 3 =
    1e6 (an outlier that holds nearly all of the mass at alpha = 1), row N // 2 = NaN, row N - 1 = -1;
    u = default_rng(1000 N + n + 1).random(n)."""
    seed = 1000 * N + n
    rng = np.random.default_rng(seed)
    td = rng.exponential(1.0, N)
    td[rng.random(N) < 0.2] = 0.0
    if N > 3:
        td[N // 3], td[N // 2], td[N - 1] = 1e6, np.nan, -1.0
    return td, np.random.default_rng(seed + 1).random(n)


def masses(td, alpha):
    """m_i = pow(fmin(fmax(td_i, 0), 1e30) + 1e-5, alpha) in float64; alpha == 1 without pow, alpha == 0 all ones.  fmax / fmin
    return the operand that is not NaN: a NaN or negative priority falls to the floor."""
    x = np.fmin(np.fmax(np.asarray(td, dtype=np.float64), 0.0), CEIL) + FLOOR
    if alpha == 1.0:
        return x
    if alpha == 0.0:
        return np.ones_like(x)
    return np.power(x, alpha)


def exact_cdf(m):
    """Correctly rounded inclusive prefix sums as longdouble: math.fsum of every prefix up to 1025 rows, a longdouble running sum
    above (64-bit significand: 65539 additions stay within 4e-15 of the total, far inside TOL)."""
    if len(m) <= 1025:
        return np.array([math.fsum(m[:k + 1]) for k in range(len(m))], dtype=np.longdouble)
    return np.cumsum(m.astype(np.longdouble))


def _search(cdf, t):
    return np.minimum(np.searchsorted(cdf, t, side="right"), len(cdf) - 1).astype(np.int64)


def sample_ref(td, alpha, u, tol=TOL):
    """-> (idx, lo, hi) int64 [n] each: the reference's row of every draw and the rows the tolerance allows."""
    cdf = exact_cdf(masses(td, alpha))
    total = cdf[-1]
    t = np.asarray(u, dtype=np.longdouble) * total
    return _search(cdf, t), _search(cdf, t - tol * total), _search(cdf, t + tol * total)


@functools.lru_cache(maxsize=None)
def probe_ref(N, alpha, n):
    """sample_ref of the probe case (N, alpha, n), computed once per process and shared (read-only arrays)."""
    td, u = probe(N, n)
    ref = sample_ref(td, alpha, u)
    for a in ref:
        a.setflags(write=False)
    return ref


def undecided(ref):
    return int((ref[1] != ref[2]).sum())


def accept(idx, ref, cap=CAP):
    """The acceptance rule: None when ``idx`` passes, else a sentence.  cap=None: neighbours allowed, no cap (the boundary case)."""
    idx = np.asarray(idx, dtype=np.int64)
    _own, lo, hi = ref
    if idx.shape != lo.shape:
        return f"{idx.shape} indices for {lo.shape} draws"
    bad = np.nonzero((idx < lo) | (idx > hi))[0]
    if bad.size:
        j = int(bad[0])
        return f"draw {j}: row {int(idx[j])} outside [{int(lo[j])}, {int(hi[j])}] ({bad.size} of {idx.size} draws)"
    if cap is not None and undecided(ref) > cap * idx.size:
        return f"{undecided(ref)} of {idx.size} draws undecided: above the cap of {cap:.0%}"
    return None


# ------------------------------------------------------------------------------------------------------------ defective twins
def _twin(mass_fn=masses, side="right", drop_last_chunk=False):
    def run(td, alpha, u):
        m = mass_fn(td, alpha)
        if drop_last_chunk and len(m) > CHUNK:
            m = m.copy()
            m[(len(m) - 1) // CHUNK * CHUNK:] = 0.0          # the rows of the last chunk never reach the sums
        with np.errstate(invalid="ignore"):
            cdf = np.cumsum(m)
            t = np.asarray(u) * cdf[-1]
            return np.minimum(np.searchsorted(cdf, t, side=side), len(m) - 1).astype(np.int64)
    return run


def _mass_nan(td, alpha):
    x = np.minimum(np.maximum(np.asarray(td, dtype=np.float64), 0.0), CEIL) + FLOOR         # np.maximum passes the NaN on
    return x if alpha == 1.0 else (np.ones_like(x) if alpha == 0.0 else np.power(x, alpha))


def _mass_no_floor(td, alpha):
    x = np.fmin(np.fmax(np.asarray(td, dtype=np.float64), 0.0), CEIL)
    return x if alpha == 1.0 else (np.ones_like(x) if alpha == 0.0 else np.power(x, alpha))


TWINS = {
    "side_left": _twin(side="left"),
    "nan_not_clamped": _twin(mass_fn=_mass_nan),
    "mass_without_floor": _twin(mass_fn=_mass_no_floor),
    "alpha_ignored": _twin(mass_fn=lambda td, alpha: masses(td, 1.0)),
    "last_chunk_dropped": _twin(drop_last_chunk=True),
}
sample_plain = _twin()                               # the float64 cumsum statement: the torch path's formulation


def tie_probe(N=256):
    """An exact case: alpha = 0 over N rows (a power of two), u = k / N -- u * total = k is exactly the prefix sum of row k - 1, so
    the right-hand rule names row k and the left-hand rule row k - 1.  -> (td, u), to be judged with tol = 0."""
    td, _ = probe(N, 1)
    return td, np.arange(N, dtype=np.float64) / N


# ------------------------------------------------------------------------------------------------------------ the refresh
def update_ref(rec, col, idx, q_sa, q_target, n_rec=None):
    """rec with rec[idx_j, col] = float64(|float32(q_sa_j) - float32(q_target_j)|), j ascending: the last draw of a row wins; an
    index outside [0, n_rec) writes nothing; no other column or row changes."""
    out = np.array(rec, dtype=np.float64, copy=True)
    n_rec = out.shape[0] if n_rec is None else n_rec
    val = np.abs(np.asarray(q_sa, dtype=np.float32) - np.asarray(q_target, dtype=np.float32)).astype(np.float64)
    for j, i in enumerate(np.asarray(idx, dtype=np.int64)):
        if 0 <= i < n_rec:
            out[i, col] = val[j]
    return out


def twin_update_first_wins(rec, col, idx, q_sa, q_target, n_rec=None):
    idx = np.asarray(idx, dtype=np.int64)
    return update_ref(rec, col, idx[::-1], np.asarray(q_sa)[::-1], np.asarray(q_target)[::-1], n_rec)


UPDATE_N = (1, 64, 65, 800)


def update_probe(n, N=257, W=111, seed=0):
    """(rec [N, W], idx [n], q_sa [n], q_target [n]): random records; draws from a third of the rows, so that rows repeat with
    DIFFERENT q_sa once n > 1; for n >= 64 the indices -1, N, N + 5 and -2^40 among them (out of range: nothing written)."""
    rng = np.random.default_rng(7000 + 10 * n + seed)
    rec = rng.standard_normal((N, W))
    idx = rng.integers(0, max(N // 3, 1), n).astype(np.int64)
    if n >= 64:
        idx[[3, 17, 40, 63]] = (-1, N, N + 5, -2 ** 40)
        idx[n - 1] = idx[0]                                  # the first and the last draw name one row
    q_sa = rng.standard_normal(n).astype(np.float32)
    q_target = rng.standard_normal(n).astype(np.float32)
    return rec, idx, q_sa, q_target
