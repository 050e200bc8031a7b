"""References of the n-step returns of the vectorised DQN loop (VecDQN(n_step=n)): the per-env window that folds one-step
records into h-step records (bridges_nstep_fold), the discounted sum of block rasters (bridges_bits_discounted_sum) and the TD
target with a discount per transition (bridges_td_target_rows) -- numpy / float64 statements with their error bounds, scripted
probe data and deliberately defective twins.  Test infrastructure, not a test module: nothing here needs a GPU, so
tests/test_cpu_nstep.py checks the references against each other and against the twins, and tests/test_gpu_nstep.py applies the
same rules to the kernels.

Bounds are first-order in u = 2**-24 (float32) or 2**-53 (float64); the operations counted stand next to each use."""
import math

import numpy as np
import torch

from gpu_helpers import U32
from mlp_conformance import NO_ROW
from robotoddler.training import records as R

U64 = 2.0 ** -53
NSTEP_MAX = 8


# ---------------------------------------------------------------------------------------------------------------------------
# The window: per env a list of pending starts.  The rule of include/bridges_hip.h, with the return of every start kept as the
# list of the rewards it has seen, so that G is the DIRECT sum  sum_k gamma^k lin_k  (math.fsum: no rounding to speak of).

class RefWindow:
    def __init__(self, n_envs, n, gamma):
        assert 1 <= n <= NSTEP_MAX
        self.E, self.n, self.gamma = int(n_envs), int(n), float(gamma)
        self.pending = [[] for _ in range(self.E)]                   # per env: [(lins, stable_s, td, tag), ...], oldest first
        self.emitted = []                                            # (tag of the start, h) of every emitted row, in row order

    def fold(self, rec, valid, tags=None):
        """rec [E, W] float64, valid [E] -> (out [E * n, W + 1], out_valid [E * n] bool, g_bound [E * n]): env e's emissions in
        rows e * n ..., oldest first; the other rows are zero.  g_bound: 2 h * 2**-53 * sum_k |gamma^k lin_k| -- per term the h - 1
        or fewer roundings of the running discount, the product and the addition, fused or not (at most 2 h roundings).
        ``tags`` [E]: a name for the transition of every env (any object); self.emitted then lists (tag of the start, h) of the rows
        emitted so far, in the order in which the valid rows of successive calls follow each other."""
        rec, valid = np.asarray(rec, dtype=np.float64), np.asarray(valid).astype(bool)
        E, W, n = self.E, rec.shape[1], self.n
        assert rec.shape[0] == E and W >= R.RECORD_WIDTH
        out = np.zeros((E * n, W + 1))
        out_valid = np.zeros(E * n, dtype=bool)
        g_bound = np.zeros(E * n)
        for e in range(E):
            if not valid[e]:
                continue
            win = self.pending[e]
            win.append(([], rec[e, R.O_STABLE_S], rec[e, R.O_TD], None if tags is None else tags[e]))
            for lins, _, _, _ in win:
                lins.append(rec[e, R.O_LIN])
            done = rec[e, R.O_DONE] > 0.5
            emit = list(win) if done else ([win[0]] if len(win) == n else [])
            for r, (lins, stable_s, td, tag) in enumerate(emit):
                h = len(lins)
                terms = [self.gamma ** k * l for k, l in enumerate(lins)]
                row = rec[e].copy()
                row[R.O_LIN], row[R.O_STABLE_S], row[R.O_TD] = math.fsum(terms), stable_s, td
                out[e * n + r, :W], out[e * n + r, W] = row, h
                out_valid[e * n + r] = True
                g_bound[e * n + r] = 2 * h * U64 * math.fsum(abs(t) for t in terms)
                self.emitted.append((tag, h))
            if done:
                win.clear()
            elif emit:
                del win[0]
        return out, out_valid, g_bound


def check_fold(got_out, got_valid, ref_out, ref_valid, g_bound, name=""):
    """out_valid exact; of the emitted rows G within its bound and every other column, h included, bit for bit."""
    got_out, got_valid = np.asarray(got_out), np.asarray(got_valid).astype(bool)
    assert got_valid.shape == ref_valid.shape and np.array_equal(got_valid, ref_valid), f"{name}: out_valid differs"
    rows = np.nonzero(ref_valid)[0]
    other = np.ones(ref_out.shape[1], dtype=bool)
    other[R.O_LIN] = False
    g, r = got_out[rows], ref_out[rows]
    assert np.array_equal(g[:, other].view(np.int64), r[:, other].view(np.int64)), f"{name}: a copied column differs"
    err = np.abs(g[:, R.O_LIN] - r[:, R.O_LIN])
    assert np.all(err <= g_bound[rows]), f"{name}: G outside its bound, worst excess {float((err - g_bound[rows]).max()):.3e}"


def episode_script(n, env):
    """(valid, done) per lock-step of env ``env`` for a window of n: an episode that ends on its first step, an invalid
    (reset-only) lock-step, an episode of exactly n steps (the done arrives on a full window), back to back one of n + 2 steps
    (longer than n), an invalid lock-step, an episode of 2 steps, back to back one of 1 step; env % 3 invalid lock-steps lead, and a
    running episode fills up to the common length 2 n + 11."""
    steps = [(False, False)] * (env % 3)
    for length, gap in ((1, True), (n, False), (n + 2, True), (2, False), (1, False)):
        steps += [(True, False)] * (length - 1) + [(True, True)]
        if gap:
            steps.append((False, False))
    T = script_length(n)
    return (steps + [(True, False)] * T)[:T]


def script_length(n):
    return 2 * n + 11


def scripted_records(n_envs, n, W, seed=0):
    """The lock-steps of episode_script as synthetic records: [(rec [E, W] float64, valid [E] bool), ...].  Every column is a random
    double (the fold copies bits); O_NB counts the steps of the episode, O_DONE is the script's, O_STABLE_S is 0 / 1 and O_TD > 0.
    An invalid lock-step carries a row of noise with O_DONE set, which the fold must ignore."""
    rng = np.random.default_rng(1000 * seed + 17 * n + W)
    scripts = [episode_script(n, e) for e in range(n_envs)]
    nb = np.zeros(n_envs)
    out = []
    for t in range(script_length(n)):
        rec = rng.standard_normal((n_envs, W))
        valid = np.array([scripts[e][t][0] for e in range(n_envs)])
        done = np.array([scripts[e][t][1] for e in range(n_envs)])
        rec[:, R.O_NB] = nb
        rec[:, R.O_DONE] = np.where(valid, done, True).astype(np.float64)
        rec[:, R.O_STABLE_S] = rng.integers(0, 2, n_envs)
        rec[:, R.O_STABLE_N] = rng.integers(0, 2, n_envs)
        rec[:, R.O_TD] = np.abs(rec[:, R.O_TD])
        nb = np.where(valid, np.where(done, 0, nb + 1), nb)
        out.append((rec, valid))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The discounted raster sum: sum[i] = sum_{k < h_i} d_k image(bits[first_i + k]), disc[i] = d_{h_i}, d_k = gamma^k.

def images(bits):
    """[R, 64] uint64 / int64 -> [R, 64, 64] float64 {0, 1}: pixel (y, x) = bit x of word y (k_bits_to_f32's order)."""
    b = np.asarray(bits).astype(np.int64).view(np.uint64)
    return ((b[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(np.float64)


def raster_probe(seed=0, B=5, K=16):
    """B transitions of K block rasters each -> (bits [B * K, 64] int64, cases): sparse random blocks, among them an empty raster
    (block 1 of every transition), a block with only bit 0 of one word and one with only bit 63 of one word (blocks 0 and 2 of
    transition 0, blocks K - 2 and K - 1 of the last); ``cases`` = for every h in (1, 2, 3, 8) a (first, h) pair of arrays: starts at
    block 0, in the middle, and with first + h = the LAST row of the table for the last transition."""
    rng = np.random.default_rng(seed)
    bits = np.zeros((B * K, 64), dtype=np.uint64)
    for r in range(B * K):
        y0, x0 = rng.integers(0, 56), rng.integers(0, 56)
        for y in range(y0, y0 + rng.integers(1, 8)):
            bits[r, y] = np.uint64(((1 << int(rng.integers(1, 8))) - 1) << int(x0))
    bits[1::K] = 0
    for r, (word, bit) in ((0, (5, 0)), (2, (40, 63)), (B * K - 2, (63, 63)), (B * K - 1, (0, 0))):
        bits[r] = 0
        bits[r, word] = np.uint64(1) << np.uint64(bit)
    cases = []
    for h in (1, 2, 3, 8):
        first = np.array([i * K + (0, 1, 5, K - h, K - h)[i % 5] for i in range(B)], dtype=np.int64)
        first[0] = 0
        cases.append((first, np.full(B, h, dtype=np.int32)))
    mixed = np.array([1, 2, 3, 8, 8][:B], dtype=np.int32)
    cases.append((np.array([i * K for i in range(B - 1)] + [B * K - 8], dtype=np.int64)[:B], mixed))
    return bits.view(np.int64), cases


def raster_sum_ref(bits, first, h, gamma):
    """float64 -> dict(sum, sum_bound [B, 64, 64], disc, disc_bound [B]).  gamma is taken as the float32 the kernel is handed.
    Bounds: d_k carries k roundings (k products), and bringing term k into the sum costs one more: (k + 1) u d_k per set pixel of
    block k, summed over the blocks that cover the pixel; a pixel no block covers is exactly zero, and h = 1 is exact (d_0 = 1 and
    nothing is added to it).  disc = d_h: h u d_h."""
    g = float(np.float32(gamma))
    img = images(bits)
    B = len(first)
    s, sb = np.zeros((B, 64, 64)), np.zeros((B, 64, 64))
    disc, db = np.zeros(B), np.zeros(B)
    for i in range(B):
        for k in range(int(h[i])):
            s[i] += g ** k * img[first[i] + k]
            sb[i] += (k + 1) * U32 * g ** k * img[first[i] + k]
        if h[i] == 1:
            sb[i] = 0.0
        disc[i], db[i] = g ** int(h[i]), int(h[i]) * U32 * g ** int(h[i])
    return dict(sum=s, sum_bound=sb, disc=disc, disc_bound=db)


def raster_sum_plain(bits, first, h, gamma, twin=None):
    """A plain float32 evaluation, terms added in ascending k -> (sum [B, 64, 64] float32, disc [B] float32).  ``twin``: one of
    'disc_h_minus_1' (the bootstrap discounted by gamma^(h-1)), 'h_plus_1_blocks' (one block too many in the sum) and
    'undiscounted' (the plain sum of the rasters)."""
    g = np.float32(gamma)
    img = images(bits).astype(np.float32)
    B = len(first)
    s, disc = np.zeros((B, 64, 64), dtype=np.float32), np.zeros(B, dtype=np.float32)
    for i in range(B):
        d, hi = np.float32(1.0), int(h[i])
        blocks = hi + 1 if twin == "h_plus_1_blocks" else hi
        for k in range(blocks):
            row = min(first[i] + k, img.shape[0] - 1)
            s[i] = s[i] + (np.float32(1.0) if twin == "undiscounted" else d) * img[row]
            if k == hi - 1 and twin == "disc_h_minus_1":
                disc[i] = d
            d = np.float32(d * g)
            if k == hi - 1 and twin != "disc_h_minus_1":
                disc[i] = d
    return s, disc


RASTER_TWINS = ("disc_h_minus_1", "h_plus_1_blocks", "undiscounted")


def check_raster_sum(got_sum, got_disc, ref, name=""):
    got_sum, got_disc = np.asarray(got_sum, dtype=np.float64), np.asarray(got_disc, dtype=np.float64)
    err = np.abs(got_sum - ref["sum"])
    assert np.all(err <= ref["sum_bound"]), f"{name}: raster sum outside its bound, worst excess {float((err - ref['sum_bound']).max()):.3e}"
    err = np.abs(got_disc - ref["disc"])
    assert np.all(err <= ref["disc_bound"]), f"{name}: disc outside its bound, worst excess {float((err - ref['disc_bound']).max()):.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# The TD target with a discount per transition, on the probe of mlp_conformance.td_probe.

def td_rows_ref(pr, discount):
    """float64 -> {q, sf: (reference, bound)}, rows.  td_ref's statement with discount[i] in place of gamma: the first maximum of
    the segment; q = lin + d * (done ? 0 : q'), sf = action raster + d * (done ? 0 : psi'); an empty segment: row NO_ROW,
    q = lin + d * (done ? 0 : -inf), sf = the action raster.  Bound: td_ref's 2 u (|a| + |d s|) -- the product and the sum, rounded
    separately or fused -- zero where done."""
    nq = pr["next_q"].double().cpu()
    lin, disc = pr["lin"].double().cpu(), discount.double().cpu()
    B = len(pr["lo"])
    q, e_q, rows = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), []
    D = pr["sf_dim"]
    sf = e_sf = None
    if D:
        act = pr["act"].double().cpu().reshape(B, -1)
        sf, e_sf = act.clone(), torch.zeros(B, D, dtype=torch.float64)
    for i, (lo, hi) in enumerate(zip(pr["lo"], pr["hi"])):
        row = lo + int(nq[lo:hi].argmax()) if hi > lo else NO_ROW            # torch.argmax: the first maximum
        rows.append(row)
        if pr["done"][i]:
            q[i] = lin[i]
            continue
        nxt = nq[row] if hi > lo else torch.tensor(-math.inf, dtype=torch.float64)
        q[i] = lin[i] + disc[i] * nxt
        e_q[i] = 2 * U32 * (abs(float(lin[i])) + abs(float(disc[i] * nxt)))
        if D and hi > lo:
            s = pr["next_sf"][row].double().cpu().reshape(-1)
            sf[i] = act[i] + disc[i] * s
            e_sf[i] = 2 * U32 * (act[i].abs() + (disc[i] * s).abs())
    e_q = torch.nan_to_num(e_q, nan=0.0, posinf=0.0)                          # an infinite target is met exactly
    return dict(q=(q, e_q), sf=(sf, e_sf) if D else None), rows


def td_rows_plain(pr, discount, twin=None):
    """The operator in plain float32 torch -> (q [B], sf [B, D] or None, rows).  twin 'scalar_gamma': every row discounted by
    discount[0] (the scalar operator handed the first row's discount)."""
    nq, B = pr["next_q"], len(pr["lo"])
    d = discount.float().to(nq.device)
    if twin == "scalar_gamma":
        d = d[:1].expand(B)
    q, sf, rows = [], [], []
    for i, (lo, hi) in enumerate(zip(pr["lo"], pr["hi"])):
        rows.append(lo + int(nq[lo:hi].argmax()) if hi > lo else NO_ROW)
        live = not pr["done"][i] and hi > lo
        nxt = nq[rows[-1]] if live else torch.zeros((), device=nq.device)
        if hi == lo and not pr["done"][i]:
            nxt = torch.full((), -math.inf, device=nq.device)
        q.append(pr["lin"][i] + d[i] * nxt)
        if pr["sf_dim"]:
            a = pr["act"][i].reshape(-1)
            sf.append(a + d[i] * pr["next_sf"][rows[-1]].reshape(-1) if live else a.clone())
    return torch.stack(q), (torch.stack(sf) if pr["sf_dim"] else None), rows


def check_td_rows(got, ref, ref_rows, name=""):
    """got = (q, sf, rows): the rows exact, q and sf within the bounds (an infinite target met exactly)."""
    assert [int(r) for r in got[2]] == [int(r) for r in ref_rows], f"{name}: arg-max rows {list(got[2])} != {ref_rows}"
    for key, g in (("q", got[0]), ("sf", got[1])):
        if ref[key] is None:
            continue
        want, bound = ref[key]
        g = g.double().cpu().reshape(want.shape)
        err = torch.where(g == want, torch.zeros_like(want), (g - want).abs())
        assert bool((err <= bound).all()), f"{name}.{key}: outside the bound, worst excess {float(torch.nan_to_num(err - bound, nan=math.inf).max()):.3e}"


def row_discounts(B, gamma, seed=0):
    """float32 [B]: per-row discounts drawn from {gamma^1 .. gamma^8} as the raster-sum kernel forms them (running float32
    products)."""
    rng = np.random.default_rng(seed)
    pows, d = [], np.float32(1.0)
    for _ in range(NSTEP_MAX):
        d = np.float32(d * np.float32(gamma))
        pows.append(d)
    return torch.tensor(np.array(pows, dtype=np.float32)[rng.integers(0, NSTEP_MAX, B)])
