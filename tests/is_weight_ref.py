"""Reference of the importance-sampling weights of prioritised replay (not a test module): the weights of a draw
(bridges_priority_weights) in numpy float64 in the DEFINING form, the cancelled form the kernel implements, the acceptance bound,
the weighted form of the SuccessorMLP loss reference (bridges_successor_loss_weighted) and three defective twins the bounds must
reject.  tests/test_cpu_is_weights.py checks all of it without a GPU; tests/test_gpu_is_weights.py holds the kernels to it.

The weights.  Row i of the N live rows is drawn with probability P(i) = m_i / total (m = priority_ref.masses).  Its weight is
(N P(i))^(-beta); every batch of B consecutive draws is one optimiser step and is divided by its own maximum, so the largest
weight of a batch is exactly 1 (the weighted step is never larger than the unweighted one).  N and total cancel in the quotient:
w_j = (min_k m_idx[k] / m_idx[j])^beta, k over the batch of j.  A draw whose index lies outside [0, N) has weight 0 and takes no
part in the maximum.
The bound.  |w - ref| <= 2^-23 ref: the kernel computes the cancelled form in float64 -- a quotient and a pow, a few ulps of
2^-53 -- and rounds to float32 once (2^-24 relative); 2^-23 leaves a factor of two over that one rounding and nothing else."""
import numpy as np
import torch

import mlp_conformance as M
from gpu_helpers import U32
from priority_ref import masses, probe  # noqa: F401  (re-exported: the cases of the weights are the sampler's probe)

W_TOL = 2.0 ** -23
W_N = (1, 2, 257, 4099)
W_ALPHA = (1.0, 0.6, 0.0)
W_BETA = (0.0, 0.4, 1.0)
W_BATCHES = ((1, 3), (32, 1), (32, 3), (33, 2), (300, 2))        # (B, n_steps): one thread, a wave's worth, a wave plus one, > 256
W_CASES = [(N, a, b, B, n) for N in W_N for a in W_ALPHA for b in W_BETA for B, n in W_BATCHES]


def _per_batch(m, idx, batch, raw_of):
    """raw_of(masses of the valid draws of one batch) -> their unnormalised weights; the batch is divided by its maximum."""
    m, idx = np.asarray(m, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    assert idx.size % batch == 0
    w = np.zeros(idx.size, dtype=np.float64)
    valid = (idx >= 0) & (idx < m.size)
    for lo in range(0, idx.size, batch):
        sel = np.nonzero(valid[lo:lo + batch])[0] + lo
        if sel.size:
            raw = raw_of(m[idx[sel]])
            w[sel] = raw / raw.max()
    return w


def weights_ref(m, idx, batch, beta):
    """The defining form: (N m / total)^(-beta), each batch divided by its maximum.  m [N] masses, idx [n] -> float64 [n]."""
    m = np.asarray(m, dtype=np.float64)
    N, total = m.size, m.sum()
    return _per_batch(m, idx, batch, lambda mb: np.power(N * mb / total, -beta))


def weights_cancelled(m, idx, batch, beta):
    """The form the kernel implements: pow(min of the batch / m, beta); beta == 0 and beta == 1 without pow."""
    def raw(mb):
        r = mb.min() / mb
        return np.ones_like(r) if beta == 0.0 else (r if beta == 1.0 else np.power(r, beta))
    return _per_batch(m, idx, batch, raw)


def accept_weights(w, ref):
    """None when ``w`` (float32 or float64 values) lies within W_TOL * ref of ``ref`` everywhere, else a sentence."""
    w, ref = np.asarray(w, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if w.shape != ref.shape:
        return f"{w.shape} weights for {ref.shape} draws"
    bad = np.nonzero(~(np.abs(w - ref) <= W_TOL * ref))[0]           # (a NaN is outside)
    if bad.size:
        j = int(bad[0])
        return f"draw {j}: weight {w[j]!r} against {ref[j]!r} ({bad.size} of {w.size} draws outside the bound)"
    return None


def reference_draws(N, alpha, n_draws, seed=0):
    """Host-side stand-in for the sampler's idx: the plain float64 cumsum + searchsorted statement on the probe's uniforms."""
    td, _ = probe(N, n_draws)
    m = masses(td, alpha)
    u = np.random.default_rng(77 * N + n_draws + seed).random(n_draws)
    cdf = np.cumsum(m)
    return m, np.minimum(np.searchsorted(cdf, u * cdf[-1], side="right"), N - 1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ twins of the weights
def twin_normalised_over_the_call(m, idx, batch, beta):
    """One maximum for the whole call instead of one per batch."""
    return weights_ref(m, idx, np.asarray(idx).size, beta)


def twin_beta_sign(m, idx, batch, beta):
    """beta applied as +beta: the rows drawn too often are weighed UP."""
    m = np.asarray(m, dtype=np.float64)
    N, total = m.size, m.sum()
    return _per_batch(m, idx, batch, lambda mb: np.power(N * mb / total, beta))


WEIGHT_TWINS = {"normalised_over_the_call": twin_normalised_over_the_call, "beta_sign": twin_beta_sign}


# ------------------------------------------------------------------------------------------------------------ the weighted loss
LOSS_ROWS = [M.LOSS_SHAPES[i] for i in (1, 2, 3, 0, 4, 5)]
LOSS_COUNTERS = (0, 2)


def loss_weights(batch, device, seed=0):
    """w [LOSS_BATCHES * batch] float32 in (0, 1]; in every batch c one row exactly 1 and (batch > 1) one row exactly 0; with
    batch == 1 the three batches hold 1, a draw and 0."""
    g = torch.Generator().manual_seed(4001 + 17 * batch + seed)
    w = 1.0 - torch.rand(M.LOSS_BATCHES * batch, generator=g) * 0.96875          # (0.03125, 1]
    for c in range(M.LOSS_BATCHES):
        if batch > 1:
            w[c * batch + c % batch], w[c * batch + (c + 1) % batch] = 1.0, 0.0
        else:
            w[c] = (1.0, float(w[c]), 0.0)[c]
    return w.float().to(device)


def _rows_weight(w, batch, rows, device):
    out = torch.zeros(rows, dtype=torch.float64, device=device)
    out[:batch] = w.double()
    return out


def weighted_loss_ref(w, y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf):
    """mlp_conformance.loss_ref with row b's loss share and gradient multiplied by w_b [batch] -- reference AND bound -- plus
    2 u |value| for the at most two further float32 roundings (the weight times a coefficient, and what that rounding is carried
    through); q is the unweighted q.  -> {q, loss_rows, dy: (reference, bound)}."""
    refs = M.loss_ref(y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf)
    wr = _rows_weight(w, batch, M.rows_of(batch), y.device)
    out = dict(q=refs["q"])
    for k, ww in (("loss_rows", wr), ("dy", wr[:, None])):
        ref, bound = refs[k]
        out[k] = (ref * ww, bound * ww + 2 * U32 * (ref * ww).abs())
    return out


def weighted_loss_lib(w, y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf):
    """The torch formulation under autograd in the dtype of y, the per-row terms times w -> {q, loss_rows, dy}, padded."""
    rows = M.rows_of(batch)
    yy = y[:batch].detach().clone().requires_grad_(True)
    psi = yy[:, :2 * px].reshape(batch, 2, px)
    q = (psi.softmax(dim=1)[:, 1] * rw).sum(-1)
    per_row = torch.zeros_like(q)
    if use_q:
        per_row = per_row + w * (q - q_t) ** 2 / batch
    if use_sf:
        per_row = per_row + w * ((psi[:, 0] - sf_t) ** 2).sum(-1) / (batch * px)
    (dy,) = torch.autograd.grad(per_row.sum(), yy)
    pad = lambda v: torch.cat([v.detach(), torch.zeros((rows - batch, *v.shape[1:]), dtype=v.dtype, device=v.device)])
    return dict(q=pad(q), loss_rows=pad(per_row), dy=pad(dy))


def twin_loss_sf_gradient_unweighted(w, y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf):
    """The q-gradient weighted, the successor-feature gradient not (the weight applied to dq and forgotten on csf), float32."""
    rows = M.rows_of(batch)
    wr = _rows_weight(w, batch, rows, y.device)
    q_part = M.loss_ref(y, rw, q_t, sf_t, batch, px, nf, use_q, False)
    sf_part = M.loss_ref(y, rw, q_t, sf_t, batch, px, nf, False, use_sf)
    right = weighted_loss_ref(w, y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf)
    return dict(q=right["q"][0].float(), loss_rows=right["loss_rows"][0].float(),
                dy=(q_part["dy"][0] * wr[:, None] + sf_part["dy"][0]).float())


def inside(name, got, ref, bound, shape=None):
    """|got - ref| <= bound at every element (exactly equal where the bound is zero); raises AssertionError, returns the largest
    err / bound over the elements with a bound."""
    assert got.shape == ref.shape and got.dtype == torch.float32, (name, shape, tuple(got.shape), tuple(ref.shape), got.dtype)
    ref, bound = ref.double(), bound.double()
    err = (got.double() - ref).abs()
    ok = err <= bound                                                              # NaN is outside
    assert bool(ok.all()), f"{name} {shape}: {int((~ok).sum())} elements outside the bound, worst excess {float(torch.nan_to_num(err - bound, nan=float('inf')).max()):.3e}"
    live = bound > 0
    q = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"Q {name} {shape} q={q:.3e}")
    return q
