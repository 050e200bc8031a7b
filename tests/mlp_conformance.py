"""Conformance of the SuccessorMLP step kernels (csrc/mlp_kernels.hip, the middle-layer stack included) and the scalar-ish DQN
kernels (csrc/dqn_kernels.hip):
shape tables, probe data, float64 references with their error bounds, the acceptance rule and deliberately defective twins.
Test infrastructure, not a test module: nothing here needs a GPU -- every function takes the device -- so
tests/test_cpu_mlp_conformance_refs.py checks on the CPU that the references accept a clean float32 evaluation and reject every
twin, and tests/test_gpu_mlp_conformance.py applies the same rule to the kernels.

Bounds are first-order forward-error bounds in u = 2**-24 (gpu_helpers.dot_bound for sums); the term count or the operations
counted stand next to each use.  They admit ANY plain float32 evaluation of the operator (the kernels' and the library's), not
one summation order."""
import math

import torch
import torch.nn.functional as F

from gpu_helpers import U32, dot_bound

FACTOR = 4.0            # q_kernel <= FACTOR * q_library, the project's figure (tests/test_gpu_conv_conformance.py)
# (name, shape) -> factor for rows whose correct kernel measures above FACTOR; each entry needs its measured pair and its reason in
# docs/MEASUREMENT_LOG.md ("Conformance of the MLP and DQN kernels").
ROW_FACTOR = {}
NO_ROW = 0x7fffffff     # argmax_row of an empty segment


def conform(name, got, lib, ref, bound, shape=None, tight=True):
    """|got - ref| <= bound at EVERY element, exactly equal where the bound is zero, q_kernel <= factor * q_library
    (q = max err / bound over the elements with a bound).  Raises AssertionError; returns (q_kernel, q_library).
    ``tight=False`` leaves the comparison of the two q out: for the rows of an ELEMENTWISE operator that hold a handful of
    elements, where either q is the largest of a few draws; the caller then judges q over its rows pooled (``conform_pooled``)."""
    assert got.shape == ref.shape and got.dtype == torch.float32, (name, shape, tuple(got.shape), tuple(ref.shape), got.dtype)
    ref, bound = ref.double(), bound.double()
    err, err_lib = (got.double() - ref).abs(), (lib.double() - ref).abs()
    err = torch.where(got.double() == ref, torch.zeros_like(err), err)            # inf == inf is no error
    err_lib = torch.where(lib.double() == ref, torch.zeros_like(err_lib), err_lib)
    inside = err <= bound                                                          # NaN is outside
    worst = float(torch.nan_to_num(err - bound, nan=math.inf).max()) if err.numel() else 0.0
    assert bool(inside.all()), f"{name} {shape}: {int((~inside).sum())} elements outside the bound, worst excess {worst:.3e}"
    live = bound > 0
    q_k = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    q_l = float((err_lib[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"Q {name} {shape} q_kernel={q_k:.3e} q_library={q_l:.3e}")
    factor = ROW_FACTOR.get((name, shape), FACTOR)
    assert not tight or q_k <= factor * q_l, f"{name} {shape}: q_kernel {q_k:.4f} > {factor} x q_library {q_l:.4f}"
    return q_k, q_l


def conform_pooled(name, parts, shape=None):
    """conform over the concatenation of ``parts`` = [(got, lib, ref, bound), ...], each flattened."""
    return conform(name, *[torch.cat([p[i].reshape(-1).to(p[2].dtype if i >= 2 else p[0].dtype) for p in parts]) for i in range(4)], shape)


def ceil_div(a, b):
    return -(-a // b)


def rows_of(batch):
    return 32 * ceil_div(batch, 32)


# ---------------------------------------------------------------------------------------------------------------------------
# Linear layers: k_lin_fwd / k_lin_fwd_finish, k_lin_bwd<false> / k_lin_dx_finish

LIN_SHAPES = [                 # (rows, K, N)
    (32, 1, 40),               # K = 1: one value in the `k0 < wend` tail, waves 1..3 with an empty K range
    (32, 3, 33),               # K % 8 = 3; N = 33: a second column tile with one live column
    (32, 7, 1),                # K % 8 = 7 (the longest tail); N = 1: every lane reads row 0 of W
    (32, 8, 31),               # K = 8: one 8-wide step and no tail in wave 0, nothing in waves 1..3; N = 31: one dead column
    (32, 9, 32),               # K % 8 = 1 behind a full 8-wide step; N = 32: exactly one tile
    (32, 31, 33),              # K = 31: one k tile short by one; waves 0..2 full 8-steps, wave 3 the tail of 7
    (32, 33, 1),               # K = 33: two k tiles, the second with one live column; waves of 16 values, wave 2 holds one
    (32, 65, 31),              # K = 65: the 64-wide loop cannot run (24 values per wave), wave 2 ends in a tail of one
    (32, 10, 2), (32, 12, 7), (32, 21, 40),        # K % 8 = 2, 4 and 5: with 70 (6) and the rows above, every remainder
    (64, 70, 33),              # two batch tiles at sizes below every split
    (32, 1030, 40),            # forward split-K: 17 splits of 64, the last with 6 values; one batch tile
    (64, 1030, 40),            # forward split-K with two batch tiles; no backward split (N <= 512)
    (32, 70, 1100),            # input gradient nsplit = 18 > 1, one batch tile
    (64, 200, 1100),           # nsplit > 1 with two batch tiles; rows != 32 weight gradient beside a split
    (96, 33, 515),             # nsplit > 1 with three batch tiles; the last split holds 3 columns
    (64, 257, 515),            # the rows != 32 weight-gradient path: 9 k tiles (the last one column), 17 n tiles
    (32, 4102, 64),            # K = 4 * 1024 + 6: rows of x and W only 8-byte aligned; the 64-wide loop with a tail of 6
    (32, 256, 128), (32, 128, 64), (32, 64, 128), (32, 128, 256),      # the middle stack's own layers
]
WS_FLOATS = 1 << 20            # the workspace mlp_ops allocates: never the limit for a row of the table


def fwd_plan(rows, K, N, ws_floats=WS_FLOATS):
    """(splits, kchunk) bridges_linear_forward chooses (csrc/api.hip); ws_floats = 0 stands for ws == NULL."""
    n_tiles, m_tiles = ceil_div(N, 32), rows // 32
    splits = 1 if (K <= 512 or n_tiles * m_tiles >= 128) else ceil_div(512, n_tiles * m_tiles)
    splits = min(splits, ceil_div(K, 64))
    per_split = rows * N
    if ws_floats <= 0:
        splits = 1
    elif splits * per_split > ws_floats:
        splits = ws_floats // per_split
    splits = max(splits, 1)
    kchunk = ceil_div(ceil_div(K, splits), 32) * 32
    return ceil_div(K, kchunk), kchunk


def bwd_plan(rows, K, N, ws_floats=WS_FLOATS):
    """(nsplit, nchunk) of the input gradient in bridges_linear_backward; nsplit = 0: refused ("workspace too small")."""
    n_ktiles, m_tiles = ceil_div(K, 32), rows // 32
    nsplit = 1 if N <= 512 else ceil_div(256, n_ktiles * m_tiles)
    nsplit = min(nsplit, ceil_div(N, 64))
    per_split = rows * K
    if nsplit * per_split > ws_floats:
        nsplit = ws_floats // per_split
    if nsplit < 1:
        return 0, 0
    nchunk = ceil_div(ceil_div(N, nsplit), 32) * 32
    return ceil_div(N, nchunk), nchunk


def dense(g, *shape):
    """Standard normal values pushed 0.05 away from zero: a dropped term always shows."""
    v = torch.randn(*shape, generator=g)
    return v + 0.05 * torch.where(v >= 0, 1.0, -1.0)


def mask_like(g, *shape):
    """A ReLU output used as a mask: positives, exact +0, -0.0 and negatives (only > 0 passes)."""
    m = torch.randn(*shape, generator=g)
    m[m.abs() < 0.3] = 0.0
    m[(m > 0.3) & (m < 0.5)] = -0.0
    return m


def edge_ramps_(t, lo, hi):
    """Distinct non-zero ramps in the first and last 8 columns of t [r, c] (fewer where c < 8; the last ramp wins an overlap)."""
    c = min(8, t.shape[1])
    r = torch.arange(c, dtype=torch.float32) / 8
    t[:, :c] = lo + r
    t[:, t.shape[1] - c:] = hi - r
    return t


def lin_probe(rows, K, N, device, seed=0):
    """x [rows, K], w [N, K], b [N], dz [rows, N], act [rows, K] (a mask) as float32 on ``device``: dense noise, ramps in the
    first and last 8 columns of both reduction axes (K in x, N in dz), in the first and last row of W, and the first and last
    batch row scaled differently."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + 31 * K + N)
    s = 1.0 / math.sqrt(K)
    x, w, b, dz = dense(g, rows, K), dense(g, N, K) * s, dense(g, N), dense(g, rows, N)
    edge_ramps_(x, 1.0, -2.0)
    edge_ramps_(dz, 0.5, -1.5)
    kk = torch.arange(K, dtype=torch.float32) / K
    w[0] = s * (1.0 + kk)
    w[N - 1] = -s * (2.0 + kk) if N > 1 else w[0]
    for t in (x, dz):
        t[0] *= 2.0
        t[-1] *= 0.5
    act = mask_like(g, rows, K)
    return {k: v.contiguous().to(device) for k, v in dict(x=x, w=w, b=b, dz=dz, act=act).items()}


def lin_forward_ref(x, w, b, relu):
    """-> (float64 act(x w^T + b), bound).  Terms: K products and the bias (K + 1), the <= ceil(K / 64) partial sums of a
    split-K launch and the three additions that join a workgroup's waves: K + ceil(K / 64) + 4.  ReLU is 1-Lipschitz."""
    K = x.shape[1]
    z = x.double() @ w.double().T + b.double()
    mag = x.double().abs() @ w.double().abs().T + b.double().abs()
    return (z.clamp_min(0) if relu else z), dot_bound(K + ceil_div(K, 64) + 4, mag)


def lin_forward_lib(x, w, b, relu):
    y = F.linear(x, w, b)
    return F.relu(y) if relu else y


def lin_backward_ref(dz, a, w, act=None):
    """-> {dW, db, dx: (float64 reference, bound)}.  dW = dz^T a and db = column sums of dz: ``rows`` terms.  dx = (dz W) [act > 0]:
    N products, the <= ceil(N / 64) partial sums of a split-N launch and the three additions between waves,
    N + ceil(N / 64) + 4 (the same count as the forward with N for K); exactly zero where the mask is off."""
    rows, N = dz.shape
    dzd, ad, wd = dz.double(), a.double(), w.double()
    on = (act > 0).double() if act is not None else torch.ones_like(ad)
    return dict(dW=(dzd.T @ ad, dot_bound(rows, dzd.abs().T @ ad.abs())),
                db=(dzd.sum(0), dot_bound(rows, dzd.abs().sum(0))),
                dx=((dzd @ wd) * on, dot_bound(N + ceil_div(N, 64) + 4, dzd.abs() @ wd.abs()) * on))


def lin_backward_lib(dz, a, w, act=None):
    """The float32 library result: autograd through F.linear."""
    a_, w_ = a.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    b_ = torch.zeros(w.shape[0], device=w.device, requires_grad=True)
    dx, dW, db = torch.autograd.grad(F.linear(a_, w_, b_), (a_, w_, b_), dz)
    return dict(dW=dW, db=db, dx=dx * (act > 0) if act is not None else dx)


# defective twins of the linear layers (float32, plain torch)
def twin_fwd_k_tail_dropped(x, w, b, relu):
    """The last K % 8 columns never reach the product (a missing `k0 < wend` tail)."""
    k8 = x.shape[1] - x.shape[1] % 8
    return lin_forward_lib(x[:, :k8], w[:, :k8], b, relu)


def twin_fwd_last_column_shifted(x, w, b, relu):
    """Column N - 1 computed from row N - 2 of W (an off-by-one in the clamp of the last tile)."""
    w2 = w.clone()
    w2[-1] = w[-2]
    return lin_forward_lib(x, w2, b, relu)


def twin_fwd_last_split_left_out(x, w, b, relu):
    """The finishing launch adds one split too few."""
    splits, kchunk = fwd_plan(x.shape[0], x.shape[1], w.shape[0])
    kk = (splits - 1) * kchunk
    return lin_forward_lib(x[:, :kk], w[:, :kk], b, relu)


def twin_dx_last_split_left_out(dz, a, w, act=None):
    nsplit, nchunk = bwd_plan(dz.shape[0], a.shape[1], dz.shape[1])
    nn = (nsplit - 1) * nchunk
    out = lin_backward_lib(dz, a, w, act)
    dx = dz[:, :nn] @ w[:nn]
    out["dx"] = dx * (act > 0) if act is not None else dx
    return out


def twin_dx_mask_ge_zero(dz, a, w, act=None):
    """The ReLU mask taken as act >= 0: +0 and -0.0 pass."""
    out = lin_backward_lib(dz, a, w, None)
    out["dx"] = out["dx"] * (act >= 0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Head and loss: k_successor_loss<PER_ROW>.  1024 threads per batch row, 4 pixels per thread cached (4096), the rest recomputed.

LOSS_SHAPES = [                # (batch, px, nf, use_q, use_sf, per_row)
    (32, 4096, 6, True, True, False),       # the flagship: the cache exactly full, one batch tile, nothing masked
    (1, 64, 0, True, True, False),          # px < 1024: threads 64.. hold nothing; nf = 0: no binary columns; batch 1 of 32 rows
    (7, 64, 6, False, True, True),          # the same with a map per transition, successor features only
    (7, 1024, 6, True, False, True),        # one pixel per thread; q only
    (33, 4096, 0, False, True, True),       # rows = 64: 31 padding rows behind a second tile
    (7, 4100, 6, True, True, False),        # 4 pixels past the cache: the `images larger than the cache` loops, threads 0..3 only
    (32, 4100, 0, True, True, True),
    (33, 5184, 6, True, True, True),        # 72 x 72: one more pixel for every thread, a second for threads 0..63
    (1, 9000, 6, True, True, False),        # the loops run four and five times
    (7, 9000, 0, True, False, True),
    (32, 9000, 6, False, True, False),
]
LOSS_BATCHES = 3               # the per-call arrays hold three batches; the counter picks one (0 and 2 are tested)


def loss_probe(batch, px, nf, per_row, device, seed=0):
    """y [rows, 2 px + 2 nf] (padding rows hold values the kernel must not use), reward [px] or [3 batch, px],
    q_t [3 batch], sf_t [3 batch, px]."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * batch + 31 * px + nf + 2 * per_row)
    rows, n = rows_of(batch), LOSS_BATCHES * batch
    y = dense(g, rows, 2 * px + 2 * nf) * 1.5
    edge_ramps_(y[:, :px], 0.25, -0.5)
    edge_ramps_(y[:, px:2 * px], -1.0, 1.25)
    y[0] *= 2.0
    y[batch - 1] *= 0.5
    reward = dense(g, n, px) if per_row else dense(g, px)
    edge_ramps_(reward.view(-1, px), 1.5, -1.0)
    q_t, sf_t = dense(g, n) * 3.0, dense(g, n, px)
    return {k: v.contiguous().to(device) for k, v in dict(y=y, reward=reward, q_t=q_t, sf_t=sf_t).items()}


def loss_batch(pr, batch, px, counter):
    """(reward [batch, px], q_t [batch], sf_t [batch, px]) of batch ``counter`` of the per-call arrays."""
    lo = counter * batch
    rw = pr["reward"][lo:lo + batch] if pr["reward"].dim() == 2 else pr["reward"].expand(batch, px)
    return rw, pr["q_t"][lo:lo + batch], pr["sf_t"][lo:lo + batch]


def loss_ref(y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf, px_used=None):
    """Float64 statement of head, loss and gradient (cv.py:104-108: q = sum_j softmax(psi)[1][j] reward[j];
    successor_dqn.py:215-232: loss = [use_q] mse(q, q_t) + [use_sf] mse(psi0, sf_t)) -> {q, loss_rows, dy: (reference, bound)},
    padded to the launch's rows with exact zeros (rows >= batch, columns >= 2 px).  loss_rows[b] is row b's share of the loss.

    Allowances, first order in u (d = p0 - p1, s = sigmoid(-d), S = sum |s rw|, B = batch):
      s        relative es = (|d| + 4) u: the rounded difference moves exp by |d| u, then exp, the addition and the division
      q        es on every product's s, a float32 sum of px products in any order (dot_bound(px, S)) and the rounding of q
      q - q_t  ABSOLUTE: the allowance of q plus u |q - q_t| (a relative one would vanish with the difference)
      loss     (2 |dq| e + 3 u dq^2) / B for the square, dot_bound(px + 8, .) for the mean of squares and its scalings, u for the sum
      dy       g1 = c rw s (1 - s), c = 2 (q - q_t) / B: the allowance of c (2 e / B + 2 u |c|) times |rw| s (1 - s), s (1 - s)
               moved by |1 - 2 s| s es plus 2 u s (it may be formed as s - s s), two products; the sf part 4 u, the sum u."""
    rows, N = rows_of(batch), 2 * px + 2 * nf
    u = U32
    yd = y[:batch].double()
    p0, p1, rwd = yd[:, :px], yd[:, px:2 * px], rw.double()
    if px_used is not None:                                # (the defective twin's view of the operator)
        p0, p1, rwd, sf_t = p0[:, :px_used], p1[:, :px_used], rwd[:, :px_used], sf_t[:, :px_used]
    d = p0 - p1
    s = 1.0 / (1.0 + torch.exp(d))
    es = (d.abs() + 4.0) * u
    S = (s * rwd).abs()
    q = (s * rwd).sum(1)
    e_q = dot_bound(px, S.sum(1)) + (S * es).sum(1) + u * q.abs()
    dq = q - q_t.double()
    e_dq = e_q + u * dq.abs()
    err = p0 - sf_t.double()
    t1 = dq * dq / batch if use_q else torch.zeros_like(q)
    t2 = (err * err).sum(1) / (batch * px) if use_sf else torch.zeros_like(q)
    e_t1 = (2 * dq.abs() * e_dq + 3 * u * dq * dq) / batch if use_q else torch.zeros_like(q)
    e_l = e_t1 + (dot_bound(px + 8, t2) if use_sf else 0.0) + u * (t1 + t2)
    c = 2.0 * dq / batch if use_q else torch.zeros_like(q)
    e_c = 2.0 * e_dq / batch + 2 * u * c.abs() if use_q else torch.zeros_like(q)
    ss = s * (1.0 - s)
    e_ss = (1.0 - 2.0 * s).abs() * s * es + 2 * u * s
    g1 = c[:, None] * rwd * ss
    e_g1 = rwd.abs() * (e_c[:, None] * ss + c.abs()[:, None] * e_ss) + 2 * u * g1.abs()
    sfp = 2.0 / (batch * px) * err if use_sf else torch.zeros_like(err)
    g0 = sfp - g1
    e_g0 = 4 * u * sfp.abs() + e_g1 + (u * g0.abs() if use_sf else 0.0)
    w = p0.shape[1]

    def pad(v, cols=None):
        out = torch.zeros((rows,) if cols is None else (rows, N), dtype=torch.float64, device=y.device)
        if cols is None:
            out[:batch] = v
        else:
            out[:batch, :w], out[:batch, px:px + w] = v[0], v[1]
        return out
    return dict(q=(pad(q), pad(e_q)), loss_rows=(pad(t1 + t2), pad(e_l)), dy=(pad((g0, g1), N), pad((e_g0, e_g1), N)))


def loss_lib(y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf):
    """The torch formulation under autograd in the dtype of y -> {q, loss_rows, dy}, padded like loss_ref."""
    rows = rows_of(batch)
    yy = y[:batch].detach().clone().requires_grad_(True)
    psi = yy[:, :2 * px].reshape(batch, 2, px)
    q = (psi.softmax(dim=1)[:, 1] * rw).sum(-1)
    per_row = torch.zeros_like(q)
    if use_q:
        per_row = per_row + (q - q_t) ** 2 / batch
    if use_sf:
        per_row = per_row + ((psi[:, 0] - sf_t) ** 2).sum(-1) / (batch * px)
    (dy,) = torch.autograd.grad(per_row.sum(), yy)
    pad = lambda v: torch.cat([v.detach(), torch.zeros((rows - batch, *v.shape[1:]), dtype=v.dtype, device=v.device)])
    return dict(q=pad(q), loss_rows=pad(per_row), dy=pad(dy))


def twin_loss_cache_only(y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf, cache=4096):
    """Pixels >= 4096 ignored: the kernel without its `images larger than the cache` loops (float32 throughout)."""
    full = loss_ref(y, rw, q_t, sf_t, batch, px, nf, use_q, use_sf, px_used=min(px, cache))
    return {k: v[0].float() for k, v in full.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# Adam: k_adam_flat, k_adam_multi, k_lin_bwd<true>

ADAM_HYPER = (1e-3, 0.9, 0.999, 1e-8)          # lr, beta1, beta2, eps: torch's defaults, the optimiser of successor_dqn.py:640
ADAM_STEPS = (1, 7)
ADAM_FLAT_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099)       # n >> 2 == 0, the n % 4 tail of 1..3, one and two grid rounds
ADAM_MULTI_N = (1, 3, 1024, 1025, 2047)                     # one chunk short / full, a second chunk of 1 and of 1023


def adam_probe(n, device, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + n)
    p, gr, m, v = dense(g, n), dense(g, n), dense(g, n) * 0.1, torch.rand(n, generator=g) * 0.01 + 1e-4
    return tuple(t.to(device) for t in (p, gr, m, v))


def adam_ref(p, g, m, v, t, hyper=ADAM_HYPER):
    """The update the comment above k_adam_flat states, in float64 from the float32 inputs -> {p, m, v: (reference, bound)}:
      m' = m + (g - m) (1 - b1);  v' = b2 v + (1 - b2) g g;  p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps).
    Operations counted (each rounds once, a float32 coefficient counts as one more):
      m'  the difference, the coefficient and the product (3 u on |(g - m)(1 - b1)|), the sum (u |m'|)
      v'  coefficient and product (2 u |b2 v|), coefficient and two products (3 u |(1 - b2) g g|), the sum (u |v'|)
      D   the root (half the relative allowance of v', plus u), the correction and the division (2 u), eps (u eps), the sum (u D)
      p'  step size, product and division (3 u |U|, U the update), m' and D carried through, the difference (u |p'|)."""
    lr, b1, b2, eps = hyper
    u = U32
    p, g, m, v = (x.double() for x in (p, g, m, v))
    dm = (g - m) * (1 - b1)
    m1 = m + dm
    e_m = u * (3 * dm.abs() + m1.abs())
    a, b = b2 * v, (1 - b2) * g * g
    v1 = a + b
    e_v = u * (2 * a.abs() + 3 * b.abs() + v1.abs())
    c2 = math.sqrt(1 - b2 ** t)
    r = v1.sqrt() / c2
    D = r + eps
    e_D = r * (e_v / (2 * v1.clamp_min(1e-300)) + 3 * u) + u * eps + u * D
    step = lr / (1 - b1 ** t)
    U = step * m1 / D
    p1 = p - U
    e_p = 3 * u * U.abs() + step * e_m / D + U.abs() * e_D / D + u * p1.abs()
    return dict(p=(p1, e_p), m=(m1, e_m), v=(v1, e_v))


def adam_lib(p, g, m, v, t, hyper=ADAM_HYPER, fused=False):
    """torch.optim.Adam taking update number t from the given moments (float32) -> {p, m, v}."""
    lr, b1, b2, eps = hyper
    par = torch.nn.Parameter(p.detach().clone())
    par.grad = g.detach().clone()
    opt = torch.optim.Adam([par], lr=lr, betas=(b1, b2), eps=eps, fused=fused)
    step = torch.tensor(float(t - 1), dtype=torch.float32, device=p.device if fused else "cpu")
    opt.state[par] = dict(step=step, exp_avg=m.detach().clone(), exp_avg_sq=v.detach().clone())
    opt.step()
    st = opt.state[par]
    return dict(p=par.detach(), m=st["exp_avg"], v=st["exp_avg_sq"])


def twin_adam_tail_not_updated(p, g, m, v, t, hyper=ADAM_HYPER):
    """The n % 4 tail of the range keeps its old values (a float4 loop without its scalar tail)."""
    out = adam_lib(p, g, m, v, t, hyper)
    n4 = p.numel() - p.numel() % 4
    for k, old in (("p", p), ("m", m), ("v", v)):
        out[k] = torch.cat([out[k][:n4], old[n4:]])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# TD target: k_td_target<PER_ROW>, one workgroup of 256 threads per transition (row j of a segment sits in thread (j - lo) % 256)

TD_LENGTHS = (1, 255, 256, 257, 513, 700)      # below, at and above one stride of the 256 threads; two and three strides
TD_SF_DIMS = (0, 4, 64, 4096)
TD_PEAK = 64.0                                 # above every random value: planted maxima


def td_probe(sf_dim, device, seed=0, strided=True):
    """Transitions over the rows of one next_q [R] (values quantised to quarters: ties are plentiful), next_sf [R, sf_dim] as
    the psi[:, 0] view of a [R, 2, h, w] tensor (``strided``) or contiguous:
      0..5   segments of TD_LENGTHS, back to back; the one of 700 carries a planted maximum at rows lo + 5 and lo + 5 + 256
             (the same thread, a later stride), the one of 513 at lo + 44 and lo + 300 (thread 44 again, one stride later) and
             the one of 257 at lo + 200 and lo + 256 -- different threads, the LATER row in the EARLIER tree slot (thread 0)
      6      a segment of three rows, all -inf: its first row is the arg-max
      7      an empty segment, done
      8, 9   (lo, hi) pairs that share rows with others: the segment of 257 again, and rows 100.. of the segment of 700
    done: transitions 1, 7 and 8."""
    g = torch.Generator().manual_seed(1000003 * seed + sf_dim)
    lo, hi, at = [], [], 0
    for n in TD_LENGTHS + (3,):
        lo.append(at)
        hi.append(at + n)
        at += n
    R = at
    next_q = torch.round(torch.randn(R, generator=g) * 4) / 4
    l257, l513, l700 = lo[3], lo[4], lo[5]
    next_q[[l700 + 5, l700 + 5 + 256, l513 + 44, l513 + 300, l257 + 200, l257 + 256]] = TD_PEAK
    next_q[lo[6]:hi[6]] = -math.inf
    lo += [hi[6], l257, l700 + 100]
    hi += [hi[6], hi[3], hi[5]]
    B = len(lo)
    done = [i in (1, 7, 8) for i in range(B)]
    lin = dense(g, B)
    out = dict(lo=lo, hi=hi, done=done, next_q=next_q.to(device), lin=lin.to(device), next_sf=None, act=None, sf_dim=sf_dim)
    if sf_dim:
        h = {4: 2, 64: 8, 4096: 64}[sf_dim]
        full = dense(g, R, 2, h, sf_dim // h).to(device)
        out["next_sf"] = full[:, 0] if strided else full[:, 0].contiguous()
        out["act"] = (torch.rand(B, 1, h, sf_dim // h, generator=g) > 0.5).float().to(device)
    return out


def td_plain(pr, gamma, last=False):
    """The operator in plain float32 torch (``last``: the defective twin that takes the LAST maximum of a tie)
    -> (q [B], sf [B, D] or None, rows list)."""
    nq, q, sf, rows = pr["next_q"], [], [], []
    for i, (lo, hi) in enumerate(zip(pr["lo"], pr["hi"])):
        if hi > lo:
            seg = nq[lo:hi]
            k = hi - lo - 1 - int(seg.flip(0).argmax()) if last else int(seg.argmax())
            rows.append(lo + k)
        else:
            rows.append(NO_ROW)
        live = not pr["done"][i] and hi > lo
        nxt = nq[rows[-1]] if live else torch.zeros((), device=nq.device)
        if hi == lo and not pr["done"][i]:
            nxt = torch.full((), -math.inf, device=nq.device)
        q.append(pr["lin"][i] + gamma * nxt)
        if pr["sf_dim"]:
            a = pr["act"][i].reshape(-1)
            sf.append(a + gamma * pr["next_sf"][rows[-1]].reshape(-1) if live else a + gamma * torch.zeros_like(a))
    return torch.stack(q), (torch.stack(sf) if pr["sf_dim"] else None), rows


def td_ref(pr, gamma):
    """The oracle's restatement (oracle.dqn.td_targets, as tests/test_gpu_dqn.py uses it) on the probe -> {q, sf: (reference,
    bound)}, rows.  The oracle takes back-to-back segments, so every non-empty (lo, hi) contributes a copy of its rows of next_q;
    the successor features are then taken by a second call on the selected rows (one row per transition).  An empty segment is
    what include/bridges_hip.h states: q = lin + gamma * (done ? 0 : -inf), sf = the action raster, row = 0x7fffffff.
    Bound: 2 u (|a| + |gamma s|) -- the product and the sum, rounded separately or fused -- and zero where done."""
    from oracle import dqn as O
    nq_dev, dev = pr["next_q"], pr["next_q"].device
    nq, lin = nq_dev.cpu(), pr["lin"].cpu()
    B = len(pr["lo"])
    live = [i for i in range(B) if pr["hi"][i] > pr["lo"][i]]
    num = [pr["hi"][i] - pr["lo"][i] for i in live]
    cat = torch.cat([nq[pr["lo"][i]:pr["hi"][i]] for i in live])
    q_live, nq_sel, _, sel = O.td_targets(cat, None, num, [pr["done"][i] for i in live], gamma, lin[live], None)
    rows, q, off = [NO_ROW] * B, torch.empty(B), 0
    e_q = torch.zeros(B, dtype=torch.float64)
    for k, i in enumerate(live):
        rows[i] = pr["lo"][i] + sel[k] - off
        off += num[k]
        q[i] = q_live[k]
        e_q[i] = 0.0 if pr["done"][i] else 2 * U32 * (abs(float(lin[i])) + abs(gamma * float(nq_sel[k])))
    for i in range(B):
        if i not in live:
            q[i] = lin[i] + gamma * (0.0 if pr["done"][i] else -math.inf)
    e_q = torch.nan_to_num(e_q, nan=0.0, posinf=0.0)                  # an infinite target is met exactly
    out = dict(q=(q.double().to(dev), e_q.to(dev)), sf=None)
    if pr["sf_dim"]:
        act = pr["act"].cpu()
        sf, e_sf = act.reshape(B, -1).clone(), torch.zeros(B, pr["sf_dim"], dtype=torch.float64)
        idx = torch.tensor([rows[i] for i in live])
        nsf = pr["next_sf"][idx.to(dev)].cpu()                         # [n_live, h, w]: channel 0 of the selected rows
        both = torch.stack([nsf, torch.zeros_like(nsf)], dim=1)       # the oracle reads [:, 0] of [n, 2, h, w]
        dn = [pr["done"][i] for i in live]
        _, _, st, _ = O.td_targets(nq[idx], both, [1] * len(live), dn, gamma, lin[live], act[live])
        for k, i in enumerate(live):
            sf[i] = st[k].reshape(-1)
            if not dn[k]:
                e_sf[i] = 2 * U32 * (act[i].reshape(-1).double().abs() + (gamma * nsf[k].reshape(-1).double()).abs())
        out["sf"] = (sf.double().to(dev), e_sf.to(dev))
    return out, rows


def td_conform(name, got, lib, ref, ref_rows, shape=None):
    """got / lib = (q, sf, rows): the rows exact, q and sf through conform."""
    assert [int(r) for r in got[2]] == [int(r) for r in ref_rows], f"{name} {shape}: arg-max rows {list(got[2])} != {ref_rows}"
    conform(name + ".q", got[0], lib[0], *ref["q"], shape)
    if ref["sf"] is not None:
        conform(name + ".sf", got[1], lib[1], *ref["sf"], shape)


# ---------------------------------------------------------------------------------------------------------------------------
# The middle stack: k_mid_fwd / k_mid_bwd<256,128,64,128,256> (one launch each way for the step's four middle Linear + ReLU
# layers, the backward launch with "rider" workgroups that apply another layer's Adam update) and k_rows2<256,128,64,true> /
# k_rows2<64,128,256,false> (the same stack for many rows, two layers a launch, the hidden activation in LDS only).

MID_DIMS = (256, 128, 64, 128, 256)
MID_ROWS_N = (1, 31, 32, 33, 63, 8193, 16389)   # partial / full / one-past tiles; 8193: the first row of a second grid round;
                                                # 16389: a third round, so the prefetch of `next` is live in the second
MID_ROWS_STRIDES = ((256, 256), (260, 257), (320, 300), (256, 300), (320, 256))      # (x_stride, y_stride) in floats
MID_ROWS_STRIDED_N = (1, 31, 32, 8193)          # the rows the strided pairs run at: the three smallest and one large
MID_REST_N = (0, 4, 4100, 16388, 4 * (249 * 4096) + 4)       # the riders' Adam range, see rider_plan


def T(K):
    """The term count of a layer's product as lin_forward_ref counts it."""
    return K + ceil_div(K, 64) + 4


def rows_plan(n_rows):
    """(workgroups, grid rounds) of either launch of bridges_mlp_mid_rows (csrc/api.hip: a workgroup per 32-row tile, the grid
    clamped to 256, the kernel strides over the tiles)."""
    tiles = ceil_div(n_rows, 32)
    grid = min(max(tiles, 1), 256)
    return grid, ceil_div(tiles, grid)


def rider_plan(rest_n):
    """(rider workgroups, stride rounds, float4 groups in the last round) of bridges_mlp_mid_backward's Adam range
    (csrc/api.hip: a rider per 4096 float4 groups, at most 248; k_mid_bwd: a rider's 1024 threads stride over the groups)."""
    n4 = rest_n >> 2
    riders = min(ceil_div(n4, 4096), 248)
    if riders == 0:
        return 0, 0, 0
    stride = riders * 1024
    return riders, ceil_div(n4, stride), n4 - (ceil_div(n4, stride) - 1) * stride


def mid_probe(device, seed=0):
    """The stack's probe data, layer l from lin_probe(32, D[l], D[l + 1]) (so every layer carries the edge ramps and scaled
    first / last rows): W [4], b [4], x = the forward's acts[0], acts [5] = the BACKWARD's activations (mask_like: positives,
    +0, -0.0 and negatives; acts[l] is both the mask of dz[l] and the A operand of dW[l]), dz4 [32, 256]."""
    D = MID_DIMS
    prs = [lin_probe(32, D[l], D[l + 1], device, seed) for l in range(4)]
    g = torch.Generator().manual_seed(1000003 * seed + 4)
    acts = [pr["act"] for pr in prs] + [mask_like(g, 32, D[4]).to(device)]
    return dict(W=[pr["w"] for pr in prs], b=[pr["b"] for pr in prs], x=prs[0]["x"], acts=acts, dz4=prs[3]["dz"])


def rows_probe(n, device, seed=0, nan_row=None):
    """x [n, 256]: the pre-activation in front of the stack for n rows -- dense noise (about half negative), ramps in the first
    and last 8 columns, -0.0 sprinkled in, first and last row scaled, and (``nan_row``) one row of NaN."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * n + 13)
    x = dense(g, n, MID_DIMS[0])
    edge_ramps_(x, 1.0, -2.0)
    x[torch.rand(n, MID_DIMS[0], generator=g) < 0.05] = -0.0
    x[0] *= 2.0
    x[-1] *= 0.5
    if nan_row is not None:
        x[nan_row] = math.nan
    return x.contiguous().to(device)


def mid_forward_lib(W, b, x, relu_in=False):
    """Plain float32 torch -> [acts[1], .., acts[4]]."""
    a, out = (F.relu(x) if relu_in else x), []
    for w_, b_ in zip(W, b):
        a = F.relu(F.linear(a, w_, b_))
        out.append(a)
    return out


def mid_forward_conform(name, x, outs, W, b, shape=None):
    """k_mid_fwd writes every activation, so each link is judged as ONE layer: outs[l] against lin_forward_ref on the stack's
    OWN input of that layer (x, outs[0], ..), the library figure F.linear + relu on the same input."""
    ins = [x] + list(outs[:-1])
    for l, (a, y) in enumerate(zip(ins, outs)):
        ref, bound = lin_forward_ref(a, W[l], b[l], True)
        conform(f"{name}.acts{l + 1}", y, lin_forward_lib(a, W[l], b[l], True), ref, bound, shape)


def chain2_ref(x, Wa, ba, Wb, bb, relu_in):
    """One k_rows2 launch: y = relu(h Wb^T + bb), h = relu(x' Wa^T + ba), x' = relu(x) if relu_in -> (float64 y, bound).  h never
    leaves LDS, so its error is carried through the second layer (ReLU is 1-Lipschitz):
      B1 = dot_bound(T(DA), |x'| |Wa|^T + |ba|);  B2 = dot_bound(T(DB), |h| |Wb|^T + |bb|) + B1 |Wb|^T."""
    xd, Wa, ba, Wb, bb = (t.double() for t in (x, Wa, ba, Wb, bb))
    if relu_in:
        xd = xd.clamp_min(0)
    h = (xd @ Wa.T + ba).clamp_min(0)
    B1 = dot_bound(T(Wa.shape[1]), xd.abs() @ Wa.abs().T + ba.abs())
    y = (h @ Wb.T + bb).clamp_min(0)
    return y, dot_bound(T(Wb.shape[1]), h.abs() @ Wb.abs().T + bb.abs()) + B1 @ Wb.abs().T


def rows_lib(W, b, x):
    """bridges_mlp_mid_rows in plain float32 torch -> (mid [n, 64], y [n, 256])."""
    a = mid_forward_lib(W, b, x, relu_in=True)
    return a[1], a[3]


def rows_conform(name, x, mid, y, W, b, shape=None, keep=None):
    """The first launch judged on ``mid`` from x, the second on ``y`` from the given ``mid`` (the kernel's own), each against
    chain2_ref; ``keep``: a row mask (the rows without a NaN, which conform would count as outside)."""
    sel = (lambda t: t) if keep is None else (lambda t: t[keep])
    ref, bound = chain2_ref(x, W[0], b[0], W[1], b[1], True)
    lb = F.relu(F.linear(F.relu(F.linear(F.relu(x), W[0], b[0])), W[1], b[1]))
    conform(f"{name}.mid", sel(mid), sel(lb), sel(ref), sel(bound), shape)
    ref, bound = chain2_ref(mid, W[2], b[2], W[3], b[3], False)
    lb = F.relu(F.linear(F.relu(F.linear(mid, W[2], b[2])), W[3], b[3]))
    conform(f"{name}.y", sel(y), sel(lb), sel(ref), sel(bound), shape)


def mid_backward_ref(W, acts, dz4):
    """k_mid_bwd in float64 with the allowance carried down the chain -> {dW0..3, db0..3, dz0: (reference, bound)}.  The masks
    come from the given acts, so no float32 / float64 decision can differ.  z_4 = dz4, B_4 = 0; for l = 3 .. 0:
      dW[l] = z_{l+1}^T acts[l]        bound dot_bound(32, |z_{l+1}|^T |acts[l]|) + B_{l+1}^T |acts[l]|
      db[l] = sum over rows of z_{l+1} bound dot_bound(32, sum |z_{l+1}|) + sum B_{l+1}
      z_l   = (z_{l+1} W[l]) [acts[l] > 0]
      B_l   = (dot_bound(T(D[l+1]), |z_{l+1}| |W[l]|) + B_{l+1} |W[l]|) [acts[l] > 0]
    z_0 is dz[0]; where a mask is off the bound is zero and the result must be exactly 0."""
    z, B, out = dz4.double(), torch.zeros_like(dz4, dtype=torch.float64), {}
    for l in (3, 2, 1, 0):
        a, w = acts[l].double(), W[l].double()
        out[f"dW{l}"] = (z.T @ a, dot_bound(32, z.abs().T @ a.abs()) + B.T @ a.abs())
        out[f"db{l}"] = (z.sum(0), dot_bound(32, z.abs().sum(0)) + B.sum(0))
        on = (acts[l] > 0).double()
        z, B = (z @ w) * on, (dot_bound(T(w.shape[0]), z.abs() @ w.abs()) + B @ w.abs()) * on
    out["dz0"] = (z, B)
    return out


def mid_backward_lib(W, acts, dz4):
    """The same chain in plain float32 torch; masks by torch.where, so a non-finite gradient under a dead unit gives 0 as
    autograd's ReLU backward does."""
    z, out = dz4, {}
    for l in (3, 2, 1, 0):
        out[f"dW{l}"], out[f"db{l}"] = z.T @ acts[l], z.sum(0)
        z = torch.where(acts[l] > 0, z @ W[l], torch.zeros_like(acts[l]))
    out["dz0"] = z
    return out


MID_BWD_KEYS = tuple(f"{k}{l}" for l in (3, 2, 1, 0) for k in ("dW", "db")) + ("dz0",)


def mid_backward_conform(name, got, W, acts, dz4, shape=None):
    refs, lb = mid_backward_ref(W, acts, dz4), mid_backward_lib(W, acts, dz4)
    for k in MID_BWD_KEYS:
        conform(f"{name}.{k}", got[k], lb[k], *refs[k], shape)


# defective twins of the stack (float32, plain torch)
def twin_mid_fwd_quarter_left_out(W, b, x, relu_in=False):
    """Layer 1 (128 -> 64) without the third of its four K quarters (a wave's partial sum never added)."""
    a = mid_forward_lib(W[:1], b[:1], x, relu_in)
    keep = [k for k in range(W[1].shape[1]) if not 64 <= k < 96]
    h = F.relu(F.linear(a[0][:, keep], W[1][:, keep], b[1]))
    return a + [h] + mid_forward_lib(W[2:], b[2:], h)


def twin_mid_fwd_last_tile_without_bias(W, b, x, relu_in=False):
    """Columns 224 .. 255 of the last layer without their bias."""
    b3 = b[3].clone()
    b3[-32:] = 0.0
    return mid_forward_lib(W, b[:3] + [b3], x, relu_in)


def twin_mid_fwd_bf16_operands(W, b, x, relu_in=False):
    """Layer 2 (64 -> 128) with both operands rounded to bfloat16 (a matrix-core instruction of the wrong type)."""
    a = mid_forward_lib(W[:2], b[:2], x, relu_in)
    h = F.relu(F.linear(a[1].bfloat16().float(), W[2].bfloat16().float(), b[2]))
    return a + [h] + mid_forward_lib(W[3:], b[3:], h)


def rows_from(fwd):
    """A forward twin as a twin of bridges_mlp_mid_rows."""
    def fn(W, b, x):
        a = fwd(W, b, x, True)
        return a[1], a[3]
    return fn


def twin_rows_relu_in_forgotten(W, b, x):
    a = mid_forward_lib(W, b, x, relu_in=False)
    return a[1], a[3]


def twin_rows_last_tile_from_row_n_minus_1(W, b, x):
    """Every row of a partial last tile computed from row n - 1 (the clamp of the fetch applied to all of the tile's rows)."""
    n = x.shape[0]
    x2 = x.clone()
    if n % 32:
        x2[n - n % 32:] = x[n - 1]
    return rows_lib(W, b, x2)


def twin_mid_bwd_inner_mask_ge_zero(W, acts, dz4):
    """The mask of dz[2] taken as acts[2] >= 0: +0 and -0.0 pass."""
    z, out = dz4, {}
    for l in (3, 2, 1, 0):
        out[f"dW{l}"], out[f"db{l}"] = z.T @ acts[l], z.sum(0)
        z = torch.where((acts[l] >= 0) if l == 2 else (acts[l] > 0), z @ W[l], torch.zeros_like(acts[l]))
    out["dz0"] = z
    return out


def twin_mid_bwd_dw_from_unmasked_gradient(W, acts, dz4):
    """dW[l], l < 3, formed from the product before its mask."""
    out = mid_backward_lib(W, acts, dz4)
    z = dz4
    for l in (3, 2, 1):
        raw = z @ W[l]
        out[f"dW{l - 1}"] = raw.T @ acts[l - 1]
        z = torch.where(acts[l] > 0, raw, torch.zeros_like(raw))
    return out


def twin_mid_bwd_db_even_rows_only(W, acts, dz4):
    """db summed over rows 0, 2, .., 30: the half-wave that holds the odd rows never joins (a lost cross-half shuffle)."""
    out = mid_backward_lib(W, acts, dz4)
    z = dz4
    for l in (3, 2, 1, 0):
        out[f"db{l}"] = z[0::2].sum(0)
        z = torch.where(acts[l] > 0, z @ W[l], torch.zeros_like(acts[l]))
    return out


def twin_rider_first_round_only(p, g, m, v, t, hyper=ADAM_HYPER):
    """Each rider thread updates its first float4 group only: the range beyond the first stride round keeps its old values."""
    out = adam_lib(p, g, m, v, t, hyper)
    riders = rider_plan(p.numel())[0]
    done = min(4 * riders * 1024, p.numel())
    for k, old in (("p", p), ("m", m), ("v", v)):
        out[k] = torch.cat([out[k][:done], old[done:]])
    return out
