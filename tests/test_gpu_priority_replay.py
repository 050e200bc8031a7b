"""GPU: prioritised replay on the device -- the sampler kernel (bridges_priority_sample) and the refresh
(bridges_priority_update) against tests/priority_ref.py (checked without a GPU by tests/test_cpu_priority_replay.py, which also
shows that the defective twins are rejected), the ring layer, and VecDQN(prioritized=True, priority_alpha=..,
priority_refresh=True): the refreshed priorities of the sampled rows, q(s_t, a_t) against the policy module's plain forward in
float64, and the default loop bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import priority_ref as P
from acting_conformance import sigmoid_allowance
from gpu_helpers import dot_bound, library_twin
from robotoddler.training import records as R
from test_gpu_double_q import GAMMA, HIDDEN, random_env, tower_env
from test_gpu_vec_dqn_tasks import make_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (R.RECORD_WIDTH, R.RECORD_WIDTH + 10)       # the plain record; a record with a task tail and a horizon


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def bits(t):
    """The tensor's bytes as int64 words: equality that holds for NaN as well."""
    return t.contiguous().view(torch.int64)


_RECORDS = {}


def records(N, W, td):
    """rec [N, W] on the device: seeded noise (shared per (N, W), never written by a test) with ``td`` in the priority column."""
    base = _RECORDS.get((N, W))
    if base is None:
        g = torch.Generator().manual_seed(100 * N + W)
        base = _RECORDS[(N, W)] = torch.randn((N, W), generator=g, dtype=torch.float64).to(DEV)
    rec = base.clone()
    rec[:, R.O_TD] = torch.from_numpy(np.asarray(td, dtype=np.float64)).to(DEV)
    return rec


def draw(rec, alpha, u, n_rec=None):
    """dqn_ops.priority_sample with a scratch buffer that ends in 64 guard words, which must come back untouched."""
    from bridges_hip import dqn_ops
    n_rec = rec.shape[0] if n_rec is None else n_rec
    need = dqn_ops.priority_sample_scratch(n_rec)
    buf = torch.full((need + 64,), -7.0, dtype=torch.float64, device=DEV)
    idx = dqn_ops.priority_sample(rec, n_rec, R.O_TD, alpha, torch.from_numpy(np.asarray(u, dtype=np.float64)).to(DEV), buf[:need])
    assert bool((buf[need:] == -7.0).all()), "the sampler wrote past its scratch"
    return idx


# ------------------------------------------------------------------------------------------------------------ 1: the sampler
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("N", P.PROBE_N)
def test_sampler_on_the_probe(N, W):
    """Every probe case of this N (alpha in {1, 0.6, 0} x n in {1, 63, 64, 65, 800}): the acceptance rule of priority_ref, two
    calls equal bit for bit, rec untouched."""
    for alpha in P.PROBE_ALPHA:
        for n in P.PROBE_DRAWS:
            td, u = P.probe(N, n)
            rec = records(N, W, td)
            before = bits(rec).clone()
            a = draw(rec, alpha, u)
            b = draw(rec, alpha, u)
            torch.cuda.synchronize()
            assert a.dtype == torch.int64 and a.shape == (n,) and torch.equal(a, b), (N, W, alpha, n)
            assert torch.equal(bits(rec), before)
            why = P.accept(a.cpu().numpy(), P.probe_ref(N, alpha, n))
            assert why is None, (N, W, alpha, n, why)


def test_sampler_reads_only_the_live_rows():
    """n_rec below the rows of the buffer: the rows beyond it -- priorities of 1e9 here -- are never drawn, and the draw is the
    one over a buffer that ends there."""
    td, u = P.probe(257, 800)
    full = np.concatenate([td, np.full(300, 1e9)])
    rec = records(557, R.RECORD_WIDTH, full)
    for alpha in P.PROBE_ALPHA:
        a = draw(rec, alpha, u, n_rec=257)
        assert int(a.max()) <= 256 and P.accept(a.cpu().numpy(), P.probe_ref(257, alpha, 800)) is None
        assert torch.equal(a, draw(records(257, R.RECORD_WIDTH, td), alpha, u))


# ------------------------------------------------------------------------------------------------------------ 2: boundaries
@pytest.mark.parametrize("alpha", P.PROBE_ALPHA)
def test_sampler_on_boundaries(alpha):
    """u = 0, u = nextafter(1, 0) and u exactly on boundaries of the float64 CDF: neighbours allowed, no cap; N = 1: row 0."""
    td, _ = P.probe(257, 1)
    cdf = np.cumsum(P.masses(td, alpha))
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0)], (cdf / cdf[-1])[[0, 1, 85, 86, 127, 128, 200, 254, 255]]])
    u = u[u < 1.0]
    a = draw(records(257, R.RECORD_WIDTH, td), alpha, u).cpu().numpy()
    ref = P.sample_ref(td, alpha, u)
    assert P.accept(a, ref, cap=None) is None, P.accept(a, ref, cap=None)
    assert a[0] == 0 and a[1] == ref[0][1] and 0 <= a.min() and a.max() <= 256
    one = draw(records(1, R.RECORD_WIDTH, [3.0]), alpha, [0.0, 0.5, np.nextafter(1.0, 0.0)])
    assert one.tolist() == [0, 0, 0]


def test_sampler_on_exact_ties_follows_the_right_hand_rule():
    """alpha = 0 over 256 and 1024 rows, u = k / N: every partial sum is an integer and exact in any order, so u * total IS the
    prefix sum of row k - 1 and the draw must name row k (searchsorted(right=True)) -- no tolerance is due."""
    for N in (256, 1024):
        td, u = P.tie_probe(N)
        a = draw(records(N, R.RECORD_WIDTH, td), 0.0, u)
        ref = P.sample_ref(td, 0.0, u, tol=0.0)
        assert P.undecided(ref) == 0 and a.tolist() == ref[0].tolist() == list(range(N))


# ------------------------------------------------------------------------------------------------------------ 3: alpha = 0
def test_alpha_zero_is_uniform_whatever_the_priorities():
    N, n = 257, 800
    td, u = P.probe(N, n)
    want = np.minimum(np.floor(u.astype(np.longdouble) * N), N - 1).astype(np.int64)
    assert P.undecided(P.probe_ref(N, 0.0, n)) == 0 and want.tolist() == P.probe_ref(N, 0.0, n)[0].tolist()
    wild = np.where(np.arange(N) % 3 == 0, np.inf, np.where(np.arange(N) % 3 == 1, np.nan, 1e300))
    for prio in (td, np.zeros(N), wild):
        assert draw(records(N, R.RECORD_WIDTH, prio), 0.0, u).tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------------------ 4: the refresh
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("n", P.UPDATE_N)
def test_update_kernel(n, W):
    """The last draw of a row wins (the draws repeat rows with different q_sa), out-of-range indices write nothing, every other
    column and row is bit-identical; also with n_rec below the buffer's rows."""
    from bridges_hip import dqn_ops
    rec_h, idx_h, q_sa, q_target = P.update_probe(n, W=W)
    for n_rec in (257, 60):
        rec = torch.from_numpy(rec_h).to(DEV)
        dqn_ops.priority_update_(rec, n_rec, R.O_TD, torch.from_numpy(idx_h).to(DEV), torch.from_numpy(q_sa).to(DEV),
                                 torch.from_numpy(q_target).to(DEV))
        torch.cuda.synchronize()
        want = P.update_ref(rec_h, R.O_TD, idx_h, q_sa, q_target, n_rec=n_rec)
        assert np.array_equal(rec.cpu().numpy().view(np.int64), want.view(np.int64)), (n, W, n_rec)
        assert n_rec < 257 or not np.array_equal(want, rec_h)                               # (below it the one draw of n = 1 may lie outside)
    if n > 1:
        assert not np.array_equal(P.twin_update_first_wins(rec_h, R.O_TD, idx_h, q_sa, q_target), P.update_ref(rec_h, R.O_TD, idx_h, q_sa, q_target))


# ------------------------------------------------------------------------------------------------------------ 5: refusals
def test_sampler_entry_point_refuses_what_the_header_says_it_refuses():
    from bridges_hip import abi, dqn_ops
    L = abi.require_gpu()
    N, W, n = 300, R.RECORD_WIDTH, 16
    td, u_h = P.probe(N, n)
    rec = records(N, W, td)
    u = torch.from_numpy(u_h).to(DEV)
    idx = torch.full((n,), 7, dtype=torch.int64, device=DEV)
    need = dqn_ops.priority_sample_scratch(N)
    scratch = torch.full((need + 1,), -7.0, dtype=torch.float64, device=DEV)
    base = dict(n_rec=N, W=W, col=R.O_TD, rec=_ptr(rec), alpha=0.6, n=n, u=_ptr(u), idx=_ptr(idx), scratch=_ptr(scratch), doubles=need)

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_priority_sample(a["n_rec"], a["W"], a["col"], a["rec"], a["alpha"], a["n"], a["u"], a["idx"], a["scratch"],
                                         a["doubles"], abi.current_stream())
    null, off = C.c_void_p(0), lambda t: C.c_void_p(t.data_ptr() + 4)
    bad = [dict(n_rec=0), dict(n_rec=-1), dict(W=R.O_TD), dict(W=1), dict(col=-1), dict(col=W), dict(alpha=-0.1), dict(alpha=1.0001),
           dict(alpha=float("nan")), dict(rec=null), dict(u=null), dict(idx=null), dict(scratch=null), dict(rec=off(rec)), dict(u=off(u)),
           dict(idx=off(idx)), dict(scratch=off(scratch)), dict(doubles=need - 1), dict(doubles=0), dict(n=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "priority_sample" in L.bridges_last_error().decode(), kw
    torch.cuda.synchronize()
    assert bool((idx == 7).all()) and bool((scratch == -7.0).all())                           # a refusal launches nothing
    assert call(n=0) == 0 and call(n=0, n_rec=0) == 0                                        # nothing to draw is not an error
    torch.cuda.synchronize()
    assert bool((idx == 7).all()) and bool((scratch == -7.0).all())
    for alpha in (0.0, 1.0):                                                                 # the ends of the range are inside it
        assert call(alpha=alpha) == 0
    torch.cuda.synchronize()
    assert P.accept(idx.cpu().numpy(), P.sample_ref(td, 1.0, u_h)) is None and float(scratch[need]) == -7.0
    need_out = C.c_int64(-1)
    assert L.bridges_priority_sample_scratch(-1, C.byref(need_out)) == -1 and L.bridges_priority_sample_scratch(N, None) == -1


def test_update_entry_point_refuses_what_the_header_says_it_refuses():
    from bridges_hip import abi
    L = abi.require_gpu()
    rec_h, idx_h, q_sa_h, q_target_h = P.update_probe(65)
    rec, idx = torch.from_numpy(rec_h).to(DEV), torch.from_numpy(idx_h).to(DEV)
    q_sa, q_target = torch.from_numpy(q_sa_h).to(DEV), torch.from_numpy(q_target_h).to(DEV)
    N, W = rec.shape
    base = dict(n_rec=N, W=W, col=R.O_TD, rec=_ptr(rec), n=65, idx=_ptr(idx), q_sa=_ptr(q_sa), q_target=_ptr(q_target))

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_priority_update(a["n_rec"], a["W"], a["col"], a["rec"], a["n"], a["idx"], a["q_sa"], a["q_target"], abi.current_stream())
    null = C.c_void_p(0)
    bad = [dict(n=-1), dict(n_rec=-1), dict(W=R.O_TD), dict(col=-1), dict(col=W), dict(rec=null), dict(idx=null), dict(q_sa=null),
           dict(q_target=null), dict(rec=C.c_void_p(rec.data_ptr() + 4)), dict(idx=C.c_void_p(idx.data_ptr() + 4)),
           dict(q_sa=C.c_void_p(q_sa.data_ptr() + 2)), dict(q_target=C.c_void_p(q_target.data_ptr() + 2))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "priority_update" in L.bridges_last_error().decode(), kw
    assert call(n=0) == 0 and call(n=0, rec=null, idx=null, q_sa=null, q_target=null) == 0
    torch.cuda.synchronize()
    assert np.array_equal(rec.cpu().numpy().view(np.int64), rec_h.view(np.int64))             # nothing was launched
    assert call(n_rec=0) == 0                                                                # no live row: every index is outside
    torch.cuda.synchronize()
    assert np.array_equal(rec.cpu().numpy().view(np.int64), rec_h.view(np.int64))
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(rec.cpu().numpy().view(np.int64), P.update_ref(rec_h, R.O_TD, idx_h, q_sa_h, q_target_h).view(np.int64))


# ------------------------------------------------------------------------------------------------------------ the ring layer
def test_ring_sample_prioritized_draws_from_the_stream_of_the_torch_path():
    """alpha = 1 is the distribution of sample(prioritized=True): from the same generator state both paths return the same
    records (the probe's priorities without the NaN and the negative row, which only the kernel clamps) and leave the same
    state; the indices are the rows of the records; update_priorities writes O_TD of those rows and nothing else."""
    td, _ = P.probe(257, 1)
    td[[257 // 2, 256]] = (0.5, 0.25)
    ring = R.ReplayRing(300, DEV)
    ring.push(records(257, R.RECORD_WIDTH, td))
    g1, g2 = (torch.Generator(device=DEV).manual_seed(11) for _ in range(2))
    want = ring.sample(64, g1, prioritized=True)
    got, idx = ring.sample_prioritized(64, g2, alpha=1.0)
    assert torch.equal(got, want) and torch.equal(g1.get_state(), g2.get_state())
    assert idx.dtype == torch.int64 and torch.equal(ring.data.index_select(0, idx), got)
    scratch = ring._priority_scratch                                                         # sized once from the capacity, kept
    assert scratch.numel() >= 300
    ring.sample_prioritized(8, g2, 0.5)
    assert ring._priority_scratch is scratch
    before = ring.data.clone()
    q_sa = torch.arange(64, dtype=torch.float32, device=DEV)
    ring.update_priorities(idx, q_sa, torch.zeros(64, device=DEV))
    want = P.update_ref(before.cpu().numpy(), R.O_TD, idx.cpu().numpy(), q_sa.cpu().numpy(), np.zeros(64, dtype=np.float32), n_rec=257)
    assert np.array_equal(ring.data.cpu().numpy().view(np.int64), want.view(np.int64))


# ------------------------------------------------------------------------------------------------------------ 6: the loop
CAPACITY, BATCH, STEPS = 256, 8, 3


def forward_with_bound(net, block, binary, action, reward, obstacle):
    """(q, bound) float64 [n]: the plain forward of a float64 copy of the module on f32 images, and a forward-error bound of a
    float32 evaluation of the same function that sums every dot product in ANY order and may form the head's weight difference
    W[1] - W[0] in float32 first.  The error e of an activation runs through the layers beside its value v: a linear or conv
    layer of fan-in K gives e' = |W| e + dot_bound(K + 1, |W| (|v| + e) + |b|) (gpu_helpers.dot_bound), ReLU and max-pool are
    1-Lipschitz, the sigmoid is 1/4-Lipschitz and adds acting_conformance.sigmoid_allowance."""
    from robotoddler.models.cv import ConvNet, SuccessorMLP
    # (a fresh module with the net's state: a net that has trained holds its captured-step driver, which does not deep-copy)
    if isinstance(net, SuccessorMLP):
        widths = [m.out_features for m in net.mlp.layers if isinstance(m, torch.nn.Linear)]
        twin = SuccessorMLP(img_size=net.img_size, hidden_dims=widths[:-1])
    else:
        assert isinstance(net, ConvNet)
        twin = ConvNet(img_size=(64, 64))
    twin.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    net64 = library_twin(twin.to(DEV)).eval()
    block, binary, action, reward, obstacle = (t.double() for t in (block, binary, action, reward, obstacle))
    n = block.shape[0]
    with torch.no_grad():
        q = net64(block, binary, action, reward, obstacle)[0]

        def linear(v, e, W, b, W_abs=None, b_abs=None, terms=None):
            W_abs, b_abs = (W.abs() if W_abs is None else W_abs), (b.abs() if b_abs is None else b_abs)
            K = (W.shape[1] + 1) if terms is None else terms
            return v @ W.T + b, e @ W_abs.T + dot_bound(K, (v.abs() + e) @ W_abs.T + b_abs)
        if isinstance(net, SuccessorMLP):
            px = 64 * 64
            lin = [m for m in net64.mlp.layers if isinstance(m, torch.nn.Linear)]
            v = torch.cat([torch.cat([block, action, reward, obstacle], dim=1).reshape(n, -1), binary], dim=1)
            e = torch.zeros_like(v)
            for l in lin[:-1]:
                v, e = linear(v, e, l.weight, l.bias)
                v = F.relu(v)
            W, b = lin[-1].weight, lin[-1].bias
            d, e = linear(v, e, W[px:2 * px] - W[:px], b[px:2 * px] - b[:px], W_abs=W[px:2 * px].abs() + W[:px].abs(),
                          b_abs=b[px:2 * px].abs() + b[:px].abs(), terms=2 * W.shape[1] + 4)
            s = torch.sigmoid(d)
            e = 0.25 * e + sigmoid_allowance(d, s)
            w = reward.reshape(n, px)
            got = (s * w).sum(dim=1)
            assert torch.allclose(got, q, rtol=1e-12, atol=1e-12)                            # the factored head IS the module's function
            return q, (w.abs() * e).sum(dim=1) + dot_bound(px, (w.abs() * (s + e)).sum(dim=1))
        v = torch.cat([block, action, reward, obstacle], dim=1)
        e = torch.zeros_like(v)
        for blk in net64.layers:
            for m in blk.layers:
                if isinstance(m, torch.nn.Conv2d):
                    K = 9 * m.in_channels + 1
                    a = F.conv2d(v.abs() + e, m.weight.abs(), m.bias.abs(), padding=1)
                    v, e = F.conv2d(v, m.weight, m.bias, padding=1), F.conv2d(e, m.weight.abs(), None, padding=1) + dot_bound(K, a)
                elif isinstance(m, torch.nn.ReLU):
                    v = F.relu(v)
                else:
                    v, e = F.max_pool2d(v, 2), F.max_pool2d(e, 2)
        v, e = torch.cat([v.reshape(n, -1), binary], dim=1), torch.cat([e.reshape(n, -1), torch.zeros_like(binary)], dim=1)
        lin = [m for m in net64.mlp.layers if isinstance(m, torch.nn.Linear)]
        for i, l in enumerate(lin):
            v, e = linear(v, e, l.weight, l.bias)
            if i < len(lin) - 1:
                v = F.relu(v)
        assert torch.allclose(v[:, 0], q, rtol=1e-12, atol=1e-12)
        return q, e[:, 0]


def transition_images(agent, n):
    """The f32 inputs of the module forward for the transitions of the last _targets call: rasters of s_t and a_t, the binary
    features, and every transition's own reward map and obstacle raster (the task's where the agent has one task)."""
    from bridges_hip import ops
    renv, bits_s, action_bits, stable_s, _bf, _af = agent._transitions
    block = ops.bits_to_f32(bits_s[:n].contiguous()).unsqueeze(1)
    action = ops.bits_to_f32(action_bits[:n].contiguous()).unsqueeze(1)
    binary = torch.zeros((n, 6), device=DEV)
    binary[:, 0] = stable_s[:n].float()
    reward = (renv.reward_maps_img[:n].unsqueeze(1) if agent.per_env_tasks else agent.env.reward_features.unsqueeze(0).expand(n, -1, -1, -1))
    obstacle = (ops.bits_to_f32(renv.env_obstacle_bits[:n].contiguous()).unsqueeze(1) if agent.per_env_obstacles
                else agent.env.obstacle_raster.unsqueeze(0).expand(n, -1, -1, -1))
    assert bool((bits_s[:n] & action_bits[:n] == 0).all()) and bool((action_bits[:n] != 0).any(dim=1).all())   # a_t is a block beside s_t
    return block, binary, action, reward.contiguous(), obstacle.contiguous()


def run_refreshing(agent, locksteps, plant=None):
    """``locksteps`` lock-steps of STEPS optimiser steps each with every refresh checked where it happens: the priorities of
    the sampled rows, the rest of the ring, q_sa against the float64 forward.  -> the number of refreshes."""
    n = STEPS * BATCH
    seen = []
    ring, inner_update, inner_targets = agent.ring, agent.ring.update_priorities, agent._targets

    def targets(rec):
        out = inner_targets(rec)
        seen.append(("targets", out[3]))
        return out

    def update(idx, q_sa, q_target):
        assert seen and seen[-1][0] == "targets" and q_target is seen[-1][1]                  # the vector _targets returned
        assert idx.shape == q_sa.shape == q_target.shape == (n,) and q_sa.dtype == torch.float32
        before = ring.data.clone()
        q64, bound = forward_with_bound(agent.policy_net, *transition_images(agent, n))
        err = (q_sa.double() - q64).abs()
        print("q_sa: max |error|", float(err.max()), "max error / bound", float((err / bound).max()))
        assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))
        # the worst-case bound is wide (fan-ins of 16 k terms, conv stacks): also the tolerance the suite holds _net_q to against
        # the module forward (test_gpu_vec_dqn_tasks.py::test_acting_forward_with_a_map_per_env) -- the refresh runs that forward.
        # Printed beside it: how far the q of the sampled transitions lie apart (the freshly initialised SuccessorMLP: 3e-4 to
        # 7e-4, above the tolerance; the ConvNet: 4e-5, and 0 where every draw is the planted row)
        assert torch.allclose(q_sa.double(), q64, rtol=1e-5, atol=1e-5), float(err.max())
        print("q of neighbouring transitions differs by up to", float((q64 - q64.roll(1)).abs().max()))
        inner_update(idx, q_sa, q_target)
        torch.cuda.synchronize()
        want = P.update_ref(before.cpu().numpy(), R.O_TD, idx.cpu().numpy(), q_sa.cpu().numpy(), q_target.cpu().numpy(), n_rec=ring.size)
        assert np.array_equal(ring.data.cpu().numpy().view(np.int64), want.view(np.int64))   # sampled rows refreshed, the rest as it was
        rows = idx.cpu().tolist()
        last = {r: j for j, r in enumerate(rows)}
        td = ring.data[:, R.O_TD].cpu()
        diff = (q_sa - q_target).abs().double().cpu()
        assert all(td[r] == diff[j] for r, j in last.items()) and 0 <= min(rows) and max(rows) < ring.size
        seen.append(("update", set(rows)))
    ring.update_priorities, agent._targets = update, targets
    try:
        for it in range(locksteps):
            if plant is not None and it == locksteps - 1:
                assert ring.size > plant
                ring.data[plant, R.O_TD] = 1e6
            agent.lockstep(STEPS)
    finally:
        del ring.update_priorities, agent._targets
    torch.cuda.synchronize()
    updates = [s[1] for s in seen if s[0] == "update"]
    if plant is not None:
        assert plant in updates[-1] and 0.0 <= float(ring.data[plant, R.O_TD]) < 1e3          # drawn, and refreshed
    return len(updates)


def refreshing_mlp(env, **kw):
    from robotoddler.training.vec_dqn import VecDQN
    pol, tgt = make_mlp(HIDDEN, seed=0), make_mlp(HIDDEN, seed=0)
    kw = dict(dict(prioritized=True, priority_alpha=0.6, priority_refresh=True), **kw)
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, CAPACITY, BATCH, GAMMA, 0.01,
                  "mse_q_values+mse_block_features", seed=3, **kw)


def test_loop_refreshes_the_sampled_rows_and_a_planted_outlier():
    """16 envs on the tower of height 2, the factored SuccessorMLP: every refresh checked; a row planted with O_TD = 1e6 before
    the last lock-step is drawn in it (fixed seeds; it holds nearly all of the mass) and holds its refreshed value afterwards."""
    agent = refreshing_mlp(tower_env(16, f32_rasters=False))
    assert run_refreshing(agent, 4, plant=5) >= 3
    assert agent.ring.width == R.RECORD_WIDTH and agent.ring.capacity == CAPACITY


def test_loop_refresh_with_three_step_returns():
    agent = refreshing_mlp(tower_env(16, f32_rasters=False), n_step=3)
    assert run_refreshing(agent, 6) >= 2 and agent.ring.width == R.RECORD_WIDTH + 1


def test_loop_refresh_with_double_q():
    assert run_refreshing(refreshing_mlp(tower_env(16, f32_rasters=False), double_q=True), 4) >= 3


def test_loop_refresh_on_per_env_tasks_and_obstacles():
    agent = refreshing_mlp(random_env(16), per_env_tasks=True, per_env_obstacles=True)
    assert run_refreshing(agent, 4) >= 3 and agent.ring.width == R.RECORD_WIDTH + 12


def test_loop_refresh_with_a_convnet_on_task_channels():
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    tgt.load_state_dict(pol.state_dict())
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), random_env(16, T=3, O=0), CAPACITY, BATCH, GAMMA, 0.01,
                   "mse_q_values", seed=3, per_env_tasks=True, task_channels=True, prioritized=True, priority_alpha=0.6, priority_refresh=True)
    assert run_refreshing(agent, 4) >= 3


def test_loop_refresh_with_a_convnet_on_f32_rasters():
    """The conv net without task channels: the module forward over the f32 images _targets built."""
    from robotoddler.models.cv import ConvNet
    from robotoddler.training.vec_dqn import VecDQN
    from robotoddler.utils.utils import init_weights
    nets = []
    for _ in range(2):
        torch.manual_seed(0)
        net = ConvNet(img_size=(64, 64)).to(DEV)
        net.apply(init_weights)
        nets.append(net)
    agent = VecDQN(nets[0], nets[1], torch.optim.Adam(nets[0].parameters(), lr=1e-4, fused=True), tower_env(16, f32_rasters=True), CAPACITY,
                   BATCH, GAMMA, 0.01, "mse_q_values", seed=3, prioritized=True, priority_alpha=0.6, priority_refresh=True)
    assert run_refreshing(agent, 4) >= 3


# ------------------------------------------------------------------------------------------------------------ 7: opt-in
def test_defaults_are_the_loop_it_was():
    """VecDQN(prioritized=True) and the same with priority_alpha=1.0, priority_refresh=False spelled out: 4 lock-steps end with
    bit-identical losses, weights and rings, and neither reaches the new ring methods."""
    def run(**kw):
        from robotoddler.training.vec_dqn import VecDQN
        pol, tgt = make_mlp(HIDDEN, seed=0), make_mlp(HIDDEN, seed=0)
        agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), tower_env(16, f32_rasters=False), CAPACITY, BATCH,
                       GAMMA, 0.01, "mse_q_values+mse_block_features", seed=3, prioritized=True, **kw)

        def raising(*a, **k):
            raise AssertionError("a new ring method was reached")
        agent.ring.sample_prioritized = agent.ring.update_priorities = raising
        losses = []
        for _ in range(4):
            losses += agent.lockstep(STEPS)[0]
        torch.cuda.synchronize()
        return agent, losses
    a, la = run()
    b, lb = run(priority_alpha=1.0, priority_refresh=False)
    assert la == lb and len(la) >= 2 * STEPS and a.ring.size == b.ring.size > 0 and torch.equal(bits(a.ring.data), bits(b.ring.data))
    assert a.ring._priority_scratch is None and float(a.ring.data[:a.ring.size, R.O_TD].abs().sum()) > 0
    for net in ("policy_net", "target_net"):
        for p, q in zip(getattr(a, net).parameters(), getattr(b, net).parameters()):
            assert torch.equal(p, q)


def test_sampler_alone_changes_the_draw_not_the_ring():
    """priority_alpha = 0.5 without the refresh: the loop draws through the kernel (other batches than alpha = 1 draws), and the
    priorities in the ring stay the rollout's."""
    agent = refreshing_mlp(tower_env(16, f32_rasters=False), priority_alpha=0.5, priority_refresh=False)
    calls, inner = [], agent.ring.sample_prioritized

    def sample(n, gen, alpha):
        before = bits(agent.ring.data).clone()
        out = inner(n, gen, alpha)
        calls.append(alpha)
        assert torch.equal(bits(agent.ring.data), before)
        return out
    agent.ring.sample_prioritized = sample
    agent.ring.update_priorities = lambda *a: (_ for _ in ()).throw(AssertionError("no refresh was asked for"))
    losses = []
    for _ in range(4):
        losses += agent.lockstep(STEPS)[0]
    assert len(calls) >= 3 and set(calls) == {0.5} and all(np.isfinite(losses)) and agent._transitions is None
