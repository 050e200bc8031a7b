"""GPU: the importance-sampling weights of prioritised replay -- the weights kernel (bridges_priority_weights) and the weighted
SuccessorMLP loss (bridges_successor_loss_weighted) against tests/is_weight_ref.py (checked without a GPU by
tests/test_cpu_is_weights.py, which also shows that the defective twins are rejected), the weighted optimiser step in its two
bodies, and VecDQN(prioritized=True, priority_beta=...): beta = 0 bit for bit the loop without the option, beta = 0.4 captured
against eager, the option beside the refresh, n-step returns and double Q-learning, and the annealing clock through a checkpoint."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import is_weight_ref as W
import mlp_conformance as M
import priority_ref as P
from robotoddler.training import records as R
from test_gpu_double_q import conv_agent, mlp_agent, random_env, tower_env
from test_gpu_mlp_step import make_batch, make_net, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.25


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def bits32(t):
    return t.contiguous().view(torch.int32)


def bits64(t):
    return t.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------------------ 1: the weights kernel
def ring_of(td):
    """rec [N, RECORD_WIDTH] on the device with ``td`` in the priority column, and a scratch for the sampler."""
    from bridges_hip import dqn_ops
    N = len(td)
    rec = torch.zeros((N, R.RECORD_WIDTH), dtype=torch.float64, device=DEV)
    rec[:, R.O_TD] = torch.from_numpy(np.asarray(td, dtype=np.float64)).to(DEV)
    return rec, torch.empty(dqn_ops.priority_sample_scratch(N), dtype=torch.float64, device=DEV)


def check_weights_case(td, alpha, beta, B, n_steps, u):
    from bridges_hip import dqn_ops
    N, case = len(td), (len(td), alpha, beta, B, n_steps)
    rec, scratch = ring_of(td)
    idx = dqn_ops.priority_sample(rec, N, R.O_TD, alpha, torch.from_numpy(u).to(DEV), scratch)
    before = scratch.clone()
    w = dqn_ops.priority_weights(idx, N, B, beta, scratch)
    again = dqn_ops.priority_weights(idx, N, B, beta, scratch)
    assert w.dtype == torch.float32 and w.shape == (B * n_steps,)
    assert torch.equal(bits32(w), bits32(again)), case                                       # two calls: identical bits
    assert torch.equal(bits64(scratch), bits64(before)), case                                # the scratch is only read
    idx_h, w_h = idx.cpu().numpy(), w.cpu().numpy()
    m = P.masses(td, alpha)
    ref = W.weights_ref(m, idx_h, B, beta)
    msg = W.accept_weights(w_h, ref)
    assert msg is None, (case, msg)
    assert np.isfinite(w_h).all() and (w_h > 0).all() and (w_h <= 1).all(), case
    assert (w_h.reshape(n_steps, B).max(axis=1) == np.float32(1.0)).all(), case              # every batch's maximum: exactly 1
    if beta == 0.0 or alpha == 0.0:
        assert (w_h == np.float32(1.0)).all(), case
    for lo in range(0, B * n_steps, B):                                                      # equal rows of a batch: equal bits
        seen = {}
        for j in range(lo, lo + B):
            assert seen.setdefault(int(idx_h[j]), w_h[j].tobytes()) == w_h[j].tobytes(), case
        if N > 3 and alpha > 0.0 and beta > 0.0 and N // 3 in seen:                          # the planted 1e6: the smallest weight
            assert np.frombuffer(seen[N // 3], dtype=np.float32)[0] == w_h[lo:lo + B].min(), case
    if B >= 32 and N > 1:
        # a planted -1 and a planted n_rec: weight 0, and their batch as the reference computed without them
        planted = idx_h.copy()
        planted[1], planted[B - 2] = -1, N
        wp = dqn_ops.priority_weights(torch.from_numpy(planted).to(DEV), N, B, beta, scratch).cpu().numpy()
        assert wp[1] == 0.0 and wp[B - 2] == 0.0, case
        msg = W.accept_weights(wp, W.weights_ref(m, planted, B, beta))
        assert msg is None, (case, msg)
        keep = np.ones(B, dtype=bool)
        keep[[1, B - 2]] = False
        msg = W.accept_weights(wp[:B][keep], W.weights_ref(m, idx_h[:B][keep], B - 2, beta))
        assert msg is None, (case, msg)
        assert np.array_equal(wp[B:], w_h[B:]), case                                         # the other batches: untouched
    return idx_h


@pytest.mark.parametrize("N", W.W_N)
def test_weights_kernel_on_the_probe(N):
    drawn_outlier = 0
    for alpha in W.W_ALPHA:
        for beta in W.W_BETA:
            for B, n_steps in W.W_BATCHES:
                td, u = P.probe(N, B * n_steps)
                idx = check_weights_case(td, alpha, beta, B, n_steps, u)
                drawn_outlier += int(N > 3 and (idx == N // 3).any())
    assert N <= 3 or drawn_outlier > 0                                                       # the outlier's claim was exercised


def test_weights_kernel_with_an_infinite_priority():
    """A +inf row counts as 1e30: its weight is tiny and finite, the batch's maximum stays exactly 1."""
    for alpha in W.W_ALPHA:
        for beta in W.W_BETA:
            td, u = P.probe(257, 96)
            td[7] = np.inf
            u[5] = 0.5                                                                       # lands on the row that holds the mass
            idx = check_weights_case(td, alpha, beta, 32, 3, u)
            assert alpha == 0.0 or (idx == 7).any()


def test_weights_describe_the_draw_not_the_refreshed_column():
    """update_priorities between the draw and the weights changes the record column, not the masses in the scratch; the ring
    layer reads its own scratch and refuses before the first draw."""
    ring = R.ReplayRing(300, DEV)
    td, _ = P.probe(257, 64)
    rec = torch.zeros((257, R.RECORD_WIDTH), dtype=torch.float64)
    rec[:, R.O_TD] = torch.from_numpy(td)
    ring.push(rec.to(DEV))
    with pytest.raises(RuntimeError, match="sample_prioritized has not run"):
        ring.sample_weights(torch.zeros(8, dtype=torch.int64, device=DEV), 8, 0.4)
    gen = torch.Generator(device=DEV).manual_seed(3)
    _, idx = ring.sample_prioritized(64, gen, 0.6)
    w = ring.sample_weights(idx, 32, 0.4)
    ring.update_priorities(idx, torch.full((64,), 5.0, device=DEV), torch.zeros(64, device=DEV))
    assert float(ring.data[int(idx[0]), R.O_TD]) == 5.0
    assert torch.equal(bits32(ring.sample_weights(idx, 32, 0.4)), bits32(w))
    assert W.accept_weights(w.cpu().numpy(), W.weights_ref(P.masses(td, 0.6), idx.cpu().numpy(), 32, 0.4)) is None


def test_weights_entry_point_refuses_what_the_header_says_it_refuses():
    from bridges_hip import abi, dqn_ops
    L = abi.require_gpu()
    N, B, n = 300, 8, 24
    td, u = P.probe(N, n)
    rec, scratch = ring_of(td)
    idx = dqn_ops.priority_sample(rec, N, R.O_TD, 0.6, torch.from_numpy(u).to(DEV), scratch)
    need = scratch.numel()
    weight = torch.full((n,), SENTINEL, device=DEV)
    base = dict(n_rec=N, n=n, batch=B, idx=_ptr(idx), beta=0.4, scratch=_ptr(scratch), doubles=need, weight=_ptr(weight))

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_priority_weights(a["n_rec"], a["n"], a["batch"], a["idx"], a["beta"], a["scratch"], a["doubles"], a["weight"],
                                          abi.current_stream())
    null, off = C.c_void_p(0), lambda t, by=4: C.c_void_p(t.data_ptr() + by)
    bad = [dict(n=-1), dict(n_rec=0), dict(n_rec=-1), dict(batch=0), dict(batch=-8), dict(batch=7), dict(batch=16), dict(beta=-0.1),
           dict(beta=1.0001), dict(beta=float("nan")), dict(idx=null), dict(scratch=null), dict(weight=null), dict(idx=off(idx)),
           dict(scratch=off(scratch)), dict(weight=off(weight, 2)), dict(doubles=need - 1), dict(doubles=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "priority_weights" in L.bridges_last_error().decode(), kw
    torch.cuda.synchronize()
    assert bool((weight == SENTINEL).all())                                                  # a refusal launches nothing
    assert call(n=0) == 0 and call(n=0, n_rec=0, batch=0) == 0                               # nothing to weigh is not an error
    torch.cuda.synchronize()
    assert bool((weight == SENTINEL).all())
    for beta in (0.0, 1.0):                                                                  # the ends of the range are inside it
        assert call(beta=beta) == 0
    assert call(batch=n) == 0 and call(batch=1) == 0 and call() == 0
    torch.cuda.synchronize()
    assert W.accept_weights(weight.cpu().numpy(), W.weights_ref(P.masses(td, 0.6), idx.cpu().numpy(), B, 0.4)) is None


# ------------------------------------------------------------------------------------------------------------ 2: the weighted loss
def lib():
    from bridges_hip import abi
    return abi.require_gpu()


def call(name, *args):
    from bridges_hip import abi
    abi.check(getattr(lib(), name)(*args), name)


def stream():
    from bridges_hip import abi
    return abi.current_stream()


def word(v, dtype=torch.int64):
    return torch.tensor(v, dtype=dtype, device=DEV)


def run_loss(shape, pr, counter, w_all=None, losses=None, n_losses=0, counter_inc=None, ticket=None, adam_step=None):
    """bridges_successor_loss_weighted with ``w_all``; None: the unweighted entry point of the shape."""
    batch, px, nf, use_q, use_sf, per_row = shape
    rows, N = M.rows_of(batch), 2 * px + 2 * nf
    dy, loss_rows, q_out = (torch.full(s, math.nan, device=DEV) for s in ((rows, N), (rows,), (rows,)))
    head = (batch, rows, px, nf, _ptr(pr["y"]), _ptr(pr["reward"]))
    tail = (_ptr(counter), _ptr(pr["q_t"] if use_q else None), _ptr(pr["sf_t"] if use_sf else None), int(use_q), int(use_sf), _ptr(dy),
            _ptr(loss_rows), _ptr(q_out), _ptr(losses), n_losses, _ptr(counter_inc), _ptr(ticket), _ptr(adam_step))
    if w_all is not None:
        call("bridges_successor_loss_weighted", *head, px if per_row else 0, *tail, _ptr(w_all), stream())
    elif per_row:
        call("bridges_successor_loss_rows", *head, px, *tail, stream())
    else:
        call("bridges_successor_loss", *head, *tail, stream())
    return dict(q=q_out, loss_rows=loss_rows, dy=dy)


def row_order_sum(loss_rows, batch):
    total = np.float32(0.0)
    for v in loss_rows[:batch].cpu().numpy():
        total = np.float32(total + v)
    return float(total)


@pytest.mark.parametrize("shape", W.LOSS_ROWS)
def test_weighted_loss_inside_the_bound(shape):
    batch, px, nf, use_q, use_sf, per_row = shape
    pr = M.loss_probe(batch, px, nf, per_row, DEV)
    w_all, ones = W.loss_weights(batch, DEV), torch.ones(M.LOSS_BATCHES * batch, device=DEV)
    for c in W.LOSS_COUNTERS:
        w = w_all[c * batch:(c + 1) * batch]
        refs = W.weighted_loss_ref(w, pr["y"], *M.loss_batch(pr, batch, px, c), batch, px, nf, use_q, use_sf)
        got = run_loss(shape, pr, word(c), w_all)
        for k in ("q", "loss_rows", "dy"):
            W.inside(f"weighted_loss.{k}.c{c}", got[k], *refs[k], shape)
        # every weight 1: the bits of the unweighted kernel; q is the unweighted q whatever the weights
        plain, unit = run_loss(shape, pr, word(c)), run_loss(shape, pr, word(c), ones)
        for k in ("q", "loss_rows", "dy"):
            assert torch.equal(bits32(unit[k]), bits32(plain[k])), (shape, c, k)
        assert torch.equal(bits32(got["q"]), bits32(plain["q"]))
        # a row of weight 0: an all-zero gradient row and loss 0; padding rows stay zero
        for b in torch.nonzero(w == 0).flatten().tolist():
            assert float(got["dy"][b].abs().max()) == 0.0 and float(got["loss_rows"][b]) == 0.0
        assert bool((got["dy"][batch:] == 0).all()) and bool((got["loss_rows"][batch:] == 0).all()) and bool((got["q"][batch:] == 0).all())


def test_weighted_loss_refuses_a_missing_weight():
    from bridges_hip import abi
    shape = W.LOSS_ROWS[0]
    batch, px, nf, use_q, use_sf, per_row = shape
    pr = M.loss_probe(batch, px, nf, per_row, DEV)
    with pytest.raises(abi.BridgesHipError, match="weight missing"):
        run_loss(shape, pr, word(0), w_all=_NullTensor())


class _NullTensor:
    """Stands in for a tensor whose pointer is NULL."""
    def data_ptr(self):
        return 0


def test_weighted_loss_logs_the_weighted_rows_through_the_ticket():
    """The ticket form: the last row workgroup to arrive logs the in-order float32 sum of the WEIGHTED rows, advances counter
    and step and re-arms the ticket."""
    shape = W.LOSS_ROWS[1]                                                                   # (7, 64, 6, sf only, per row)
    batch, px, nf, use_q, use_sf, per_row = shape
    pr = M.loss_probe(batch, px, nf, per_row, DEV)
    w_all = W.loss_weights(batch, DEV)
    sums = [row_order_sum(run_loss(shape, pr, word(c), w_all)["loss_rows"], batch) for c in range(3)]
    unweighted = [row_order_sum(run_loss(shape, pr, word(c))["loss_rows"], batch) for c in range(3)]
    assert all(s < u for s, u in zip(sums, unweighted))
    counter, losses = word(0), torch.full((3,), SENTINEL, device=DEV)
    ticket, adam_step = word(0, torch.int32), torch.zeros((), device=DEV)
    for c in range(3):
        run_loss(shape, pr, counter, w_all, losses=losses, n_losses=3, counter_inc=counter, ticket=ticket, adam_step=adam_step)
        assert float(losses[c]) == sums[c] and int(counter) == c + 1 and float(adam_step) == c + 1.0 and int(ticket) == 0
    assert losses.tolist() == sums


def test_weighted_loss_logs_the_weighted_rows_through_the_head_backward():
    """The form the step uses: the loss kernel hands nothing on, bridges_linear_backward_log sums the weighted rows in order."""
    shape = W.LOSS_ROWS[0]                                                                   # (1, 64, 0, q and sf, one map)
    batch, px, nf, use_q, use_sf, per_row = shape
    rows, N, K = M.rows_of(batch), 2 * px + 2 * nf, 32
    pr = M.loss_probe(batch, px, nf, per_row, DEV)
    w_all = torch.tensor([0.625, 1.0, 0.25], device=DEV)                                      # batch 1: one weight per batch
    g = torch.Generator().manual_seed(9)
    a_in, weight = torch.randn((rows, K), generator=g).to(DEV), torch.randn((N, K), generator=g).to(DEV)
    dW, db = torch.empty((N, K), device=DEV), torch.empty(N, device=DEV)
    counter, losses, adam_step = word(0), torch.full((3,), SENTINEL, device=DEV), torch.zeros((), device=DEV)
    want = []
    for c in range(3):
        got = run_loss(shape, pr, counter, w_all)
        want.append(row_order_sum(got["loss_rows"], batch))
        plain = run_loss(shape, pr, counter)
        assert float(got["loss_rows"][0]) == float(np.float32(w_all[c].item()) * np.float32(plain["loss_rows"][0].item()))
        call("bridges_linear_backward_log", rows, K, N, _ptr(got["dy"]), _ptr(a_in), _ptr(weight), _ptr(dW), _ptr(db), None, None, None, 0,
             _ptr(got["loss_rows"]), batch, _ptr(losses), 3, _ptr(counter), _ptr(adam_step), stream())
        assert int(counter) == c + 1 and float(adam_step) == c + 1.0
    assert losses.tolist() == want and bool(torch.isfinite(dW).all())


# ------------------------------------------------------------------------------------------------------------ 3: the step
def step_weights(n, seed=0):
    g = torch.Generator().manual_seed(600 + seed)
    w = 1.0 - torch.rand(n, generator=g) * 0.96875
    w[0], w[1] = 1.0, 0.0
    return w.float().to(DEV)


def test_hand_written_step_with_weights_follows_the_autograd_body(monkeypatch):
    """One optimiser step (forward, weighted loss, backward, Adam) of the hand-written body against the autograd body of the same
    driver class with the same weights, on identically seeded nets: the tolerances of
    test_gpu_mlp_step.test_three_adam_steps_follow_the_autograd_run for that pair unweighted.  The unweighted step on the same
    batch differs from both."""
    from robotoddler.training import train_step as T
    from robotoddler.training.successor_dqn import flatten_nets
    B, size, parts = 32, 64, ["mse_q_values", "mse_block_features"]
    px = size * size
    block, action, binary, reward, obstacle, q_t, sf_t = make_batch(B, size, seed=11)
    w = step_weights(B)
    out = {}
    for fused_env, weights in (("1", True), ("0", True), ("1", False)):
        monkeypatch.setenv("BRIDGES_FUSED_MLP_STEP", fused_env)
        net = make_net(seed=3)
        flatten_nets(net)                                                                    # as make_nets leaves a policy net
        opt = torch.optim.Adam(net.parameters(), lr=1e-3, fused=True)
        fused = T.fused_step_enabled(net, parts)
        assert fused == (fused_env == "1")
        drv = T.CapturedTrainStep(net, opt, B, parts, (size, size), fused, eager_body=fused, warmup=1, weights=weights)
        assert drv.key[4] is weights
        drv._build(1)
        if fused:                                                                            # the warm-up call: the body's launches queued eagerly
            losses = drv.run(1, block.reshape(B, px), action.reshape(B, px), binary, reward.reshape(px).contiguous(),
                             obstacle.reshape(px).contiguous(), q_t, sf_t, **(dict(weights=w) if weights else {}))
        else:
            for dst, src in ((drv.block, block), (drv.action, action), (drv.binary, binary), (drv.reward, reward), (drv.obstacle, obstacle),
                             (drv.q, q_t), (drv.sf, sf_t), (drv.w, w)):
                T._put(dst, src)
            drv._autograd_body()
            losses = drv.losses[:1]
        torch.cuda.synchronize()
        drv.sync()
        out[(fused_env, weights)] = (float(losses[0]), [p.detach().clone() for p in net.parameters()])
    (la, pa), (lb, pb), (lc, pc) = out[("1", True)], out[("0", True)], out[("1", False)]
    np.testing.assert_allclose(la, lb, rtol=2e-5)
    for a, b in zip(pa, pb):
        assert rel_err(a, b) < 2e-4
    assert lc > la and any(not torch.equal(a, c) for a, c in zip(pa, pc))                    # the weights reached the step


# ------------------------------------------------------------------------------------------------------------ 4: the loop
STEPS, LOCKSTEPS = 3, 6                                      # two warm-up calls (eager), then four lock-steps on the captured step


def _conv_task_agent(env, **kw):
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    from test_gpu_double_q import GAMMA
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    tgt.load_state_dict(pol.state_dict())
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 4096, 8, GAMMA, 0.01, "mse_q_values", seed=3,
                  per_env_tasks=True, task_channels=True, **kw)


AGENTS = dict(mlp=(mlp_agent, lambda: tower_env(16, f32_rasters=False)), conv=(conv_agent, lambda: tower_env(16, f32_rasters=True)),
              conv_task=(_conv_task_agent, lambda: random_env(16, T=3, O=0)))


@functools.lru_cache(maxsize=None)
def loop_run(kind, graph, fused, beta):
    """LOCKSTEPS lock-steps of 16 envs on the tower of height 2, B = 8, STEPS optimiser steps each, priority_alpha = 0.6 ->
    (losses, flat policy parameters, ring bits, whether a graph was captured, weights handed to the step), computed once."""
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("BRIDGES_TRAIN_GRAPH", graph)
        mp.setenv("BRIDGES_FUSED_MLP_STEP", fused)
        make, env = AGENTS[kind]
        kw = {} if beta is None else dict(priority_beta=beta)
        agent = make(env(), prioritized=True, priority_alpha=0.6, **kw)
        handed, inner = [], agent.ring.sample_weights
        agent.ring.sample_weights = lambda idx, batch, b: handed.append(inner(idx, batch, b)) or handed[-1]
        losses = []
        for _ in range(2 * LOCKSTEPS):                       # (a lock-step before the ring holds a batch trains nothing)
            if len(losses) < STEPS * LOCKSTEPS:
                losses += agent.lockstep(STEPS)[0]
        torch.cuda.synchronize()
        drv = agent.policy_net._fused_trainer
        return dict(losses=np.array(losses), params=torch.cat([p.detach().flatten() for p in agent.policy_net.parameters()]).cpu(),
                    ring=bits64(agent.ring.data).cpu(), size=agent.ring.size, captured=agent._graph_state is not None,
                    weights=[h.cpu() for h in handed], conv_rows=bool(drv.conv_rows) if drv is not None else None,
                    key=drv.key[4] if drv is not None else None)
    finally:
        mp.undo()


def test_loop_with_beta_zero_is_the_loop_without_the_option_bit_for_bit():
    """All weights are 1 and multiplying by 1 is exact: the parameters and the ring of priority_beta = 0 are those of
    priority_alpha = 0.6 alone, through the eager warm-up and the captured hand-written step."""
    plain, zero = loop_run("mlp", "1", "1", None), loop_run("mlp", "1", "1", 0.0)
    assert plain["captured"] and zero["captured"] and plain["key"] is False and zero["key"] is True
    assert plain["weights"] == [] and len(zero["weights"]) == LOCKSTEPS and all(bool((w == 1).all()) for w in zero["weights"])
    assert len(plain["losses"]) == STEPS * LOCKSTEPS
    assert torch.equal(plain["params"].view(torch.int32), zero["params"].view(torch.int32))
    assert plain["size"] == zero["size"] > 0 and torch.equal(plain["ring"], zero["ring"])


def check_captured_against_eager(a, b, conv):
    """The tolerance of test_gpu_vec_dqn.test_graph_captured_train_step_equals_eager."""
    assert a["captured"] and not b["captured"] and len(a["losses"]) == len(b["losses"]) == STEPS * LOCKSTEPS
    assert (a["losses"] >= 0).all() and np.isfinite(a["losses"]).all()
    np.testing.assert_allclose(a["losses"], b["losses"], rtol=1e-4, atol=1e-6)
    assert torch.allclose(a["params"], b["params"], rtol=1e-4, atol=15 * 1e-4 if conv else 1e-6), float((a["params"] - b["params"]).abs().max())
    for w in a["weights"]:
        assert w.shape == (STEPS * 8,) and bool((w > 0).all()) and bool((w.view(STEPS, 8).max(dim=1).values == 1).all())


def test_loop_with_beta_trains_other_weights_captured_as_eager():
    """priority_beta = 0.4: other parameters than the run without it; the captured autograd step against the eager one (the pair
    the existing tolerance was set for), and the captured hand-written step against the captured autograd step on the first
    captured lock-step, up to which both runs are the same bits (test_gpu_vec_dqn's tolerance for that pair)."""
    plain, hand = loop_run("mlp", "1", "1", None), loop_run("mlp", "1", "1", 0.4)
    assert hand["captured"] and hand["key"] is True and not torch.equal(plain["params"], hand["params"])
    assert any(bool((w < 1).any()) for w in hand["weights"])
    captured, eager = loop_run("mlp", "1", "0", 0.4), loop_run("mlp", "0", "0", 0.4)
    check_captured_against_eager(captured, eager, conv=False)
    first = slice(2 * STEPS, 3 * STEPS)
    assert np.array_equal(hand["losses"][:2 * STEPS], captured["losses"][:2 * STEPS])      # the eager warm-up: the same bits
    np.testing.assert_allclose(hand["losses"][first], captured["losses"][first], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("kind", ["conv", "conv_task"])
def test_convnet_loop_with_beta_captured_as_eager(kind):
    """The conv nets' autograd body with the weights (task_channels: on the rows ops.conv_input builds), captured against eager."""
    captured, eager = loop_run(kind, "1", "1", 0.4), loop_run(kind, "0", "1", 0.4)
    check_captured_against_eager(captured, eager, conv=True)
    assert captured["key"] is True and captured["conv_rows"] == (kind == "conv_task")
    assert any(bool((w < 1).any()) for w in captured["weights"])


def test_loop_with_beta_beside_refresh_three_step_returns_and_double_q():
    agent = mlp_agent(tower_env(16, f32_rasters=False), prioritized=True, priority_alpha=0.6, priority_beta=0.4, priority_refresh=True,
                      n_step=3, double_q=True)
    losses = []
    for _ in range(8):
        losses += agent.lockstep(STEPS)[0]
    assert len(losses) >= 4 * STEPS and all(np.isfinite(losses)) and min(losses) >= 0.0
    assert agent._graph_state is not None and agent.priority_beta_calls == len(losses) // STEPS


def test_annealing_continues_through_a_checkpoint(tmp_path):
    """A run resumed from save_extra / load_extra mid-anneal hands the sampler's weights the beta_now of the uninterrupted run."""
    def agent_of():
        a = mlp_agent(tower_env(16, f32_rasters=False), prioritized=True, priority_alpha=0.6, priority_beta=0.4, priority_beta_anneal=10)
        seen, inner = [], a.ring.sample_weights
        a.ring.sample_weights = lambda idx, batch, beta: seen.append(beta) or inner(idx, batch, beta)
        return a, seen
    whole, seen_whole = agent_of()
    for _ in range(4):
        whole.lockstep(STEPS)
    before = len(seen_whole)
    assert before >= 2 and whole.priority_beta_calls == before
    whole.save_extra(str(tmp_path / "agent.pt"), lockstep=4)
    whole.ring.save(str(tmp_path / "ring.pt"))
    resumed, seen_resumed = agent_of()
    assert resumed.load_extra(str(tmp_path / "agent.pt")) == {"lockstep": 4}
    resumed.ring.load(str(tmp_path / "ring.pt"))
    for a in (whole, resumed):
        a.lockstep(STEPS)
    assert seen_whole == [0.4 + 0.6 * k / 10 for k in range(before + 1)] and seen_resumed == seen_whole[before:]
    assert "priority_beta_calls" in torch.load(str(tmp_path / "agent.pt"), weights_only=True)
