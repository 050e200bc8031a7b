"""GPU: n-step returns of the vectorised DQN (VecDQN(n_step=n)) -- the fold of one-step records into h-step records
(bridges_nstep_fold), the discounted sum of block rasters (bridges_bits_discounted_sum), the TD target with a discount per transition
(bridges_td_target_rows) and the loop that uses them.  References, bounds, probes and scripts come from tests/nstep_ref.py (checked
without a GPU by tests/test_cpu_nstep.py, which also shows that the defective twins are rejected); the loop is compared with the
one-step loop of the same seed."""
import ctypes as C
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import nstep_ref as N
from gpu_helpers import U32
from mlp_conformance import td_probe
from robotoddler.training import records as R
from test_gpu_vec_dqn_tasks import PKG, ROOT, WORKER, make_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.8


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ------------------------------------------------------------------------------------------------------------ 1: the fold
def window_state(rows, n):
    return (torch.zeros(rows, dtype=torch.int32, device=DEV),
            *(torch.zeros((rows, n), dtype=torch.float64, device=DEV) for _ in range(4)))


@pytest.mark.parametrize("W", [R.RECORD_WIDTH, R.RECORD_WIDTH + 3, R.RECORD_WIDTH + 9])
@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("E", [5, 70, 300])
def test_fold_on_scripted_episodes(E, n, W):
    """E below one workgroup's four envs + 1, across a workgroup, across several; the script of nstep_ref.episode_script (an episode
    that ends on its first step, one of exactly n steps, one of n + 2, reset-only lock-steps between episodes, back-to-back episodes)
    with the envs out of phase.  out_valid, the emission order, h and every copied column exact; G within 2 h 2^-53 sum |gamma^k lin_k|
    of the direct sum; the window state after the last lock-step holds what the reference still has pending."""
    from bridges_hip import dqn_ops
    ref = N.RefWindow(E, n, GAMMA)
    state = window_state(E, n)
    for t, (rec, valid) in enumerate(N.scripted_records(E, n, W)):
        out, out_valid = dqn_ops.nstep_fold(torch.from_numpy(rec).to(DEV), torch.from_numpy(valid).to(DEV), GAMMA, n, *state)
        assert tuple(out.shape) == (E * n, W + 1) and out.dtype == torch.float64 and out_valid.dtype == torch.bool
        N.check_fold(out.cpu().numpy(), out_valid.cpu().numpy(), *ref.fold(rec, valid), name=f"lock-step {t}")
    assert state[0].cpu().tolist() == [len(p) for p in ref.pending]
    assert max(state[0].cpu().tolist()) <= n - 1


def test_fold_with_n_1_is_the_identity():
    from bridges_hip import dqn_ops
    E, W = 9, R.RECORD_WIDTH + 3
    state = window_state(E, 1)
    for rec, valid in N.scripted_records(E, 1, W):
        out, out_valid = dqn_ops.nstep_fold(torch.from_numpy(rec).to(DEV), torch.from_numpy(valid).to(DEV), GAMMA, 1, *state)
        out, out_valid = out.cpu().numpy(), out_valid.cpu().numpy()
        assert np.array_equal(out_valid, valid)
        assert np.array_equal(out[valid][:, :W].view(np.int64), rec[valid].view(np.int64)) and np.all(out[valid][:, W] == 1.0)
    assert not state[0].any()


def test_fold_refuses_what_the_header_says_it_refuses():
    from bridges_hip import abi
    L = abi.require_gpu()
    E, W, n = 4, R.RECORD_WIDTH, 3
    rec = torch.zeros((E, W + 1), dtype=torch.float64, device=DEV)
    valid = torch.zeros(E, dtype=torch.uint8, device=DEV)
    count, acc, disc, ss, td = window_state(E, abi.NSTEP_MAX)
    out = torch.full((E * abi.NSTEP_MAX, W + 2), 7.0, dtype=torch.float64, device=DEV)
    ov = torch.full((E * abi.NSTEP_MAX,), 7, dtype=torch.uint8, device=DEV)
    stream = abi.current_stream()
    call = lambda n=n, W=W, rec=_ptr(rec), count=_ptr(count), out=_ptr(out): L.bridges_nstep_fold(
        E, W, n, rec, _ptr(valid), GAMMA, count, _ptr(acc), _ptr(disc), _ptr(ss), _ptr(td), out, _ptr(ov), stream)
    assert call() == 0
    for bad in (dict(n=0), dict(n=abi.NSTEP_MAX + 1), dict(W=R.RECORD_WIDTH - 1), dict(rec=C.c_void_p(0)), dict(out=C.c_void_p(0)),
                dict(rec=C.c_void_p(rec.data_ptr() + 4)), dict(count=C.c_void_p(count.data_ptr() + 2))):
        out.fill_(7.0)
        ov.fill_(7)
        assert call(**bad) != 0, bad
        assert "nstep_fold" in L.bridges_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((ov == 7).all())                      # a refusal launches nothing


# ------------------------------------------------------------------------------------------------------------ 2: the raster sum
def test_discounted_raster_sum_on_the_probe():
    """B = 5 transitions of 16 blocks, h in {1, 2, 3, 8} and mixed, first + h up to the last row; an empty raster and blocks of one
    pixel at bit 0 / bit 63 among them.  (k + 1) u d_k per set pixel, zero elsewhere, disc within h u d_h; h = 1 equals bits_to_f32 bit
    for bit; disc alone (no sum) is the same disc."""
    from bridges_hip import ops
    bits_np, cases = N.raster_probe()
    bits = torch.from_numpy(bits_np).to(DEV)
    for first, h in cases:
        s, d = ops.bits_discounted_sum(bits, torch.from_numpy(first).to(DEV), torch.from_numpy(h).to(DEV), GAMMA)
        assert s.dtype == torch.float32 and tuple(s.shape) == (len(first), 64, 64) and d.dtype == torch.float32
        N.check_raster_sum(s.cpu().numpy(), d.cpu().numpy(), N.raster_sum_ref(bits_np, first, h, GAMMA), name=f"h={h.tolist()}")
        if (h == 1).all():
            assert torch.equal(s, ops.bits_to_f32(bits[torch.from_numpy(first).to(DEV)]))
        none, d2 = ops.bits_discounted_sum(bits, torch.from_numpy(first).to(DEV), torch.from_numpy(h).to(DEV), GAMMA, want_sum=False)
        assert none is None and torch.equal(d, d2)
        plain_s, plain_d = N.raster_sum_plain(bits_np, first, h, GAMMA)                # ascending k in float32: the same bits
        assert np.array_equal(s.cpu().numpy(), plain_s) and np.array_equal(d.cpu().numpy(), plain_d)


def test_discounted_raster_sum_reads_nothing_outside_the_table():
    """h and first are clamped to the table: a count above 8, a negative one, a first row at and past the end give finite images of
    the rows that exist (none: zeros) and never a fault."""
    from bridges_hip import ops
    bits_np, _ = N.raster_probe()
    bits = torch.from_numpy(bits_np).to(DEV)
    rows = bits.shape[0]
    first = torch.tensor([rows - 2, rows, rows + 5, -3, 0], dtype=torch.int64, device=DEV)
    h = torch.tensor([8, 3, 1, 2, -1], dtype=torch.int32, device=DEV)
    s, d = ops.bits_discounted_sum(bits, first, h, GAMMA)
    img = N.images(bits_np)
    g = float(np.float32(GAMMA))
    assert np.allclose(s[0].cpu().numpy(), img[-2] + g * img[-1], rtol=1e-6, atol=0) and not s[1].any() and not s[2].any()
    assert np.allclose(s[3].cpu().numpy(), img[0] + g * img[1], rtol=1e-6, atol=0) and not s[4].any()
    assert bool(torch.isfinite(d).all())


# ------------------------------------------------------------------------------------------------------------ 3: the target
def run_td(pr, gamma, discount=None):
    from bridges_hip import dqn_ops
    seg = (torch.tensor(pr["lo"], dtype=torch.int32, device=DEV), torch.tensor(pr["hi"], dtype=torch.int32, device=DEV))
    q, sf, rows = dqn_ops.td_target(seg, pr["next_q"], pr["lin"], torch.tensor(pr["done"], device=DEV), gamma, next_sf=pr["next_sf"],
                                    action_raster=pr["act"], discount=discount)
    return q, sf, rows.cpu().tolist()


@pytest.mark.parametrize("sf_dim", [0, 4, 4096])
def test_td_target_rows_on_the_segment_probes(sf_dim):
    """A discount filled with gamma is bridges_td_target bit for bit (rows, q, sf); per-row discounts from {gamma^1 .. gamma^8}
    are within td_ref's 2 u (|a| + |d s|) of the float64 statement, exact where done; both segment forms and the strided next_sf are
    the probe's."""
    pr = td_probe(sf_dim, DEV)
    B = len(pr["lo"])
    want = run_td(pr, GAMMA)
    got = run_td(pr, 123.0, discount=torch.full((B,), GAMMA, dtype=torch.float32, device=DEV))      # the scalar is not read
    assert got[2] == want[2] and torch.equal(got[0], want[0]) and (sf_dim == 0 or torch.equal(got[1], want[1]))
    disc = N.row_discounts(B, GAMMA).to(DEV)
    ref, rows = N.td_rows_ref(pr, disc)
    got = run_td(pr, GAMMA, discount=disc)
    N.check_td_rows(got, ref, rows, name=f"sf_dim={sf_dim}")
    dn = torch.tensor(pr["done"], device=DEV)
    assert torch.equal(got[0][dn], pr["lin"][dn])
    if sf_dim:
        assert torch.equal(got[1][dn], pr["act"].reshape(B, -1)[dn])


def test_next_targets_passes_the_discount_to_both_targets():
    from bridges_hip import dqn_ops
    pr = td_probe(4096, DEV)
    B = len(pr["lo"])
    seg = (torch.tensor(pr["lo"], dtype=torch.int32, device=DEV), torch.tensor(pr["hi"], dtype=torch.int32, device=DEV))
    disc = N.row_discounts(B, GAMMA).to(DEV)
    done = torch.tensor(pr["done"], device=DEV)
    q, sf = dqn_ops.next_targets(seg, pr["next_q"], done, GAMMA, next_sf=lambda best: pr["next_sf"][best].contiguous(),
                                 action_raster=pr["act"], lin=pr["lin"], discount=disc)
    want = run_td(pr, GAMMA, discount=disc)
    assert torch.equal(q, want[0]) and torch.equal(sf, want[1])
    with pytest.raises(ValueError, match="lin"):
        dqn_ops.next_targets(seg, pr["next_q"], done, GAMMA, discount=disc)


# ------------------------------------------------------------------------------------------------------------ 4: the loop
E_LOOP, MAX_STEPS, BATCH, N_STEP = 8, 4, 4, 3
H = 0.8


def tower_env(seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    return VecAssemblyGym(E_LOOP, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)],
                          [(0.5, 0, 2 * H + H / 2)], max_steps=MAX_STEPS, seed=seed, **kw)


def random_env(seed=0):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomObstacles, RandomTargets, VecAssemblyGym
    return VecAssemblyGym(E_LOOP, [load_urdf("shapes/trapezoid.urdf")], RandomObstacles([((-3.0, 3.0), (0.3, 2.5))]), RandomTargets(2),
                          max_steps=MAX_STEPS, seed=seed, f32_rasters=False)


def mlp_agent(env, n_step, loss="mse_q_values+mse_block_features", **kw):
    from robotoddler.training.vec_dqn import VecDQN
    pol, tgt = make_mlp(seed=0), make_mlp(seed=0)
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 4096, BATCH, GAMMA, 0.01, loss, seed=3,
                  n_step=n_step, **kw)


def conv_agent(env, n_step):
    from robotoddler.models.cv import ConvNet
    from robotoddler.training.vec_dqn import VecDQN
    from robotoddler.utils.utils import init_weights
    nets = []
    for _ in range(2):
        torch.manual_seed(0)
        net = ConvNet(img_size=(64, 64)).to(DEV)
        net.apply(init_weights)
        nets.append(net)
    return VecDQN(nets[0], nets[1], torch.optim.Adam(nets[0].parameters(), lr=1e-4, fused=True), env, 4096, BATCH, GAMMA, 0.01,
                  "mse_q_values", seed=3, n_step=n_step)


def ring_rows(agent):
    assert agent.ring.size < agent.ring.capacity
    return agent.ring.data[:agent.ring.size].clone()


def rollout_pair(make_env, make_agent, locksteps=8):
    """An n_step = N_STEP agent and the same-seed one-step agent, ``locksteps`` lock-steps without optimiser steps each -> (agent,
    its ring rows, one-step agent, its one-step records [(rec with tail [E, W], valid [E]), ...])."""
    multi, single = make_agent(make_env(), N_STEP), make_agent(make_env(), 1)
    log = []
    act = single.act

    def logged_act():
        rec, valid = act()
        log.append((single.with_task(rec).clone(), valid.clone()))
        return rec, valid
    single.act = logged_act
    for _ in range(locksteps):
        multi.lockstep(0)
        single.lockstep(0)
    torch.cuda.synchronize()
    assert multi.env_steps == single.env_steps > 0 and multi.episodes_done == single.episodes_done
    return multi, ring_rows(multi), single, log


def reference_ring(log, n=N_STEP):
    """The reference window over the logged one-step records -> (rows [m, W + 1], g_bound [m], [(global index of the start's one-step
    record among the valid ones, h), ...])."""
    win = N.RefWindow(E_LOOP, n, GAMMA)
    rows, bounds, at = [], [], 0
    for rec, valid in log:
        rec, valid = rec.cpu().numpy(), valid.cpu().numpy().astype(bool)
        tags = np.full(E_LOOP, -1)
        tags[valid] = at + np.arange(int(valid.sum()))
        at += int(valid.sum())
        out, out_valid, g_bound = win.fold(rec, valid, tags=tags)
        rows.append(out[out_valid])
        bounds.append(g_bound[out_valid])
    return np.concatenate(rows), np.concatenate(bounds), win.emitted


def check_ring(multi_rows, log):
    ref_rows, g_bound, emitted = reference_ring(log)
    got = multi_rows.cpu().numpy()
    assert got.shape == ref_rows.shape and got.shape[0] >= E_LOOP
    keep = np.ones(got.shape[1], dtype=bool)
    keep[R.O_LIN] = False
    assert np.array_equal(got[:, keep].view(np.int64), ref_rows[:, keep].view(np.int64))
    assert np.all(np.abs(got[:, R.O_LIN] - ref_rows[:, R.O_LIN]) <= g_bound)
    hs = {h for _, h in emitted}
    assert hs == {1, 2, 3}, hs                                                         # full windows and the tails of episodes
    return emitted


def check_targets(multi, multi_rows, single, log, emitted):
    """_targets of every ring row against the one-step _targets of the same-seed agent's records; t = the start of the row's window,
    tau = t + h - 1 its last step (consecutive valid records of one env), nq / psi' = the bootstrap of step tau, which both read:
        q_n  = G + gamma^(h-1) (q_1[tau] - lin[tau]),    sf_n = sum_{k < h-1} gamma^k raster_k + gamma^(h-1) sf_1[tau].
    Bounds, first order in u = 2^-24, with X = gamma^(h-1) (q_1[tau] - lin[tau]) ~ gamma^h nq:
      the kernel's q_n = fl(fl32(G) + fl(d nq)), d = the float32 gamma multiplied h - 1 times: u (3 |G| + (2 h + 1) |X|);
      the reference's X carries q_1[tau]'s own roundings (gamma, the product, the sum: u (3 |gamma nq| + |lin|)) times gamma^(h-1);
      together  u (3 |G| + (2 h + 4) |X| + gamma^(h-1) |lin[tau]|).
    sf_n per pixel likewise with S = sum_{k < h} gamma^k raster_k and Y = gamma^(h-1) (sf_1[tau] - raster_tau) ~ gamma^h psi':
      u (sum_k (k + 1) gamma^k raster_k  +  2 |S|  +  (2 h + 4) |Y|  +  gamma^(h-1) raster_tau).
    The inputs (block raster, action raster, binary features; the task's map and obstacle bits) are those of step t, bit for bit.
    Both bounds take nq / psi' as the SAME float32 numbers on both sides, so the one-step targets of the steps tau are computed by
    one call on the records tau of the ring rows, in the ring's order: the scratch envs of the two agents then hold the same next
    states in the same slots and the target net runs on the same rows in the same shapes (a GEMM of another shape may round
    differently, which no bound in u |Y| covers); a second call on all records gives the inputs of the steps t and the rasters."""
    valid_recs = torch.cat([rec[valid] for rec, valid in log])
    env_of = torch.cat([torch.nonzero(valid).squeeze(1) for _, valid in log]).cpu().tolist()
    # the valid records of one env, in time order: position -> global index
    by_env = {e: [i for i, v in enumerate(env_of) if v == e] for e in range(E_LOOP)}
    windows = []
    for t, h in emitted:
        chain = by_env[env_of[t]]
        p = chain.index(t)
        windows.append(chain[p:p + h])
        assert len(windows[-1]) == h
    taus = torch.tensor([w[-1] for w in windows], device=DEV)
    last = [o.clone() if torch.is_tensor(o) else o for o in single._targets(valid_recs[taus])]
    one = single._targets(valid_recs)
    one = type(one)(*(o.clone() if torch.is_tensor(o) else o for o in one))
    many = multi._targets(multi_rows)
    torch.cuda.synchronize()
    use_sf = one[4] is not None
    lin1 = valid_recs[:, R.O_LIN].float().double()
    for i, (t, h) in enumerate(emitted):
        steps = windows[i]
        tau = steps[-1]
        for k in (0, 1, 2):                                                            # block_f, binary, action_f of step t
            if one[k] is not None:
                assert torch.equal(many[k][i], one[k][t]), (i, k)
        for k in one._fields[5:]:                                                      # the task's map and obstacle bits, the bit rasters
            if getattr(one, k) is not None:
                assert torch.equal(getattr(many, k)[i], getattr(one, k)[t]), (i, k)
        G = float(multi_rows[i, R.O_LIN])
        gh1 = GAMMA ** (h - 1)
        X = gh1 * (float(last[3][i]) - float(lin1[tau]))
        bound = U32 * (3 * abs(G) + (2 * h + 4) * abs(X) + gh1 * abs(float(lin1[tau])))
        assert abs(float(many[3][i]) - (G + X)) <= bound, (i, h, float(many[3][i]), G + X, bound)
        if use_sf:
            rasters = [one[2][s].double().reshape(-1) for s in steps]
            S = sum(GAMMA ** k * r for k, r in enumerate(rasters))
            Y = gh1 * (last[4][i].double().reshape(-1) - rasters[-1])
            b = U32 * (sum((k + 1) * GAMMA ** k * r for k, r in enumerate(rasters)) + 2 * S.abs() + (2 * h + 4) * Y.abs() + gh1 * rasters[-1])
            err = (many[4][i].double().reshape(-1) - (S + Y)).abs()
            assert bool((err <= b).all()), (i, h, float((err - b).max()))


def test_ring_and_targets_on_the_fixed_tower():
    """(a) the ring after 8 lock-steps equals the reference window over the one-step records of the same-seed n_step = 1 agent;
    (b) _targets of every ring row against the one-step _targets."""
    multi, rows, single, log = rollout_pair(lambda: tower_env(f32_rasters=False), mlp_agent)
    assert rows.shape[1] == R.RECORD_WIDTH + 1
    emitted = check_ring(rows, log)
    check_targets(multi, rows, single, log, emitted)


def test_ring_and_targets_on_random_targets_and_obstacles():
    """(d) the same on RandomTargets(2) plus one random obstacle per env: the tail rides through the fold, and the task of a row is
    the task of every step of its window."""
    mk = lambda env, n: mlp_agent(env, n, per_env_tasks=True, per_env_obstacles=True)
    multi, rows, single, log = rollout_pair(random_env, mk)
    assert rows.shape[1] == R.RECORD_WIDTH + 9 + 1
    emitted = check_ring(rows, log)
    check_targets(multi, rows, single, log, emitted)


def test_targets_of_a_convnet_on_the_fixed_tower():
    """(d) the conv Q-network on the fixed task: rows through _forward_rows, no successor features."""
    multi, rows, single, log = rollout_pair(lambda: tower_env(f32_rasters=True), conv_agent)
    emitted = check_ring(rows, log)
    check_targets(multi, rows, single, log, emitted)


def test_the_loop_trains_on_three_step_returns():
    """(c) four lock-steps with 2 optimiser steps each: finite losses, changed weights; the captured step sees what it always saw."""
    agent = mlp_agent(tower_env(f32_rasters=False), N_STEP)
    before = [p.detach().clone() for p in agent.policy_net.parameters()]
    losses = []
    for _ in range(4):
        ls, rec = agent.lockstep(2)
        losses += ls
        assert rec.shape[1] == R.RECORD_WIDTH + 1
    torch.cuda.synchronize()
    assert len(losses) >= 2 and all(np.isfinite(l) for l in losses)
    assert any(not torch.equal(b, p) for b, p in zip(before, agent.policy_net.parameters()))
    agent.reset_window()
    assert not agent._window[0].any()


def test_n_step_1_is_the_loop_it_was():
    """n_step = 1 keeps the ring's width, launches no fold and pushes the one-step records."""
    agent = mlp_agent(tower_env(f32_rasters=False), 1)
    for _ in range(3):
        agent.lockstep(0)
    assert agent.ring.width == R.RECORD_WIDTH and agent._window is None and agent._counts_host.numel() == 2
    assert agent.ring.size == agent.env_steps


LOOP = ["--model", "SuccessorMLP", "--loss_function", "mse_q_values+mse_block_features", "--tower_height", "2", "--max_steps", "4",
        "--num_envs", "8", "--num_episodes", "40", "--num_training_steps", "2", "--batch_size", "4", "--seed", "3",
        "--learning_rate", "1e-4", "--gamma", "0.8", "--n_step", "3"]


def _port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _child_env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "BRIDGES_DIST_BACKEND", "BENCH_DIST_BACKEND")}
    env.update(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4", **extra)
    return env


def test_the_loop_through_a_one_rank_rccl_group_equals_the_plain_run(tmp_path):
    """(e) with the forced one-rank process group the fold runs after the all-gather on the uncompacted rows and the episodes are
    counted from the done rows with h = 1: ring, weights, losses and episodes_done equal the run without a group."""
    res = {}
    for name, extra in (("plain", {}), ("rccl", dict(BRIDGES_FORCE_COLLECTIVE="1"))):
        script, outp = tmp_path / f"worker_{name}.py", tmp_path / f"{name}.json"
        script.write_text(WORKER % dict(root=ROOT, pkg=PKG, out=str(outp), argv=LOOP))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
               "--master-port", str(_port()), str(script)]
        out = subprocess.run(cmd, env=_child_env(**extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        res[name] = json.load(open(outp))
    p, r = res["plain"], res["rccl"]
    assert p["active"] is False and r["active"] is True and r["backend"] == "nccl"
    assert p["ring_width"] == r["ring_width"] == R.RECORD_WIDTH + 1
    assert p["locksteps"] == r["locksteps"] >= 5 and p["episodes"] == r["episodes"] >= 40
    assert p["env_steps"] == r["env_steps"] > 0 and p["ring_size"] == r["ring_size"] > 8
    assert p["ring_hash"] == r["ring_hash"] and p["policy_hash"] == r["policy_hash"]
    assert p["losses"] == r["losses"] and len(p["losses"]) >= 3


def test_find_syncs_counts_no_new_host_wait():
    """(f) tools/find_syncs.py reports the same number of host waits per lock-step with --n_step 3 as without (3 and 3 on an
    MI355X when this was written; the test asks for equality, not for the figure)."""
    counts = {}
    for name, extra in (("one_step", []), ("n_step_3", ["--n_step", "3"])):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "find_syncs.py"), "--envs", "64", *extra], env=_child_env(),
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        m = re.search(r"^(\d+) synchronising calls in one lock-step", out.stdout, flags=re.M)
        assert m, out.stdout[-2000:]
        counts[name] = int(m.group(1))
        print(name, counts[name], "host waits per lock-step")
    assert counts["n_step_3"] == counts["one_step"], counts
