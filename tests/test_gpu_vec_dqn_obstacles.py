"""GPU: the vectorised SuccessorMLP DQN on per-env obstacles (VecDQN(per_env_tasks=True, per_env_obstacles=True)) -- the
two-operand bit-packed first layer, the input rows with an obstacle raster per transition read as bits, acting, records that carry
targets and obstacles, replay that rebuilds both, the optimiser step, the captured step and the loop.  The oracles are what is
merged and tested already: the single-operand / f32-obstacle entry points (bit for bit where both state the same sum), the
float64 / module / autograd formulations at the tolerances of tests/test_gpu_vec_dqn_tasks.py."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_helpers import U32
from test_gpu_vec_dqn_tasks import PKG, ROOT, WORKER, make_mlp, make_step_net, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANGES = [((-3.0, 3.0), (0.3, 2.5))] * 2          # two obstacles, both x in [-3, 3), z in [0.3, 2.5)
MAX_STEPS = 6
HIDDEN = [(256, 128, 64, 128, 256), (256, 128, 192)]


def make_vec(E, obstacles, targets, max_steps=MAX_STEPS, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    kw.setdefault("f32_rasters", False)
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], obstacles, targets, max_steps=max_steps, seed=seed, **kw)


def random_env(E=64, seed=0, **kw):
    from bridges_hip.vec_env import RandomObstacles, RandomTargets
    return make_vec(E, RandomObstacles(RANGES), RandomTargets(3), seed=seed, **kw)


def make_agent(env, hidden=HIDDEN[0], seed=0, B=16, loss="mse_q_values+mse_block_features", **kw):
    from robotoddler.training.vec_dqn import VecDQN
    pol, tgt = make_mlp(hidden, seed), make_mlp(hidden, seed)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-4)
    kw.setdefault("per_env_obstacles", True)
    return VecDQN(pol, tgt, opt, env, 8192, B, 0.95, 0.01, loss, seed=3, per_env_tasks=True, **kw)


def pack_bits(mask):
    """bool [n, 64, 64] -> int64 [n, 64]: bit x of word y = pixel (y, x) (bit 63 = the sign bit)."""
    return (mask.long() << torch.arange(64, device=mask.device)).sum(dim=-1)


def unpack_bits(bits):
    """int64 [n, 64] -> float64 [n, 4096] of 0 / 1, pixel p = 64 y + x."""
    return ((bits.unsqueeze(-1) >> torch.arange(64, device=bits.device)) & 1).reshape(bits.shape[0], -1).double()


def special_rasters(n, g, shift):
    """n sparse random rasters (~40 pixels); by (i + shift) % 6: 1 = empty, 2 = a full row (all 64 bits of row 17, so bit 63 -- the
    sign bit of the int64 -- is set) beside the random pixels, 3 = pixels in rows 0 and 63 only (bits 0 and 63 among them)."""
    mask = torch.rand((n, 64, 64), generator=g) < 0.01
    kind = (torch.arange(n) + shift) % 6
    mask[kind == 1] = False
    mask[kind == 2, 17, :] = True
    edge = torch.zeros((64, 64), dtype=torch.bool)
    edge[0, [0, 5, 63]] = True
    edge[63, [0, 31, 62, 63]] = True
    mask[kind == 3] = edge
    return pack_bits(mask).to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1: bits_linear2
@pytest.mark.parametrize("d", [4, 256, 260])
@pytest.mark.parametrize("n", [1, 5, 300])
def test_bits_linear2_equals_the_chained_calls_bit_for_bit(n, d):
    """bridges_bits_linear2 against bridges_bits_linear on operand a followed by bridges_bits_linear on operand b with the first
    result as base: torch.equal; and against the float64 sum of the selected weight rows within gamma_K * sum |terms|,
    K = set pixels + 1 (Higham eq. 3.5, as tests/gpu_helpers.py dot_bound), per output row."""
    from bridges_hip import ops
    g = torch.Generator().manual_seed(1000 * n + d)
    wt_a, wt_b = torch.randn((4096, d), generator=g).to(DEV), torch.randn((4096, d), generator=g).to(DEV)
    table = torch.randn((7, d), generator=g).to(DEV)
    ident = torch.arange(n, device=DEV)
    seen = set()
    for shift in (range(6) if n == 1 else (0, 3)):
        bits_a, bits_b = special_rasters(n, g, shift), special_rasters(n, g, shift + 2)
        pool_a = special_rasters(11, g, shift + 1)
        row_a = torch.randint(0, 11, (n,), generator=g).to(DEV)
        row_b = torch.randperm(n, generator=g).to(DEV)
        seen |= {("a", int(k)) for k in (torch.arange(n) + shift) % 6} | {("b", int(k)) for k in (torch.arange(n) + shift + 2) % 6}
        for base, base_row in ((None, None), (table[3:4].expand(n, d).contiguous(), ident), (table, None),
                               (table, torch.randint(0, 7, (n,), generator=g).to(DEV))):
            for ba, ra, rb in ((bits_a, None, None), (pool_a, row_a, None), (pool_a, row_a, row_b)):
                got = ops.bits_linear2(ba, wt_a, bits_b, wt_b, bits_row_a=ra, bits_row_b=rb, base=base, base_row=base_row)
                first = ops.bits_linear(ba, wt_a, bits_row=ra, base=base, base_row=base_row)
                want = ops.bits_linear(bits_b, wt_b, bits_row=rb if rb is not None else ident, base=first, base_row=ident)
                assert tuple(got.shape) == (n, d) and torch.equal(got, want), (shift, float((got - want).abs().max()))
                ma = unpack_bits(ba if ra is None else ba[ra])
                mb = unpack_bits(bits_b if rb is None else bits_b[rb])
                b64 = 0.0 if base is None else (base[base_row] if base_row is not None else base[:1].expand(n, d)).double()
                ref = b64 + ma @ wt_a.double() + mb @ wt_b.double()
                mag = (0.0 if base is None else b64.abs()) + ma @ wt_a.double().abs() + mb @ wt_b.double().abs()
                K = (ma.sum(dim=1) + mb.sum(dim=1) + 1).unsqueeze(1)
                bound = mag * (K * U32 / (1.0 - K * U32)) + K * 2.0 ** -126
                err = (got.double() - ref).abs()
                assert bool((err <= bound).all()), (shift, float((err - bound).max()))
    assert seen >= {(o, k) for o in "ab" for k in (1, 2, 3)}                     # every special raster met in either operand
    # argument rules of bridges_bits_linear: d % 4 == 0
    from bridges_hip import abi
    from bridges_hip.ops import _ptr, _stream
    L = abi.require_gpu()
    out = torch.empty((n, d), device=DEV)
    assert L.bridges_bits_linear2(n, _ptr(bits_a), None, _ptr(wt_a), _ptr(bits_b), None, _ptr(wt_b), d + 2, None, None, _ptr(out), _stream()) == -1
    assert L.bridges_bits_linear2(n, _ptr(bits_a), None, _ptr(wt_a), None, None, _ptr(wt_b), d, None, None, _ptr(out), _stream()) == -1


# ------------------------------------------------------------------------------------------------------------ 2: k_mlp_input
def input_batch(n, g):
    px = 4096
    r = lambda *s: torch.rand(*s, device=DEV, generator=g)
    block, action, binary = (r(n, px) < 0.05).float(), (r(n, px) < 0.01).float(), (r(n, 6) < 0.5).float()
    reward = r(n, px)
    mask = r(n, 64, 64) < 0.03
    mask[1] = False                                                       # one empty raster
    mask[2] = False
    mask[2, 63, 63] = True                                                # bit 63 of row 63 alone
    mask[3, 63, 63] = True
    return block, action, binary, reward, pack_bits(mask)


@pytest.mark.parametrize("batch", [20, 32])
def test_input_rows_with_obstacle_bits(batch):
    """bridges_mlp_input_task_rows / _batches_task_rows: x is exactly the concatenation the module forward builds with every
    transition's raster expanded by bits_to_f32 (a copy kernel: bit for bit), padding rows are zero, the counter form equals the
    slice of the batches form, one raster on every transition equals the _rows entry points on its f32 image, px != 4096 is
    refused."""
    from bridges_hip import abi, ops
    from bridges_hip.ops import _ptr, _stream
    L = abi.require_gpu()
    rows, px, nf, n_batches = 32, 4096, 6, 3
    n = n_batches * batch
    g = torch.Generator(device=DEV).manual_seed(batch)
    block, action, binary, reward, obst = input_batch(n, g)
    assert not obst[1].any() and int(obst[2, 63]) == -2 ** 63 and not obst[2, :63].any()
    K = 4 * px + nf
    want = torch.cat([block, action, reward, ops.bits_to_f32(obst).reshape(n, px), binary], dim=1)
    x_all = torch.full((n_batches * rows, K), -1.0, device=DEV)
    abi.check(L.bridges_mlp_input_batches_task_rows(n_batches, batch, rows, px, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), px,
                                                    _ptr(obst), _ptr(x_all), _stream()), "bridges_mlp_input_batches_task_rows")
    for c in range(n_batches):
        assert torch.equal(x_all[c * rows:c * rows + batch], want[c * batch:(c + 1) * batch]), c
        assert not x_all[c * rows + batch:(c + 1) * rows].any()
        x = torch.full((rows, K), -1.0, device=DEV)
        counter = torch.full((), c, dtype=torch.int64, device=DEV)
        abi.check(L.bridges_mlp_input_task_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), px,
                                                _ptr(obst), _ptr(x), _stream()), "bridges_mlp_input_task_rows")
        assert torch.equal(x, x_all[c * rows:(c + 1) * rows]), c
    # one raster on every transition = the f32-obstacle entry points on its image; reward_stride 0 and px
    for k in (0, 2):
        same = obst[k:k + 1].expand(n, 64).contiguous()
        img = ops.bits_to_f32(obst[k:k + 1]).reshape(px).contiguous()
        for stride, rw in ((px, reward), (0, reward[5].contiguous())):
            xa, xb = torch.full((n_batches * rows, K), -1.0, device=DEV), torch.full((n_batches * rows, K), -2.0, device=DEV)
            abi.check(L.bridges_mlp_input_batches_rows(n_batches, batch, rows, px, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(rw), stride,
                                                       _ptr(img), _ptr(xa), _stream()), "bridges_mlp_input_batches_rows")
            abi.check(L.bridges_mlp_input_batches_task_rows(n_batches, batch, rows, px, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(rw),
                                                            stride, _ptr(same), _ptr(xb), _stream()), "bridges_mlp_input_batches_task_rows")
            assert torch.equal(xa, xb), (k, stride)
            counter = torch.full((), 1, dtype=torch.int64, device=DEV)
            ya, yb = torch.full((rows, K), -1.0, device=DEV), torch.full((rows, K), -2.0, device=DEV)
            abi.check(L.bridges_mlp_input_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(rw), stride,
                                               _ptr(img), _ptr(ya), _stream()), "bridges_mlp_input_rows")
            abi.check(L.bridges_mlp_input_task_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(rw), stride,
                                                    _ptr(same), _ptr(yb), _stream()), "bridges_mlp_input_task_rows")
            assert torch.equal(ya, yb), (k, stride)
    # px = 1024 (32 x 32 images) has no bit-packed form: refused, nothing written
    small = torch.full((n_batches * rows, 4 * 1024 + nf), -1.0, device=DEV)
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    assert L.bridges_mlp_input_batches_task_rows(n_batches, batch, rows, 1024, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), 1024,
                                                 _ptr(obst), _ptr(small), _stream()) == -1
    assert L.bridges_mlp_input_task_rows(batch, rows, 1024, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), 1024,
                                         _ptr(obst), _ptr(small), _stream()) == -1
    assert b"4096" in L.bridges_last_error() and bool((small == -1.0).all())
    assert L.bridges_mlp_input_task_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), 1,
                                         _ptr(obst), _ptr(x), _stream()) == -1


# ------------------------------------------------------------------------------------------------------------ 3: acting forward
def masked_by_obstacle_alone(env):
    """Raw candidates that overlap their env's obstacle raster, not its state raster, and are masked."""
    E = env.E
    off, n_cand = env.cand_offset[:E].long(), env.n_cand[:E].long()
    total = int(env.cand_offset[E])
    ci = torch.arange(total, device=DEV)
    env_of = torch.searchsorted(env.cand_offset[1:E + 1].long().contiguous(), ci, right=True).clamp(max=E - 1)
    live = ci < (off + n_cand)[env_of]
    cb = env.cand_bits[:total]
    hits_obstacle = ((cb & env.env_obstacle_bits[env_of]) != 0).any(dim=1)
    hits_state = ((cb & env.state_bits[env_of]) != 0).any(dim=1)
    return int((live & hits_obstacle & ~hits_state & (env.cand_mask[:total] == 0)).sum())


@pytest.mark.parametrize("hidden", HIDDEN)
def test_acting_forward_with_an_obstacle_raster_per_env(hidden):
    """_net_q on 64 envs that each drew their own targets and obstacles, after 0, 3 and 6 lock-steps (the sixth ends every episode
    that is left: the obstacles are redrawn): against the module forward fed every row's own map and obstacle raster at
    rtol = atol = 1e-5 (the bound of test_acting_forward_with_a_map_per_env), and rows shared by (state, targets, obstacles)
    against every env's own rows, exactly."""
    from bridges_hip import ops
    from robotoddler.training.vec_dqn import VecDQN
    E = 64
    env = random_env(E, seed=0)
    agent = make_agent(env, hidden, seed=3)
    net = agent.policy_net
    bits0 = env.env_obstacle_bits.clone()
    assert bool((bits0 != 0).any(dim=1).all())                                            # no raster is empty ...
    assert torch.unique(bits0, dim=0).shape[0] == E                                       # ... and no two are equal
    masked = 0
    try:
        for it in range(7):
            if it in (0, 3, 6):
                stable = agent._stable_flags(env)
                VecDQN.DEDUP_STATES = False
                env._dqn_rows = None
                idx, row_env, (lo_a, hi_a), rep_a = agent._rows(env, stable)
                assert rep_a is None
                idx, row_env = idx.clone(), row_env.clone()
                n = idx.numel()
                q = agent._net_q(net, env, idx, row_env, stable).clone()
                assert q.shape == (n,) and n > 200
                binary = torch.zeros((n, 6), device=DEV)
                binary[:, 0] = stable[row_env].float()
                rasters = env.obstacle_rasters
                with torch.no_grad():
                    net.eval()
                    q_mod = net(ops.bits_to_f32(env.state_bits[row_env]).unsqueeze(1), binary, ops.bits_to_f32(env.cand_bits[idx]).unsqueeze(1),
                                env.reward_maps_img[row_env].unsqueeze(1), rasters[row_env].unsqueeze(1))[0]
                assert torch.allclose(q, q_mod, rtol=1e-5, atol=1e-5), (it, float((q - q_mod).abs().max()))
                VecDQN.DEDUP_STATES = True
                env._dqn_rows = None
                idx_s, env_s, (lo_s, hi_s), rep = agent._rows(env, stable)
                q_s = agent._net_q(net, env, idx_s, env_s, stable)
                src = torch.cat([torch.arange(int(lo_s[e]), int(hi_s[e]), device=DEV) for e in range(E)])
                assert src.numel() == n and torch.equal(q_s[src], q), (it, float((q_s[src] - q).abs().max()))
                env._dqn_rows = None
                masked += masked_by_obstacle_alone(env)
            env.select_random()
            env.step()
    finally:
        VecDQN.DEDUP_STATES = True
    assert masked > 0
    assert int(env.task_episode.min()) >= 1 and not torch.equal(env.env_obstacle_bits, bits0)


# ------------------------------------------------------------------------------------------------------------ 4: records and replay
def test_records_carry_targets_and_obstacles_held_before_the_step():
    from robotoddler.training import records as R
    E = 64
    env = random_env(E, seed=11)
    agent = make_agent(env, seed=1)
    W = R.RECORD_WIDTH + 9 + 6
    assert agent.ring.width == agent.ring.data.shape[1] == W == 126
    cap, inner = {}, env.step

    def step(sel_index=None):
        cap.update(targets=env.env_targets.clone(), obstacles=env.env_obstacles.clone(), episode=env.task_episode.clone())
        inner(sel_index)

    env.step = step
    crossed = 0
    for it in range(2 * MAX_STEPS):
        rec, valid = agent.act()
        full = agent.with_task(rec)
        assert tuple(rec.shape) == (E, R.RECORD_WIDTH) and tuple(full.shape) == (E, W)
        assert torch.equal(full[:, :R.RECORD_WIDTH], rec)
        assert torch.equal(full[:, R.RECORD_WIDTH:R.RECORD_WIDTH + 9].reshape(E, 3, 3), cap["targets"])
        assert torch.equal(full[:, R.RECORD_WIDTH + 9:].reshape(E, 2, 3), cap["obstacles"])
        over = env.task_episode != cap["episode"]                              # the envs whose episode ended in this step
        if bool(over.any()):
            now = env.env_obstacles.reshape(E, -1)
            assert bool((full[over, R.RECORD_WIDTH + 9:] != now[over]).any(dim=1).all()), it
            assert torch.equal(full[~over, R.RECORD_WIDTH + 9:], now[~over])
        crossed += int(over.sum())
        agent.ring.push(full[valid])
    assert crossed >= E                                                       # max_steps 6: every env crossed a boundary
    assert len(agent.ring) > 5 * E


def rollout_agent(E=64, seed=11, locksteps=12, **kw):
    env = random_env(E, seed=seed)
    agent = make_agent(env, seed=1, **kw)
    with torch.no_grad():                                       # the target net is a copy of the policy net: make it its own
        for p in agent.target_net.parameters():
            p.mul_(1.05)
    for _ in range(locksteps):
        rec, valid = agent.act()
        agent.ring.push(agent.with_task(rec)[valid])
    return env, agent


@pytest.mark.parametrize("n", [10, 16, 40])
def test_replay_rebuilds_every_transitions_obstacles(n):
    from bridges_hip import ops
    from robotoddler.training import records as R
    env, agent = rollout_agent()
    gamma = agent.gamma
    rec = agent.ring.sample(n, agent.sample_gen)
    assert rec.shape[1] == 126
    batch = agent._targets(rec)
    action_f, q_target, sf_target, maps, obst_bits = batch.action_f, batch.q_target, batch.sf_target, batch.reward_maps, batch.obstacle_bits
    renv = agent.replay_env
    assert renv.E >= n and renv.per_env_tasks and renv.per_env_obstacles and renv.random_obstacles is None and renv.random_targets is None
    assert tuple(maps.shape) == (n, 4096) and tuple(obst_bits.shape) == (n, 64) and obst_bits.dtype == torch.int64
    tg = rec[:, R.RECORD_WIDTH:R.RECORD_WIDTH + 9].reshape(n, 3, 3)
    ob = rec[:, R.RECORD_WIDTH + 9:].reshape(n, 2, 3)
    assert torch.equal(renv.env_targets[:n], tg) and torch.equal(renv.env_obstacles[:n], ob)
    assert bool((renv.env_obstacles[n:] == ob[0]).all())
    assert torch.unique(ob.reshape(n, -1), dim=0).shape[0] > n // 2          # the sample spans many obstacle draws
    # an env created with those targets and obstacles, loaded with the same states: rasters and next-state masks
    fx = make_vec(n, ob.cpu().contiguous(), tg.cpu().contiguous())
    assert torch.equal(obst_bits, fx.env_obstacle_bits) and torch.equal(renv.env_obstacle_bits[:n], fx.env_obstacle_bits)
    assert torch.equal(renv.reward_maps[:n], fx.reward_maps)
    fx.load_records(rec[:, :R.RECORD_WIDTH].contiguous())
    total = int(fx.cand_offset[n])
    assert total == int(renv.cand_offset[n]) > 0
    assert torch.equal(renv.cand_offset[:n + 1], fx.cand_offset[:n + 1]) and torch.equal(renv.n_valid[:n], fx.n_valid[:n])
    assert torch.equal(renv.cand_mask[:total], fx.cand_mask[:total]) and torch.equal(renv.cand_bits[:total], fx.cand_bits[:total])
    # the targets from the module forward of the target net, every candidate row with the map and the obstacles of its transition
    tgt = agent.target_net
    idx, row_env = renv.valid_rows()
    keep = row_env < n
    idx, row_env = idx[keep].clone(), row_env[keep].clone()
    stable_n = rec[:, R.O_STABLE_N] > 0.5
    m = idx.numel()
    bin_rows = torch.zeros((m, 6), device=DEV)
    bin_rows[:, 0] = stable_n[row_env].float()
    with torch.no_grad():
        tgt.eval()
        q_all, sf_all, _ = tgt(ops.bits_to_f32(renv.state_bits[row_env]).unsqueeze(1), bin_rows, ops.bits_to_f32(renv.cand_bits[idx]).unsqueeze(1),
                               renv.reward_maps_img[row_env].unsqueeze(1), ops.bits_to_f32(obst_bits[row_env]).unsqueeze(1))
    lin = rec[:, R.O_LIN].float()
    done = (rec[:, R.O_DONE] > 0.5) | (renv.n_valid[:n] == 0)
    want_q, want_sf = lin.clone(), action_f.reshape(n, -1).clone()
    live = 0
    for i in range(n):
        rows = torch.nonzero(row_env == i).squeeze(1)
        if bool(done[i]) or rows.numel() == 0:
            continue
        best = rows[int(torch.argmax(q_all[rows]))]
        want_q[i] += gamma * q_all[best]
        want_sf[i] += gamma * sf_all[best, 0].reshape(-1)
        live += 1
    assert live >= n // 3
    assert torch.allclose(q_target, want_q, rtol=1e-5, atol=1e-5), float((q_target - want_q).abs().max())
    assert torch.allclose(sf_target, want_sf, rtol=1e-5, atol=1e-5), float((sf_target - want_sf).abs().max())
    with pytest.raises(ValueError, match="126"):
        agent._targets(rec[:, :R.RECORD_WIDTH + 9])


# ------------------------------------------------------------------------------------------------------------ 5: optimiser step
def step_batch(n, seed, one_raster=False):
    """The batch of tests/test_gpu_vec_dqn_tasks.py::step_batch at 64x64 with a reward map AND a bit-packed obstacle raster per
    transition (one_raster: the same raster on every transition)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    px = 4096
    r = lambda *s: torch.rand(*s, device=DEV, generator=g)
    block, action, binary = (r(n, px) < 0.05).float(), (r(n, px) < 0.01).float(), (r(n, 6) < 0.5).float()
    reward = r(n, px)
    mask = r(n, 64, 64) < 0.03
    if one_raster:
        mask[:] = mask[0].clone()
    q_t, sf_t = torch.randn(n, device=DEV, generator=g) * 3, r(n, px)
    return block, action, binary, reward, pack_bits(mask), q_t, sf_t


def autograd_step(net, batch, rows, use_q=True, use_sf=True):
    from bridges_hip import ops
    block, action, binary, reward, obst, q_t, sf_t = batch
    B = rows.stop - rows.start
    img = lambda t: t.reshape(-1, 1, 64, 64)
    for p in net.parameters():
        p.grad = None
    q, sf, _ = net(img(block[rows]), binary[rows], img(action[rows]), img(reward[rows]), img(ops.bits_to_f32(obst[rows])))
    mse = torch.nn.MSELoss()
    loss = 0.
    if use_q:
        loss = loss + mse(q, q_t[rows])
    if use_sf:
        loss = loss + mse(sf[:, 0].reshape(B, -1), sf_t[rows])
    loss.backward()
    return float(loss.detach()), q.detach(), [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("prebuilt", [False, True])
@pytest.mark.parametrize("B", [32, 20])
def test_fused_step_with_map_and_obstacle_bits_per_transition_matches_autograd(B, prebuilt):
    """The bounds of test_fused_step_with_a_map_per_transition_matches_autograd: loss 1e-5 relative, q and every gradient (the
    first layer's obstacle columns included) 1e-5 relative to the largest entry."""
    from bridges_hip.mlp_ops import FusedSuccessorStep
    net = make_step_net(HIDDEN[0], 64, seed=B)
    n_batches = 3
    batch = step_batch(n_batches * B, seed=B + 64)
    block, action, binary, reward, obst, q_t, sf_t = batch
    refs = [autograd_step(net, batch, slice(i * B, (i + 1) * B)) for i in range(n_batches)]
    px = 4096
    w_obst_grad = refs[0][2][0][:, 3 * px:4 * px]
    assert float(w_obst_grad.abs().max()) > 0                                  # the obstacle columns do get a gradient
    for p in net.parameters():
        p.grad = None
    fused = FusedSuccessorStep(net, B, True, True)
    if prebuilt:
        fused.allocate_inputs(n_batches)
        fused.prepare_inputs(n_batches, block, action, binary, reward, obst)
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    losses = torch.zeros(n_batches, device=DEV)
    for i in range(n_batches):
        fused.launch(counter, block, action, binary, reward, obst, q_t, sf_t, losses)
        loss_ref, q_ref, grads_ref = refs[i]
        assert int(counter) == i + 1
        assert abs(float(losses[i]) - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref)), (i, float(losses[i]), loss_ref)
        assert rel_err(fused.q[:B], q_ref) < 1e-5
        for p, gref in zip(net.parameters(), grads_ref):
            assert rel_err(p.grad, gref) < 1e-5, (i, tuple(p.shape), rel_err(p.grad, gref))


def test_three_adam_steps_with_obstacle_bits_follow_the_autograd_run():
    """test_three_adam_steps_with_a_map_per_transition_follow_the_autograd_run with an obstacle raster per transition, same
    tolerances; then every transition on ONE raster: losses and parameters equal the f32-obstacle path bit for bit."""
    from bridges_hip import ops
    from bridges_hip.dqn_ops import FlatParameters
    from bridges_hip.mlp_ops import FusedSuccessorStep
    B = 32
    batch = step_batch(3 * B, seed=5)
    block, action, binary, reward, obst, q_t, sf_t = batch
    net_a, net_b = make_step_net(HIDDEN[0], 64, 9), make_step_net(HIDDEN[0], 64, 9)
    net_b._flat_params = FlatParameters(net_b)
    opt_a = torch.optim.Adam(net_a.parameters(), lr=1e-3, fused=True)
    opt_b = torch.optim.Adam(net_b.parameters(), lr=1e-3, fused=True)
    losses_a = []
    for i in range(3):
        losses_a.append(autograd_step(net_a, batch, slice(i * B, (i + 1) * B))[0])
        opt_a.step()
    fused = FusedSuccessorStep(net_b, B, True, True, optimizer=opt_b)
    assert fused.fused_adam
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    losses_b = torch.zeros(3, device=DEV)
    for i in range(3):
        fused.launch(counter, block, action, binary, reward, obst, q_t, sf_t, losses_b)
    assert int(counter) == 3 and float(fused.adam_step) == 3.0
    np.testing.assert_allclose(losses_b.cpu().numpy(), np.array(losses_a), rtol=2e-5)
    for pa, pb in zip(net_a.parameters(), net_b.parameters()):
        assert rel_err(pb.detach(), pa.detach()) < 2e-4
        sa, sb = opt_a.state[pa], opt_b.state[pb]
        assert rel_err(sb["exp_avg"], sa["exp_avg"]) < 1e-4 and rel_err(sb["exp_avg_sq"], sa["exp_avg_sq"]) < 1e-4
    # one raster on every transition: the bits path and the f32 path build the same rows, so everything after is the same bits
    block, action, binary, reward, obst, q_t, sf_t = step_batch(3 * B, seed=6, one_raster=True)
    assert bool((obst == obst[0]).all()) and bool(obst[0].any())
    img = ops.bits_to_f32(obst[:1]).reshape(-1).contiguous()
    out = {}
    for kind, obstacle in (("bits", obst), ("f32", img)):
        for prebuilt in (False, True):
            net = make_step_net(HIDDEN[0], 64, 9)
            net._flat_params = FlatParameters(net)
            opt = torch.optim.Adam(net.parameters(), lr=1e-3, fused=True)
            fused = FusedSuccessorStep(net, B, True, True, optimizer=opt)
            if prebuilt:
                fused.allocate_inputs(3)
                fused.prepare_inputs(3, block, action, binary, reward, obstacle)
            counter, losses = torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros(3, device=DEV)
            for i in range(3):
                fused.launch(counter, block, action, binary, reward, obstacle, q_t, sf_t, losses)
            out[kind, prebuilt] = (losses.clone(), net._flat_params.flat.detach().clone())
    for prebuilt in (False, True):
        (la, fa), (lb, fb) = out["bits", prebuilt], out["f32", prebuilt]
        assert bool((la > 0).all()) and torch.equal(la, lb) and torch.equal(fa, fb), prebuilt


# ------------------------------------------------------------------------------------------------------------ 6: captured step
@pytest.mark.parametrize("loss", ["mse_q_values+mse_block_features", "mse_block_features"])
def test_captured_step_with_obstacle_bits_equals_the_eager_launches(loss, monkeypatch):
    """CapturedTrainStep(task_rows=True, obstacle_rows=True, task=(None, None)): 4 calls x 3 optimiser steps, the maps and the
    bit-packed rasters of every call copied into the static buffers the captured launches read, against the same launches queued
    eagerly on the same batches: losses and weights bit for bit."""
    from bridges_hip.dqn_ops import FlatParameters
    from robotoddler.training import train_step as T
    B, n, calls = 32, 3, 4
    parts = loss.split('+')
    batches = [step_batch(n * B, seed=100 + c) for c in range(calls)]
    out = {}
    for mode, graph, prepared, warmup in (("eager", "0", False, 1), ("graph", "1", False, 1), ("prepared", "1", True, 0)):
        monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", graph)
        net = make_step_net(HIDDEN[0], 64, 4)
        net._flat_params = FlatParameters(net)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True)
        for g in opt.param_groups:
            g['capturable'] = True
        drv = T.CapturedTrainStep.of(net, opt, B, parts, n, img=(64, 64), fused=True, graph_default=True, warmup=warmup,
                                     eager_body=True, prepared=prepared, task=(None, None), task_rows=True, obstacle_rows=True)
        losses = []
        for block, action, binary, reward, obst, q_t, sf_t in batches:
            got = drv.run(n, block, action, binary, reward, obst, q_t if 'mse_q_values' in parts else None,
                          sf_t if 'mse_block_features' in parts else None)
            losses += got.tolist()
        assert bool(drv._graphs) == (graph == "1")
        if graph == "1":
            assert drv.obstacle.dtype == torch.int64 and tuple(drv.obstacle.shape) == (n * B, 64)
            assert torch.equal(drv.obstacle, batches[-1][4])
        T.release(net)
        out[mode] = (np.array(losses), torch.cat([p.detach().flatten() for p in net.parameters()]).cpu())
    for mode in ("graph", "prepared"):
        assert len(out[mode][0]) == len(out["eager"][0]) == n * calls
        assert (out[mode][0] >= 0).all()
        assert np.array_equal(out[mode][0], out["eager"][0]), (mode, out[mode][0], out["eager"][0])
        assert torch.equal(out[mode][1], out["eager"][1]), (mode, float((out[mode][1] - out["eager"][1]).abs().max()))
    with pytest.raises(ValueError, match="obstacle rasters"):
        T.CapturedTrainStep(None, None, B, parts, (64, 64), True, task=(None, torch.zeros(4096)), task_rows=True, obstacle_rows=True)
    with pytest.raises(ValueError, match="obstacle rasters"):
        T.CapturedTrainStep(None, None, B, parts, (64, 64), True, task=(torch.zeros(4096), None), obstacle_rows=True)


def test_vec_dqn_graph_steps_on_per_env_obstacles_follow_its_eager_steps(monkeypatch):
    """As test_vec_dqn_graph_steps_on_per_env_tasks_follow_its_eager_steps: the eager lock-steps (autograd on the module, the
    obstacle rasters expanded by bits_to_f32) agree bit for bit between the two runs, the losses of the first graph call to 1e-4,
    the weights to Adam's sensitivity."""
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    lr, n_steps, out = 1e-4, 3, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", mode)
        env = random_env(64, seed=7)
        torch.manual_seed(11)
        pol, tgt = make_nets(args, torch.device(DEV))
        agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=lr, fused=True), env, 100000, 16, 0.95, 0.01,
                       "mse_q_values+mse_block_features", seed=2, per_env_tasks=True, per_env_obstacles=True)
        losses = [agent.lockstep(n_steps)[0] for _ in range(3)]
        assert (agent._graph_state is not None) == (mode == "1")
        out[mode] = (losses, torch.cat([p.detach().flatten() for p in pol.parameters()]).cpu())
    for k in range(2):
        assert out["1"][0][k] == out["0"][0][k] and len(out["1"][0][k]) == n_steps
    a, b = np.array(out["1"][0][2]), np.array(out["0"][0][2])
    assert len(a) == n_steps and (a >= 0).all()
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-7)
    diff = (out["1"][1] - out["0"][1]).abs()
    assert float(diff.max()) <= 2 * n_steps * lr and float(diff.mean()) < 0.02 * lr


# ------------------------------------------------------------------------------------------------------------ 7: the loop
LOOP = ["--model", "SuccessorMLP", "--loss_function", "mse_q_values+mse_block_features", "--random_targets", "3", "--random_obstacles", "2",
        "--num_envs", "64", "--eval_envs", "16", "--num_training_steps", "2", "--batch_size", "16", "--seed", "3", "--learning_rate", "1e-4",
        "--max_steps", "6"]


def test_the_loop_trains_on_random_obstacles_and_resumes(tmp_path):
    """run_vectorised with --random_targets 3 --random_obstacles 2 on 64 envs: finite losses, evaluations on held-out tasks, 126-column
    records in the ring and the checkpoint; a run resumed from the checkpoint reproduces the losses of the lock-steps that follow
    (as test_the_loop_trains_on_random_targets_and_resumes); the checkpoint of a targets-only run is refused."""
    from robotoddler.training import records as R
    from robotoddler.training.successor_dqn import build_parser, main
    from robotoddler.training.vec_dqn import run_vectorised
    ckpt_dir = tmp_path / "obst"
    common = [*LOOP, "--checkpoint_every", "150", "--evaluate_every", "120", "--replay_buffer_capacity", "30000"]
    args = vars(build_parser().parse_args([*common, "--num_episodes", "290", "--save_checkpoint", str(ckpt_dir)]))
    a, agent = run_vectorised(args, torch.device(DEV), return_agent=True)
    assert agent.per_env_tasks and agent.per_env_obstacles and agent.env.random_obstacles is not None and agent.env.random_targets is not None
    assert agent.ring.width == agent.ring.data.shape[1] == R.RECORD_WIDTH + 15 == 126 and len(agent.ring) > 500
    losses = [h["avg_loss"] for h in a if h["avg_loss"] is not None]
    assert losses and all(np.isfinite(losses)) and min(losses) >= 0
    assert a[-1]["episodes"] >= 290
    evals = [h["evaluation"] for h in a if "evaluation" in h]
    assert evals and all(ev["episodes"] == 16 and 0.0 <= ev["success_rate"] <= 1.0 for ev in evals)
    tails = agent.ring.data[:len(agent.ring), R.RECORD_WIDTH + 9:].reshape(-1, 2, 3)
    assert bool(((tails[:, :, 0] >= -3) & (tails[:, :, 0] < 3) & (tails[:, :, 1] == 0) & (tails[:, :, 2] >= 0.3) & (tails[:, :, 2] < 2.5)).all())
    assert torch.unique(tails[:, 0, 0]).numel() > 64
    ckpts = sorted(int(d) for d in os.listdir(ckpt_dir) if d.isdigit())
    # the lock-step that ends the run may itself cross the second multiple of 150 (it can finish up to 64 episodes) and write a
    # second checkpoint; only the first is resumed from, and that lock-step is the last one logged either way
    print("checkpoints", ckpts, "episodes per lock-step", [h["episodes"] for h in a])
    assert ckpts and ckpts[0] < 290
    first = os.path.join(str(ckpt_dir), str(ckpts[0]))
    assert torch.load(os.path.join(first, "replay_buffer.pt"), weights_only=True)["records"].shape[1] == 126
    assert tuple(torch.load(os.path.join(first, "agent.pt"), weights_only=True)["task_shape"]) == (3, 2)
    b = main([*common, "--num_episodes", "290", "--load_checkpoint", first])
    by_step = {h["lockstep"]: h for h in a}
    assert b[0]["lockstep"] == min(k for k, h in by_step.items() if h["episodes"] >= ckpts[0]) + 1
    n = 0
    for h in b[:10]:
        ref = by_step[h["lockstep"]]
        assert h["episodes"] == ref["episodes"] and h["env_steps"] == ref["env_steps"] and h["epsilon"] == ref["epsilon"]
        assert h["avg_loss"] == pytest.approx(ref["avg_loss"], rel=1e-4), h["lockstep"]
        n += 1
    assert n >= 5
    # a targets-only run's checkpoint does not load into this loop
    plain_dir = tmp_path / "plain"
    plain = [a_ for i, a_ in enumerate(common) if a_ != "--random_obstacles" and common[i - 1] != "--random_obstacles"]
    main([*plain, "--num_episodes", "160", "--save_checkpoint", str(plain_dir)])
    plain_first = os.path.join(str(plain_dir), str(min(int(d) for d in os.listdir(plain_dir) if d.isdigit())))
    with pytest.raises(ValueError, match="120 columns.*126"):
        main([*common, "--num_episodes", "290", "--load_checkpoint", plain_first])


def test_the_loop_on_random_obstacles_through_a_one_rank_rccl_group_equals_the_plain_run(tmp_path):
    """As test_the_loop_on_random_targets_through_a_one_rank_rccl_group_equals_the_plain_run: the 126-column records pass through
    all_gather_into_tensor; ring and weights agree bit for bit with the run without a process group."""
    def port():
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", 0))
            return s.getsockname()[1]

    argv = [*LOOP[:LOOP.index("--eval_envs")], *LOOP[LOOP.index("--eval_envs") + 2:], "--num_episodes", "200"]
    res = {}
    for name, extra in (("plain", {}), ("rccl", dict(BRIDGES_FORCE_COLLECTIVE="1"))):
        script, outp = tmp_path / f"worker_{name}.py", tmp_path / f"{name}.json"
        script.write_text(WORKER % dict(root=ROOT, pkg=PKG, out=str(outp), argv=argv))
        env = {k: v for k, v in os.environ.items()
               if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "BRIDGES_DIST_BACKEND", "BENCH_DIST_BACKEND")}
        env.update(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4", **extra)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
               "--master-port", str(port()), str(script)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        res[name] = json.load(open(outp))
    p, r = res["plain"], res["rccl"]
    assert p["active"] is False and r["active"] is True and r["backend"] == "nccl"
    assert p["ring_width"] == r["ring_width"] == 126
    assert p["locksteps"] == r["locksteps"] >= 5 and p["episodes"] == r["episodes"] >= 200
    assert p["env_steps"] == r["env_steps"] > 0 and p["ring_size"] == r["ring_size"] > 64
    assert p["ring_hash"] == r["ring_hash"] and p["policy_hash"] == r["policy_hash"]
    assert p["losses"] == r["losses"] and len(p["losses"]) >= 3


# ------------------------------------------------------------------------------------------------------------ 8: nothing moved
def test_a_targets_only_agent_is_what_it_was():
    """VecDQN(per_env_tasks=True) on an env without per-env obstacles, built positionally as tests/test_gpu_vec_dqn_tasks.py builds it,
    against the same agent with the new argument spelled out at its default: losses and weights of 4 lock-steps bit for bit, the
    120-column records, the one shared f32 obstacle map in the captured step; and the refusals on real envs."""
    from bridges_hip.vec_env import RandomTargets
    from robotoddler.training import records as R
    from robotoddler.training.vec_dqn import VecDQN
    out = []
    for kw in ({}, dict(per_env_obstacles=False)):
        env = make_vec(64, [], RandomTargets(), seed=7)
        pol, tgt = make_mlp(HIDDEN[0], 0), make_mlp(HIDDEN[0], 0)
        agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 8192, 16, 0.95, 0.01,
                       "mse_q_values+mse_block_features", seed=3, per_env_tasks=True, **kw)
        assert not agent.per_env_obstacles and agent.ring.width == R.RECORD_WIDTH + 9 == 120 and not agent.replay_env.per_env_obstacles
        losses = [agent.lockstep(2)[0] for _ in range(4)]
        drv = pol._fused_trainer
        assert drv.task_rows and not drv.obstacle_rows and drv._graphs
        assert drv.obstacle.dtype == torch.float32 and tuple(drv.obstacle.shape) == (4096,) and not drv.obstacle.any()
        batch = agent._targets(agent.ring.sample(16, agent.sample_gen))
        assert batch.reward_maps is not None and batch.obstacle_bits is None
        out.append((losses, torch.cat([p.detach().flatten() for p in pol.parameters()]).clone()))
    assert out[0][0] == out[1][0] and all(len(l) == 2 for l in out[0][0][1:]) and torch.equal(out[0][1], out[1][1])
    # refusals on real envs
    env_o = random_env(4)
    mlp = lambda: make_mlp((32, 16), 0)
    mk = lambda env, **kw: VecDQN(mlp(), mlp(), None, env, 64, 8, 0.9, 0.05, "mse_q_values", **kw)
    with pytest.raises(ValueError, match="per-env obstacles.*per_env_obstacles=True"):
        mk(env_o, per_env_tasks=True)
    with pytest.raises(ValueError, match="one shared obstacle list"):
        mk(make_vec(4, [], RandomTargets()), per_env_tasks=True, per_env_obstacles=True)
    pol = mlp()
    agent = VecDQN(pol, mlp(), torch.optim.Adam(pol.parameters(), lr=1e-4), env_o, 64, 8, 0.9, 0.05, "mse_q_values", per_env_tasks=True,
                   per_env_obstacles=True)
    with pytest.raises(ValueError, match="per-env obstacles"):
        agent.evaluate(make_vec(4, [], RandomTargets()))
    with pytest.raises(ValueError):
        env_o.load_task(torch.zeros((4, 9), dtype=torch.float64, device=DEV), torch.zeros((4, 6), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="explicit per-env obstacles"):
        make_vec(4, [], torch.zeros((4, 3, 3), dtype=torch.float64)).load_task(torch.zeros((4, 9), dtype=torch.float64, device=DEV),
                                                                               torch.zeros((4, 6), dtype=torch.float64, device=DEV))
