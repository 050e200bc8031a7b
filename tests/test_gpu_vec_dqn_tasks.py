"""GPU: the vectorised SuccessorMLP DQN on per-env tasks (VecDQN(per_env_tasks=True)) -- the per-row / strided / keyed
operators, records that carry their task, replay that rebuilds it, acting and the optimiser step with a reward map per row, the
loop.  The oracles are what is merged and tested already: the shared-map entry points (bit for bit where every row names one
map), the float64 / module / autograd formulations at the tolerances the existing tests of the shared-map path use
(tests/test_gpu_dqn.py, tests/test_gpu_mlp_step.py, tests/test_gpu_vec_dqn.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from task_draw import draw_targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")

TASKS4 = np.array([[(-1.0, 0.0, 1.5), (1.0, 0.0, 1.0), (2.0, 0.0, 2.5)],
                   [(0.5, 0.0, 0.9), (3.0, 0.0, 1.0), (-2.0, 0.0, 0.4)],
                   [(1.5, 0.0, 2.0), (1.8, 0.0, 2.2), (4.0, 0.0, 3.0)],
                   [(-0.5, 0.0, 0.3), (0.0, 0.0, 1.1), (0.5, 0.0, 1.9)]])


def rel_err(a, b):
    b = b.double()
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def make_vec(E, targets, max_steps=6, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [], targets, max_steps=max_steps, seed=seed, **kw)


def four_task_env(E=256, seed=5, **kw):
    """E envs over the 4 tasks of TASKS4, env e on task e % 4."""
    per_env = torch.from_numpy(TASKS4[np.arange(E) % 4].copy())
    return make_vec(E, per_env, seed=seed, **kw), np.arange(E) % 4


def make_mlp(hidden=(256, 128, 64, 128, 256), seed=0):
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.utils.utils import init_weights
    torch.manual_seed(seed)
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=list(hidden)).to(DEV)
    net.apply(init_weights)
    return net


def make_agent(env, hidden=(256, 128, 64, 128, 256), seed=0, per_env_tasks=True, B=16, loss="mse_q_values+mse_block_features", **kw):
    from robotoddler.training.vec_dqn import VecDQN
    pol, tgt = make_mlp(hidden, seed), make_mlp(hidden, seed)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-4)
    return VecDQN(pol, tgt, opt, env, 8192, B, 0.95, 0.01, loss, seed=3, per_env_tasks=per_env_tasks, **kw)


# ------------------------------------------------------------------------------------------------------------ 1, 2: operators
HEAD_CASES = [(1, 4096), (129, 4096), (1000, 100), (4099, 4096)]      # of test_head_sigmoid_dot_matches_the_two_pass_head


def head_inputs(n, N, n_maps):
    g = torch.Generator(device="cpu").manual_seed(n + N)
    h = torch.relu(torch.randn((n, 256), generator=g)).to(DEV)
    Wd = (torch.randn((N, 256), generator=g) * 0.05).to(DEV)
    bd = (torch.randn(N, generator=g) * 0.1).to(DEV)
    w_all = (torch.rand((n_maps, N), generator=g) * 0.02).to(DEV)
    return h, Wd, bd, w_all, g


@pytest.mark.parametrize("n,N", HEAD_CASES)
def test_head_rows_with_one_map_equals_the_shared_map_head_bit_for_bit(n, N):
    from bridges_hip import ops
    h, Wd, bd, w_all, _ = head_inputs(n, N, 5)
    for k in (0, 3):
        w_row = torch.full((n,), k, dtype=torch.int32, device=DEV)
        for splits in (None, 1, 2, 4):
            if splits is not None and splits > (N + 31) // 32:
                continue
            got = ops.head_sigmoid_dot(h, Wd, bd, w_all, splits=splits, w_row=w_row)
            want = ops.head_sigmoid_dot(h, Wd, bd, w_all[k], splits=splits)
            assert torch.equal(got, want), (k, splits, float((got - want).abs().max()))


@pytest.mark.parametrize("n,N", HEAD_CASES)
@pytest.mark.parametrize("order", ["env_major", "shuffled"])
def test_head_rows_with_distinct_maps_matches_float64(n, N, order):
    """>= 8 distinct random maps; 1e-5 against the float64 value, the figure of the shared-map head's test."""
    from bridges_hip import ops
    M = 11
    h, Wd, bd, w_all, g = head_inputs(n, N, M)
    w_row = (torch.arange(n) * M // max(n, 1)).to(torch.int32) if order == "env_major" else torch.randint(0, M, (n,), generator=g).to(torch.int32)
    if n >= M:
        assert len(set(w_row.tolist())) >= 8
    w_row = w_row.to(DEV)
    want = (torch.sigmoid(h.double() @ Wd.double().T + bd.double()) * w_all.double()[w_row.long()]).sum(dim=1)
    for splits in (None, 3):
        if splits is not None and splits > (N + 31) // 32:
            continue
        got = ops.head_sigmoid_dot(h, Wd, bd, w_all, splits=splits, w_row=w_row)
        assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-5), float((got.double() - want).abs().max())
    padded = torch.zeros((n, 320), device=DEV)
    padded[:, :256] = h                                                          # row stride != K
    assert torch.equal(ops.head_sigmoid_dot(padded[:, :256], Wd, bd, w_all, w_row=w_row), ops.head_sigmoid_dot(h, Wd, bd, w_all, w_row=w_row))


def test_sigmoid_dot_rows():
    """bridges_sigmoid_dot_rows on the inputs of test_sigmoid_dot_matches_torch: one map = the shared entry point bit for bit;
    distinct maps (env-major and shuffled) at 1e-5 against float64."""
    from bridges_hip import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    d = (torch.randn((777, 4096), generator=g) * 3).to(DEV)
    w_all = (torch.rand((9, 4096), generator=g) * 0.02).to(DEV)
    for k in (0, 8):
        w_row = torch.full((777,), k, dtype=torch.int32, device=DEV)
        assert torch.equal(ops.sigmoid_dot(d, w_all, w_row=w_row), ops.sigmoid_dot(d, w_all[k]))
    for w_row in ((torch.arange(777) * 9 // 777).to(torch.int32), torch.randint(0, 9, (777,), generator=g).to(torch.int32)):
        assert len(set(w_row.tolist())) >= 8
        w_row = w_row.to(DEV)
        got = ops.sigmoid_dot(d, w_all, w_row=w_row)
        want = (torch.sigmoid(d.double()) * w_all.double()[w_row.long()]).sum(dim=1)
        assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-5), float((got.double() - want).abs().max())
    view = torch.randn((50, 8192), generator=g).to(DEV)[:, 4096:]                # row stride != k
    w_row = torch.randint(0, 9, (50,), generator=g).to(torch.int32).to(DEV)
    want = (torch.sigmoid(view.double()) * w_all.double()[w_row.long()]).sum(dim=1)
    assert torch.allclose(ops.sigmoid_dot(view, w_all, w_row=w_row).double(), want, rtol=1e-5, atol=1e-5)


def step_batch(n, size, seed, per_row):
    """The batch of tests/test_gpu_mlp_step.py::make_batch, with one reward map per transition when per_row."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    px = size * size
    block = (torch.rand(n, 1, size, size, device=DEV, generator=g) < 0.05).float()
    action = (torch.rand(n, 1, size, size, device=DEV, generator=g) < 0.01).float()
    binary = (torch.rand(n, 6, device=DEV, generator=g) < 0.5).float()
    reward = torch.rand(n if per_row else 1, px, device=DEV, generator=g)
    obstacle = (torch.rand(px, device=DEV, generator=g) < 0.03).float()
    q_t = torch.randn(n, device=DEV, generator=g) * 3
    sf_t = torch.rand(n, px, device=DEV, generator=g)
    return block.reshape(n, px), action.reshape(n, px), binary, reward, obstacle, q_t, sf_t


@pytest.mark.parametrize("batch,px,nf,use_q,use_sf", [(32, 4096, 6, 1, 1), (20, 4096, 6, 1, 0), (7, 1024, 6, 0, 1), (32, 20000, 2, 1, 1)])
def test_strided_input_and_loss_entry_points_equal_the_old_ones_on_copies_of_one_map(batch, px, nf, use_q, use_sf):
    """bridges_mlp_input_rows / _batches_rows / bridges_successor_loss_rows with reward_stride = px over n copies of one map
    against bridges_mlp_input / _batches / bridges_successor_loss on that map: x, dy, loss_rows, q_out, losses bit for bit;
    stride 0 through the new entry points as well; any other stride is refused."""
    from bridges_hip import abi
    from bridges_hip.ops import _ptr, _stream
    L = abi.require_gpu()
    n_batches, rows = 3, 32 * ((batch + 31) // 32)
    n = n_batches * batch
    g = torch.Generator(device=DEV).manual_seed(batch + px)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g)
    block, action, binary = (r(n, px) < 0.05).float(), (r(n, px) < 0.01).float(), (r(n, nf) < 0.5).float()
    reward, obstacle = r(px), (r(px) < 0.03).float()
    copies = reward.expand(n, px).contiguous()
    K, N = 4 * px + nf, 2 * px + 2 * nf
    y = torch.randn(rows, N, device=DEV, generator=g)
    q_t, sf_t = torch.randn(n, device=DEV, generator=g) * 3, r(n, px)
    for c in range(n_batches):
        counter = torch.full((), c, dtype=torch.int64, device=DEV)
        x_old, x_new, x_zero = (torch.full((rows, K), -1.0, device=DEV) for _ in range(3))
        abi.check(L.bridges_mlp_input(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), _ptr(obstacle),
                                      _ptr(x_old), _stream()), "bridges_mlp_input")
        abi.check(L.bridges_mlp_input_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(copies), px,
                                           _ptr(obstacle), _ptr(x_new), _stream()), "bridges_mlp_input_rows")
        abi.check(L.bridges_mlp_input_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), 0,
                                           _ptr(obstacle), _ptr(x_zero), _stream()), "bridges_mlp_input_rows")
        assert torch.equal(x_old, x_new) and torch.equal(x_old, x_zero)
        outs = []
        for stride, rw in ((None, reward), (px, copies), (0, reward)):
            dy, lr, qo = torch.full((rows, N), -1.0, device=DEV), torch.full((rows,), -1.0, device=DEV), torch.full((rows,), -1.0, device=DEV)
            losses, cnt = torch.zeros(n_batches, device=DEV), counter.clone()
            tail = (_ptr(cnt), _ptr(q_t) if use_q else None, _ptr(sf_t) if use_sf else None, use_q, use_sf, _ptr(dy), _ptr(lr), _ptr(qo),
                    _ptr(losses), n_batches, _ptr(cnt), None, None, _stream())
            if stride is None:
                abi.check(L.bridges_successor_loss(batch, rows, px, nf, _ptr(y), _ptr(rw), *tail), "bridges_successor_loss")
            else:
                abi.check(L.bridges_successor_loss_rows(batch, rows, px, nf, _ptr(y), _ptr(rw), stride, *tail), "bridges_successor_loss_rows")
            assert int(cnt) == c + 1
            outs.append((dy, lr, qo, losses))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(a, b)
    xa, xb = torch.full((n_batches * rows, K), -1.0, device=DEV), torch.full((n_batches * rows, K), -1.0, device=DEV)
    abi.check(L.bridges_mlp_input_batches(n_batches, batch, rows, px, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), _ptr(obstacle),
                                          _ptr(xa), _stream()), "bridges_mlp_input_batches")
    abi.check(L.bridges_mlp_input_batches_rows(n_batches, batch, rows, px, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(copies), px,
                                               _ptr(obstacle), _ptr(xb), _stream()), "bridges_mlp_input_batches_rows")
    assert torch.equal(xa, xb)
    assert L.bridges_mlp_input_batches_rows(n_batches, batch, rows, px, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(copies), px + 4,
                                            _ptr(obstacle), _ptr(xb), _stream()) == -1
    assert L.bridges_mlp_input_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(copies), 1,
                                    _ptr(obstacle), _ptr(x_new), _stream()) == -1


def test_strided_input_rows_with_distinct_maps_hold_each_transitions_map():
    """x of bridges_mlp_input_rows / _batches_rows with a map per transition: exactly the concatenation the module forward builds
    (cv.py:100-103) -- a copy kernel, so bit for bit."""
    from bridges_hip import abi
    from bridges_hip.ops import _ptr, _stream
    L = abi.require_gpu()
    batch, rows, px, nf, n_batches = 20, 32, 4096, 6, 3
    n = n_batches * batch
    block, action, binary, reward, obstacle, _, _ = step_batch(n, 64, 77, per_row=True)
    want = torch.cat([block, action, reward, obstacle.expand(n, px), binary], dim=1)
    x_all = torch.full((n_batches * rows, 4 * px + nf), -1.0, device=DEV)
    abi.check(L.bridges_mlp_input_batches_rows(n_batches, batch, rows, px, nf, _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), px,
                                               _ptr(obstacle), _ptr(x_all), _stream()), "bridges_mlp_input_batches_rows")
    for c in range(n_batches):
        assert torch.equal(x_all[c * rows:c * rows + batch], want[c * batch:(c + 1) * batch])
        assert not x_all[c * rows + batch:(c + 1) * rows].any()
        x = torch.full((rows, 4 * px + nf), -1.0, device=DEV)
        counter = torch.full((), c, dtype=torch.int64, device=DEV)
        abi.check(L.bridges_mlp_input_rows(batch, rows, px, nf, _ptr(counter), _ptr(block), _ptr(action), _ptr(binary), _ptr(reward), px,
                                           _ptr(obstacle), _ptr(x), _stream()), "bridges_mlp_input_rows")
        assert torch.equal(x, x_all[c * rows:(c + 1) * rows])


def _state_keys(env, flag, task):
    nb = env.n_blocks.cpu().numpy()
    shape, pose, occ = env.blk_shape.cpu().numpy(), env.blk_pose.cpu().numpy().view(np.int64), env.blk_occ.cpu().numpy()
    fl = flag.cpu().numpy().astype(np.uint8)
    tg = env.env_targets.cpu().numpy().view(np.int64)
    return [(int(nb[e]), shape[e, :nb[e]].tobytes(), pose[e, :nb[e]].tobytes(), occ[e, :nb[e]].tobytes(), int(fl[e]),
             tg[e].tobytes() if task else b"") for e in range(env.E)]


def _first_of_key(keys):
    first = {}
    return np.array([first.setdefault(k, e) for e, k in enumerate(keys)])


def test_keyed_groups_with_a_constant_key_equal_the_plain_groups():
    from bridges_hip import abi
    from bridges_hip.ops import _ptr, _stream
    L = abi.require_gpu()
    env, _ = four_task_env(200, seed=3)
    E = env.E
    for it in range(5):
        flag = ((env.step_flags[:, 1] != 0) | (env.n_blocks == 0)).to(torch.uint8).contiguous()
        plain = env.state_groups(flag)
        for n_extra in (1, 9, 70):
            extra = torch.full((E, n_extra), 0x1234567 + it, dtype=torch.int64, device=DEV)
            hkey, rep = torch.empty(E, dtype=torch.int64, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV)
            b = env.buf
            abi.check(L.bridges_env_groups_keyed(E, env.K, _ptr(b["n_blocks"]), _ptr(b["blk_shape"]), _ptr(b["blk_pose"]), _ptr(b["blk_occ"]),
                                                 _ptr(flag), _ptr(extra), n_extra, _ptr(hkey), _ptr(rep), _stream()), "bridges_env_groups_keyed")
            assert torch.equal(rep, plain), (it, n_extra)
        assert torch.equal(env.state_groups(flag, task=False), plain)
        env.select_random()
        env.step()


# ------------------------------------------------------------------------------------------------------------ 4: grouping
def test_groups_are_shared_by_state_and_task():
    env, task_of = four_task_env(256, seed=3)
    E = env.E
    tg = env.env_targets.cpu().numpy()
    shared_some = False
    for it in range(6):
        flag = (env.step_flags[:, 1] != 0) | (env.n_blocks == 0)
        rep = env.state_groups(flag, task=True).cpu().numpy()
        assert np.array_equal(rep, _first_of_key(_state_keys(env, flag, True))), it
        assert np.array_equal(tg[rep], tg)                                  # never grouped across tasks
        if it == 0:
            assert np.array_equal(rep, task_of) and len(set(rep.tolist())) == 4      # freshly reset: the first env of e's task
        shared_some |= bool((rep != np.arange(E)).any()) and it > 0
        rep_plain = env.state_groups(flag).cpu().numpy()
        assert np.array_equal(rep_plain, _first_of_key(_state_keys(env, flag, False))), it      # task=False: today's result
        if it == 0:
            assert (rep_plain == 0).all()
        env.select_random()
        env.step()
    assert shared_some
    # two envs in the same state whose tasks differ in ONE bit of one coordinate
    t = env.env_targets.clone()
    t[:] = t[0]
    t[7, 2, 2] = torch.nextafter(t[7, 2, 2], t[7, 2, 2] + 1)
    env.set_targets(t)
    rep = env.state_groups(None, task=True).cpu().numpy()
    assert rep[7] == 7 and (np.delete(rep, 7) == 0).all()


@pytest.mark.parametrize("hidden", [(256, 128, 64, 128, 256), (256, 128, 192)])
def test_acting_on_rows_shared_by_state_and_task_equals_every_envs_own_rows(hidden):
    from robotoddler.training.vec_dqn import VecDQN
    env, _ = four_task_env(256, seed=17, f32_rasters=False)
    agent = make_agent(env, hidden, seed=12)
    E = env.E
    try:
        for it in range(5):
            stable = agent._stable_flags(env)
            VecDQN.DEDUP_STATES = False
            env._dqn_rows = None
            idx_a, env_a, (lo_a, hi_a), rep_a = agent._rows(env, stable)
            assert rep_a is None
            idx_a, env_a = idx_a.clone(), env_a.clone()
            q_a = agent._policy_q(env, idx_a, env_a, stable).clone()
            VecDQN.DEDUP_STATES = True
            env._dqn_rows = None
            idx_s, env_s, (lo_s, hi_s), rep = agent._rows(env, stable)
            q_s = agent._policy_q(env, idx_s, env_s, stable)
            assert idx_s.numel() < idx_a.numel()
            src = torch.cat([torch.arange(int(lo_s[e]), int(hi_s[e]), device=DEV) for e in range(E)])
            assert src.numel() == idx_a.numel()
            assert torch.allclose(q_s[src], q_a, rtol=1e-5, atol=1e-5), float((q_s[src] - q_a).abs().max())
            env._dqn_rows = None
            agent.act()
    finally:
        VecDQN.DEDUP_STATES = True


# ------------------------------------------------------------------------------------------------------------ 3: acting forward
@pytest.mark.parametrize("hidden", [(256, 128, 64, 128, 256), (256, 128, 192)])
def test_acting_forward_with_a_map_per_env(hidden):
    """_net_q of the per-env-task agent against (a) the module forward with every row's own map and (b) _net_q of a fixed-task
    agent on an env of task k with the same seed, for the envs of task k -- all rows, rtol = atol = 1e-5."""
    from bridges_hip import ops
    E, seed = 256, 9
    env, task_of = four_task_env(E, seed=seed, f32_rasters=True)
    fixed = [make_vec(E, [tuple(t) for t in TASKS4[k]], seed=seed, f32_rasters=False) for k in range(4)]
    agent = make_agent(env, hidden, seed=3)
    fixed_agents = [make_agent(f, hidden, seed=3, per_env_tasks=False) for f in fixed]
    net = agent.policy_net
    for f in fixed_agents:
        assert torch.equal(torch.cat([p.flatten() for p in f.policy_net.parameters()]), torch.cat([p.flatten() for p in net.parameters()]))
    for it in range(4):
        for v in [env] + fixed:
            v.select_random()
            v.step()
        stable = agent._stable_flags(env)
        idx, row_env = env.valid_rows()
        n = idx.numel()
        q = agent._net_q(net, env, idx, row_env, stable)
        assert q.shape == (n,) and n > 2000
        # (a) the module forward, row by row its env's map
        binary = torch.zeros((n, 6), device=DEV)
        binary[:, 0] = stable[row_env].float()
        q_mod = []
        with torch.no_grad():
            net.eval()
            for o in range(0, n, 2048):
                sl = slice(o, min(o + 2048, n))
                q_mod.append(net(env.state_raster[row_env[sl]].unsqueeze(1), binary[sl], env.cand_raster[idx[sl]].unsqueeze(1),
                                 env.reward_maps_img[row_env[sl]].unsqueeze(1),
                                 env.obstacle_raster.unsqueeze(0).expand(sl.stop - sl.start, -1, -1, -1))[0])
        q_mod = torch.cat(q_mod)
        assert torch.allclose(q, q_mod, rtol=1e-5, atol=1e-5), (it, float((q - q_mod).abs().max()))
        # (b) the fixed-task agent of every task on the envs of that task
        for k, (f, fa) in enumerate(zip(fixed, fixed_agents)):
            mine = torch.from_numpy(task_of == k).to(DEV)
            assert torch.equal(env.n_blocks[mine], f.n_blocks[mine]) and torch.equal(env.blk_pose[mine], f.blk_pose[mine])
            assert torch.equal(env.blk_shape[mine], f.blk_shape[mine]) and torch.equal(env.n_valid[:E][mine], f.n_valid[:E][mine])
            idx_f, env_f = f.valid_rows()
            q_f = fa._net_q(fa.policy_net, f, idx_f, env_f, fa._stable_flags(f))
            a, b = q[mine[row_env]], q_f[mine[env_f]]
            assert a.numel() == b.numel() > 0
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), (it, k, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------------------ 5: records
def test_records_carry_the_task_the_transition_was_taken_under():
    from bridges_hip.vec_env import RandomTargets
    from robotoddler.training import records as R
    E, seed = 64, 11
    env = make_vec(E, RandomTargets(), seed=seed, f32_rasters=False)
    agent = make_agent(env, seed=1)
    assert agent.ring.width == R.RECORD_WIDTH + 9 == 120 and agent.ring.data.shape[1] == 120
    cap, inner = {}, env.step

    def step(sel_index=None):                                   # what the lock-step held right before env.step()
        sel = env.cand_offset[:E].long() + sel_index.long()
        cap.update(snap=R.snapshot(env), sel_rows=(env.cand_desc[sel].clone(), env.cand_pose[sel].clone()),
                   targets=env.env_targets.clone(), episode=env.task_episode.clone())
        inner(sel_index)

    env.step = step
    ended = redrawn = 0
    for it in range(24):
        rec, valid = agent.act()
        want, want_valid = R.make_records(env, cap["snap"], cap["sel_rows"])
        assert torch.equal(valid, want_valid)
        assert tuple(rec.shape) == (E, R.RECORD_WIDTH) and torch.equal(rec, want), it
        full = agent.with_task(rec)
        assert tuple(full.shape) == (E, 120) and torch.equal(full[:, :R.RECORD_WIDTH], want)
        assert torch.equal(full[:, R.RECORD_WIDTH:].reshape(E, 3, 3), cap["targets"])
        tail, ep = full[:, R.RECORD_WIDTH:].reshape(E, 3, 3).cpu().numpy(), cap["episode"].cpu().numpy()
        for e in range(E):
            assert np.array_equal(tail[e], np.array(draw_targets(seed, e, int(ep[e])))), (it, e)
        ended += int((valid & (rec[:, R.O_DONE] > 0.5)).sum())
        redrawn += int((env.task_episode != cap["episode"]).sum())
        agent.ring.push(full[valid])
    assert ended > E and redrawn > E and int(env.task_episode.min()) >= 1
    assert len(agent.ring) > 10 * E


# ------------------------------------------------------------------------------------------------------------ 6: replay
def rollout_agent(E=64, seed=11, locksteps=12, **kw):
    from bridges_hip.vec_env import RandomTargets
    env = make_vec(E, RandomTargets(), seed=seed, f32_rasters=False)
    agent = make_agent(env, seed=1, **kw)
    with torch.no_grad():                                       # the target net is a copy of the policy net: make it its own
        for p in agent.target_net.parameters():
            p.mul_(1.05)
    for _ in range(locksteps):
        rec, valid = agent.act()
        agent.ring.push(agent.with_task(rec)[valid])
    return env, agent


@pytest.mark.parametrize("n", [10, 16, 40])
def test_replay_rebuilds_every_transitions_task(n):
    from bridges_hip import ops
    from robotoddler.training import records as R
    env, agent = rollout_agent()
    gamma = agent.gamma
    rec = agent.ring.sample(n, agent.sample_gen)
    assert rec.shape[1] == 120
    batch = agent._targets(rec)
    action_f, q_target, sf_target, maps = batch.action_f, batch.q_target, batch.sf_target, batch.reward_maps
    renv = agent.replay_env
    Er = renv.E
    assert Er >= n and renv.per_env_tasks and tuple(maps.shape) == (n, 4096)
    tails = rec[:, R.RECORD_WIDTH:].reshape(n, 3, 3)
    assert torch.equal(renv.env_targets[:n], tails) and bool((renv.env_targets[n:] == tails[0]).all())
    for i in range(n):
        fx = make_vec(1, [tuple(t) for t in tails[i].tolist()], f32_rasters=False)
        assert torch.equal(renv.reward_maps[i], fx.reward_map), i
        assert torch.equal(maps[i].reshape(64, 64), fx.reward_map), i
        assert torch.equal(renv.reward_prefix[i], fx.reward_prefix), i
    # the targets from the module forward of the target net, every candidate row with the map of its transition
    tgt = agent.target_net
    idx, row_env = renv.valid_rows()
    idx, row_env = idx.clone(), row_env.clone()
    keep = row_env < n
    idx, row_env = idx[keep], row_env[keep]
    stable_n = rec[:, R.O_STABLE_N] > 0.5
    m = idx.numel()
    bin_rows = torch.zeros((m, 6), device=DEV)
    bin_rows[:, 0] = stable_n[row_env].float()
    with torch.no_grad():
        tgt.eval()
        q_all, sf_all, _ = tgt(ops.bits_to_f32(renv.state_bits[row_env]).unsqueeze(1), bin_rows, ops.bits_to_f32(renv.cand_bits[idx]).unsqueeze(1),
                               renv.reward_maps_img[row_env].unsqueeze(1), renv.obstacle_raster.unsqueeze(0).expand(m, -1, -1, -1))
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
    with pytest.raises(ValueError, match="120"):
        agent._targets(rec[:, :R.RECORD_WIDTH])


def batch_agent(mode, E=16, B=8):
    """An agent of every mode that fills other fields of the batch, on E envs (two obstacles per env where the mode has them)."""
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomObstacles, RandomTargets, VecAssemblyGym
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    tasks, obstacles, conv = mode != "plain", mode.endswith("obstacles"), mode.startswith("conv")
    env = VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], RandomObstacles([((-3.0, 3.0), (0.3, 2.5))] * 2) if obstacles else [],
                         RandomTargets() if tasks else [tuple(t) for t in TASKS4[0]], max_steps=6, seed=11, f32_rasters=not tasks)
    if not conv:
        return make_agent(env, per_env_tasks=tasks, B=B, per_env_obstacles=obstacles)
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 8192, B, 0.95, 0.01, "mse_q_values", seed=3,
                  per_env_tasks=True, per_env_obstacles=obstacles, task_channels=True)


@pytest.mark.parametrize("mode", ["plain", "tasks", "tasks+obstacles", "conv", "conv+obstacles"])
def test_target_batch_fields_by_mode(mode):
    """Which fields of _targets' batch a mode fills, their shapes and dtypes, the bit rasters against the f32 images where both
    exist, and one optimiser step on what train_steps picks from the batch by name."""
    from bridges_hip import ops
    from robotoddler.training.vec_dqn import TargetBatch
    agent = batch_agent(mode)
    for _ in range(5):
        rec, valid = agent.act()
        agent.ring.push(agent.with_task(rec)[valid])
    n, px = 16, 4096
    batch = agent._targets(agent.ring.sample(n, agent.sample_gen))
    assert isinstance(batch, TargetBatch)
    is_f32 = lambda t, *shape: torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == shape
    is_bits = lambda t: torch.is_tensor(t) and t.dtype == torch.int64 and tuple(t.shape) == (n, 64)
    assert is_f32(batch.binary, n, 6) and is_f32(batch.q_target, n) and is_bits(batch.state_bits) and is_bits(batch.action_bits)
    if mode.startswith("conv"):                              # (mse_q_values alone: no successor-feature target either)
        assert batch.block_f is None and batch.action_f is None and batch.sf_target is None
    else:
        assert is_f32(batch.block_f, n, 1, 64, 64) and is_f32(batch.action_f, n, 1, 64, 64) and is_f32(batch.sf_target, n, px)
        assert torch.equal(ops.bits_to_f32(batch.state_bits), batch.block_f.squeeze(1))
        assert torch.equal(ops.bits_to_f32(batch.action_bits), batch.action_f.squeeze(1))
    assert batch.reward_maps is None if mode == "plain" else is_f32(batch.reward_maps, n, px)
    assert is_bits(batch.obstacle_bits) if mode.endswith("obstacles") else batch.obstacle_bits is None
    losses = agent.train_steps(1)
    assert len(losses) == 1 and np.isfinite(losses[0])


# ------------------------------------------------------------------------------------------------------------ 7: optimiser step
def autograd_step_rows(net, batch, rows, size, use_q, use_sf):
    block, action, binary, reward, obstacle, q_t, sf_t = batch
    B = rows.stop - rows.start
    img = lambda t: t.reshape(-1, 1, size, size)
    for p in net.parameters():
        p.grad = None
    q, sf, _ = net(img(block[rows]), binary[rows], img(action[rows]), img(reward[rows]), obstacle.reshape(1, 1, size, size).expand(B, -1, -1, -1))
    mse = torch.nn.MSELoss()
    loss = 0.
    if use_q:
        loss = loss + mse(q, q_t[rows])
    if use_sf:
        loss = loss + mse(sf[:, 0].reshape(B, -1), sf_t[rows])
    loss.backward()
    return float(loss.detach()), q.detach(), [p.grad.clone() for p in net.parameters()]


def make_step_net(hidden, size, seed):
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.utils.utils import init_weights
    torch.manual_seed(seed)
    net = SuccessorMLP(img_size=(size, size), hidden_dims=list(hidden)).to(DEV)
    net.apply(init_weights)
    return net


@pytest.mark.parametrize("prebuilt", [False, True])
@pytest.mark.parametrize("B,size,hidden,use_q,use_sf", [(32, 64, (256, 128, 64, 128, 256), True, True),
                                                        (32, 64, (256, 128, 64, 128, 256), False, True),
                                                        (16, 64, (256, 128, 64, 128, 256), True, False),
                                                        (4, 64, (128, 64, 128), True, True),
                                                        (48, 32, (96, 40), True, True)])
def test_fused_step_with_a_map_per_transition_matches_autograd(B, size, hidden, use_q, use_sf, prebuilt):
    """The cases and tolerances of tests/test_gpu_mlp_step.py::test_fused_step_matches_autograd, every transition with a reward map
    of its own: loss, q and every gradient (the first layer's reward columns included) against autograd on the module."""
    from bridges_hip.mlp_ops import FusedSuccessorStep
    net = make_step_net(hidden, size, seed=B)
    n_batches = 3
    batch = step_batch(n_batches * B, size, seed=B + size, per_row=True)
    block, action, binary, reward, obstacle, q_t, sf_t = batch
    refs = [autograd_step_rows(net, batch, slice(i * B, (i + 1) * B), size, use_q, use_sf) for i in range(n_batches)]
    for p in net.parameters():
        p.grad = None
    fused = FusedSuccessorStep(net, B, use_q, use_sf)
    if prebuilt:
        fused.allocate_inputs(n_batches)
        fused.prepare_inputs(n_batches, block, action, binary, reward, obstacle)
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    losses = torch.zeros(n_batches, device=DEV)
    for i in range(n_batches):
        fused.launch(counter, block, action, binary, reward, obstacle, q_t, sf_t, losses)
        loss_ref, q_ref, grads_ref = refs[i]
        assert int(counter) == i + 1
        assert abs(float(losses[i]) - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref)), (i, float(losses[i]), loss_ref)
        assert rel_err(fused.q[:B], q_ref) < 1e-5
        for p, gref in zip(net.parameters(), grads_ref):
            assert rel_err(p.grad, gref) < 1e-5, (i, tuple(p.shape), rel_err(p.grad, gref))


def test_three_adam_steps_with_a_map_per_transition_follow_the_autograd_run():
    """tests/test_gpu_mlp_step.py::test_flat_adam_launch_follows_torch_adam with per-transition maps: losses and parameters after
    three optimiser steps of the fused step (Adam inside its launches) against autograd + torch.optim.Adam, same tolerances."""
    from bridges_hip.dqn_ops import FlatParameters
    from bridges_hip.mlp_ops import FusedSuccessorStep
    B, size = 32, 64
    hidden = (256, 128, 64, 128, 256)
    batch = step_batch(3 * B, size, seed=5, per_row=True)
    block, action, binary, reward, obstacle, q_t, sf_t = batch
    net_a, net_b = make_step_net(hidden, size, 9), make_step_net(hidden, size, 9)
    net_b._flat_params = FlatParameters(net_b)
    opt_a = torch.optim.Adam(net_a.parameters(), lr=1e-3, fused=True)
    opt_b = torch.optim.Adam(net_b.parameters(), lr=1e-3, fused=True)
    losses_a = []
    for i in range(3):
        losses_a.append(autograd_step_rows(net_a, batch, slice(i * B, (i + 1) * B), size, True, True)[0])
        opt_a.step()
    fused = FusedSuccessorStep(net_b, B, True, True, optimizer=opt_b)
    assert fused.fused_adam
    counter = torch.zeros((), dtype=torch.int64, device=DEV)
    losses_b = torch.zeros(3, device=DEV)
    for i in range(3):
        fused.launch(counter, block, action, binary, reward, obstacle, q_t, sf_t, losses_b)
    assert int(counter) == 3 and float(fused.adam_step) == 3.0
    np.testing.assert_allclose(losses_b.cpu().numpy(), np.array(losses_a), rtol=2e-5)
    for pa, pb in zip(net_a.parameters(), net_b.parameters()):
        assert rel_err(pb.detach(), pa.detach()) < 2e-4
        sa, sb = opt_a.state[pa], opt_b.state[pb]
        assert rel_err(sb["exp_avg"], sa["exp_avg"]) < 1e-4 and rel_err(sb["exp_avg_sq"], sa["exp_avg_sq"]) < 1e-4


@pytest.mark.parametrize("loss", ["mse_q_values+mse_block_features", "mse_block_features"])
def test_captured_step_with_a_map_per_transition_equals_the_eager_launches(loss, monkeypatch):
    """CapturedTrainStep(task_rows=True): 6 calls x 4 optimiser steps = 24 steps, the per-transition maps of every call copied into
    the static buffer the captured launches read, against the same launches queued eagerly (BRIDGES_TRAIN_GRAPH=0) on the same
    batches: losses and weights at the tolerances of test_graph_captured_train_step_equals_eager."""
    from bridges_hip.dqn_ops import FlatParameters
    from robotoddler.training import train_step as T
    B, size, n, calls = 32, 64, 4, 6
    hidden = (256, 128, 64, 128, 256)
    parts = loss.split('+')
    batches = [step_batch(n * B, size, seed=100 + c, per_row=True) for c in range(calls)]
    out = {}
    # eager launches; the graph as train_policy_net drives it (first call eager, rows built inside the step); the graph as
    # VecDQN drives it (captured on its first call, the first layer's rows of all batches pre-built per call)
    for mode, graph, prepared, warmup in (("eager", "0", False, 1), ("graph", "1", False, 1), ("prepared", "1", True, 0)):
        monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", graph)
        net = make_step_net(hidden, size, 4)
        net._flat_params = FlatParameters(net)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True)
        for g in opt.param_groups:
            g['capturable'] = True
        obstacle = batches[0][4]
        drv = T.CapturedTrainStep.of(net, opt, B, parts, n, img=(size, size), fused=True, graph_default=True, warmup=warmup,
                                     eager_body=True, prepared=prepared, task=(None, obstacle), task_rows=True)
        losses = []
        for block, action, binary, reward, _obst, q_t, sf_t in batches:
            got = drv.run(n, block, action, binary, reward, None, q_t if 'mse_q_values' in parts else None,
                          sf_t if 'mse_block_features' in parts else None)
            losses += got.tolist()
        assert bool(drv._graphs) == (graph == "1")
        T.release(net)
        out[mode] = (np.array(losses), torch.cat([p.detach().flatten() for p in net.parameters()]).cpu())
    for mode in ("graph", "prepared"):
        assert len(out[mode][0]) == len(out["eager"][0]) == n * calls >= 18
        assert (out[mode][0] >= 0).all()
        np.testing.assert_allclose(out[mode][0], out["eager"][0], rtol=1e-4, atol=1e-6)
        assert torch.allclose(out[mode][1], out["eager"][1], rtol=1e-4, atol=1e-6), (mode, float((out[mode][1] - out["eager"][1]).abs().max()))
    with pytest.raises(ValueError, match="per-transition"):
        T.CapturedTrainStep(None, None, B, parts, (size, size), False, task=(None, None), task_rows=True)


def test_vec_dqn_graph_steps_on_per_env_tasks_follow_its_eager_steps(monkeypatch):
    """VecDQN(per_env_tasks=True).lockstep with the captured hand-written step against the same loop stepping eagerly through
    autograd on the module with per-transition maps (BRIDGES_TRAIN_GRAPH=0): as
    test_hand_written_mlp_step_in_the_graph_follows_the_autograd_graph -- the eager lock-steps agree bit for bit, the losses of the
    first graph call to 1e-4, the weights to Adam's sensitivity."""
    from bridges_hip.vec_env import RandomTargets
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    lr, n_steps, out = 1e-4, 3, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", mode)
        env = make_vec(64, RandomTargets(), seed=7, f32_rasters=False)
        torch.manual_seed(11)
        pol, tgt = make_nets(args, torch.device(DEV))
        agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=lr, fused=True), env, 100000, 16, 0.95, 0.01,
                       "mse_q_values+mse_block_features", seed=2, per_env_tasks=True)
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


# ------------------------------------------------------------------------------------------------------------ 8: the loop
LOOP = ["--model", "SuccessorMLP", "--loss_function", "mse_q_values+mse_block_features", "--random_targets", "3", "--num_envs", "256",
        "--eval_envs", "32", "--num_training_steps", "2", "--batch_size", "16", "--seed", "3", "--learning_rate", "1e-4"]


def test_the_loop_trains_on_random_targets_and_resumes(tmp_path):
    """run_vectorised with --random_targets 3 on 256 envs: finite losses, per-episode statistics, evaluations on the held-out tasks,
    120-column records in the ring and in the checkpoint; a second run resumed from the first checkpoint reproduces the losses
    of the lock-steps that follow (as test_load_checkpoint_resumes_the_vectorised_loop)."""
    from robotoddler.training import records as R
    from robotoddler.training.successor_dqn import build_parser, main
    from robotoddler.training.vec_dqn import run_vectorised
    # (one checkpoint only: the saving run resets its envs at every checkpoint, the resumed run below saves none; the ring must not have wrapped at the checkpoint: a saved ring is reloaded oldest record first, i.e. rotated, and uniform
    # sampling indexes slots -- as in test_load_checkpoint_resumes_the_vectorised_loop, whose ring is not full either)
    common = [*LOOP, "--checkpoint_every", "600", "--evaluate_every", "500", "--replay_buffer_capacity", "30000"]
    args = vars(build_parser().parse_args([*common, "--num_episodes", "1150", "--save_checkpoint", str(tmp_path)]))
    a, agent = run_vectorised(args, torch.device(DEV), return_agent=True)
    assert agent.per_env_tasks and agent.env.per_env_tasks and agent.env.random_targets is not None
    assert agent.ring.width == agent.ring.data.shape[1] == R.RECORD_WIDTH + 9 == 120 and len(agent.ring) > 1000
    losses = [h["avg_loss"] for h in a if h["avg_loss"] is not None]
    assert losses and all(np.isfinite(losses)) and min(losses) >= 0
    assert sum(h["episodes_finished"] or 0 for h in a) >= 800 and a[-1]["episodes"] >= 1150
    evals = [h["evaluation"] for h in a if "evaluation" in h]
    assert evals and all(ev["episodes"] == 32 and 0.0 <= ev["success_rate"] <= 1.0 for ev in evals)
    # the live records' tails are tasks of the sampler's range
    tails = agent.ring.data[:len(agent.ring), R.RECORD_WIDTH:].reshape(-1, 3, 3)
    assert bool(((tails[:, :, 0] >= -4) & (tails[:, :, 0] < 4) & (tails[:, :, 1] == 0) & (tails[:, :, 2] >= 0) & (tails[:, :, 2] < 4)).all())
    assert torch.unique(tails[:, 0, 0]).numel() > 256
    ckpts = sorted(int(d) for d in os.listdir(tmp_path) if d.isdigit())
    assert ckpts and ckpts[0] < 1150
    first = os.path.join(str(tmp_path), str(ckpts[0]))
    blob = torch.load(os.path.join(first, "replay_buffer.pt"), weights_only=True)
    assert blob["records"].shape[1] == 120
    b = main([*common, "--num_episodes", "1150", "--load_checkpoint", first])
    by_step = {h["lockstep"]: h for h in a}
    assert b[0]["lockstep"] == min(k for k, h in by_step.items() if h["episodes"] >= ckpts[0]) + 1
    n = 0
    for h in b[:20]:
        ref = by_step[h["lockstep"]]
        assert h["episodes"] == ref["episodes"] and h["env_steps"] == ref["env_steps"]
        assert h["epsilon"] == ref["epsilon"]
        assert h["avg_loss"] == pytest.approx(ref["avg_loss"], rel=1e-4), h["lockstep"]
        n += 1
    assert n >= 10


WORKER = r'''
import hashlib, json, os, sys
sys.path[:0] = [%(root)r, %(pkg)r]
import numpy as np, torch
import torch.distributed as dist
from robotoddler.training import distributed as D
from robotoddler.training import successor_dqn as S
from robotoddler.training.vec_dqn import run_vectorised
args = vars(S.build_parser().parse_args(%(argv)r))
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
hist, agent = run_vectorised(args, dev, return_agent=True)
torch.cuda.synchronize()
ring = agent.ring
order = (ring.head - ring.size + torch.arange(ring.size, device=ring.data.device)) %% ring.capacity
rec = ring.data[order].cpu().numpy()
w = agent.policy_net._flat_params.flat.detach().cpu().numpy()
out = dict(locksteps=len(hist), ring_size=int(ring.size), ring_width=int(ring.data.shape[1]), ring_hash=hashlib.sha256(rec.tobytes()).hexdigest(),
           policy_hash=hashlib.sha256(w.tobytes()).hexdigest(), episodes=int(agent.episodes_done), env_steps=int(agent.env_steps),
           losses=[h["avg_loss"] for h in hist if h["avg_loss"] is not None],
           active=bool(D.active()), backend=(dist.get_backend() if dist.is_initialized() else None))
if D.active():
    dist.barrier()
    dist.destroy_process_group()
json.dump(out, open(%(out)r, "w"))
'''


def test_the_loop_on_random_targets_through_a_one_rank_rccl_group_equals_the_plain_run(tmp_path):
    """As tests/test_gpu_one_rank_rccl.py::test_vectorised_loop_through_rccl_equals_the_plain_single_rank_loop: the 120-column records
    pass through all_gather_into_tensor; ring and weights agree bit for bit with the run without a process group."""
    def port():
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", 0))
            return s.getsockname()[1]

    argv = [*LOOP[:LOOP.index("--eval_envs")], *LOOP[LOOP.index("--eval_envs") + 2:], "--num_episodes", "900"]
    res = {}
    for name, extra in (("plain", {}), ("rccl", dict(BRIDGES_FORCE_COLLECTIVE="1"))):
        script, outp = tmp_path / f"worker_{name}.py", tmp_path / f"{name}.json"
        script.write_text(WORKER % dict(root=ROOT, pkg=PKG, out=str(outp), argv=argv))
        env = {k: v for k, v in os.environ.items()
               if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "BRIDGES_DIST_BACKEND", "BENCH_DIST_BACKEND")}
        env.update(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4", **extra)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
               "--master-port", str(port()), str(script)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        res[name] = json.load(open(outp))
    p, r = res["plain"], res["rccl"]
    assert p["active"] is False and r["active"] is True and r["backend"] == "nccl"
    assert p["ring_width"] == r["ring_width"] == 120
    assert p["locksteps"] == r["locksteps"] >= 5 and p["episodes"] == r["episodes"] >= 900
    assert p["env_steps"] == r["env_steps"] > 0 and p["ring_size"] == r["ring_size"] > 256
    assert p["ring_hash"] == r["ring_hash"] and p["policy_hash"] == r["policy_hash"]
    assert p["losses"] == r["losses"] and len(p["losses"]) >= 3


# ------------------------------------------------------------------------------------------------------------ 9: refusals on real envs
def test_refusals_and_defaults_on_real_envs(monkeypatch):
    from bridges_hip.vec_env import RandomTargets
    from robotoddler.models.cv import ConvNet, SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    vec = make_vec(4, RandomTargets(), f32_rasters=False)
    mlp = lambda s=64: SuccessorMLP(img_size=(s, s), hidden_dims=[32, 16]).to(DEV)
    mk = lambda pol, tgt, env, **kw: VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 64, 8, 0.9, 0.05,
                                           "mse_q_values", **kw)
    with pytest.raises(ValueError, match="per-env tasks.*per_env_tasks=True"):
        mk(mlp(), mlp(), vec)                                              # the default still refuses, and names the option
    with pytest.raises(ValueError, match="ConvNet"):
        mk(ConvNet(img_size=(64, 64)).to(DEV), ConvNet(img_size=(64, 64)).to(DEV), vec, per_env_tasks=True)
    with pytest.raises(ValueError, match="64x64"):
        mk(mlp(32), mlp(32), vec, per_env_tasks=True)
    with pytest.raises(ValueError, match="fixed task"):
        mk(mlp(), mlp(), make_vec(4, [(0.5, 0.0, 1.0)], f32_rasters=False), per_env_tasks=True)
    monkeypatch.setenv("BRIDGES_FUSED_MLP_STEP", "0")
    with pytest.raises(ValueError, match="fused optimiser step"):
        mk(mlp(), mlp(), vec, per_env_tasks=True)
    monkeypatch.delenv("BRIDGES_FUSED_MLP_STEP")
    agent = mk(mlp(), mlp(), vec, per_env_tasks=True)
    assert agent.ring.width == 120 and agent.replay_env.per_env_tasks and agent.replay_env.random_targets is None
    with pytest.raises(ValueError, match="per-env tasks"):
        agent.evaluate(make_vec(4, [(0.5, 0.0, 1.0)], f32_rasters=False))
    with pytest.raises(ValueError):
        make_vec(4, [(0.5, 0.0, 1.0)], f32_rasters=False).state_groups(None, task=True)
    with pytest.raises(ValueError):
        vec.load_targets(torch.zeros((4, 3, 3), dtype=torch.float64, device=DEV))     # a sampling env keeps its own targets
