"""GPU: the conv Q-networks of the vectorised DQN on per-env tasks and obstacles (VecDQN(per_env_tasks=True, task_channels=True)):
the rows ops.conv_input builds against the torch formulation on f32 rasters, q through both, rows shared by (state, candidate,
flag, task), an env set holding one task against the fixed-task agent, the optimiser step (captured, eager, plain loop), the
whole loop without f32 rasters, and the paths that must not have moved.  The tolerances are those of tests/test_gpu_vec_dqn.py:
1e-5 for q over another batch composition (test_distinct_row_forward_equals_the_forward_of_every_row), and for the optimiser
steps losses to rtol 1e-4 / atol 1e-6, weights to rtol 1e-4 / atol 15 lr (test_graph_captured_train_step_equals_eager)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_STEPS = 4
RANGE = ((-3.0, 3.0), (0.3, 2.5))
Q_TOL = dict(rtol=1e-5, atol=1e-5)
LR = 1e-4


def make_vec(E, obstacles, targets, max_steps=MAX_STEPS, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    kw.setdefault("f32_rasters", False)
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], obstacles, targets, max_steps=max_steps, seed=seed, **kw)


def random_env(E, T=2, O=1, seed=0, **kw):
    from bridges_hip.vec_env import RandomObstacles, RandomTargets
    return make_vec(E, RandomObstacles([RANGE] * O) if O else [], RandomTargets(T), seed=seed, **kw)


def make_nets(model, seed=5):
    from robotoddler.training.successor_dqn import build_parser, make_nets as mk
    torch.manual_seed(seed)
    return mk(vars(build_parser().parse_args(["--model", model])), torch.device(DEV))


LOSS = dict(ConvNet="mse_q_values", UNet="mse_q_values+mse_block_features", SuccessorMLP="mse_q_values+mse_block_features")


def make_agent(env, model="ConvNet", seed=5, B=8, capacity=64, **kw):
    from robotoddler.training.vec_dqn import VecDQN
    pol, tgt = make_nets(model, seed)
    opt = torch.optim.Adam(pol.parameters(), lr=LR, fused=True)
    kw.setdefault("per_env_obstacles", bool(getattr(env, "per_env_obstacles", False)))
    return VecDQN(pol, tgt, opt, env, capacity, B, 0.95, 0.01, LOSS[model], seed=3, per_env_tasks=True, task_channels=True, **kw)


def torch_rows(env, idx, row_env):
    """The four channels of the rows as separately allocated tensors: the torch formulation of ops.conv_input."""
    from bridges_hip import ops
    block = ops.bits_to_f32(env.state_bits).index_select(0, row_env).unsqueeze(1)
    action = ops.bits_to_f32(env.cand_bits).index_select(0, idx).unsqueeze(1)
    reward = env.reward_maps.index_select(0, row_env).unsqueeze(1)
    obst = ops.bits_to_f32(env.env_obstacle_bits).index_select(0, row_env) if env.per_env_obstacles \
        else ops.bits_to_f32(env.obstacle_bits.reshape(1, 64)).expand(idx.numel(), -1, -1)
    return block, action, reward, obst.unsqueeze(1).contiguous()


# ------------------------------------------------------------------------------------------------------------ 1: the rows
def test_row_features_equal_the_torch_formulation_on_f32_rasters():
    env = random_env(12, seed=4, f32_rasters=True)
    agent = make_agent(env)
    for _ in range(3):
        agent.act()
    idx, row_env = env.valid_rows()
    assert idx.numel() > 12
    stable = agent._stable_flags(env)
    block, binary, action, reward, obstacle = agent._row_features(env, idx, row_env, stable)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(block[:, 0]), bits(env.state_raster[row_env]))
    assert torch.equal(bits(action[:, 0]), bits(env.cand_raster[idx]))
    assert torch.equal(bits(reward[:, 0]), bits(env.reward_maps[row_env]))
    assert torch.equal(bits(obstacle[:, 0]), bits(env.obstacle_rasters[row_env]))
    assert torch.equal(binary[:, 0], stable[row_env].float()) and not binary[:, 1:].any()
    # the views are the consecutive channels of one tensor: the nets stack them back without a copy
    from bridges_hip.dqn_ops import stack_channels
    x = stack_channels(block, action, reward, obstacle)
    assert x.data_ptr() == block.data_ptr() and tuple(x.shape) == (idx.numel(), 4, 64, 64) and x.is_contiguous()
    for got, want in zip((block, action, reward, obstacle), torch_rows(env, idx, row_env)):
        assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------------------ 2: same inputs, same q
@pytest.mark.parametrize("model", ["ConvNet", "UNet"])
def test_q_through_the_new_rows_is_q_of_the_torch_built_rows(model, monkeypatch):
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "DEDUP_ROWS", False)
    monkeypatch.setattr(VecDQN, "ROW_CHUNK", 64)
    env = random_env(16, seed=4)
    agent = make_agent(env, model)
    for _ in range(2):
        agent.act()
    idx, row_env = env.valid_rows()
    n, C = idx.numel(), VecDQN.ROW_CHUNK
    assert n > C                                                          # more than one chunk, the last one padded
    stable = agent._stable_flags(env)
    net = agent.policy_net
    with torch.no_grad():
        net.eval()
        q, _, _, inverse = agent._forward_rows(net, env, idx, row_env, stable)
        assert inverse is None
        pad = (-n) % C
        idx_p, env_p = torch.cat([idx, idx[:1].expand(pad)]), torch.cat([row_env, row_env[:1].expand(pad)])
        want = []
        for o in range(0, n + pad, C):
            block, action, reward, obstacle = torch_rows(env, idx_p[o:o + C], env_p[o:o + C])
            binary = torch.zeros((C, 6), device=DEV)
            binary[:, 0] = stable[env_p[o:o + C]].float()
            want.append(net(block, binary, action, reward, obstacle)[0])
        want = torch.cat(want)[:n]
    assert torch.equal(q, want), float((q - want).abs().max())


# ------------------------------------------------------------------------------------------------------------ 3: the task key
def two_tasks(E, T=2):
    a = torch.tensor([[0.5, 0.0, 1.9], [-1.0, 0.0, 1.1]], dtype=torch.float64)[:T]
    b = torch.tensor([[0.5, 0.0, 1.9], [-1.0, 0.0, 2.7]], dtype=torch.float64)[:T]          # one coordinate of one target differs
    return torch.stack([a if e % 2 == 0 else b for e in range(E)])


@pytest.mark.parametrize("model", ["ConvNet", "UNet"])
def test_rows_are_shared_by_state_and_task(model, monkeypatch):
    """8 freshly reset envs: with two tasks among them a Q pass feeds twice one env's rows, with one task once; q per env is what
    feeding every row gives."""
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "DEDUP_STATES", False)
    E = 8
    env = make_vec(E, [], two_tasks(E))
    agent = make_agent(env, model)
    per_env = int(env.n_valid[0])
    assert per_env > 1 and bool((env.n_valid[:E] == per_env).all())

    def q_pass():
        idx, row_env = env.valid_rows()
        assert idx.numel() == E * per_env
        stable = agent._stable_flags(env)
        agent.rows_fed = 0
        q = agent._policy_q(env, idx, row_env, stable)
        return q, agent.rows_fed

    q_shared, fed = q_pass()
    assert fed == 2 * per_env
    monkeypatch.setattr(VecDQN, "DEDUP_ROWS", False)
    q_all, fed_all = q_pass()
    assert fed_all == E * per_env
    assert torch.allclose(q_shared, q_all, **Q_TOL), float((q_shared - q_all).abs().max())
    by_env = q_all.reshape(E, per_env)
    assert not torch.equal(by_env[0], by_env[1])                           # the two tasks do ask for other values
    monkeypatch.setattr(VecDQN, "DEDUP_ROWS", True)
    env.set_targets(two_tasks(E)[:1].expand(E, -1, -1).contiguous())
    q_one, fed_one = q_pass()
    assert fed_one == per_env
    assert torch.allclose(q_one.reshape(E, per_env), by_env[0].expand(E, -1), **Q_TOL)


# ------------------------------------------------------------------------------------------------------------ 4: one task in every env
@pytest.mark.parametrize("model", ["ConvNet", "UNet"])
def test_an_env_set_holding_one_task_is_the_fixed_task_agent(model):
    from robotoddler.training.vec_dqn import VecDQN
    E = 8
    targets, obstacles = [(0.5, 0.0, 1.9), (-1.0, 0.0, 1.1)], [(1.2, 0.0, 0.3)]
    env_t = random_env(E, T=2, O=1, seed=2)
    env_t.set_targets(torch.tensor(targets, dtype=torch.float64).expand(E, -1, -1).contiguous(), reset=False)
    env_t.set_obstacles(torch.tensor(obstacles, dtype=torch.float64).expand(E, -1, -1).contiguous())
    env_f = make_vec(E, obstacles, targets, seed=2, f32_rasters=True)
    # the device's map and obstacle raster of the task are the host's, bit for bit
    assert torch.equal(env_t.reward_maps.view(torch.int32), env_f.reward_map.view(torch.int32).expand(E, -1, -1))
    assert torch.equal(env_t.env_obstacle_bits, env_f.obstacle_bits.reshape(1, 64).expand(E, -1))
    agent_t = make_agent(env_t, model)
    pol, tgt = make_nets(model)
    agent_f = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=LR, fused=True), env_f, 64, 8, 0.95, 0.01, LOSS[model], seed=3)
    agent_t.rows_fed = agent_f.rows_fed = 0
    rec_t, valid_t = agent_t.act(greedy=True)
    rec_f, valid_f = agent_f.act(greedy=True)
    assert agent_t.rows_fed > 0
    if agent_t.rows_fed == agent_f.rows_fed:                                # the same chunk shapes: the same kernels on the same bits
        assert torch.equal(agent_t._q_sel, agent_f._q_sel), float((agent_t._q_sel - agent_f._q_sel).abs().max())
    else:
        assert torch.allclose(agent_t._q_sel, agent_f._q_sel, **Q_TOL)
    assert torch.equal(valid_t, valid_f) and bool(valid_t.all())
    assert torch.equal(env_t.state_bits, env_f.state_bits) and torch.equal(env_t.n_blocks, env_f.n_blocks)      # the same actions


# ------------------------------------------------------------------------------------------------------------ 5: the train step
def recorded(E, O, seed=9, locksteps=5):
    """Records of a short rollout on per-env tasks (width 111 + 3 T + 3 O) to fill every variant's ring with."""
    env = random_env(E, O=O, seed=seed)
    agent = make_agent(env, "ConvNet")
    out = []
    for _ in range(locksteps):
        rec, valid = agent.act()
        out.append(agent.with_task(rec)[valid])
    return torch.cat(out)


def plain_steps(agent, n_steps):
    """VecDQN.train_steps' eager loop on torch-built per-transition inputs: four separately allocated channel tensors."""
    from bridges_hip import dqn_ops, ops
    B = agent.B
    rec = agent.ring.sample(n_steps * B, agent.sample_gen, agent.prioritized)
    batch = agent._targets(rec)
    binary, q_target, sf_target, maps, obst_bits = batch.binary, batch.q_target, batch.sf_target, batch.reward_maps, batch.obstacle_bits
    block_f, action_f = ops.bits_to_f32(batch.state_bits).unsqueeze(1), ops.bits_to_f32(batch.action_bits).unsqueeze(1)
    reward_f = maps.reshape(-1, 1, 64, 64).clone()
    obst_f = (ops.bits_to_f32(obst_bits) if obst_bits is not None
              else ops.bits_to_f32(agent.env.obstacle_bits.reshape(1, 64)).expand(n_steps * B, -1, -1).contiguous()).unsqueeze(1)
    agent.policy_net.train()
    losses = []
    reduce = dqn_ops.ReduceTables(agent.device)
    for i in range(n_steps):
        sl = slice(i * B, (i + 1) * B)
        q, sf, _ = agent.policy_net(block_f[sl], binary[sl], action_f[sl], reward_f[sl], obst_f[sl])
        loss = agent._loss(q, sf, q_target[sl], sf_target[sl] if sf_target is not None else None)
        agent.opt.zero_grad()
        with dqn_ops.deferred_wgrad_reduce(reduce):
            loss.backward()
        agent.opt.step()
        losses.append(float(loss.detach()))
    return losses


@pytest.mark.parametrize("model,O", [("ConvNet", 1), ("UNet", 1), ("ConvNet", 0)])
def test_train_step_captured_eager_and_plain_loop_agree(model, O, monkeypatch):
    """Two warm-up calls (eager in every variant) and then 2 calls of 2 steps: the captured step, BRIDGES_TRAIN_GRAPH=0, and the
    plain loop on torch-built inputs.  O = 0: targets only, the shared obstacle raster with stride 0."""
    from robotoddler.training import train_step as T
    E, B, n_steps, calls = 16, 8, 2, 4
    records = recorded(E, O)
    assert records.shape[0] >= 4 * B and records.shape[1] == 111 + 6 + 3 * O
    out = {}
    for variant in ("captured", "eager", "plain"):
        monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", "1" if variant == "captured" else "0")
        agent = make_agent(random_env(E, O=O, seed=9), model)
        agent.ring.push(records)
        losses, ptrs = [], []
        for c in range(calls):
            losses += plain_steps(agent, n_steps) if variant == "plain" else agent.train_steps(n_steps)
            drv = getattr(agent.policy_net, "_fused_trainer", None)
            if variant == "captured" and c >= 2:
                assert drv.conv_rows and drv._graphs and drv.block is None and drv.action is None
                assert tuple(drv.x_all.shape) == (n_steps * B, 4, 64, 64)
                ptrs.append(drv.x_all.data_ptr())
        if variant == "captured":
            assert agent._graph_state is not None and len(set(ptrs)) == 1 and len(drv._graphs) == 1     # one capture, replayed
            assert drv.obstacle_rows == bool(O) and (drv.obstacle is None) == bool(O)
        elif variant == "eager":
            assert agent._graph_state is None
        T.sync_optimizer(agent.policy_net)
        out[variant] = (np.array(losses), torch.cat([p.detach().flatten() for p in agent.policy_net.parameters()]).cpu())
    for variant in ("captured", "eager"):
        a, b = out[variant], out["plain"]
        print(variant, "losses", a[0], "plain", b[0], "max |weight difference|", float((a[1] - b[1]).abs().max()))
        assert len(a[0]) == len(b[0]) == n_steps * calls and (a[0] >= 0).all()
        np.testing.assert_allclose(a[0], b[0], rtol=1e-4, atol=1e-6)
        assert torch.allclose(a[1], b[1], rtol=1e-4, atol=15 * LR), float((a[1] - b[1]).abs().max())


# ------------------------------------------------------------------------------------------------------------ 6: the whole loop
@pytest.mark.parametrize("model,O,prioritized", [("ConvNet", 1, False), ("UNet", 1, False), ("ConvNet", 0, False), ("ConvNet", 1, True)])
def test_the_loop_runs_without_f32_rasters(model, O, prioritized, tmp_path):
    from robotoddler.training import records as R
    E, T = 16, 2
    env = random_env(E, T=T, O=O, seed=6)
    assert env.cand_raster is None and env.state_raster is None
    agent = make_agent(env, model, prioritized=prioritized)
    assert not agent._replay_f32() and agent.replay_env.cand_raster is None
    W = R.RECORD_WIDTH + 3 * T + 3 * O
    assert agent.ring.width == W == 111 + 3 * T + 3 * O
    cap, inner_step, inner_act = {}, env.step, agent.act

    def step(sel_index=None):
        cap.update(targets=env.env_targets.clone(), obstacles=env.env_obstacles.clone() if O else None)
        inner_step(sel_index)

    def act(*a, **k):                                                     # (keeps the lock-step's valid mask)
        rec, valid = inner_act(*a, **k)
        cap["valid"] = valid
        return rec, valid

    env.step, agent.act = step, act
    losses = []
    for _ in range(5):
        l, allrec = agent.lockstep(2)
        losses += l
        v = cap["valid"]
        assert allrec.shape[1] == W and allrec.shape[0] == int(v.sum())
        assert torch.equal(allrec[:, R.RECORD_WIDTH:R.RECORD_WIDTH + 3 * T], cap["targets"].reshape(E, -1)[v])
        if O:
            assert torch.equal(allrec[:, R.RECORD_WIDTH + 3 * T:], cap["obstacles"].reshape(E, -1)[v])
    assert len(losses) >= 6 and all(np.isfinite(losses)) and min(losses) >= 0
    if prioritized:
        assert bool((agent.ring.data[:len(agent.ring), R.O_TD] >= 0).all()) and bool((agent.ring.data[:len(agent.ring), R.O_TD] > 0).any())
    eval_env = random_env(8, T=T, O=O, seed=77)
    ev = agent.evaluate(eval_env)
    assert ev["episodes"] == 8 and 0.0 <= ev["success_rate"] <= 1.0 and np.isfinite(ev["reward"])
    # checkpoint round trip of the ring and of what the nets / ring do not hold
    agent.ring.save(str(tmp_path / "ring.pt"))
    agent.save_extra(str(tmp_path / "agent.pt"), lockstep=5)
    again = make_agent(random_env(E, T=T, O=O, seed=6), model, prioritized=prioritized)
    again.ring.load(str(tmp_path / "ring.pt"))
    assert again.load_extra(str(tmp_path / "agent.pt")) == dict(lockstep=5)
    order = lambda r: r.data[(r.head - r.size + torch.arange(r.size, device=r.data.device)) % r.capacity]     # oldest first
    assert len(again.ring) == len(agent.ring) and torch.equal(order(again.ring), order(agent.ring))
    assert again.epsilon == agent.epsilon and again.env_steps == agent.env_steps and torch.equal(again.step_images, agent.step_images)
    l, _ = again.lockstep(2)
    assert len(l) == 2 and all(np.isfinite(l))


# ------------------------------------------------------------------------------------------------------------ 7: opt-in
def test_the_other_paths_never_build_conv_rows(monkeypatch):
    from bridges_hip import ops
    from bridges_hip.vec_env import RandomTargets
    from robotoddler.training.vec_dqn import VecDQN
    calls, inner = [], ops.conv_input

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    monkeypatch.setattr(ops, "conv_input", counted)
    tower = dict(obstacles=[(0.5, 0.0, 0.4)], targets=[(0.5, 0.0, 1.2)])
    for model, env, kw in (("ConvNet", make_vec(16, tower["obstacles"], tower["targets"], f32_rasters=True), {}),
                           ("SuccessorMLP", make_vec(16, tower["obstacles"], tower["targets"]), {}),
                           ("SuccessorMLP", make_vec(16, [], RandomTargets(2)), dict(per_env_tasks=True))):
        pol, tgt = make_nets(model)
        agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=LR, fused=True), env, 64, 8, 0.95, 0.01, LOSS[model], seed=3, **kw)
        assert not agent.task_channels
        for _ in range(4):
            l, _ = agent.lockstep(2)
        assert len(l) == 2 and all(np.isfinite(l)) and not calls
    pol, tgt = make_nets("ConvNet")
    with pytest.raises(ValueError, match="ConvNet.*task_channels=True"):
        VecDQN(pol, tgt, None, make_vec(4, [], RandomTargets(2)), 64, 8, 0.95, 0.01, "mse_q_values", per_env_tasks=True)
    # and the new mode does
    agent = make_agent(random_env(8), "ConvNet")
    agent.lockstep(0)
    assert calls


CLI = ["--loss_function", "mse_q_values", "--random_targets", "3", "--task_channels", "--num_envs", "16", "--eval_envs", "8",
       "--num_training_steps", "2", "--batch_size", "8", "--seed", "3", "--learning_rate", "1e-4", "--max_steps", "4",
       "--replay_buffer_capacity", "64", "--num_episodes", "40", "--evaluate_every", "20"]


@pytest.mark.parametrize("extra", [["--model", "ConvNet", "--random_obstacles", "2"], ["--model", "UNet"]])
def test_cli_runs_the_new_mode(extra):
    from robotoddler.training.successor_dqn import main
    hist = main([*CLI, *extra])
    assert hist and hist[-1]["episodes"] >= 40
    losses = [h["avg_loss"] for h in hist if h["avg_loss"] is not None]
    assert losses and all(np.isfinite(losses)) and min(losses) >= 0
    evals = [h["evaluation"] for h in hist if "evaluation" in h]
    assert evals and all(ev["episodes"] == 8 for ev in evals)
