"""GPU: VecDQN.beam_search on a small SuccessorMLP (hidden [8]), M = 8 held-out tasks, max_steps 6: width 1 is the greedy episode;
the structures a width-4 search returns replay to the success, reward and return it reports, bit for bit; no training state
changes; per-env obstacles and a ConvNet with task_channels run a search; and the search waits for the device per depth only
where acting waits."""
import hashlib
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, MAX_STEPS, GAMMA = 8, 6, 0.95
RANGE = ((-3.0, 3.0), (0.3, 2.5))


def make_vec(E, obstacles, targets, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    kw.setdefault("f32_rasters", False)
    kw.setdefault("max_steps", MAX_STEPS)
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], obstacles, targets, seed=seed, **kw)


def random_env(E, T=2, O=0, seed=0, **kw):
    from bridges_hip.vec_env import RandomObstacles, RandomTargets
    return make_vec(E, RandomObstacles([RANGE] * O) if O else [], RandomTargets(T), seed=seed, **kw)


def make_mlp(seed=0):
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.utils.utils import init_weights
    torch.manual_seed(seed)
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8]).to(DEV)
    net.apply(init_weights)
    with torch.no_grad():                                    # spread the q of the candidates (the default init leaves them ~1e-5 apart)
        for p in net.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
    return net


def make_agent(O=0, **kw):
    from robotoddler.training.vec_dqn import VecDQN
    env = random_env(32, O=O, seed=2)
    pol, tgt = make_mlp(1), make_mlp(1)
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 4096, 16, GAMMA, 0.01, "mse_q_values+mse_block_features", seed=3,
                  per_env_tasks=True, per_env_obstacles=bool(O), **kw)


def greedy_rollout(agent, env):
    """One greedy episode per env through _act_on -> per env (success, discounted lin_reward, discounted reward, steps), the sums
    in float64 by the search's own recurrence (ret += disc * r; disc *= gamma)."""
    from robotoddler.training import records as R
    E = env.E
    images = torch.zeros((env.K + 1, env.img, env.img), dtype=torch.float32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    env.reset()
    ret, ret_r, disc = np.zeros(E), np.zeros(E), np.ones(E)
    out = [None] * E
    for d in range(env.K):
        rec, valid, _q = agent._act_on(env, images, gen, 0.0, True)
        rec, valid = rec.cpu().numpy(), valid.cpu().numpy().astype(bool)
        for e in range(E):
            if out[e] is not None or not valid[e]:
                continue
            ret[e] = ret[e] + disc[e] * rec[e, R.O_LIN]
            ret_r[e] = ret_r[e] + disc[e] * rec[e, R.O_REWARD]
            disc[e] = disc[e] * GAMMA
            if rec[e, R.O_DONE] > 0.5:
                out[e] = (bool(rec[e, R.O_REWARD] == env.n_targets), ret[e], ret_r[e], d + 1)
    assert all(o is not None for o in out)
    return out


def replay(eval_env, structures):
    """Every task's returned actions in a fresh env of one env per task -> per task (success, lin return, reward return), and the
    checks that every action was a valid candidate and placed the block the structure lists."""
    from robotoddler.training.vec_dqn import beam_env_like
    env = beam_env_like(eval_env, 1)
    E = env.E
    assert E == len(structures)
    env.reset()
    ret, ret_r, disc = np.zeros(E), np.zeros(E), np.ones(E)
    out = [None] * E
    for d in range(env.K):
        off, mask = env.cand_offset.cpu().numpy(), env.cand_mask.cpu().numpy()
        first_valid = [int(np.argmax(mask[off[e]:off[e + 1]])) if off[e + 1] > off[e] else 0 for e in range(E)]   # (after its end: anything valid)
        a = np.array([s["actions"][d] if d < s["num_steps"] else first_valid[e] for e, s in enumerate(structures)], dtype=np.int32)
        pose = env.cand_pose.cpu().numpy()
        desc = env.cand_desc.cpu().numpy()
        for e, s in enumerate(structures):
            if d < s["num_steps"]:
                assert mask[off[e] + a[e]] == 1, f"task {e}, depth {d}: the action is no valid candidate"
                assert pose[off[e] + a[e]].tobytes() == np.array(s["pose"][d]).tobytes() and desc[off[e] + a[e], 2] == s["shape"][d]
        env.step(torch.from_numpy(a).to(DEV))
        lin, rew, flags = env.lin_reward.cpu().numpy().astype(np.float64), env.reward.cpu().numpy().astype(np.float64), env.step_flags.cpu().numpy()
        for e, s in enumerate(structures):
            if d < s["num_steps"]:
                ret[e] = ret[e] + disc[e] * lin[e]
                ret_r[e] = ret_r[e] + disc[e] * rew[e]
                disc[e] = disc[e] * GAMMA
                ended = bool(flags[e, 5] or flags[e, 6])
                assert ended == (d == s["num_steps"] - 1), f"task {e}: the episode ends at depth {d}, the structure has {s['num_steps']} steps"
                if ended:
                    out[e] = (bool(rew[e] == env.n_targets), ret[e], ret_r[e], float(rew[e]))
    return out


def check_replay(eval_env, res):
    got = replay(eval_env, res["structures"])
    for e, (s, g) in enumerate(zip(res["structures"], got)):
        assert g is not None and g[0] == s["success"], e
        assert np.float64(g[1]).tobytes() == np.float64(s["lin_reward"]).tobytes(), (e, g[1], s["lin_reward"])
        assert np.float64(g[2]).tobytes() == np.float64(s["reward"]).tobytes() and g[3] == s["final_reward"], e
        assert len(s["shape"]) == len(s["pose"]) == len(s["actions"]) == s["num_steps"] >= 1
    n = len(got)
    assert res["success_rate"] == sum(s["success"] for s in res["structures"]) / n and res["episodes"] == n
    assert res["lin_reward"] == pytest.approx(np.mean([s["lin_reward"] for s in res["structures"]]), rel=1e-12, abs=1e-15)


def test_width_1_is_the_greedy_episode():
    from robotoddler.training.vec_dqn import beam_env_like
    agent = make_agent()
    eval_env = random_env(M, seed=77)
    want = greedy_rollout(agent, eval_env)
    beam_env = beam_env_like(eval_env, 1)
    assert beam_env.E == M and torch.equal(beam_env.env_targets, eval_env.env_targets) and beam_env.random_targets is None
    res = agent.beam_search(beam_env, 1)
    assert res["beam_width"] == 1 and res["episodes"] == M
    for e, (s, w) in enumerate(zip(res["structures"], want)):
        assert s["success"] == w[0] and s["num_steps"] == w[3], e
        assert np.float64(s["lin_reward"]).tobytes() == np.float64(w[1]).tobytes(), (e, s["lin_reward"], w[1])
        assert np.float64(s["reward"]).tobytes() == np.float64(w[2]).tobytes(), e
    ev = agent.evaluate(eval_env, epsilon=0.0)
    assert res["success_rate"] == ev["success_rate"] and res["num_steps"] == ev["num_steps"]
    # evaluate() sums in float32 (log_episode's arithmetic), the search in float64: K terms of magnitude <= |reward|
    assert res["reward"] == pytest.approx(ev["reward"], rel=1e-5, abs=1e-6)
    assert res["lin_reward"] == pytest.approx(ev["lin_reward"], rel=1e-5, abs=1e-6)
    assert agent.beam_search(beam_env, 1) == res             # again: the same numbers (the search starts afresh every time)


def _training_state(agent):
    ring, env = agent.ring, agent.env
    h = hashlib.sha256()
    for t in (ring.data, agent.policy_net._flat_params.flat if hasattr(agent.policy_net, "_flat_params") else
              torch.cat([p.detach().flatten() for p in agent.policy_net.parameters()]), agent.step_images, env.n_blocks, env.blk_pose,
              env.state_bits, env.draw_counter, env.env_targets, env.task_episode, env.cand_mask, agent.explore_gen.get_state(),
              agent.sample_gen.get_state(), torch.cuda.get_rng_state(), torch.get_rng_state()):
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest(), ring.size, ring.head, agent.epsilon, agent.env_steps, agent.episodes_done


def test_width_4_replays_to_what_it_reports_and_touches_no_training_state():
    from robotoddler.training.vec_dqn import beam_env_like
    agent = make_agent()
    for _ in range(3):
        agent.lockstep(1)
    eval_env = random_env(M, seed=77)
    beam_env = beam_env_like(eval_env, 4)
    assert beam_env.E == 4 * M and torch.equal(beam_env.env_targets, eval_env.env_targets.repeat_interleave(4, dim=0))
    torch.cuda.synchronize()
    before = _training_state(agent)
    res = agent.beam_search(beam_env, 4)
    torch.cuda.synchronize()
    assert _training_state(agent) == before
    check_replay(eval_env, res)
    assert agent.beam_search(beam_env, 4) == res             # again: the same search (it starts afresh every time)


def test_per_env_obstacles_run_a_search():
    from robotoddler.training.vec_dqn import beam_env_like
    agent = make_agent(O=1)
    eval_env = random_env(M, O=1, seed=78)
    beam_env = beam_env_like(eval_env, 2)
    assert torch.equal(beam_env.env_obstacles, eval_env.env_obstacles.repeat_interleave(2, dim=0)) and beam_env.random_obstacles is None
    res = agent.beam_search(beam_env, 2)
    check_replay(eval_env, res)


def test_convnet_with_task_channels_runs_a_search():
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN, beam_env_like
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    env = random_env(16, O=1, seed=2)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 64, 8, GAMMA, 0.01, "mse_q_values", seed=3,
                   per_env_tasks=True, per_env_obstacles=True, task_channels=True)
    eval_env = random_env(4, O=1, seed=79, max_steps=3)       # (three depths: every depth is one padded conv forward)
    res = agent.beam_search(beam_env_like(eval_env, 2), 2)
    check_replay(eval_env, res)


def test_a_fixed_task_is_passed_through_and_refusals_come_in_words():
    from robotoddler.training.vec_dqn import VecDQN, beam_env_like
    H = 0.8
    fixed = make_vec(4, [(0.5, 0., H / 2)], [(0.5, 0, H + H / 2)], seed=3)
    beam_env = beam_env_like(fixed, 3)
    assert beam_env.E == 12 and not beam_env.per_env_tasks and beam_env.targets == fixed.targets and beam_env.obstacles == fixed.obstacles
    pol, tgt = make_mlp(1), make_mlp(1)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), make_vec(8, [(0.5, 0., H / 2)], [(0.5, 0, H + H / 2)]), 256, 8,
                   GAMMA, 0.01, "mse_q_values", seed=3)
    res = agent.beam_search(beam_env, 3)
    assert res["episodes"] == 4 and len(res["structures"]) == 4
    assert all(s == res["structures"][0] for s in res["structures"])          # one task, one answer
    with pytest.raises(ValueError, match="of its own"):
        agent.beam_search(agent.env, 1)
    with pytest.raises(ValueError, match=r"M \* 5"):
        agent.beam_search(beam_env, 5)
    with pytest.raises(ValueError, match="draws tasks per episode"):
        make_agent().beam_search(random_env(8, seed=1), 4)


def test_a_task_family_goes_in_as_explicit_arrays_and_reports_by_class():
    from bridges_hip.vec_env import RandomBridges
    from robotoddler.training.vec_dqn import VecDQN, beam_env_like
    fam = lambda E, seed: make_vec(E, [], RandomBridges("span", sizes=(1, 3)), seed=seed)
    pol, tgt = make_mlp(1), make_mlp(1)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), fam(32, 2), 4096, 16, GAMMA, 0.01,
                   "mse_q_values+mse_block_features", seed=3, per_env_tasks=True, per_env_obstacles=True)
    eval_env = fam(M, 80)
    beam_env = beam_env_like(eval_env, 2)
    classes = eval_env.task_class.tolist()
    assert beam_env.task_family is None and beam_env.beam_task_class == classes and beam_env.beam_n_classes == 4
    assert torch.equal(beam_env.env_targets, eval_env.env_targets.repeat_interleave(2, dim=0))
    assert torch.equal(beam_env.env_obstacles, eval_env.env_obstacles.repeat_interleave(2, dim=0))       # parked slots included
    res = agent.beam_search(beam_env, 2)
    check_replay(eval_env, res)
    assert res["episodes_by_class"] == [classes.count(n) for n in range(4)] and sum(res["episodes_by_class"]) == M
    for n in range(4):
        mine = [s["success"] for s, c in zip(res["structures"], classes) if c == n]
        assert res["success_by_class"][n] == (sum(mine) / len(mine) if mine else None)
    ev = agent.evaluate(eval_env)
    assert ev["episodes_by_class"] == res["episodes_by_class"]                # the same tasks as evaluate() plays


def _waits(fn):
    """Host waits while fn() runs: synchronising torch calls (sync debug mode) and explicit stream / event / device synchronisations."""
    seen = []
    saved = (torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize)

    def counting(name, inner):
        def f(*a, **k):
            seen.append(name)
            return inner(*a, **k)
        return f
    torch.cuda.Stream.synchronize = counting("stream", saved[0])
    torch.cuda.Event.synchronize = counting("event", saved[1])
    torch.cuda.synchronize = counting("device", saved[2])
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        seen += ["op"] * sum("synchroniz" in str(x.message) for x in w)
    finally:
        torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize = saved
    return seen


def test_no_wait_per_depth_beyond_actings_own():
    from robotoddler.training.vec_dqn import beam_env_like
    agent = make_agent()
    eval_env = random_env(M, seed=77)
    beam_env = beam_env_like(eval_env, 4)
    agent.evaluate(eval_env)
    agent.beam_search(beam_env, 4)                           # (allocations and caches of the first call are behind us)
    ev = _waits(lambda: agent.evaluate(eval_env))
    bs = _waits(lambda: agent.beam_search(beam_env, 4))
    # evaluate(): acting's row count per depth (valid_rows) and one wait for the statistics; the search: the same per depth, one
    # read-back at the end
    print("waits of evaluate():", ev, "of beam_search():", bs)
    assert len(bs) <= len(ev), (bs, ev)
    # per depth: acting's wait for the row count (valid_rows: one stream synchronisation, which the debug mode reports as well)
    assert bs.count("stream") == ev.count("stream") == beam_env.K, (bs, ev)
    assert bs.count("op") <= ev.count("op") and bs.count("op") <= beam_env.K + 1, (bs, ev)   # + the one read-back at the end
    assert bs.count("event") == bs.count("device") == 0, bs
