"""GPU: action sets restricted to the stable placements (stable_actions_only) in the lock-step env, the replay scratch env,
the vectorised DQN and the single-env loop.  With the option on, the available actions of a state are
filter_actions ∩ {a : is_action_stable_rbe(env, a)} (a solver error counts as unstable)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.env import OracleGym, bridge_setup, horizontal_bridge_setup, policy_draw

pytestmark = pytest.mark.gpu

TASKS = dict(tower4=(bridge_setup, dict(num_stories=4), ["trapezoid"], 15, 0.8),
             mixed=(horizontal_bridge_setup, dict(num_obstacles=4, trapezoid=True, hexagon=True), ["trapezoid", "hexagon"], 12, 2.0))


def make_env(task, E, seed, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    fn, skw, names, max_steps, mu = TASKS[task]
    setup = fn(**skw)
    return VecAssemblyGym(E, [load_urdf(f"shapes/{n}.urdf") for n in names], setup["obstacles"], setup["targets"],
                          max_steps=max_steps, seed=seed, mu=mu, **kw)


class StableOracleLockstep:
    """oracle.env.OracleLockstep with the candidate mask narrowed to the stable placements: a state with valid but no stable
    candidate is a reset-only lock-step as well."""

    def __init__(self, gym, capacity=16):
        self.gym, self.capacity = gym, capacity
        gym.reset()
        self._candidates()

    def _candidates(self):
        c = self.gym.candidates()
        stable = np.zeros(len(c["actions"]), dtype=bool)
        for a in np.flatnonzero(c["mask"]):
            stable[a] = bool(self.gym.is_action_stable(c["actions"][a]))
        c["mask"] = c["mask"] & stable
        self.cand = c
        self.needs_reset = not c["mask"].any()

    def lockstep(self, pick_valid_rank):
        g = self.gym
        out = dict(valid_step=False)
        if self.needs_reset:
            g.reset()
        else:
            valid = np.flatnonzero(self.cand["mask"])
            a = int(valid[pick_valid_rank(len(valid))])
            _stable, reward, term, trunc = g.step(self.cand["actions"][a])
            trunc = trunc or len(g.blocks) >= self.capacity
            out = dict(valid_step=True, action_index=a, reward=reward, done=bool(term or trunc))
            if out["done"]:
                g.reset()
        self._candidates()
        out["no_actions"] = self.needs_reset
        return out


@pytest.mark.parametrize("task", ["tower4", "mixed"])
def test_restricted_lockstep_matches_the_oracle(task):
    E, seed, n_lock = 64, 17, 12
    fn, skw, names, max_steps, mu = TASKS[task]
    vec = make_env(task, E, seed, f32_rasters=False, stable_actions_only=True)
    oracles = [StableOracleLockstep(OracleGym(**fn(**skw), max_steps=max_steps, mu=mu)) for _ in range(E)]
    counters = [0] * E
    narrowed = no_actions = 0

    def compare():
        nonlocal narrowed
        off, n_cand = vec.cand_offset.cpu().numpy(), vec.n_cand.cpu().numpy()
        mask, nvalid = vec.cand_mask.cpu().numpy().astype(bool), vec.n_valid.cpu().numpy()
        for e, o in enumerate(oracles):
            A = len(o.cand["actions"])
            assert n_cand[e] == A, (e, n_cand[e], A)
            assert np.array_equal(mask[off[e]:off[e] + A], o.cand["mask"]), e
            assert nvalid[e] == int(o.cand["mask"].sum()), e
    compare()
    for it in range(n_lock):
        vec.select_random()
        sel = vec.sel_index.cpu().numpy()
        outs = []
        for e, o in enumerate(oracles):
            def pick(nv, e=e):
                r = policy_draw(seed, e, counters[e]) % nv
                counters[e] += 1
                return r
            outs.append(o.lockstep(pick))
        vec.step()
        fl = {k: v.cpu().numpy() for k, v in vec.flags().items()}
        reward = vec.reward.cpu().numpy()
        for e, out in enumerate(outs):
            assert bool(fl["valid_step"][e]) == out["valid_step"], (it, e)
            assert bool(fl["no_actions"][e]) == out["no_actions"], (it, e)
            no_actions += int(out["no_actions"])
            if out["valid_step"]:
                assert sel[e] == out["action_index"], (it, e)
                assert bool(fl["done"][e]) == out["done"], (it, e)
                assert reward[e] == out["reward"], (it, e)
        compare()
        narrowed += sum(int(o.cand["mask"].sum() < o.gym.candidates()["mask"].sum()) for o in oracles[:8])
    assert narrowed > 0                      # the restriction removed candidates somewhere
    st = vec.read_stats()
    assert st["lp_errors"] == 0 and st["if_overflow"] == 0


def _raw(env, name):
    from bridges_hip import abi
    abi.check(getattr(env.L, name)(env._env, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def test_restriction_at_scale_and_the_option_off_changes_nothing():
    """1024 envs: after every lock-step the narrowed mask = the unrestricted mask ∧ (cand_stable == 1), n_valid its count,
    and an env left without a stable candidate is a no-action state whose next lock-step is reset-only; its record says done.
    Without the option the env is bit for bit the env driven by the plain entry points."""
    from robotoddler.training import records as R
    E = 1024
    vec = make_env("tower4", E, 5, f32_rasters=False, stable_actions_only=True)
    empty_states = 0
    for it in range(10):
        vec.select_random()
        sel_compact = vec.cand_offset[:E].long() + vec.sel_index.long()
        rec = R.pack_state(vec, sel_compact)
        vec.step()
        valid = R.pack_result(vec, rec)
        narrowed, stable = vec.cand_mask.clone(), vec.cand_stable.clone()
        nvalid, fl = vec.n_valid.clone(), vec.flags()
        _raw(vec, "bridges_env_refresh")                       # the unrestricted candidate set of the same states
        full = vec.cand_mask.clone()
        total = vec.total_candidates()
        assert torch.equal(narrowed[:total], full[:total] & (stable[:total] == 1).to(full.dtype)), it
        assert bool((stable[:total][full[:total].bool()] != 2).all())
        per_env = torch.zeros(E, dtype=torch.int64, device=vec.device).index_add_(
            0, vec.cand_env[:total].long(), narrowed[:total].long())
        assert torch.equal(per_env, nvalid.long())
        empty = nvalid == 0
        assert torch.equal(fl["no_actions"], empty)
        assert bool((rec[empty & valid, R.O_DONE] == 1).all())
        empty_states += int((empty & valid).sum())
        vec.restrict_to_stable()
        assert torch.equal(vec.cand_mask, narrowed)
        was_empty = empty.clone()
        vec.select_random()
        vec.step()
        assert not bool(vec.flags()["valid_step"][was_empty].any())          # reset-only
        assert bool((vec.n_blocks[was_empty] == 0).all())
    assert empty_states > 0

    from bridges_hip import abi
    a = make_env("tower4", E, 9, f32_rasters=False, stable_actions_only=False)
    b = make_env("tower4", E, 9, f32_rasters=False)
    for it in range(20):
        a.select_random()
        a.step()
        _raw(b, "bridges_env_select_random")
        _raw(b, "bridges_env_step")
        for name in ("cand_mask", "n_valid", "step_flags", "state_bits", "cand_bits", "n_cand", "cand_offset"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (it, name)
    assert a.read_stats() == b.read_stats()
    assert abi.lib().bridges_env_restrict_to_stable(None, None) != 0


def test_loaded_states_decide_their_candidates_like_the_rollout():
    """Records of a restricted rollout loaded into a restricted scratch env (load_records): the contact lists are rebuilt, so
    candidate stability runs, and its verdicts equal the rollout env's (warm path) and the unfused operator path (cold)."""
    from gpu_helpers import candidate_stability_unfused
    from robotoddler.training import records as R
    E = 1024
    roll = make_env("tower4", E, 11, f32_rasters=False, stable_actions_only=True)
    scratch = make_env("tower4", E, 0, f32_rasters=False, stable_actions_only=True)
    plain = make_env("tower4", E, 0, f32_rasters=False)
    compared = states = 0
    for it in range(6):
        roll.select_random()
        rec = R.pack_state(roll, roll.cand_offset[:E].long() + roll.sel_index.long())
        roll.step()
        valid = R.pack_result(roll, rec)
        live = (valid & (rec[:, R.O_DONE] < 0.5)).cpu().numpy()           # the rollout env still holds s' of these records
        # the rollout env's verdicts on the unrestricted candidates of s'
        r_off, r_nc = roll.cand_offset.cpu().numpy(), roll.n_cand.cpu().numpy()
        r_stable = roll.cand_stable.cpu().numpy()
        scratch.load_records(rec)
        plain.load_records(rec)
        with pytest.raises(Exception):
            plain.candidate_stability_mask()                               # no contact lists without the option
        s_off, s_nc = scratch.cand_offset.cpu().numpy(), scratch.n_cand.cpu().numpy()
        s_stable = scratch.cand_stable.cpu().numpy()
        p_mask = plain.cand_mask.cpu().numpy().astype(bool)
        rows, st_u, err_u = candidate_stability_unfused(plain)
        assert not bool(err_u.any())
        assert torch.equal(torch.from_numpy(s_stable).to(rows.device)[rows] == 1, st_u), it
        assert np.array_equal(s_off, plain.cand_offset.cpu().numpy())
        for e in np.flatnonzero(live):
            assert r_nc[e] == s_nc[e], (it, e)
            a = r_stable[r_off[e]:r_off[e] + r_nc[e]]
            b = s_stable[s_off[e]:s_off[e] + s_nc[e]]
            m = p_mask[s_off[e]:s_off[e] + s_nc[e]]
            assert np.array_equal(a[m] == 1, b[m] == 1), (it, e, np.flatnonzero((a == 1) != (b == 1)))
            compared += int(m.sum())
            states += 1
        n = scratch.candidate_stability_mask()                             # callable on loaded states now
        assert int(n) == int(scratch.n_valid.sum())
        assert not bool(scratch.flags()["lp_error"].any())
    assert states >= 1024 and compared > 10000


@pytest.mark.parametrize("model", ["SuccessorMLP", "ConvNet"])
def test_vec_dqn_acts_and_targets_over_stable_candidates(model):
    from robotoddler.training import records as R
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", model]))
    dev = torch.device("cuda")
    torch.manual_seed(3)
    pol, tgt = make_nets(args, dev)
    E = 256
    env = make_env("tower4", E, 21, f32_rasters=VecDQN.acting_needs_f32_rasters(pol), stable_actions_only=True)
    with pytest.raises(ValueError):
        VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 8192, 16, 0.95, 0.01, "mse_q_values")
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 8192, 16, 0.95, 0.01, "mse_q_values",
                   stable_actions_only=True)
    assert agent.replay_env.stable_actions_only
    orig_step, picked = env.step, [0]

    def checked_step(sel=None):
        has = env.n_valid[:E] > 0
        ci = env.cand_offset[:E].long() + sel.to(env.device).long()
        assert bool((env.cand_stable[ci][has] == 1).all()) and bool((env.cand_mask[ci][has] == 1).all())
        picked[0] += int(has.sum())
        return orig_step(sel)
    env.step = checked_step
    was_empty = None
    for it in range(8):
        rec, valid = agent.act()
        if was_empty is not None:                                # a state without stable candidates: reset-only lock-step
            assert not bool(valid[was_empty].any()) and bool((env.n_blocks[was_empty] == 0).all())
        was_empty = (env.n_valid[:E] == 0) & valid
        assert bool((rec[was_empty, R.O_DONE] == 1).all())
        agent.ring.push(rec[valid])
        agent.train_steps(2)
        agent.update_target()
    assert picked[0] > 1000
    # TD targets: a masked max over the replay env's stable next candidates, in plain torch
    n = 64
    rec = agent.ring.sample(n, agent.sample_gen)
    q_target = agent._targets(rec).q_target
    renv = agent.replay_env
    total = renv.total_candidates()
    full = renv.cand_mask[:total].bool()
    assert bool((renv.cand_stable[:total][full] == 1).all())
    idx = torch.nonzero(full).squeeze(1)
    row_env = renv.cand_env[idx].long()
    stable_n = rec[:, R.O_STABLE_N] > 0.5
    stable_all = torch.zeros(renv.E, dtype=torch.bool, device=dev)
    stable_all[:n] = stable_n
    stable_all[n:] = stable_n[0]
    q = agent._net_q(agent.target_net, renv, idx, row_env, stable_all).float()
    qmax = torch.full((renv.E,), -float("inf"), device=dev).scatter_reduce(0, row_env, q, reduce="amax")[:n]
    done = (rec[:, R.O_DONE] > 0.5) | (renv.n_valid[:n] == 0)
    want = rec[:, R.O_LIN].float() + torch.where(done, torch.zeros_like(qmax), 0.95 * qmax)
    assert torch.allclose(q_target, want, rtol=1e-5, atol=1e-6), float((q_target - want).abs().max())


def test_command_line_loops_with_stable_actions_only():
    from assembly_gym.envs.assembly_env import AssemblyEnv
    from assembly_gym.envs.gym_env import AssemblyGym, sparse_reward
    from assembly_gym.utils.stability import is_action_stable_rbe
    from robotoddler.training import successor_dqn as S
    from robotoddler.utils.actions import filter_actions, generate_actions
    hist = S.main(["--num_envs", "256", "--stable_actions_only", "--num_episodes", "300", "--tower_height", "2", "--model",
                   "SuccessorMLP", "--loss_function", "mse_q_values", "--num_training_steps", "2", "--seed", "1"])
    assert hist and hist[-1]["episodes"] >= 300
    hist = S.main(["--stable_actions_only", "--num_episodes", "2", "--tower_height", "2", "--model", "SuccessorMLP",
                   "--num_training_steps", "1", "--evaluate_every", "1000", "--seed", "1"])
    assert len(hist) == 2
    # the single-env rollout's action lists = filter_actions, then a per-action is_action_stable_rbe filter
    args = vars(S.build_parser().parse_args(["--tower_height", "2", "--model", "SuccessorMLP"]))
    dev = torch.device("cuda")
    pol, _ = S.make_nets(args, dev)
    setup = S.make_setup_fct(args)
    xg, offs, xlim, ylim, img = np.linspace(-2, 0, 10), [0], (-3, 7), (0., 10), (64, 64)
    checked = 0
    for ep in range(3):
        env = AssemblyGym(reward_fct=sparse_reward, max_steps=10, restrict_2d=True, assembly_env=AssemblyEnv(render=False))
        g = torch.Generator().manual_seed(ep)
        policy = lambda q, *a, **k: int(torch.randint(0, q.shape[0], (1,), generator=g))
        transitions, _ = S.rollout_episode(env, policy, pol, xg, setup, offset_values=offs, img_size=img, xlim=xlim, ylim=ylim,
                                           device=dev, stable_actions_only=True)
        ref = AssemblyGym(reward_fct=sparse_reward, max_steps=10, restrict_2d=True, assembly_env=AssemblyEnv(render=False))
        obs, _ = ref.reset(**setup())
        kw = dict(img_size=img, device=dev, xlim=xlim, ylim=ylim)
        _rf, obstacle_f = S.get_task_features(obs, **kw)
        for tr in transitions:
            obs, *_ = ref.step(tr.action)
            block_f, _ = S.get_state_features(obs, **kw)
            acts = [*generate_actions(ref, x_discr_ground=xg, offset_values=offs)]
            feats = S.get_action_features(ref, acts, **kw)
            kept, _ = filter_actions(ref, acts, feats, block_features=block_f, obstacle_features=obstacle_f, xlim=xlim, ylim=ylim)
            want = [a for a in kept if is_action_stable_rbe(ref, a)]
            key = lambda a: (a.target_block, a.target_face, a.shape, a.face, float(a.offset_x))
            assert [key(a) for a in tr.next_available_actions] == [key(a) for a in want]
            assert tr.next_actions_features.shape[0] == max(1, len(want))
            checked += len(want)
    assert checked > 0
