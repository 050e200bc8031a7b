"""CPU: the hindsight relabelling rule (tests/hindsight_ref.py) against the oracle env -- an episode relabelled under targets its
own structure reached carries, step for step, the reward, the linear reward, the done flag and the open targets that an oracle
env reset to those targets gives for the same placements -- the properties of the counter-based choice of goal blocks, and every
refusal of VecDQN(hindsight=...) / --hindsight that needs no GPU."""
import types

import numpy as np
import pytest
import torch

import hindsight_ref as H
from oracle import raster as OR
from oracle.env import OracleGym, OracleLockstep, policy_draw
from oracle.geometry import create_block
from oracle.shapes import get_shape
from robotoddler.training import records as R
from task_draw import draw_targets

T, SEED, MAX_STEPS = 3, 11, 5
W = R.RECORD_WIDTH + 3 * T


def rollout(env_id, n_episodes, shape="trapezoid"):
    """Seeded random episodes of one oracle env on task_draw targets -> [(rows [m, W], flags [m, 8], actions, episode)]."""
    shapes = [get_shape(shape)]
    episodes = []
    counter = 0
    for ep in range(n_episodes):
        targets = draw_targets(SEED, env_id, ep, T)
        lock = OracleLockstep(OracleGym(shapes, [], targets, max_steps=MAX_STEPS))
        rows, flags, actions = [], [], []
        while True:
            def pick(nv):
                nonlocal counter
                counter += 1
                return policy_draw(SEED, env_id, counter) % nv
            if lock.needs_reset:
                break
            out = lock.lockstep(pick)
            row = np.zeros(W)
            row[R.O_NB] = out["n_blocks"] - 1
            row[R.O_ASHAPE] = out["action"][2]
            row[R.O_APOSE:R.O_APOSE + 4] = (*out["pose"][0], *out["pose"][1])
            row[R.O_ATB], row[R.O_ATF], row[R.O_AFACE] = out["action"][0], out["action"][1], out["action"][3]
            row[R.O_REWARD], row[R.O_LIN] = out["reward"], np.float32(out["lin_reward"])
            row[R.O_DONE] = float(out["done"] or out["no_actions"])
            row[R.O_STABLE_N] = float(out["stable_frozen"])
            row[R.RECORD_WIDTH:] = np.asarray(targets).reshape(-1)
            fl = np.zeros(8, dtype=np.uint8)
            fl[H.F_VALID], fl[H.F_STABLE_FROZEN], fl[H.F_STABLE_UNFROZEN] = 1, out["stable_frozen"], out["stable_unfrozen"]
            fl[H.F_TERMINATED], fl[H.F_TRUNCATED], fl[H.F_DONE] = out["terminated"], out["truncated"], out["done"]
            fl[H.F_NO_ACTIONS] = out["no_actions"]
            rows.append(row); flags.append(fl); actions.append(out["action"])
            if row[R.O_DONE]:
                break
        if rows:
            episodes.append((np.stack(rows), np.stack(flags), actions, ep))
    return shapes, episodes


@pytest.fixture(scope="module")
def episodes():
    out = []
    for env_id in (0, 1, 2):
        shapes, eps = rollout(env_id, 3)
        out += [(env_id, shapes) + e for e in eps]
    return out


def test_relabelled_episode_is_what_the_oracle_env_gives_under_the_hindsight_targets(episodes):
    checked = early = collapsed = 0
    for env_id, shapes, rows, flags, actions, ep in episodes:
        for g in (0, 1):
            trace = []
            new = H.relabel_episode(rows, flags, shapes, SEED, env_id, ep, g, T, task_cls=H.OracleTask, trace=trace)
            if H.eligible(rows) == 0:
                assert len(new) == 0 and not trace
                continue
            targets, picks, lefts = trace[0]
            collapsed += H.eligible(rows) < len(rows)
            gym = OracleGym(shapes, [], targets, max_steps=MAX_STEPS)
            X, Y = OR.pixel_grid(gym.xlim, gym.ylim, gym.img_size)
            for t in range(len(new)):
                block = create_block(shapes, gym.blocks, actions[t])
                base = np.float32(gym.reward_map[OR.contains_2d(block, X, Y)].astype(np.float64).sum())
                _stable, reward, term, trunc = gym.step(actions[t])
                fs, us = gym.stabilities_freezing()
                assert (fs, us) == (bool(flags[t][H.F_STABLE_FROZEN]), bool(flags[t][H.F_STABLE_UNFROZEN]))
                lin = base if us else (base / np.float32(100) if fs else np.float32(0))          # successor_dqn.py:397-401
                done = term or trunc or len(gym.blocks) >= 16 or bool(flags[t][H.F_NO_ACTIONS])
                assert new[t][R.O_REWARD] == reward, (env_id, ep, g, t)
                assert np.float32(new[t][R.O_LIN]) == np.float32(lin), (env_id, ep, g, t)
                assert bool(new[t][R.O_DONE]) == bool(done), (env_id, ep, g, t)
                open_now = sorted(targets[k] for k in range(T) if (lefts[t] >> k) & 1)
                assert open_now == sorted(gym.targets_remaining), (env_id, ep, g, t)
                assert np.array_equal(new[t][R.RECORD_WIDTH:], np.asarray(targets).reshape(-1))
                untouched = [c for c in range(R.RECORD_WIDTH) if c not in (R.O_REWARD, R.O_LIN, R.O_DONE)]
                assert np.array_equal(new[t][untouched], rows[t][untouched])
                # the replay ends where the relabelled episode ends, and not before
                if len(gym.targets_remaining) == 0:
                    assert t == len(new) - 1, (env_id, ep, g, t)
                checked += 1
            if len(new) < len(rows):
                assert len(gym.targets_remaining) == 0, (env_id, ep, g)
            early += len(new) < len(rows)
            # a hindsight target is the box centre of one of the episode's own blocks: that block reaches it
            for k, b in enumerate(picks):
                assert H.block_of(rows[b], shapes).aabb_contains(targets[k])
    assert checked >= 20 and early >= 1


def test_the_choice_of_blocks():
    for mp in range(1, 17):
        for Tn in (1, 3, 8):
            for g in range(4):
                picks = H.choose_blocks(SEED, 5, 2, g, mp, Tn)
                assert len(picks) == Tn and all(0 <= p < mp for p in picks)
                assert picks == H.choose_blocks(SEED, 5, 2, g, mp, Tn)                          # the same bits on every call
                if mp >= Tn:
                    assert len(set(picks)) == Tn                                                # distinct blocks
                else:
                    assert sorted(picks[:mp]) == list(range(mp))                                # a permutation, then t mod m'
                    assert all(picks[t] == picks[t % mp] for t in range(Tn))
    # slots, episodes, envs and seeds are separate streams: over 16 blocks their choices differ somewhere
    base = [H.choose_blocks(SEED, 5, 2, 0, 16, 3)]
    others = [H.choose_blocks(SEED, 5, 2, 1, 16, 3), H.choose_blocks(SEED, 5, 3, 0, 16, 3), H.choose_blocks(SEED, 6, 2, 0, 16, 3),
              H.choose_blocks(SEED + 1, 5, 2, 0, 16, 3)]
    assert all(o != base[0] for o in others)
    assert len({tuple(H.choose_blocks(SEED, 5, 2, g, 16, 3)) for g in range(4)}) == 4
    # every block can be chosen first: the draw covers the range
    assert {H.choose_blocks(SEED, e, 0, 0, 5, 1)[0] for e in range(200)} == set(range(5))
    # the word itself: integers only, the construction of the header
    from oracle.env import M64, splitmix64
    h = splitmix64(((((SEED & 0xFFFFFFFF) << 32) | 5) ^ 0x68696E645F726E67) & M64)
    assert H.hind_draw(SEED, 5, 2, 1, 0) == splitmix64(splitmix64(splitmix64(h ^ 2) ^ 1) ^ 0)


def test_collapsed_last_block_is_no_goal_and_an_empty_choice_emits_nothing():
    shapes = [get_shape("trapezoid")]
    row = np.zeros(W)
    row[R.O_APOSE:R.O_APOSE + 4] = (0.0, 0.0, 1.0, 0.0)
    fl = np.zeros(8, dtype=np.uint8)
    fl[H.F_VALID] = 1
    assert len(H.relabel_episode(row[None], fl[None], shapes, SEED, 0, 0, 0, T, task_cls=H.OracleTask)) == 0     # m' == 0
    two = np.stack([row, row])
    two[0][R.O_STABLE_N] = 1.0
    two[1][R.O_APOSE] = 1.5
    fls = np.stack([fl, fl])
    fls[0][H.F_STABLE_FROZEN] = fls[0][H.F_STABLE_UNFROZEN] = 1
    trace = []
    new = H.relabel_episode(two, fls, shapes, SEED, 0, 0, 0, T, task_cls=H.OracleTask, trace=trace)
    assert trace[0][1] == [0, 0, 0]                                                             # m' = 1 < T: block 0 three times
    # block 0 reaches target 0, the quirk skips target 1, target 2 is reached too: one target stays open after the first step
    assert trace[0][2][0] == 0b010 and len(new) == 2 and new[0][R.O_REWARD] == 1.0 and new[0][R.O_DONE] == 0.0
    assert new[1][R.O_REWARD] == -1.0 and new[1][R.O_LIN] == 0.0 and new[1][R.O_DONE] == 1.0     # the collapse stays a collapse


def test_the_probes_of_the_gpu_test_hold_every_case():
    """The scripted episodes tests/test_gpu_hindsight.py feeds the kernels, judged by the restatement alone: every case of the
    rule occurs among them, all of them in the 64-env and the 130-env probe on three targets (one target has neither m' < T nor
    a target to skip)."""
    union = set()
    for E, Tn, G, O, shape in H.PROBE_CONFIGS:
        seen = H.census(H.probe(E, Tn, O, shape, seed=H.probe_seed(E)), H.PROBE_SEED, H.PROBE_BASE, G)
        union |= seen
        if E >= 64:
            assert seen == set(H.CASES) - ({"few", "quirk"} if Tn == 1 else set()), (E, Tn, G, O, shape, seen)
    assert union == set(H.CASES)
    p = H.probe(64, 3, 0, "trapezoid", seed=H.probe_seed(64))
    assert p["buf"].shape == (64, 16, R.RECORD_WIDTH + 9) and H.probe(5, 3, 2, "hexagon", seed=1)["buf"].shape[2] == R.RECORD_WIDTH + 15


# ------------------------------------------------------------------------------------------------------------------------ VecDQN
def stand_in_env(**kw):
    base = dict(per_env_tasks=True, per_env_obstacles=False, img=64, n_targets=3, n_obstacles=0, device="cpu", K=4, E=2,
                stable_actions_only=False, max_steps=4)
    base.update(kw)
    return types.SimpleNamespace(**base)


def host_agent(monkeypatch, env, **kw):
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "_make_replay_env", lambda self, n: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8])
    return VecDQN(net, net, torch.optim.Adam(net.parameters(), lr=1e-4), env, 16, 4, 0.9, 0.05, "mse_block_features", **kw)


def test_vecdqn_refusals(monkeypatch):
    from robotoddler.training import distributed as D
    from robotoddler.training.curriculum import Curriculum
    a = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True)
    assert a.hindsight is None and a.hindsight_buffer is None and a._counts_host.numel() == 2
    b = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", hindsight_goals=2)
    assert b.hindsight == "final" and b._counts_host.numel() == 3
    hb = b.hindsight_buffer
    assert tuple(hb.rows.shape) == (2, 4, R.RECORD_WIDTH + 9) and tuple(hb.flags.shape) == (2, 4, 8) and hb.goals == 2
    assert tuple(hb.out.shape) == (2 * 4 * 2, R.RECORD_WIDTH + 9) and int(hb.length.sum()) == 0
    with pytest.raises(ValueError, match="hindsight"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="future")
    with pytest.raises(ValueError, match="hindsight_goals"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight_goals=2)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="hindsight_goals"):
            host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", hindsight_goals=bad)
    with pytest.raises(ValueError, match="per_env_tasks"):
        host_agent(monkeypatch, stand_in_env(per_env_tasks=False), hindsight="final")
    with pytest.raises(ValueError, match="task family"):
        host_agent(monkeypatch, stand_in_env(task_family=object()), per_env_tasks=True, hindsight="final")
    with pytest.raises(ValueError, match="curriculum"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", curriculum=Curriculum())
    with pytest.raises(ValueError, match="n_step"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", n_step=2)
    monkeypatch.setattr(D, "active", lambda: True)
    with pytest.raises(ValueError, match="one rank"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final")


def test_checkpoint_entries_and_the_refusal_of_another_setting(monkeypatch, tmp_path):
    plain = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True)
    one = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final")
    two = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", hindsight_goals=2)
    p0, p1 = str(tmp_path / "plain.pt"), str(tmp_path / "one.pt")
    plain.save_extra(p0, lockstep=1)
    assert "hindsight" not in torch.load(p0, weights_only=True)                                   # the file of a plain run is as it was
    one.hindsight_buffer.rows.normal_()
    one.hindsight_buffer.length[:] = torch.tensor([2, 0], dtype=torch.int32)
    one.hindsight_buffer.episode[:] = torch.tensor([7, 1], dtype=torch.int32)
    one.save_extra(p1, lockstep=3)
    assert tuple(torch.load(p1, weights_only=True)["hindsight"]) == ("final", 1)
    again = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final")
    assert again.load_extra(p1) == dict(lockstep=3)
    for name in ("rows", "flags", "length", "episode"):
        assert torch.equal(getattr(again.hindsight_buffer, name), getattr(one.hindsight_buffer, name))
    for agent, path in ((two, p1), (plain, p1), (one, p0)):
        with pytest.raises(ValueError, match="hindsight"):
            agent.load_extra(path)
    assert plain.load_extra(p0) == dict(lockstep=1)
    one.reset_window()                                                                            # env.reset() abandons the episodes
    assert int(one.hindsight_buffer.length.sum()) == 0


def test_buffer_write_appends_valid_envs_only():
    hb = R.HindsightBuffer(3, R.RECORD_WIDTH + 3, "cpu", goals=1, n_blocks=4)
    rec = torch.arange(3 * hb.width, dtype=torch.float64).reshape(3, hb.width)
    fl = torch.arange(24, dtype=torch.uint8).reshape(3, 8)
    hb.write(rec, fl, torch.tensor([True, False, True]), torch.tensor([4, 5, 6], dtype=torch.int32))
    hb.write(rec + 1000, fl + 100, torch.tensor([True, True, False]), torch.tensor([4, 9, 7], dtype=torch.int32))
    assert hb.length.tolist() == [2, 1, 1] and hb.episode.tolist() == [4, 9, 6]
    assert torch.equal(hb.rows[0, 0], rec[0]) and torch.equal(hb.rows[0, 1], rec[0] + 1000)
    assert torch.equal(hb.rows[1, 0], rec[1] + 1000) and torch.equal(hb.rows[2, 0], rec[2])
    assert torch.equal(hb.flags[0, 1], fl[0] + 100) and torch.equal(hb.flags[2, 0], fl[2])


# ------------------------------------------------------------------------------------------------------------------ command line
def test_command_line_refusals():
    from robotoddler.training import successor_dqn as S
    parse = lambda *argv: vars(S.build_parser().parse_args(list(argv)))
    plain = parse()
    assert not {"hindsight", "hindsight_goals"} & set(plain)                                      # SUPPRESS: a plain parse is as it was
    S.check_hindsight(plain)
    assert S.hindsight_from_args(plain) == {}
    ok = parse("--num_envs", "8", "--random_targets", "3", "--hindsight", "final")
    assert S.hindsight_from_args(ok) == dict(hindsight="final", hindsight_goals=1)
    assert S.hindsight_from_args(dict(ok, hindsight_goals=4)) == dict(hindsight="final", hindsight_goals=4)
    with pytest.raises(SystemExit, match="--hindsight final"):
        S.check_hindsight(parse("--hindsight_goals", "2"))
    with pytest.raises(SystemExit, match="--random_targets"):
        S.check_hindsight(parse("--num_envs", "8", "--hindsight", "final"))
    with pytest.raises(SystemExit, match="1..4"):
        S.check_hindsight(dict(ok, hindsight_goals=5))
    with pytest.raises(SystemExit, match="--n_step"):
        S.check_hindsight(dict(ok, n_step=2))
    with pytest.raises(SystemExit, match="task family"):
        S.check_hindsight(dict(ok, random_bridge_length=(1, 3)))
    with pytest.raises(SystemExit, match="--curriculum"):
        S.check_hindsight(dict(ok, curriculum=True))
    with pytest.raises(SystemExit):
        parse("--hindsight", "future")
    with pytest.raises(SystemExit, match="--random_targets"):
        S.main(["--hindsight", "final"])                                                          # refused before the GPU is asked for


def test_entry_point_is_declared_with_its_rule():
    import os
    from bridges_hip import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bridges_hip.h")).read()
    assert "int bridges_hindsight_relabel(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G," in header
    assert "0x68696E645F726E67" in header and bytes.fromhex("68696E645F726E67") == b"hind_rng"
    assert "bridges_hindsight_relabel" in abi.EXPORTED_SYMBOLS and len(abi.SIGNATURES["bridges_hindsight_relabel"]) == 24
    assert "bridges_hindsight_relabel_scratch" in abi.EXPORTED_SYMBOLS
    from bridges_hip import dqn_ops
    assert dqn_ops.hindsight_relabel_scratch(130, 4) >= 4 * 130 * 4 and dqn_ops.hindsight_relabel_scratch(0, 1) > 0
