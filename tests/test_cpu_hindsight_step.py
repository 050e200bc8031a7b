"""CPU: the rule of hindsight relabelling with per-step goals (tests/hindsight_step_ref.py; hindsight experience replay's "future")
-- the probes of the GPU test hold every case of it, every deliberately defective twin is told apart on them, the properties
that follow from the rule (target 0 is reached by step f, one target: done exactly at the first block that holds it, n_step = 1
through the fold is the one-step row), the oracle env replayed under a row's targets -- and every acceptance and refusal of
VecDQN(hindsight="per_step") / --hindsight per_step that needs no GPU."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import hindsight_step_ref as S
from oracle import raster as OR
from oracle.env import M64, OracleGym, splitmix64
from oracle.geometry import create_block
from robotoddler.training import records as R
from test_cpu_hindsight import MAX_STEPS, SEED, T, rollout

PSEED, PBASE = S.PROBE_SEED, S.PROBE_BASE
BIG = (64, 3, 4, 0, "trapezoid")
GAMMA = 0.95
ROWS = dict(zip(S.PROBE_CONFIGS, (1, 76, 843, 754, 384, 449)))


class FlatTask:
    """A task whose base is a function of the block alone: twins that differ in goals, masks or counts need no reward map."""
    def __init__(self, targets):
        self.k = float(sum(t[0] + 2 * t[2] for t in targets))

    def base(self, block):
        x0, z0, x1, z1 = block.aabb
        return np.float32(abs(self.k + x0 + z1) % 7)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def probe(cfg):
    E, Tn, _G, O, shape = cfg
    return S.probe(E, Tn, O, shape, seed=S.probe_seed(E))


@functools.lru_cache(maxsize=None)
def rows_of(cfg, n=None, twin=None, task=FlatTask):
    p = probe(cfg)
    trace = []
    out = S.relabel(p["buf"], p["flags"], p["length"], p["ended"], p["episode"], p["shapes"], PSEED, PBASE, cfg[2], cfg[1], n_step=n,
                    gamma=None if n is None else GAMMA, task_cls=task, twin=twin, trace=trace)
    out.setflags(write=False)
    return out, trace


def test_the_probes_hold_every_case_and_emit_the_rows_of_the_rule():
    assert S.census(probe(BIG), PSEED, PBASE, BIG[2]) == set(S.CASES)          # a condition, not a measurement
    for cfg in S.PROBE_CONFIGS:
        assert len(rows_of(cfg)[0]) == ROWS[cfg], cfg


@pytest.mark.parametrize("twin", S.TWINS)
def test_every_defective_twin_differs_from_the_rule_on_the_probes(twin):
    n = 3 if twin in S.FOLD_TWINS else None
    differs = []
    for cfg in ((5, 3, 4, 2, "hexagon"), BIG):
        ref, bad = rows_of(cfg, n)[0], rows_of(cfg, n, twin)[0]
        differs.append(ref.shape != bad.shape or not np.array_equal(bits(ref), bits(bad)))
    assert differs[1], twin                                                    # the big probe tells every twin apart
    if twin not in S.FOLD_TWINS:                                               # and the one-step twins through the fold as well
        ref, bad = rows_of(BIG, 3)[0], rows_of(BIG, 3, twin)[0]
        assert ref.shape != bad.shape or not np.array_equal(bits(ref), bits(bad))


def test_order_and_untouched_columns():
    p = probe(BIG)
    out, trace = rows_of(BIG)
    keys = [(e, g, t) for e, g, t, _ in trace]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)                # (env, slot, t) ascending, one row at most
    Tn = BIG[1]
    untouched = [c for c in range(p["buf"].shape[2]) if c not in (R.O_REWARD, R.O_LIN, R.O_DONE)
                 and not R.RECORD_WIDTH <= c < R.RECORD_WIDTH + 3 * Tn]
    for row, (e, g, t, tr) in zip(out, trace):
        assert np.array_equal(bits(row[untouched]), bits(p["buf"][e, t][untouched]))
        assert np.array_equal(row[R.RECORD_WIDTH:R.RECORD_WIDTH + 3 * Tn], np.asarray(tr["targets"]).reshape(-1))
        assert t < S.eligible(p["buf"][e, :p["length"][e]])                      # never the collapsed last step
    assert not any(not p["ended"][e] for e, _g, _t, _ in trace)                # envs in mid-episode emit nothing


def test_target_zero_is_block_f_and_is_reached_at_or_before_step_f():
    for cfg in ((5, 3, 4, 2, "hexagon"), BIG, (64, 1, 4, 2, "trapezoid")):
        p = probe(cfg)
        for e, g, t, tr in rows_of(cfg)[1]:
            rows = p["buf"][e, :p["length"][e]]
            f, targets = tr["f"], tr["targets"]
            assert t <= f < S.eligible(rows) and tr["picks"][0] == f and all(b <= f for b in tr["picks"])
            assert targets[0] == S.box_centre(S.block_of(rows[f], p["shapes"]))
            left = (1 << cfg[1]) - 1
            for s in range(f + 1):
                left = S.reach(left, targets, S.block_of(rows[s], p["shapes"]))
            assert not left & 1, (cfg, e, g, t)
            if f + 1 >= cfg[1]:
                assert len(set(tr["picks"])) == cfg[1]                         # distinct blocks while the structure has enough


def test_one_target_is_done_exactly_where_the_first_block_containing_it_is_placed():
    cfg = (64, 1, 4, 2, "trapezoid")
    p = probe(cfg)
    out, trace = rows_of(cfg)
    done = 0
    for row, (e, g, t, tr) in zip(out, trace):
        rows, fl = p["buf"][e, :p["length"][e]], p["flags"][e]
        first = next(s for s in range(len(rows)) if S.block_of(rows[s], p["shapes"]).aabb_contains(tr["targets"][0]))
        assert first >= t and first <= tr["f"]                                 # (a row exists: no earlier block held the target)
        assert (tr["left_after"] == 0) == (first == t)
        other = bool(not fl[t][S.F_STABLE_FROZEN] or fl[t][S.F_TRUNCATED] or fl[t][S.F_NO_ACTIONS])
        assert bool(row[R.O_DONE]) == (first == t or other)
        if fl[t][S.F_STABLE_FROZEN]:
            assert row[R.O_REWARD] == (1.0 if first == t else -1.0)
        done += first == t
    assert done >= 50 and done < len(out)


def test_n_step_one_through_the_fold_is_the_one_step_row_with_a_column_of_one():
    for cfg in ((5, 3, 4, 2, "hexagon"), BIG):
        one, fold = rows_of(cfg)[0], rows_of(cfg, 1)[0]
        assert fold.shape == (len(one), one.shape[1] + 1)
        assert np.array_equal(bits(fold[:, :-1]), bits(one)) and np.all(fold[:, -1] == 1.0)
    one, fold = rows_of((5, 3, 4, 2, "hexagon"), task=S.DeviceTask)[0], rows_of((5, 3, 4, 2, "hexagon"), 1, task=S.DeviceTask)[0]
    assert np.array_equal(bits(fold[:, :-1]), bits(one)) and np.all(fold[:, -1] == 1.0)


def test_the_h_step_row_is_the_fold_of_its_walk():
    p = probe(BIG)
    for n in (2, 3, 8):
        out, trace = rows_of(BIG, n)
        assert len(out) == ROWS[BIG]
        hs = set()
        for row, (e, g, t, tr) in zip(out, trace):
            m = int(p["length"][e])
            h, last = tr["h"], tr["last"]
            assert row[-1] == h and 1 <= h <= n and last == t + h - 1 < m and int(row[R.O_NB]) == last
            assert row[R.O_STABLE_S] == p["buf"][e, t, R.O_STABLE_S] and row[R.O_TD] == p["buf"][e, t, R.O_TD]
            if h < n:                                                          # the window was cut: the walk ended at last
                left = tr["left_before"]
                for s in range(t, last + 1):
                    left = S.reach(left, tr["targets"], S.block_of(p["buf"][e, s], p["shapes"]))
                assert left == 0 or last == m - 1
            hs.add(h)
        assert hs == set(range(1, n + 1)) if n < 8 else len(hs) >= 6


def test_the_draw_is_the_construction_of_the_header():
    h0 = splitmix64(((((SEED & 0xFFFFFFFF) << 32) | 5) ^ 0x68696E645F726E67) & M64)
    h2 = splitmix64(splitmix64(h0 ^ 2) ^ 1)
    assert S.step_draw(SEED, 5, 2, 1, 3, 2) == splitmix64(splitmix64(h2 ^ (4 << 8)) ^ 2)
    for mp in range(1, 17):
        for t in range(mp):
            f, picks = S.choose_step_blocks(SEED, 5, 2, 0, t, mp, 3)
            assert t <= f < mp and picks[0] == f and all(0 <= b <= f for b in picks)
            assert (f, picks) == S.choose_step_blocks(SEED, 5, 2, 0, t, mp, 3)
    # steps are separate streams, and the future block covers [t, m')
    assert len({tuple(S.choose_step_blocks(SEED, 5, 2, 0, t, 16, 3)[1]) for t in range(8)}) >= 7
    assert {S.choose_step_blocks(SEED, e, 0, 0, 2, 6, 1)[0] for e in range(200)} == {2, 3, 4, 5}


def test_the_row_is_what_the_oracle_env_gives_at_step_t_under_its_targets():
    checked = early = skipped = 0
    for env_id in (0, 1, 2):
        shapes, eps = rollout(env_id, 3)
        for rows, flags, actions, ep in eps:
            for g in (0, 1):
                for t in range(len(rows)):
                    tr = {}
                    row = S.relabel_step(rows, flags, shapes, SEED, env_id, ep, g, t, T, task_cls=S.OracleTask, trace=tr)
                    if row is None:
                        skipped += 1
                        continue
                    targets = tr["targets"]
                    gym = OracleGym(shapes, [], targets, max_steps=MAX_STEPS)
                    X, Y = OR.pixel_grid(gym.xlim, gym.ylim, gym.img_size)
                    for s in range(t):
                        _stable, _r, term, _trunc = gym.step(actions[s])
                        assert not term, (env_id, ep, g, t, s)                 # the transition exists: the episode ran on
                    block = create_block(shapes, gym.blocks, actions[t])
                    base = np.float32(gym.reward_map[OR.contains_2d(block, X, Y)].astype(np.float64).sum())
                    _stable, reward, term, trunc = gym.step(actions[t])
                    fs, us = gym.stabilities_freezing()
                    lin = base if us else (base / np.float32(100) if fs else np.float32(0))
                    done = term or trunc or len(gym.blocks) >= 16 or bool(flags[t][S.F_NO_ACTIONS])
                    assert row[R.O_REWARD] == reward, (env_id, ep, g, t)
                    assert np.float32(row[R.O_LIN]) == np.float32(lin), (env_id, ep, g, t)
                    assert bool(row[R.O_DONE]) == bool(done), (env_id, ep, g, t)
                    open_now = sorted(targets[k] for k in range(T) if (tr["left_after"] >> k) & 1)
                    assert open_now == sorted(gym.targets_remaining), (env_id, ep, g, t)
                    early += len(gym.targets_remaining) == 0
                    checked += 1
    print(f"{checked} rows replayed, {early} ended on their hindsight targets, {skipped} work items without a row")
    assert checked >= 20 and early >= 1


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


def test_vecdqn_accepts_per_step_and_keeps_every_refusal(monkeypatch):
    from robotoddler.training import distributed as D
    from robotoddler.training.curriculum import Curriculum
    from robotoddler.training.vec_dqn import VecDQN
    assert 'strategy "future"' in VecDQN.__init__.__doc__ and "stays refused" in VecDQN.__init__.__doc__
    b = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step", hindsight_goals=2)
    assert b.hindsight == "per_step" and b._counts_host.numel() == 3
    hb = b.hindsight_buffer
    assert hb.strategy == "per_step" and hb.goals == 2 and tuple(hb.out.shape) == (2 * 4 * 2, R.RECORD_WIDTH + 9)
    assert hb._scratch.numel() == 2 * 4 * 2 * 2                                # a count and a mask per (env, slot)
    f = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step", n_step=2, hindsight_fold=True)
    assert f.hindsight_buffer.fold and f.hindsight_buffer.strategy == "per_step"
    assert tuple(f.hindsight_buffer.out.shape) == (2 * 4, R.RECORD_WIDTH + 9 + 1)
    assert host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final").hindsight_buffer.strategy == "final"
    with pytest.raises(ValueError, match="hindsight"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="future")      # the strategy's other name stays refused
    with pytest.raises(ValueError, match="strategy"):
        R.HindsightBuffer(2, R.RECORD_WIDTH + 9, "cpu", strategy="future")
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="hindsight_goals"):
            host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step", hindsight_goals=bad)
    with pytest.raises(ValueError, match=r"per_step.*per_env_tasks"):
        host_agent(monkeypatch, stand_in_env(per_env_tasks=False), hindsight="per_step")
    with pytest.raises(ValueError, match=r"per_step.*task family"):
        host_agent(monkeypatch, stand_in_env(task_family=object()), per_env_tasks=True, hindsight="per_step")
    with pytest.raises(ValueError, match=r"per_step.*curriculum"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step", curriculum=Curriculum())
    with pytest.raises(ValueError, match=r"per_step.*n_step"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step", n_step=2)
    monkeypatch.setattr(D, "active", lambda: True)
    with pytest.raises(ValueError, match=r"per_step.*one rank"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step")


def test_a_checkpoint_of_one_strategy_is_refused_by_the_other(monkeypatch, tmp_path):
    final = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final")
    step = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step")
    pf, ps = str(tmp_path / "final.pt"), str(tmp_path / "step.pt")
    final.save_extra(pf, lockstep=2)
    step.hindsight_buffer.rows.normal_()
    step.hindsight_buffer.length[:] = torch.tensor([2, 1], dtype=torch.int32)
    step.save_extra(ps, lockstep=3)
    assert tuple(torch.load(pf, weights_only=True)["hindsight"]) == ("final", 1)              # the key "final" always wrote
    assert tuple(torch.load(ps, weights_only=True)["hindsight"]) == ("per_step", 1)
    assert set(torch.load(ps, weights_only=True)) == set(torch.load(pf, weights_only=True))   # no new key
    for agent, path in ((final, ps), (step, pf)):
        with pytest.raises(ValueError, match="hindsight"):
            agent.load_extra(path)
    again = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="per_step")
    assert again.load_extra(ps) == dict(lockstep=3)
    for name in ("rows", "flags", "length", "episode"):
        assert torch.equal(getattr(again.hindsight_buffer, name), getattr(step.hindsight_buffer, name))
    assert host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final").load_extra(pf) == dict(lockstep=2)


# ------------------------------------------------------------------------------------------------------------------ command line
def test_command_line_accepts_per_step_and_keeps_every_refusal():
    from robotoddler.training import successor_dqn as D
    parse = lambda *argv: vars(D.build_parser().parse_args(list(argv)))
    assert not {"hindsight", "hindsight_goals", "hindsight_fold"} & set(parse())               # a plain parse is as it was
    ok = parse("--num_envs", "8", "--random_targets", "3", "--hindsight", "per_step")
    assert D.hindsight_from_args(ok) == dict(hindsight="per_step", hindsight_goals=1)
    assert D.hindsight_from_args(dict(ok, hindsight_goals=4)) == dict(hindsight="per_step", hindsight_goals=4)
    assert D.hindsight_from_args(dict(ok, n_step=3, hindsight_fold=True)) == dict(hindsight="per_step", hindsight_goals=1,
                                                                                  hindsight_fold=True)
    with pytest.raises(SystemExit, match="per_step"):
        D.check_hindsight(parse("--hindsight_goals", "2"))
    with pytest.raises(SystemExit, match=r"--hindsight per_step.*--random_targets"):
        D.check_hindsight(parse("--num_envs", "8", "--hindsight", "per_step"))
    with pytest.raises(SystemExit, match="1..4"):
        D.check_hindsight(dict(ok, hindsight_goals=5))
    with pytest.raises(SystemExit, match=r"--hindsight per_step.*--n_step"):
        D.check_hindsight(dict(ok, n_step=2))
    with pytest.raises(SystemExit, match=r"--hindsight per_step.*task family"):
        D.check_hindsight(dict(ok, random_bridge_length=(1, 3)))
    with pytest.raises(SystemExit, match=r"--hindsight per_step.*--curriculum"):
        D.check_hindsight(dict(ok, curriculum=True))
    with pytest.raises(SystemExit):
        parse("--hindsight", "future")
    with pytest.raises(SystemExit, match="--random_targets"):
        D.main(["--hindsight", "per_step"])                                                    # refused before the GPU is asked for


def test_the_tools_take_the_value_through_the_shared_arguments():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tool in ("train_throughput.py", "learning_curve.py", "find_syncs.py"):
        src = open(os.path.join(root, "tools", tool)).read()
        assert "add_training_arguments(ap" in src and "agent_options_from_args(vars(a)" in src, tool
    from robotoddler.training import successor_dqn as D
    import argparse
    ap = argparse.ArgumentParser()
    D.add_training_arguments(ap, prioritized_flag=True)
    a = vars(ap.parse_args(["--hindsight", "per_step", "--hindsight_goals", "2"]))
    assert a["hindsight"] == "per_step" and a["hindsight_goals"] == 2
    assert "--strategy" in open(os.path.join(root, "tools", "hindsight_relabel_bench.py")).read()


def test_entry_points_are_declared_with_their_rule():
    from bridges_hip import abi, dqn_ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bridges_hip.h")).read()
    assert "int bridges_hindsight_per_step(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G," in header
    assert "int bridges_hindsight_per_step_nstep(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G," in header
    assert "int bridges_hindsight_per_step_scratch(int32_t E, int32_t G, int64_t* bytes);" in header
    rule = header[header.index('("per_step" strategy'):header.index("int bridges_hindsight_per_step_scratch")]
    for words in ("h3 = splitmix64(h2 ^ ((t + 1) << 8))", "f = t + ((u_0 * (m' - t)) >> 32)", "swap(idx[0], idx[f])",
                  "j = i + ((u_i * (n - i)) >> 32)", "idx[q mod n]", "was over before step t", "\"future\"", "An open end flushes"):
        assert words in rule, words
    for name, n_args in (("bridges_hindsight_per_step", 24), ("bridges_hindsight_per_step_nstep", 26),
                         ("bridges_hindsight_per_step_scratch", 3)):
        assert name in abi.EXPORTED_SYMBOLS and len(abi.SIGNATURES[name]) == n_args
    assert abi.SIGNATURES["bridges_hindsight_per_step"] == abi.SIGNATURES["bridges_hindsight_relabel"]
    assert abi.SIGNATURES["bridges_hindsight_per_step_nstep"] == abi.SIGNATURES["bridges_hindsight_relabel_nstep"]
    assert dqn_ops.hindsight_relabel_scratch(130, 4, "per_step") == 2 * 4 * 130 * 4 and dqn_ops.hindsight_relabel_scratch(0, 1, "per_step") > 0
    assert dqn_ops.hindsight_relabel_scratch(130, 4) == 4 * 130 * 4                            # "final"'s stays what it was
    with pytest.raises(ValueError, match="strategy"):
        dqn_ops.hindsight_relabel_scratch(130, 4, "future")
