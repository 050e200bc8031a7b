"""CPU-only: the reference of Boltzmann exploration (tests/boltzmann_ref.py) -- against a plain statement of the rule, the probe
condition of its tables, the twins the tables must reject -- and the host side of the option: the Softmax policy of the single-env
loop, the command line, VecDQN's arguments, its checkpoint entry and its log keys."""
import math
import random

import numpy as np
import pytest
import torch

import boltzmann_ref as B
from test_cpu_nstep import host_agent, stand_in_env

NAN, INF = float("nan"), float("inf")


# --------------------------------------------------------------------------------------------------------------------- the rule
TINY = [
    ([0.0], 1.0), ([1.0, 2.0], 1.0), ([2.0, 1.0, 2.0], 0.1), ([0.5, 0.5, 0.5, 0.5], 1e-6), ([3.0, -1.0, 2.5], 1e30),
    ([1.0, NAN, 2.0, -INF, 0.5], 1.0), ([NAN, INF, 3.0, INF], 0.5), ([NAN, -INF], 1.0), ([1000.0, 999.0], 1.0),
    ([-1e38, 1e38], 1e-6), ([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], 0.25),
]


@pytest.mark.parametrize("q,T", TINY)
def test_reference_equals_the_plain_statement_on_tiny_cases(q, T):
    for u in (0.0, 0.05, 0.3, 0.5, 0.77, 0.95, 1.0 - 2.0 ** -24):
        row, p, ex, _margin = B.select_env(np.asarray(q, np.float32), u, T)
        want = B.brute_force(q, u, T)
        assert (row, ex) == (want[0], want[2]), (q, T, u)
        assert p == pytest.approx(want[1], rel=1e-15, abs=0.0), (q, T, u)


def test_reference_limits_of_the_temperature():
    """T -> 0: uniform among the exact ties of the maximum; T -> inf: uniform among the eligible rows; q / T far above 709: finite."""
    q = np.asarray([1.0, 3.0, NAN, 3.0, 2.9999998, -INF, 3.0], np.float32)
    rows = [B.select_env(q, u, 1e-30)[0] for u in (0.0, 0.3, 0.34, 0.6, 0.67, 0.99)]
    assert rows == [1, 1, 3, 3, 6, 6]
    rows = [B.select_env(q, (k + 0.5) / 5, 1e30)[0] for k in range(5)]
    assert rows == [0, 1, 3, 4, 6]
    row, p, ex, _ = B.select_env(np.asarray([3e38, 2.9e38], np.float32), 0.5, 1e-6)
    assert (row, p, ex) == (0, 1.0, 0.0)


def test_reference_of_a_whole_case_and_its_edges():
    case = B.random_probe(1.0)
    ref = B.reference(case)
    E = len(case["u"])
    lengths = case["seg_hi"] - case["seg_lo"]
    assert sorted(set(lengths.tolist())) == sorted(B.SEG_LENGTHS) and E == 4 * len(B.SEG_LENGTHS)
    empty = lengths == 0
    assert (ref["row"][empty] == 0).all() and (ref["q_sel"][empty] == 0).all() and (ref["p_sel"][empty] == 0).all()
    assert (ref["explore_w"][empty] == 0).all()
    has = ~empty
    assert ((ref["row"][has] >= case["seg_lo"][has]) & (ref["row"][has] < case["seg_hi"][has])).all()
    assert (ref["sel_index"][has] == 2 * (ref["row"][has] - case["seg_lo"][has]) + 1).all()          # the layout of the table
    assert ((ref["p_sel"][has] > 0) & (ref["p_sel"][has] <= 1)).all()
    single = lengths == 1
    assert (ref["p_sel"][single] == 1).all() and (ref["explore_w"][single] == 0).all()
    assert 0 < ref["explore_w"].sum() < has.sum()                                                     # both outcomes are probed
    g = B.reference(case, greedy=True)
    assert (g["explore_w"] == 0).all() and (g["p_sel"][has] == 1).all() and (g["p_sel"][empty] == 0).all()
    for e in np.flatnonzero(has):
        assert g["row"][e] == case["seg_lo"][e] + int(np.argmax(case["q"][case["seg_lo"][e]:case["seg_hi"][e]]))


def test_exact_probe_names_every_boundary():
    case, want = B.exact_probe()
    ref = B.reference(case)
    assert np.array_equal(ref["row"], want)
    assert len(want) == sum(n + 1 for n in (1, 2, 4, 8, 16, 32, 64, 128, 256)) <= 4096
    n256 = (case["seg_hi"] - case["seg_lo"]) == 256
    rel = (want - case["seg_lo"])[n256]
    assert {63, 64, 127, 128, 191, 192, 255} <= set(rel.tolist())                                  # both sides of every chunk edge
    assert np.allclose(ref["p_sel"], 1.0 / (case["seg_hi"] - case["seg_lo"]), rtol=0, atol=0)
    rep = case["rep"]
    assert np.array_equal(ref["sel_index"], want - case["seg_lo"])                                 # relative to the representative


def test_probe_condition_no_random_draw_lies_in_the_band():
    """Every draw of every table whose arithmetic is not exact keeps its target further than MARGIN (relative to the total) from
    every prefix sum: a condition on the INPUTS (the seeds are fixed), so the kernel is compared on all of them."""
    cases = B.margin_cases()
    assert len(cases) == len(B.TEMPERATURES) + len(B.NONFINITE) + 1
    worst = min(float(B.reference(c)["margin"].min()) for c in cases)
    assert worst > B.MARGIN, worst
    shared = B.shared_probe()
    assert len(shared["u"]) == 4096 and len(set(B.reference(shared)["row"].tolist())) > 64            # the draws spread over the rows


@pytest.mark.parametrize("twin", B.TWINS)
def test_every_defective_twin_is_rejected(twin):
    rejected = [i for i, c in enumerate(B.all_cases()) if B.differs(B.reference(c, twin=twin), B.reference(c))]
    assert rejected, twin


def test_the_rule_itself_passes_its_own_comparison():
    for c in B.all_cases():
        assert not B.differs(B.reference(c), B.reference(c))


# ------------------------------------------------------------------------------------------------------- Softmax, single-env loop
def test_softmax_schedule_is_the_closed_form():
    from robotoddler.training.successor_dqn import Softmax
    p = Softmax()
    assert (p.temp, p.temp_start, p.temp_end, p.decay) == (1, 1, 0.1, 0.99)
    for k in range(1, 40):
        assert p.step() is p
        assert p.temp == pytest.approx(0.9 * 0.99 ** k + 0.1, rel=1e-12)
    resumed = Softmax(temp_start=2.0, temp_end=0.5, decay=0.9, episode=7)
    assert resumed.temp == pytest.approx(1.5 * 0.9 ** 7 + 0.5, rel=1e-15)
    for bad in (dict(temp_end=0.0), dict(temp_end=-1.0), dict(temp_start=0.05), dict(decay=0.0), dict(decay=1.5),
                dict(temp_start=INF), dict(temp_end=NAN), dict(decay=NAN)):
        with pytest.raises(ValueError):
            Softmax(**bad)
    assert Softmax(temp_start=0.3, temp_end=0.3, decay=1.0).step().temp == 0.3


def test_softmax_draws_the_reference_row_from_the_random_stream(monkeypatch):
    from robotoddler.training import successor_dqn as S
    rng = np.random.default_rng(5)
    p = S.Softmax(temp_start=0.7, temp_end=0.2, decay=0.9)
    stream = [0.0, 0.11, 0.5, 0.93, 1.0 - 2.0 ** -30]
    tables = [rng.standard_normal(9).astype(np.float32), np.asarray([1.0, NAN, 2.0, -INF, 0.5], np.float32),
              np.asarray([NAN, -INF], np.float32), np.asarray([1000.0, 999.0], np.float32)]
    for q in tables:
        for u in stream:
            monkeypatch.setattr(S.random, "random", lambda u=u: u)
            got = p(torch.from_numpy(q), 3, None, None)                                            # rollout_episode's call
            assert isinstance(got, int) and got == B.select_env(q, u, p.temp)[0], (q, u)
        p.step()
    # the stream is ``random``'s: seeding it fixes the draws
    monkeypatch.undo()
    q = torch.from_numpy(tables[0])
    random.seed(3)
    a = [p(q) for _ in range(20)]
    random.seed(3)
    assert a == [p(q) for _ in range(20)] and len(set(a)) > 1


def test_log_episode_writes_the_temperature():
    from types import SimpleNamespace
    from robotoddler.training.successor_dqn import Softmax, log_episode
    t = SimpleNamespace(reward=torch.tensor(1.0), lin_reward=torch.tensor(0.5), next_binary_features=torch.zeros(1, 6))
    info, _ = log_episode(1, [t], None, 0.9, policy=Softmax(temp_start=0.6, temp_end=0.2))
    assert info["temperature"] == 0.6 and "epsilon" not in info


# ------------------------------------------------------------------------------------------------------------------ command line
def test_temperature_flags_need_the_option():
    from robotoddler.training import successor_dqn as S
    parse = lambda *argv: vars(S.build_parser().parse_args(list(argv)))
    plain = parse()
    assert not {"exploration", "temp_start", "temp_end", "temp_decay"} & set(plain)                # SUPPRESS: a plain parse is as it was
    S.check_exploration(plain)
    assert S.exploration_from_args(plain) == {}
    for flag in ("--temp_start", "--temp_end", "--temp_decay"):
        with pytest.raises(SystemExit, match="--exploration boltzmann"):
            S.check_exploration(parse(flag, "0.5"))
        with pytest.raises(SystemExit, match="--exploration boltzmann"):
            S.check_exploration(parse(flag, "0.5", "--exploration", "epsilon_greedy"))
    with pytest.raises(SystemExit, match="--exploration boltzmann"):
        S.main(["--temp_start", "0.5"])                                                           # refused before the GPU is asked for
    assert S.exploration_from_args(parse("--exploration", "boltzmann")) == dict(exploration="boltzmann", temp_start=1.0,
                                                                               temp_end=0.1, temp_decay=0.999)
    got = S.exploration_from_args(parse("--exploration", "boltzmann", "--temp_start", "2", "--temp_end", "0.5", "--temp_decay", "0.9"))
    assert got == dict(exploration="boltzmann", temp_start=2.0, temp_end=0.5, temp_decay=0.9)
    for bad in (["--temp_end", "0"], ["--temp_start", "0.05"], ["--temp_decay", "1.5"], ["--temp_start", "inf"], ["--temp_end", "nan"]):
        with pytest.raises(SystemExit):
            S.check_exploration(parse("--exploration", "boltzmann", *bad))
    with pytest.raises(SystemExit, match="eval_epsilon"):
        S.check_exploration(parse("--exploration", "boltzmann", "--eval_epsilon", "0.1"))
    with pytest.raises(SystemExit):
        parse("--exploration", "softmax")


# ----------------------------------------------------------------------------------------------------------------------- VecDQN
def test_vecdqn_arguments(monkeypatch):
    a = host_agent(monkeypatch, stand_in_env())
    assert a.exploration == "epsilon_greedy" and a._counts_host.numel() == 2
    b = host_agent(monkeypatch, stand_in_env(), exploration="boltzmann")
    assert (b.exploration, b.temperature, b.temp_start, b.temp_end, b.temp_decay) == ("boltzmann", 1.0, 1.0, 0.1, 0.999)
    assert b._counts_host.numel() == 3 and b.explored_fraction is None
    c = host_agent(monkeypatch, stand_in_env(), exploration="boltzmann", n_step=2, temp_start=0.5, temp_end=0.5, temp_decay=1.0)
    assert c._counts_host.numel() == 4 and c.temperature == 0.5
    with pytest.raises(ValueError, match="exploration"):
        host_agent(monkeypatch, stand_in_env(), exploration="softmax")
    for kw in (dict(temp_start=0.5), dict(temp_end=0.05), dict(temp_decay=0.9), dict(exploration="epsilon_greedy", temp_start=2.0)):
        with pytest.raises(ValueError, match="exploration='boltzmann'"):
            host_agent(monkeypatch, stand_in_env(), **kw)
    for kw in (dict(temp_end=0.0), dict(temp_end=-0.1), dict(temp_start=0.05), dict(temp_end=2.0), dict(temp_decay=0.0),
               dict(temp_decay=1.01), dict(temp_start=INF), dict(temp_start=NAN), dict(temp_end=NAN), dict(temp_decay=NAN)):
        with pytest.raises(ValueError):
            host_agent(monkeypatch, stand_in_env(), exploration="boltzmann", **kw)


def test_evaluate_refuses_epsilon_on_a_boltzmann_agent(monkeypatch):
    b = host_agent(monkeypatch, stand_in_env(), exploration="boltzmann")
    with pytest.raises(ValueError, match="exploration='boltzmann'"):
        b.evaluate(stand_in_env(), epsilon=0.1)


def test_checkpoint_entry_only_with_the_option(tmp_path):
    from robotoddler.training.vec_dqn import VecDQN

    def agent(exploration):
        a = VecDQN.__new__(VecDQN)
        a.n_task_targets, a.n_task_obstacles = 0, 0
        a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
        a.step_images = torch.zeros((3, 4, 4))
        a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        if exploration is not None:
            a.exploration, a.temp_start, a.temperature = exploration, 0.8, 0.8
        return a
    plain, path = str(tmp_path / "plain.pt"), str(tmp_path / "agent.pt")
    for old in (agent(None), agent("epsilon_greedy")):
        old.save_extra(plain, lockstep=5)
        assert "temperature" not in torch.load(plain, weights_only=True)
    b = agent("boltzmann")
    b.temperature = 0.4321
    b.save_extra(path, lockstep=9)
    assert torch.load(path, weights_only=True)["temperature"] == 0.4321
    c = agent("boltzmann")
    assert c.load_extra(path) == dict(lockstep=9) and c.temperature == 0.4321
    d = agent("boltzmann")
    d.temperature = 0.1
    assert d.load_extra(plain) == dict(lockstep=5) and d.temperature == 0.8                        # no key: temp_start
    e = agent("epsilon_greedy")
    e.load_extra(path)
    assert e.temperature == 0.8                                                                    # the entry is not read


def test_log_values_gain_two_keys_in_boltzmann_mode_only():
    from robotoddler.training.vec_dqn import EPISODE_KEYS, lockstep_log_values
    info = dict(mean_reward=0.1, mean_lin_reward=0.2, avg_loss=0.3, lockstep_env_steps=4, epsilon=0.5, env_steps=6, steps_per_s=7.0,
                **{k: None for k in EPISODE_KEYS})
    plain = lockstep_log_values(info)
    assert "temperature" not in plain and "explored_fraction" not in plain
    vals = lockstep_log_values(dict(info, temperature=0.7, explored_fraction=0.25))
    assert vals["temperature"] == 0.7 and vals["explored_fraction"] == 0.25
    assert {k: v for k, v in vals.items() if k not in ("temperature", "explored_fraction")} == plain


def test_entry_point_is_declared_with_its_rule():
    import os
    from bridges_hip import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bridges_hip.h")).read()
    assert "int bridges_boltzmann_select(int32_t E, int32_t n_rows," in header and "first j with c_j > target (strict)" in header
    assert "bridges_boltzmann_select" in abi.EXPORTED_SYMBOLS and len(abi.SIGNATURES["bridges_boltzmann_select"]) == 17
    assert math.isclose(B.MARGIN, 2.0 ** -40)
