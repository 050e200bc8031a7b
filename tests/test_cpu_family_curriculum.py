"""CPU: the host side of weighted task families and their curriculum -- the threshold table from integer weights (equal weights
reproduce the uniform draw for every u), the restated curriculum update, RandomBridges(weights=...)' argument checks, the host's
table against the restatement, and the CLI's options and refusals."""
import random

import pytest

from family_draw import family_draw, family_word
from weighted_family_draw import MAX_WEIGHT, class_of, curriculum_update, thresholds, weighted_family_draw

TOP = 1 << 32


# ------------------------------------------------------------------------------------------------- thresholds from weights
@pytest.mark.parametrize("C", range(1, 9))
def test_equal_weights_reproduce_the_uniform_draw(C):
    rng = random.Random(C)
    for w in (1, 3, 7, 65536, MAX_WEIGHT):
        thr = thresholds([w] * C)
        assert thr == [-((-(k + 1) * TOP) // C) for k in range(C - 1)] and len(thr) == C - 1
        us = {0, TOP - 1} | {t + d for t in thr for d in (-1, 0, 1)} | {rng.randrange(TOP) for _ in range(2000)}
        for u in us:
            if 0 <= u < TOP:
                assert class_of(u, 0, thr) == (u * C) >> 32, (w, u)
    for lo, hi in ((1, 4), (0, 7), (2, 2), (1, 3)):
        thr = thresholds([5] * (hi - lo + 1))
        for e in range(64):
            for k in range(6):
                assert weighted_family_draw(3, e, k, lo, hi, thr) == family_draw(3, e, k, lo, hi)
                assert weighted_family_draw(3, e, k, lo, hi, None) == family_draw(3, e, k, lo, hi)


def test_zero_weight_classes_are_never_drawn():
    cases = {(0, 3, 1): {1, 2}, (2, 0, 1): {0, 2}, (1, 3, 0): {0, 1}, (0, 0, 1, 0, 0): {2}, (0, 0, 0, 0, 0, 0, 1, 0): {6}}
    for weights, live in cases.items():
        thr = thresholds(weights)
        assert all(0 <= t <= TOP for t in thr) and thr == sorted(thr)
        us = [0, TOP - 1] + [t + d for t in thr for d in (-1, 0) if 0 <= t + d < TOP]
        us += [family_word(1, e, 0) >> 32 for e in range(500)]
        assert {class_of(u, 0, thr) for u in us} == live, weights
    assert thresholds((1, 3, 0)) == [1 << 30, TOP]                           # a trailing zero weight: 2^32, above every u
    assert thresholds((0, 3, 1)) == [0, 3 << 30]
    assert thresholds((0, 0, 0, 0, 0, 0, 1, 0)) == [0] * 6 + [TOP]


def test_thresholds_are_exact_ceilings_and_one_class_has_no_table():
    assert thresholds([9]) == [] and class_of(123, 2, []) == 2
    assert thresholds([1, 2]) == [1431655766] and 3 * 1431655766 >= TOP > 3 * 1431655765
    assert thresholds([1, 0, 2, 5]) == [536870912, 536870912, 1610612736]
    assert thresholds([MAX_WEIGHT] * 8)[-1] == 7 << 29
    # the device's conventions where the host refuses: a zero sum is the table of equal weights, a weight above 2^20 counts as 2^20
    assert thresholds([0, 0, 0]) == thresholds([1, 1, 1]) and thresholds([MAX_WEIGHT + 5, MAX_WEIGHT]) == [1 << 31]
    # the share of u that falls to a class is its weight's, to within one word
    weights = (3, 1, 4, 1, 5)
    edges = [0] + thresholds(weights) + [TOP]
    for k, w in enumerate(weights):
        assert abs((edges[k + 1] - edges[k]) - w * TOP / sum(weights)) < 1.0


def test_host_table_is_the_restatement():
    from bridges_hip.vec_env import family_thresholds
    rng = random.Random(0)
    for _ in range(300):
        C = rng.randint(1, 8)
        ws = [rng.choice([0, 1, rng.randint(0, MAX_WEIGHT)]) for _ in range(C)]
        if sum(ws):
            assert family_thresholds(ws) == thresholds(ws), ws


# ------------------------------------------------------------------------------------------------- the curriculum update
def row(e, s):
    return [float(e), 1.0, 2.0, 3.0, 4.0, float(s), 0.0, 0.0]


def test_curriculum_weights_of_unseen_perfect_and_failing_classes():
    w_min = 6554
    sums = [row(50, 50), [0.0] * 8, row(20, 20), row(10, 0), row(3, 3)]
    state = [[0.5, 1.0]] + [[0.0, 0.0] for _ in range(4)]
    w, thr = curriculum_update(sums, state, 1, 4, 0.25, w_min, 4)
    assert w == [w_min + 65536, w_min, w_min + 65536, w_min + 65536]        # unseen, all success, all fail, still unseen
    assert thr == thresholds(w)
    assert sums[0] == row(50, 50) and state[0] == [0.5, 1.0]                # outside the family: untouched
    assert sums[2] == [0.0] * 8 and sums[3] == [0.0] * 8                    # consumed rows are zeroed
    assert sums[4] == row(3, 3) and state[4] == [0.0, 0.0]                  # below min_episodes: left to accumulate
    assert state[1] == [0.0, 0.0] and state[2] == [1.0, 1.0] and state[3] == [0.0, 1.0]
    sums[4] = [a + b for a, b in zip(sums[4], row(1, 0))]                   # one more episode reaches min_episodes = 4
    w, _ = curriculum_update(sums, state, 1, 4, 0.25, w_min, 4)
    assert state[4] == [0.75, 1.0] and w[3] == w_min + 16384 and sums[4] == [0.0] * 8
    assert w[:3] == [w_min + 65536, w_min, w_min + 65536]                   # nothing new: the weights follow the state


def test_curriculum_ema_order_of_operations():
    beta, ema0 = 0.3, 1.0 / 3.0
    state, sums = [[ema0, 1.0]], [row(7, 3)]
    curriculum_update(sums, state, 0, 0, beta, 1, 1)
    rate = 3.0 / 7.0
    assert state[0][0] == ema0 + beta * (rate - ema0)
    assert state[0][0] != (1.0 - beta) * ema0 + beta * rate                 # the other textbook form rounds differently here
    # the first rate is taken as it is, and the weight rounds half up on fail * 65536
    state, sums = [[0.0, 0.0]], [row(7, 3)]
    w, thr = curriculum_update(sums, state, 0, 0, beta, 5, 1)
    assert state[0] == [rate, 1.0] and w == [5 + int((1.0 - rate) * 65536.0 + 0.5)] and thr == []
    # an ema outside [0, 1] (a hand-made state) is clamped
    for ema, want in ((1.5, 1), (-0.5, 1 + 65536)):
        w, _ = curriculum_update([[0.0] * 8], [[ema, 1.0]], 0, 0, beta, 1, 1)
        assert w == [want]


# ------------------------------------------------------------------------------------------------- RandomBridges(weights=...)
def test_random_bridges_weights_validation():
    from bridges_hip.vec_env import RandomBridges
    fam = RandomBridges("span", sizes=(1, 4), weights=[1, 0, 2, 5])
    assert fam.weights == (1, 0, 2, 5) and RandomBridges("span", sizes=(1, 4)).weights is None
    assert RandomBridges("tower", sizes=(2, 2), weights=(7,)).weights == (7,)
    assert RandomBridges("span", sizes=(1, 2), weights=(1 << 20, 0)).weights == (1 << 20, 0)
    for bad, msg in (((1, 2, 3), "one weight per class"), ((1, 2, 3, 4, 5), "one weight per class"), ((1, -1, 2, 5), "0 <= w"),
                     ((1, (1 << 20) + 1, 2, 5), "0 <= w"), ((0, 0, 0, 0), "not all be zero"), ((1, 0.5, 2, 5), "integers"),
                     ("abcd", "integers"), (5, "integers")):
        with pytest.raises(ValueError, match=msg):
            RandomBridges("span", sizes=(1, 4), weights=bad)


def test_curriculum_settings_validation():
    from robotoddler.training.curriculum import Curriculum
    c = Curriculum()
    assert (c.beta, c.floor, c.every, c.min_episodes, c.w_min) == (0.25, 0.1, 10, 16, 6554)
    assert Curriculum(floor=0.0).w_min == 1 and Curriculum(floor=1.0).w_min == 65536
    for kw in (dict(beta=-0.1), dict(beta=1.5), dict(floor=2.0), dict(every=0), dict(every=2.5), dict(min_episodes=0)):
        with pytest.raises(ValueError):
            Curriculum(**kw)


# ------------------------------------------------------------------------------------------------- the CLI
BASE = ["--model", "SuccessorMLP", "--num_envs", "8"]


def parse(argv):
    from robotoddler.training import successor_dqn as S
    args = vars(S.build_parser().parse_args(argv))
    S.check_random_targets(args)
    return args


def test_cli_parses_the_options():
    from robotoddler.training.curriculum import Curriculum
    from robotoddler.training.vec_dqn import curriculum_from_args
    args = parse(BASE + ["--random_bridge_length", "1:3", "--family_weights", "1,0,4"])
    assert args["family_weights"] == (1, 0, 4) and curriculum_from_args(args) is None
    args = parse(BASE + ["--random_tower_height", "0:2", "--curriculum"])
    assert curriculum_from_args(args) == Curriculum()
    args = parse(BASE + ["--random_bridge_length", "1:3", "--curriculum", "--curriculum_every", "5", "--curriculum_beta", "0.5",
                         "--curriculum_floor", "0.02"])
    assert curriculum_from_args(args) == Curriculum(beta=0.5, floor=0.02, every=5) and "family_weights" not in args
    conv = ["--model", "ConvNet", "--num_envs", "8", "--task_channels", "--random_bridge_length", "1:2", "--curriculum"]
    assert curriculum_from_args(parse(conv)) == Curriculum()
    assert "curriculum" not in parse(BASE) and "family_weights" not in parse(BASE)


@pytest.mark.parametrize("argv,msg", [
    (BASE + ["--curriculum"], "--curriculum weighs the classes of a task family"),
    (BASE + ["--family_weights", "1,2"], "--family_weights weighs the classes of a task family"),
    (BASE + ["--random_targets", "2", "--curriculum"], "--curriculum weighs the classes of a task family"),
    (BASE + ["--curriculum_every", "5"], "--curriculum_every weighs the classes of a task family"),
    (["--model", "SuccessorMLP", "--random_bridge_length", "1:3", "--curriculum"], "needs the vectorised loop"),
    (["--model", "SuccessorMLP", "--random_bridge_length", "1:3", "--family_weights", "1,1,1"], "needs the vectorised loop"),
    (BASE + ["--random_bridge_length", "1:3", "--family_weights", "1,2"], "one weight per class"),
    (BASE + ["--random_bridge_length", "1:3", "--family_weights", "0,0,0"], "not all be zero"),
    (BASE + ["--random_bridge_length", "1:3", "--family_weights", "1,2,2000000"], "0 <= w"),
    (BASE + ["--random_bridge_length", "1:3", "--curriculum", "--family_weights", "1,1,1"], "cannot be combined"),
    (BASE + ["--random_bridge_length", "1:3", "--curriculum_beta", "0.5"], "give --curriculum as well"),
    (BASE + ["--random_bridge_length", "1:3", "--curriculum", "--curriculum_beta", "1.5"], "--curriculum_beta must be in"),
    (BASE + ["--random_bridge_length", "1:3", "--curriculum", "--curriculum_every", "0"], "--curriculum_every must be"),
])
def test_cli_refusals(argv, msg):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert msg in str(e.value), e.value


def test_cli_refuses_weights_that_are_no_integers(capsys):
    with pytest.raises(SystemExit):
        parse(BASE + ["--random_bridge_length", "1:3", "--family_weights", "1,x,2"])
    assert "expected W,W,..." in capsys.readouterr().err


def test_log_values_carry_the_weights():
    from robotoddler.training.vec_dqn import EPISODE_KEYS, lockstep_log_values
    info = dict(mean_reward=0.0, mean_lin_reward=0.0, avg_loss=None, lockstep_env_steps=1, epsilon=0.1, env_steps=1, steps_per_s=1.0,
                **{k: None for k in EPISODE_KEYS})
    assert not any(k.startswith("curriculum_weight") for k in lockstep_log_values(info))
    vals = lockstep_log_values(dict(info, curriculum_weights=[70000, 6554, 40000], class_lo=1))
    assert {k: v for k, v in vals.items() if k.startswith("curriculum_weight")} == dict(
        curriculum_weight_n1=70000, curriculum_weight_n2=6554, curriculum_weight_n3=40000)
