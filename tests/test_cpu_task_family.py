"""CPU: the host side of the task families (RandomBridges / bridges_task_family) -- the restated draw of ONE integer per env
and episode, the coordinates it names against the oracle's setup functions, parked obstacle slots on the oracle's rasteriser, the
ctypes mirror of the new struct, RandomBridges' argument checks, the CLI's refusals, and the per-class fold's restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from class_stats_ref import RestatedByClass
from family_draw import FAMI_SALT, PARK_Z, draw_family, family_draw, family_task, family_word
from obstacle_draw import obstacle_draw
from oracle import raster as R
from oracle.env import XLIM, YLIM, bridge_setup, horizontal_bridge_setup
from oracle.geometry import Block
from oracle.shapes import get_shape
from task_draw import task_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draw_against_the_pinned_words():
    assert FAMI_SALT == int.from_bytes(b"fami_rng", "big")
    r = family_word(5, 17, 3)
    assert r == 0x3A70A4E6B9689D3E and r >> 32 == 980460774
    assert [family_draw(5, 17, 3, lo, hi) for lo, hi in ((1, 4), (2, 3), (0, 4))] == [1, 2, 1]
    drawn = [family_draw(0, e, 0, 1, 4) for e in range(32)]
    assert drawn == [int(v) for v in "2 4 1 1 1 1 3 1 3 4 1 2 3 1 1 2 1 3 4 2 3 3 4 1 3 4 2 1 1 4 4 2".split()]
    assert [drawn.count(k) for k in (1, 2, 3, 4)] == [12, 6, 7, 7]


def test_draw_is_in_range_and_a_stream_of_its_own():
    for seed in (0, 3, 2 ** 31 + 5, 2 ** 32 - 1):
        for env in (0, 1, 4095, 70000, 2 ** 32 - 1):
            for ep in (0, 1, 977):
                assert family_draw(seed, env, ep, 3, 3) == 3                  # lo == hi: no choice
                for lo, hi in ((0, 4), (0, 1), (1, 4), (2, 3)):
                    n = family_draw(seed, env, ep, lo, hi)
                    assert isinstance(n, int) and lo <= n <= hi
    # every class of the widest range occurs, and about equally often
    ns = [family_draw(7, e, 0, 0, 4) for e in range(5000)]
    assert min(ns.count(k) for k in range(5)) > 850 and max(ns.count(k) for k in range(5)) < 1150
    base = (5, 17, 3)
    for i, other in enumerate([6, 18, 4]):
        key = list(base)
        key[i] = other
        assert family_word(*key) != family_word(*base), i
    # targets, obstacles and families draw from different streams: same key, other words
    for e in range(8):
        for k in range(8):
            w = family_word(5, e, k)
            assert w not in {task_draw(5, e, k, t, a) for t in range(8) for a in (0, 1, 2)}
            assert w not in {obstacle_draw(5, e, k, o, a) for o in range(4) for a in (0, 1, 2)}


@pytest.mark.parametrize("n", range(5))
def test_coordinates_are_the_setup_functions_numbers(n):
    hi = 4
    span = horizontal_bridge_setup(num_obstacles=n)
    targets, obstacles = family_task("span", n, hi)
    assert [tuple(map(float, t)) for t in span["targets"]] == targets
    assert [tuple(map(float, o)) for o in span["obstacles"]] == obstacles[:n] and len(span["obstacles"]) == n
    tower = bridge_setup(num_stories=n)
    targets, obstacles = family_task("tower", n, hi)
    assert [tuple(map(float, t)) for t in tower["targets"]] == targets
    assert [tuple(map(float, o)) for o in tower["obstacles"]] == obstacles[:n] and len(tower["obstacles"]) == n
    assert obstacles[n:] == [(0.0, 0.0, PARK_Z)] * (hi - n) and len(obstacles) == hi
    # other sizes go through the same expressions
    assert family_task("span", n, hi, size=0.45)[0] == [tuple(map(float, t)) for t in
                                                        horizontal_bridge_setup(square_size=0.45, num_obstacles=n)["targets"]]
    assert family_task("tower", n, hi, size=0.7)[1][:n] == [tuple(map(float, o)) for o in bridge_setup(H=0.7, num_stories=n)["obstacles"]]
    # and RandomBridges.task states them once more, for the callers of the package
    from bridges_hip.vec_env import RandomBridges
    for kind in ("span", "tower"):
        assert RandomBridges(kind, sizes=(0, hi)).task(n) == family_task(kind, n, hi)
    assert draw_family("span", 0, 0, 0, 1, 4) == (2, *family_task("span", 2, 4))


@pytest.mark.parametrize("size", [64, 32])
@pytest.mark.parametrize("kind", ["span", "tower"])
def test_parked_slots_rasterise_to_nothing_on_the_oracle(kind, size):
    cube06 = get_shape("cube06")
    render = lambda pts: R.render_blocks_2d([Block(cube06, (p[0], p[2])) for p in pts], XLIM, YLIM, (size, size))
    for n in range(5):
        targets, obstacles = family_task(kind, n, 4)
        with_parked, live = render(obstacles), render(obstacles[:n])
        assert with_parked.shape == (size, size) and np.array_equal(with_parked, live), n
        assert bool(live.any()) == (n > 0), n
        assert render(targets).any(), n                       # the target lies inside the image


def test_task_family_struct_against_the_compiler():
    from bridges_hip import abi
    fields = ["family", "n_lo", "n_hi", "pad_", "size", "x", "task_class"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bridges_hip.h"\nint main(){printf("%zu %d %d %d %d %.1f", '
           'sizeof(bridges_task_family), BRIDGES_FAMILY_NONE, BRIDGES_FAMILY_SPAN, BRIDGES_FAMILY_TOWER, BRIDGES_MAX_OBSTACLES, '
           '(double)BRIDGES_PARK_Z);' + "".join(f'printf(" %zu", offsetof(bridges_task_family, {f}));' for f in fields)
           + 'printf("\\n");return 0;}\n')
    exe = os.path.join(ROOT, "tests", "_family_abi_sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        out = subprocess.check_output([exe]).decode().split()
    finally:
        os.remove(exe)
    T = abi.TaskFamily
    assert [f[0] for f in T._fields_] == fields
    assert int(out[0]) == ctypes.sizeof(T) == 40
    assert [int(v) for v in out[1:5]] == [abi.FAMILY_NONE, abi.FAMILY_SPAN, abi.FAMILY_TOWER, abi.MAX_OBSTACLES] == [0, 1, 2, 4]
    assert float(out[5]) == abi.PARK_Z == PARK_Z == -1000.0
    assert [int(v) for v in out[6:]] == [getattr(T, f).offset for f in fields] == [0, 4, 8, 12, 16, 24, 32]
    # the structs the feature must not grow are what they were
    assert ctypes.sizeof(abi.TaskBuffers) == 112 + 32 * abi.MAX_OBSTACLES and ctypes.sizeof(abi.Task) == 544
    for sym, n_args in (("bridges_env_set_task_family", 2), ("bridges_episode_stats_by_class", 13)):
        assert sym in abi.SIGNATURES and sym in abi.EXPORTED_SYMBOLS and len(abi.SIGNATURES[sym]) == n_args
    text = open(os.path.join(ROOT, "include", "bridges_hip.h")).read()
    assert "int bridges_env_set_task_family(bridges_env* env, const bridges_task_family* fam);" in text
    assert "0x66616D695F726E67" in text and "n  = n_lo + (int)(((r >> 32) * (uint64)(n_hi - n_lo + 1)) >> 32)" in text


def test_random_bridges_checks_its_arguments():
    from bridges_hip import abi
    from bridges_hip.vec_env import RandomBridges
    r = RandomBridges()
    assert (r.kind, r.lo, r.hi, r.size, r.x) == ("span", 1, 4, 0.6, 0.5) and r.family == abi.FAMILY_SPAN
    t = RandomBridges("tower", sizes=(0, 3))
    assert (t.size, t.x, t.num_obstacles, t.n_classes, t.family) == (0.8, 0.5, 3, 4, abi.FAMILY_TOWER)
    assert RandomBridges("span", sizes=(2, 2), size=0.45, x=1.0).size == 0.45
    for bad in (dict(kind="arch"), dict(sizes=(2, 1)), dict(sizes=(-1, 2)), dict(sizes=(0, 0)), dict(sizes=(1, abi.MAX_OBSTACLES + 1)),
                dict(sizes=(1.5, 3)), dict(sizes=(1,)), dict(size=0.0), dict(size=-0.6)):
        with pytest.raises(ValueError):
            RandomBridges(**bad)


BASE = ["--num_envs", "64", "--model", "SuccessorMLP"]


def _check(argv):
    from robotoddler.training.successor_dqn import build_parser, check_random_targets
    args = vars(build_parser().parse_args(argv))
    check_random_targets(args)
    return args


def test_cli_flags_parse_and_a_plain_parse_keeps_its_keys():
    from robotoddler.training.successor_dqn import build_parser
    plain = vars(build_parser().parse_args([]))
    assert sorted(plain) == ['aim', 'aim_repo', 'batch_size', 'bridge_length', 'checkpoint_every', 'device', 'evaluate_every',
                             'gamma', 'image_size', 'learning_rate', 'load_checkpoint', 'log_images', 'loss_function', 'max_steps',
                             'model', 'num_envs', 'num_episodes', 'num_training_steps', 'prioritized_replay',
                             'replay_buffer_capacity', 'save_checkpoint', 'seed', 'shapes', 'stable_actions_only', 'tau',
                             'tower_height', 'verbose', 'wandb']
    assert _check(BASE + ["--random_bridge_length", "1:4"])["random_bridge_length"] == (1, 4)
    assert _check(BASE + ["--random_tower_height", "0:3", "--shapes", "hexagon"])["random_tower_height"] == (0, 3)
    assert _check(BASE + ["--random_bridge_length", "2:2", "--shapes", "both"])["shapes"] == "both"
    for model in ("ConvNet", "UNet"):
        assert _check(["--num_envs", "64", "--model", model, "--task_channels", "--random_tower_height", "1:2"])["task_channels"]
    with pytest.raises(SystemExit):
        build_parser().parse_args(BASE + ["--random_bridge_length", "1-4"])


@pytest.mark.parametrize("argv,words", [
    (BASE + ["--random_bridge_length", "1:4", "--random_tower_height", "1:2"], "give one of them"),
    (BASE + ["--random_bridge_length", "1:4", "--random_targets", "2"], "--random_targets / --random_obstacles"),
    (BASE + ["--random_tower_height", "1:4", "--random_targets", "2", "--random_obstacles", "1"], "--random_targets / --random_obstacles"),
    (BASE + ["--random_bridge_length", "1:4", "--random_obstacles", "1"], "--random_targets / --random_obstacles"),
    (BASE + ["--random_bridge_length", "1:4", "--tower_height", "2"], "one fixed task"),
    (BASE + ["--random_tower_height", "1:4", "--bridge_length", "3"], "one fixed task"),
    (["--model", "SuccessorMLP", "--random_bridge_length", "1:4"], "--num_envs N, N > 1"),
    (["--num_envs", "1", "--model", "SuccessorMLP", "--random_tower_height", "1:4"], "--num_envs N, N > 1"),
    (BASE + ["--random_bridge_length", "1:4", "--image_size", "32x32"], "64x64"),
    (BASE + ["--random_bridge_length", "1:5"], "HI <= 4"),
    (BASE + ["--random_tower_height=-1:3"], "0 <= LO"),
    (BASE + ["--random_tower_height", "3:2"], "LO <= HI"),
    (BASE + ["--random_bridge_length", "0:0"], "1 <= HI"),
    (["--num_envs", "64", "--model", "ConvNet", "--random_bridge_length", "1:4"], "needs --task_channels"),
    (["--num_envs", "64", "--model", "UNet", "--random_tower_height", "1:4"], "needs --task_channels"),
    (BASE + ["--random_bridge_length", "1:4", "--task_channels"], "--task_channels is for the conv Q-networks"),
])
def test_cli_refusals_in_words(argv, words):
    with pytest.raises(SystemExit) as err:
        _check(argv)
    assert words in str(err.value), str(err.value)


def test_refusals_without_the_new_flags_keep_their_wording():
    for argv, words in ((BASE + ["--task_channels"], "--task_channels is valid only together with --random_targets T"),
                        (BASE + ["--random_obstacles", "2"], "--random_obstacles O is valid only together with --random_targets T"),
                        (BASE + ["--random_targets", "2", "--tower_height", "2"], "it cannot be combined with --tower_height or --bridge_length"),
                        (BASE + ["--random_targets", "2", "--shapes", "hexagon"], "--random_targets is tower_setup: --shapes trapezoid")):
        with pytest.raises(SystemExit) as err:
            _check(argv)
        assert words in str(err.value)


def test_log_values_gain_the_per_class_keys_for_family_runs_only():
    from robotoddler.training.vec_dqn import EPISODE_KEYS, lockstep_log_values
    info = dict(mean_reward=-0.5, mean_lin_reward=0.125, avg_loss=0.5, lockstep_env_steps=300, epsilon=0.4, env_steps=900,
                steps_per_s=1e5, **{k: None for k in EPISODE_KEYS})
    plain = lockstep_log_values(info)
    assert not any(k.startswith("success_rate_n") for k in plain)
    fam = lockstep_log_values(dict(info, success_by_class=[None, 0.5, None, 0.25], class_lo=1))
    assert list(fam)[:len(plain)] == list(plain)
    assert {k: fam[k] for k in list(fam)[len(plain):]} == dict(success_rate_n1=0.5, success_rate_n2=None, success_rate_n3=0.25)


def _synthetic(E, K, n_calls, seed, n_targets, n_classes):
    from test_gpu_episode_stats import _synthetic_calls
    rng = np.random.default_rng(seed + 1000)
    return [(rec, valid, rng.integers(0, n_classes, E).astype(np.int32)) for rec, valid in _synthetic_calls(E, K, n_calls, seed, n_targets)]


def test_by_class_restatement_against_the_one_class_restatement():
    from test_gpu_episode_stats import Restated
    E, K, gamma, n_targets = 70, 6, 0.95, 1
    for first_only in (False, True):
        calls = _synthetic(E, K, 30, 11, n_targets, 4)
        one, ref = RestatedByClass(E, K, gamma, n_targets, 1, first_only), Restated(E, K, gamma, n_targets, first_only)
        by = RestatedByClass(E, K, gamma, n_targets, 4, first_only)
        for rec, valid, cls in calls:
            one.fold(rec, valid, np.zeros(E, dtype=np.int32))
            ref.fold(rec, valid)
            by.fold(rec, valid, cls)
        assert one.episodes[0] == ref.episodes and len(ref.episodes) > 20
        assert np.array_equal(one.run, ref.run) and np.array_equal(one.counted, ref.counted)
        ref.check(one.sums()[0])
        one.check(one.sums())
        # the classes partition the episodes; run and counted do not depend on the classes
        assert sorted(ep for c in by.episodes for ep in c) == sorted(ref.episodes) and all(by.episodes)
        assert np.array_equal(by.run, ref.run) and np.array_equal(by.counted, ref.counted)
        # a class out of range is filed nowhere and still advances the env
        out = RestatedByClass(E, K, gamma, n_targets, 2, first_only)
        for rec, valid, cls in calls:
            out.fold(rec, valid, cls - 1)                         # classes -1 .. 2 against 2 rows
        assert out.episodes[0] == by.episodes[1] and out.episodes[1] == by.episodes[2]
        assert np.array_equal(out.counted, ref.counted)


def test_deferred_stats_report_by_class_only_when_asked():
    from robotoddler.training.episode_stats import DeferredStats

    class _Done:
        def synchronize(self):
            pass
    import torch
    plain = DeferredStats(torch.tensor([2., 1., .5, 6., 2., 1., 0., 0.], dtype=torch.float64), _Done()).get()
    assert list(plain) == ["episodes", "reward", "lin_reward", "num_steps", "stable", "success_rate"] and plain["success_rate"] == 0.5
    rows = torch.tensor([[2., 1., .5, 6., 2., 1., 0., 0.], [0.] * 8, [2., 1., .5, 6., 2., 1., 0., 0.]], dtype=torch.float64)
    by = DeferredStats(rows, _Done(), n_classes=2).get()
    assert list(by) == list(plain) + ["by_class"] and {k: by[k] for k in plain} == plain
    assert by["by_class"][0]["episodes"] == 0 and by["by_class"][0]["success_rate"] is None and by["by_class"][1] == plain
