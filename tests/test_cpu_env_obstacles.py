"""CPU: the host side of the per-env obstacles -- the restated obstacle draw, the ctypes mirror of the grown
bridges_task_buffers, RandomObstacles' argument checks and VecDQN's refusal."""
import ctypes
import os
import subprocess

import pytest

from obstacle_draw import OBST_SALT, draw_obstacles, obstacle_draw, obstacle_uniform
from task_draw import task_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draw_against_hand_computed_values():
    """(seed, env, episode, obstacle, axis) = (5, 17, 3, 1, 2) on z ~ U[0.3, 2.5), every intermediate word worked out with a
    separate C program on uint64_t / double (no fused multiply-add): the key word, the three splitmix64 rounds, the 53 bits."""
    assert OBST_SALT == int.from_bytes(b"obst_rng", "big")
    key = ((5 << 32) | 17) ^ OBST_SALT
    assert key == 0x6F6273715F726E76
    r = obstacle_draw(5, 17, 3, 1, 2)
    assert r == 0x3956B393DDF94A1F
    assert r >> 11 == 2017425369055017
    v = obstacle_uniform(5, 17, 3, 1, 2, 0.3, 2.5)
    assert v == float.fromhex("0x1.95e3e2f103e28p-1") and repr(v) == "0.7927542609413125"
    assert draw_obstacles(5, 17, 3, [((0.0, 1.0), (0.0, 1.0)), ((-3.0, 3.0), (0.3, 2.5))])[1][2] == v


def test_draw_is_in_range_per_obstacle_and_a_stream_of_its_own():
    ranges = [((-3.0, 3.0), (0.3, 2.5)), ((1.0, 1.5), (2.0, 2.0)), ((-1.0, 0.0), (0.0, 4.0)), ((6.0, 7.0), (5.0, 9.0))]
    for seed in (0, 3, 2 ** 31 + 5):
        for env in (0, 1, 4095, 70000):
            for ep in (0, 1, 977):
                obs = draw_obstacles(seed, env, ep, ranges)
                assert obs == draw_obstacles(seed, env, ep, ranges) and len(obs) == 4
                for (x, y, z), ((x0, x1), (z0, z1)) in zip(obs, ranges):
                    assert (x0 <= x < x1) and y == 0.0 and (z0 <= z < z1 or z0 == z1 == z)
    base = (5, 17, 3, 1, 0)
    r0 = obstacle_draw(*base)
    for i, other in enumerate([6, 18, 4, 2, 2]):
        key = list(base)
        key[i] = other
        assert obstacle_draw(*key) != r0, i
    # targets and obstacles of an episode come from different streams: same key, other numbers
    for e in range(8):
        for k in range(8):
            assert not ({obstacle_draw(5, e, k, o, a) for o in range(4) for a in (0, 2)}
                        & {task_draw(5, e, k, t, a) for t in range(8) for a in (0, 2)})
    xs = [obstacle_uniform(7, e, 0, 0, 0, -3.0, 3.0) for e in range(3000)]
    bins = [sum(1 for x in xs if lo <= x < lo + 1) for lo in range(-3, 3)]
    assert min(bins) > 400 and max(bins) < 600


def test_task_buffer_struct_keeps_its_offsets_and_grows_at_the_end():
    """ctypes mirror of bridges_task_buffers vs the C compiler's view of the header: the fields of the struct before per-env
    obstacles sit where they sat (offsets written down from that header: nine 8-byte words, then two ranges), the new ones
    follow z_range in the order the header declares them."""
    from bridges_hip import abi
    old = ["env_targets", "target_bits", "reward_map", "reward_prefix", "task_episode", "env_obstacle_bits", "gauss_k",
           "target_shape", "sample", "x_range", "z_range"]
    new = ["env_obstacles", "n_obstacles", "sample_obstacles", "obs_x_range", "obs_z_range"]
    fields = old + new
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bridges_hip.h"\nint main(){printf("%zu %d", sizeof(bridges_task_buffers), '
           'BRIDGES_MAX_OBSTACLES);' + "".join(f'printf(" %zu", offsetof(bridges_task_buffers, {f}));' for f in fields)
           + 'printf("\\n");return 0;}\n')
    exe = os.path.join(ROOT, "tests", "_obstacle_abi_sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    T = abi.TaskBuffers
    assert [f[0] for f in T._fields_] == fields
    assert out[:2] == [ctypes.sizeof(T), abi.MAX_OBSTACLES] and abi.MAX_OBSTACLES == 4
    assert out[2:] == [getattr(T, f).offset for f in fields]
    assert out[2:2 + len(old)] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 80]          # the struct as it was: 96 bytes
    assert out[2 + len(old):] == [96, 104, 108, 112, 112 + 16 * abi.MAX_OBSTACLES] and out[0] == 112 + 32 * abi.MAX_OBSTACLES
    assert T.obs_x_range.size == T.obs_z_range.size == 16 * abi.MAX_OBSTACLES
    # the structs a caller without per-env tasks fills are what they were
    assert ctypes.sizeof(abi.Task) == 544 and ctypes.sizeof(abi.EnvBuffers) == 8 * len(abi.EnvBuffers._fields_)
    assert [f[0] for f in abi.OBSTACLE_BUFFER_FIELDS] == ["env_obstacles", "env_obstacle_bits"]


def test_random_obstacles_checks_its_arguments():
    from bridges_hip import abi
    from bridges_hip.vec_env import RandomObstacles
    r = RandomObstacles(ranges=[((-3, 3), (0.3, 2.5)), ((1.0, 1.0), (2.0, 2.0))])       # a degenerate range is a point, not empty
    assert r.num_obstacles == 2 and r.ranges[0] == ((-3.0, 3.0), (0.3, 2.5)) and r.ranges[1] == ((1.0, 1.0), (2.0, 2.0))
    assert RandomObstacles([((0, 1), (0, 1))] * abi.MAX_OBSTACLES).num_obstacles == abi.MAX_OBSTACLES
    for bad in ([], [((0, 1), (0, 1))] * (abi.MAX_OBSTACLES + 1), [((1.0, 0.0), (0.0, 1.0))], [((0.0, 1.0), (2.0, 1.0))],
                [((0.0, 1.0), (0.0, 1.0)), ((0.0, 1.0), (3.0, 2.0))]):
        with pytest.raises(ValueError):
            RandomObstacles(bad)


class _FakeEnv:
    """What VecDQN.__init__ looks at before it refuses."""

    def __init__(self, per_env_tasks):
        self.per_env_obstacles, self.per_env_tasks = True, per_env_tasks


@pytest.mark.parametrize("per_env_tasks", [False, True])
def test_vec_dqn_refuses_per_env_obstacles(per_env_tasks):
    from robotoddler.training.vec_dqn import VecDQN
    for flag in (False, True):
        with pytest.raises(ValueError, match="per-env obstacles"):
            VecDQN(None, None, None, _FakeEnv(per_env_tasks), 64, 8, 0.9, 0.05, "mse_q_values", per_env_tasks=flag)
