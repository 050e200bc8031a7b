"""CPU: the host side of the per-env tasks -- the restated target draw, the ctypes mirror of bridges_task_buffers and the
export list."""
import ctypes
import os
import re
import subprocess

import pytest

from oracle.env import policy_draw
from task_draw import draw_targets, task_draw, task_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draw_is_deterministic_and_in_range():
    for seed in (0, 3, 2 ** 31 + 5):
        for env in (0, 1, 4095, 70000):
            for ep in (0, 1, 977):
                t = draw_targets(seed, env, ep)
                assert t == draw_targets(seed, env, ep) and len(t) == 3
                for x, y, z in t:
                    assert -4.0 <= x < 4.0 and y == 0.0 and 0.0 <= z < 4.0
    # other ranges, other target counts
    t = draw_targets(1, 2, 3, num_targets=8, x_range=(1.0, 1.5), z_range=(2.0, 2.0))
    assert len(t) == 8 and all(1.0 <= x < 1.5 and z == 2.0 for x, _, z in t)
    # the distribution: 4000 draws of U[-4, 4) fill all eight unit bins about evenly and average near 0
    xs = [task_uniform(7, e, 0, 0, 0, -4.0, 4.0) for e in range(4000)]
    bins = [sum(1 for x in xs if lo <= x < lo + 1) for lo in range(-4, 4)]
    assert min(bins) > 400 and max(bins) < 600 and abs(sum(xs) / len(xs)) < 0.15


def test_draw_depends_on_every_key_and_is_not_the_policy_stream():
    base = (5, 17, 3, 1, 0)
    r0 = task_draw(*base)
    for i, other in enumerate([6, 18, 4, 2, 2]):
        key = list(base)
        key[i] = other
        assert task_draw(*key) != r0, i
    seen = {task_draw(5, e, k, t, a) for e in range(16) for k in range(16) for t in range(3) for a in (0, 2)}
    assert len(seen) == 16 * 16 * 3 * 2
    # the synthetic policy draws from (seed, env, counter): same seed / env, counter = episode must not coincide
    for e in range(8):
        for k in range(8):
            assert policy_draw(5, e, k) not in {task_draw(5, e, k, t, a) for t in range(8) for a in range(3)}
    # seed and env id are 32-bit fields of one key word
    assert task_draw(1, 0, 0, 0, 0) != task_draw(0, 1, 0, 0, 0)


def test_task_buffer_struct_size_matches_the_header():
    """ctypes mirror of bridges_task_buffers vs the C compiler's view of the header (as test_struct_sizes_match_the_header)."""
    from bridges_hip import abi
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bridges_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", '
           'sizeof(bridges_task_buffers), offsetof(bridges_task_buffers, gauss_k), offsetof(bridges_task_buffers, sample), '
           'offsetof(bridges_task_buffers, x_range), offsetof(bridges_task_buffers, z_range), BRIDGES_GAUSS_TAPS);return 0;}\n')
    exe = os.path.join(ROOT, "tests", "_task_abi_sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    try:
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    T = abi.TaskBuffers
    assert out == [ctypes.sizeof(T), T.gauss_k.offset, T.sample.offset, T.x_range.offset, T.z_range.offset, abi.GAUSS_TAPS]
    # the device buffers lead the struct, in the order of TASK_BUFFER_FIELDS
    assert [f[0] for f in T._fields_][:len(abi.TASK_BUFFER_FIELDS)] == [f[0] for f in abi.TASK_BUFFER_FIELDS]
    # the structs a caller without per-env tasks fills are what they were
    assert ctypes.sizeof(abi.Task) == 544 and ctypes.sizeof(abi.EnvBuffers) == 8 * len(abi.EnvBuffers._fields_)


def test_every_symbol_the_header_declares_is_exported():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"^(?:const char\*|int)\s+(bridges_\w+)\s*\(", text, flags=re.M))
    assert {"bridges_env_set_task_buffers", "bridges_env_load_targets", "bridges_env_step"} <= declared
    assert declared == set(abi.EXPORTED_SYMBOLS)
    assert abi.SIGNATURES["bridges_env_set_task_buffers"][1]._type_ is abi.TaskBuffers


def test_random_targets_checks_its_arguments():
    from bridges_hip.vec_env import RandomTargets
    r = RandomTargets()
    assert (r.num_targets, r.x_range, r.z_range) == (3, (-4.0, 4.0), (0.0, 4.0))      # tower_setup, gym_env.py:64-79
    for bad in (dict(num_targets=0), dict(num_targets=9), dict(x_range=(1.0, 0.0)), dict(z_range=(2.0, 1.0))):
        with pytest.raises(ValueError):
            RandomTargets(**bad)
