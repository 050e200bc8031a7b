"""Python restatement of the device's per-env target draw (include/bridges_hip.h, bridges_env_set_task_buffers), built on the
oracle's splitmix64.  Test infrastructure: the tests compare the device's env_targets with these numbers exactly."""
from oracle.env import M64, splitmix64

TASK_SALT = 0x7461736B5F726E67      # "task_rng"


def task_draw(seed, env_id, episode, target, axis):
    """Uniform u64 for (seed, global env id, episode, target, axis)."""
    h0 = splitmix64(((((seed & 0xFFFFFFFF) << 32) | (env_id & 0xFFFFFFFF)) ^ TASK_SALT) & M64)
    h1 = splitmix64(h0 ^ (episode & M64))
    return splitmix64(h1 ^ (3 * target + axis))


def task_uniform(seed, env_id, episode, target, axis, lo, hi):
    u = float(task_draw(seed, env_id, episode, target, axis) >> 11) * 2.0 ** -53      # exact: 53 bits
    span = hi - lo
    step = span * u
    return lo + step


def draw_targets(seed, env_id, episode, num_targets=3, x_range=(-4.0, 4.0), z_range=(0.0, 4.0)):
    """The targets env `env_id` holds in its episode number `episode` (0 = the episode that follows a reset of the whole env)."""
    return [(task_uniform(seed, env_id, episode, t, 0, *x_range), 0.0, task_uniform(seed, env_id, episode, t, 2, *z_range))
            for t in range(num_targets)]
