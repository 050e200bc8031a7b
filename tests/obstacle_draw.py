"""Python restatement of the device's per-env obstacle draw (include/bridges_hip.h, bridges_env_set_task_buffers), built on the
oracle's splitmix64.  Test infrastructure: the tests compare the device's env_obstacles with these numbers exactly."""
from oracle.env import M64, splitmix64

OBST_SALT = 0x6F6273745F726E67      # "obst_rng"


def obstacle_draw(seed, env_id, episode, obstacle, axis):
    """Uniform u64 for (seed, global env id, episode, obstacle, axis)."""
    h0 = splitmix64(((((seed & 0xFFFFFFFF) << 32) | (env_id & 0xFFFFFFFF)) ^ OBST_SALT) & M64)
    h1 = splitmix64(h0 ^ (episode & M64))
    return splitmix64(h1 ^ (3 * obstacle + axis))


def obstacle_uniform(seed, env_id, episode, obstacle, axis, lo, hi):
    u = float(obstacle_draw(seed, env_id, episode, obstacle, axis) >> 11) * 2.0 ** -53      # exact: 53 bits
    span = hi - lo
    step = span * u
    return lo + step


def draw_obstacles(seed, env_id, episode, ranges):
    """The obstacles env `env_id` holds in its episode number `episode` (0 = the episode that follows a reset of the whole env);
    ranges: one ((x0, x1), (z0, z1)) per obstacle."""
    return [(obstacle_uniform(seed, env_id, episode, o, 0, *xr), 0.0, obstacle_uniform(seed, env_id, episode, o, 2, *zr))
            for o, (xr, zr) in enumerate(ranges)]
