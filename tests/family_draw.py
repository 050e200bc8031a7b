"""Python restatement of the device's task-family draw (include/bridges_hip.h, bridges_env_set_task_family), built on the
oracle's splitmix64: ONE integer n per (seed, global env id, episode), and the target and obstacles that n names -- the numbers of
the reference's horizontal_bridge_setup / bridge_setup, with the unused obstacle slots parked.  Test infrastructure: the tests
compare the device's env_targets, env_obstacles and task_class with these numbers exactly."""
from oracle.env import M64, splitmix64

FAMI_SALT = 0x66616D695F726E67      # "fami_rng"
PARK_Z = -1000.0                    # BRIDGES_PARK_Z
DEFAULT_SIZE = dict(span=0.6, tower=0.8)


def family_word(seed, env_id, episode):
    """Uniform u64 for (seed, global env id, episode)."""
    h0 = splitmix64(((((seed & 0xFFFFFFFF) << 32) | (env_id & 0xFFFFFFFF)) ^ FAMI_SALT) & M64)
    h1 = splitmix64(h0 ^ (episode & M64))
    return splitmix64(h1)


def family_draw(seed, env_id, episode, lo, hi):
    """n in [lo, hi]: the high 32 bits of the word scaled to the hi - lo + 1 classes, in integer arithmetic only."""
    return lo + (((family_word(seed, env_id, episode) >> 32) * (hi - lo + 1)) >> 32)


def family_task(kind, n, hi, size=None, x=0.5):
    """-> (targets [1 x (x, y, z)], obstacles [hi x (x, y, z)]) of class n: slots o < n live, slots o >= n parked."""
    s = DEFAULT_SIZE[kind] if size is None else size
    if kind == "span":
        target = (n * s + 2.5 * s, 0.0, s / 2)
        live = [((o + 1) * s, 0.0, s / 2) for o in range(n)]
    else:
        target = (x, 0.0, n * s + s / 2)
        live = [(x, 0.0, o * s + s / 2) for o in range(n)]
    return [target], live + [(0.0, 0.0, PARK_Z)] * (hi - n)


def draw_family(kind, seed, env_id, episode, lo, hi, size=None, x=0.5):
    """(n, targets, obstacles) env `env_id` holds in its episode number `episode` (0 = the episode that follows a reset of the
    whole env)."""
    n = family_draw(seed, env_id, episode, lo, hi)
    return (n, *family_task(kind, n, hi, size, x))
