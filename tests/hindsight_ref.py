"""Reference of the hindsight goal relabelling of the vectorised DQN loop (VecDQN(hindsight="final"), bridges_hindsight_relabel,
the rule in include/bridges_hip.h): the counter-based choice of goal blocks, the bounding-box centres that become targets and the
walk that rewrites reward, linear reward and done of every record.  Test infrastructure, not a test module: nothing here needs a
GPU.  Geometry, rasters and reward maps are the oracle's (oracle/geometry.py, oracle/raster.py); tests/test_cpu_hindsight.py
checks the statement against the oracle env, tests/test_gpu_hindsight.py compares the kernels with it bit for bit.

Two task models share the walk:
  OracleTask   the oracle env's own features: R.convolve_with_gaussian and the float64 sum of the map under the raster, rounded
               to float32 (OracleGym.candidates) -- what an OracleGym built on the hindsight targets computes;
  DeviceTask   the device's arithmetic: the host's set-pixel-by-set-pixel map (bridges_hip.vec_env.gaussian_reward_map, which
               the per-env task features restate operation for operation), float64 row prefix sums left to right, per row
               prefix[hi] - prefix[lo] of the run, the 64 parts added in the pair tree of the wave reduction, one rounding
               (tests/geometry_conformance.py lin_np).
"""
import functools

import numpy as np

from oracle import raster as OR
from oracle.env import M64, XLIM, YLIM, splitmix64
from oracle.geometry import Block
from oracle.shapes import get_shape
from robotoddler.training import records as R

HIND_SALT = 0x68696E645F726E67      # "hind_rng"
F_VALID, F_STABLE_FROZEN, F_STABLE_UNFROZEN, F_TERMINATED, F_TRUNCATED, F_DONE, F_NO_ACTIONS, F_LP_ERROR = range(8)


# ---------------------------------------------------------------------------------------------------------------------------
# the draw

def hind_draw(seed, env_id, episode, slot, i):
    """Uniform u64 for (seed, global env id, task_episode of the episode, relabelling slot, draw index)."""
    h0 = splitmix64(((((seed & 0xFFFFFFFF) << 32) | (env_id & 0xFFFFFFFF)) ^ HIND_SALT) & M64)
    h1 = splitmix64(h0 ^ (episode & 0xFFFFFFFF))
    h2 = splitmix64(h1 ^ (slot & M64))
    return splitmix64(h2 ^ (i & M64))


def choose_blocks(seed, env_id, episode, slot, n_eligible, n_targets):
    """Partial Fisher-Yates over the eligible block indices, integers only: the block of every target (t mod m' beyond m')."""
    mp, T = int(n_eligible), int(n_targets)
    assert mp >= 1
    idx = list(range(mp))
    for i in range(min(T, mp)):
        u = hind_draw(seed, env_id, episode, slot, i) >> 32
        j = i + ((u * (mp - i)) >> 32)
        idx[i], idx[j] = idx[j], idx[i]
    return [idx[t % mp] for t in range(T)]


# ---------------------------------------------------------------------------------------------------------------------------
# geometry of a record

def block_of(row, shapes):
    """The block a record placed, posed from its recorded shape id and pose: oracle Block (pos + R(c, s) * local vertex)."""
    sh = int(row[R.O_ASHAPE])
    px, pz, c, s = (float(v) for v in row[R.O_APOSE:R.O_APOSE + 4])
    return Block(shapes[sh], (px, pz), (c, s))


def box_centre(block):
    x0, z0, x1, z1 = block.aabb
    return ((x0 + x1) * 0.5, 0.0, (z0 + z1) * 0.5)


def eligible(rows):
    """m': every block of the episode, but the last when its step was not frozen-stable."""
    m = len(rows)
    return m - 1 if (m and not rows[m - 1][R.O_STABLE_N] > 0.5) else m


def goals(rows, shapes, seed, env_id, episode, slot, n_targets):
    """-> (targets [(x, 0, z)] * T, chosen block indices), or (None, None) when no block is eligible."""
    mp = eligible(rows)
    if mp <= 0:
        return None, None
    picks = choose_blocks(seed, env_id, episode, slot, mp, n_targets)
    return [box_centre(block_of(rows[b], shapes)) for b in picks], picks


def reach(left, targets, block):
    """k_step's reached-test on the mask of open targets: the open target after a reached one is skipped for this block."""
    skip = False
    for t, tg in enumerate(targets):
        if not (left >> t) & 1:
            continue
        if skip:
            skip = False
            continue
        if block.aabb_contains(tg):
            left &= ~(1 << t)
            skip = True
    return left


# ---------------------------------------------------------------------------------------------------------------------------
# tasks: the reward map of a set of targets and the linear reward of a block under it

class OracleTask:
    def __init__(self, targets, xlim=XLIM, ylim=YLIM, img_size=(64, 64)):
        cube = get_shape("cube06")
        self.X, self.Y = OR.pixel_grid(xlim, ylim, img_size)
        tr = OR.render_blocks_2d([Block(cube, (t[0], t[2])) for t in targets], xlim, ylim, img_size)
        self.reward_map = OR.convolve_with_gaussian(tr.astype(np.float32), 101, 16)

    def base(self, block):
        raster = OR.contains_2d(block, self.X, self.Y)
        return np.float32(self.reward_map[raster].astype(np.float64).sum())


class DeviceTask:
    def __init__(self, targets, xlim=XLIM, ylim=YLIM, img_size=(64, 64)):
        from bridges_hip.vec_env import gaussian_reward_map
        cube = get_shape("cube06")
        assert tuple(img_size) == (64, 64)
        self.X, self.Y = OR.pixel_grid(xlim, ylim, img_size)
        tr = OR.render_blocks_2d([Block(cube, (t[0], t[2])) for t in targets], xlim, ylim, img_size)
        self.reward_map = gaussian_reward_map(tr.astype(np.float32))
        self.prefix = np.zeros((64, 65), dtype=np.float64)
        self.prefix[:, 1:] = np.cumsum(self.reward_map.astype(np.float64), axis=1)

    def base(self, block):
        raster = OR.contains_2d(block, self.X, self.Y)
        parts = np.zeros(64)
        for r in range(64):
            cols = np.flatnonzero(raster[r])
            if len(cols):
                parts[r] = self.prefix[r, cols[-1] + 1] - self.prefix[r, cols[0]]
        while len(parts) > 1:
            parts = parts[0::2] + parts[1::2]
        return np.float32(parts[0])


def lin_rule(base, st_free, st_frozen):
    """successor_dqn.py:397-401 in float32, as k_step states it."""
    base = np.float32(base)
    return base if st_free else (base / np.float32(100) if st_frozen else np.float32(0))


# ---------------------------------------------------------------------------------------------------------------------------
# the walk

def relabel_episode(rows, flags, shapes, seed, env_id, episode, slot, n_targets, task_cls=DeviceTask, trace=None):
    """rows [m, W] float64 (records with their task tail), flags [m, 8] uint8 of one finished episode -> the relabelled rows
    [n <= m, W].  ``trace``: a list that receives (targets, picks, [left after every emitted step])."""
    rows = np.asarray(rows, dtype=np.float64)
    T = int(n_targets)
    targets, picks = goals(rows, shapes, seed, env_id, episode, slot, T)
    if targets is None:
        return np.zeros((0, rows.shape[1]))
    task = task_cls(targets)
    left, out, lefts = (1 << T) - 1, [], []
    for t in range(len(rows)):
        block = block_of(rows[t], shapes)
        left = reach(left, targets, block)
        st_frozen, st_free = bool(flags[t][F_STABLE_FROZEN]), bool(flags[t][F_STABLE_UNFROZEN])
        truncated, no_actions = bool(flags[t][F_TRUNCATED]), bool(flags[t][F_NO_ACTIONS])
        n_reached, all_reached = T - bin(left).count("1"), left == 0
        row = rows[t].copy()
        row[R.O_REWARD] = -1.0 if not st_frozen else float(n_reached if all_reached else -1 + n_reached)
        row[R.O_LIN] = float(lin_rule(task.base(block), st_free, st_frozen))
        row[R.O_DONE] = 1.0 if (not st_frozen or all_reached or truncated or no_actions) else 0.0
        row[R.RECORD_WIDTH:R.RECORD_WIDTH + 3 * T] = np.asarray(targets, dtype=np.float64).reshape(-1)
        out.append(row)
        lefts.append(left)
        if all_reached:
            break
    if trace is not None:
        trace.append((targets, picks, lefts))
    return np.stack(out)


def relabel(buf, flags, length, ended, episode, shapes, seed, env_id_base, n_goals, n_targets, task_cls=DeviceTask, trace=None):
    """The operator: buf [E, K, W], flags [E, K, 8], length [E], ended [E], episode [E] -> rows [count, W], env ascending, then
    slot, then step.  ``trace``: a list that receives (env, slot, targets, picks, lefts) of every (env, slot) with rows."""
    buf = np.asarray(buf, dtype=np.float64)
    out = [np.zeros((0, buf.shape[2]))]
    for e in range(buf.shape[0]):
        m = int(length[e])
        if not ended[e] or m <= 0:
            continue
        for g in range(int(n_goals)):
            tr = []
            rows = relabel_episode(buf[e, :m], np.asarray(flags)[e, :m], shapes, seed, env_id_base + e, int(episode[e]), g, n_targets,
                                   task_cls=task_cls, trace=tr)
            out.append(rows)
            if trace is not None and tr:
                trace.append((e, g) + tr[0])
    return np.concatenate(out, axis=0)


# ---------------------------------------------------------------------------------------------------------------------------
# scripted probe episodes: the operator reads records, not physics, so the probe writes poses and flags directly

# (E, T, G, O, shape) of the operator's GPU test: 130 envs are more than one chunk of the scan and no multiple of 64
PROBE_SEED, PROBE_BASE = 7, 1000                # seed and env_id_base of the draw
PROBE_CONFIGS = ((1, 1, 1, 0, "trapezoid"), (5, 3, 4, 2, "hexagon"), (64, 3, 4, 0, "trapezoid"), (64, 1, 4, 2, "trapezoid"),
                 (130, 1, 1, 2, "hexagon"), (130, 3, 1, 0, "hexagon"))


def probe_seed(E):
    return 100 + E


KINDS = ("one_step", "collapse", "empty", "few", "full", "mid", "cluster", "random")
CASES = ("one_step", "collapse", "empty", "few", "early", "quirk", "full", "mid")


def probe(E, T, O, shape, seed, K=16):
    """-> dict(shapes, buf [E, K, W], flags [E, K, 8], length, ended, episode): env e plays KINDS[e % 8] --
    one_step  one stable block;                       collapse  2..6 blocks, the last one falls (not frozen-stable);
    empty     one block that falls (m' == 0);         few       two stable blocks (m' = 2 < T = 3);
    full      K blocks, truncated at the last;        mid       three blocks, the episode still runs (ended = 0);
    cluster   six blocks within 0.2 of each other: every goal lies in every block, so the walk ends early and the skipped
              target stays open for a step;           random    1..K blocks anywhere on the canvas.
    Every column the operator does not rewrite holds noise: a copied column must come out as it went in."""
    rng = np.random.default_rng(seed)
    shapes = [get_shape(shape), get_shape("cube06")]                 # the env's table: the task's shapes, then cube06
    W = R.RECORD_WIDTH + 3 * T + 3 * O
    buf = rng.normal(size=(E, K, W))
    flags = np.zeros((E, K, 8), dtype=np.uint8)
    length, ended = np.zeros(E, dtype=np.int32), np.ones(E, dtype=bool)
    episode = rng.integers(0, 1 << 20, size=E).astype(np.int32)
    for e in range(E):
        kind = KINDS[e % len(KINDS)]
        m = dict(one_step=1, collapse=int(rng.integers(2, 7)), empty=1, few=2, full=K, mid=3, cluster=6)\
            .get(kind, int(rng.integers(1, K + 1)))
        length[e] = m
        ended[e] = kind != "mid"
        centre = (rng.uniform(-1.0, 5.0), rng.uniform(0.5, 5.0))
        for t in range(m):
            last = t == m - 1
            frozen = not (last and kind in ("collapse", "empty")) and not (last and kind == "random" and rng.random() < 0.3)
            free = frozen and rng.random() < 0.7
            if kind == "cluster":
                x, z = centre[0] + rng.uniform(-0.1, 0.1), centre[1] + rng.uniform(-0.1, 0.1)
            else:
                x, z = rng.uniform(-2.5, 6.5), rng.uniform(0.2, 7.0)
            ang = rng.uniform(-np.pi, np.pi) if kind != "cluster" else 0.0
            row = buf[e, t]
            row[R.O_NB], row[R.O_ASHAPE] = t, 0
            row[R.O_APOSE:R.O_APOSE + 4] = (x, z, np.cos(ang), np.sin(ang))
            row[R.O_STABLE_N] = float(frozen)
            truncated = last and m == K
            no_actions = last and frozen and not truncated and kind == "random" and rng.random() < 0.3
            done = ended[e] and last
            row[R.O_DONE] = float(done)
            row[R.O_REWARD] = -1.0 if not frozen else float(rng.integers(-1, T))
            row[R.O_LIN] = float(np.float32(rng.uniform(0, 2)))
            flags[e, t] = (1, frozen, free, not frozen, truncated, (not frozen) or truncated, no_actions, 0)
    return dict(shapes=shapes, buf=buf, flags=flags, length=length, ended=ended, episode=episode, T=T, O=O, K=K)


def census(p, seed, env_id_base, G):
    """Which CASES the probe p holds under (seed, env_id_base, G slots), by the restatement itself (no tasks are built)."""
    seen = set()
    for e in range(len(p["length"])):
        m = int(p["length"][e])
        rows = p["buf"][e, :m]
        if not p["ended"][e]:
            seen |= {"mid"} if m else set()
            continue
        mp = eligible(rows)
        seen |= {"empty"} if mp == 0 else set()
        seen |= {"collapse"} if 0 < mp < m else set()
        seen |= {"few"} if 0 < mp < p["T"] else set()
        seen |= {"full"} if m == p["K"] else set()
        seen |= {"one_step"} if m == 1 and mp == 1 else set()
        for g in range(G if mp else 0):
            targets, _ = goals(rows, p["shapes"], seed, env_id_base + e, int(p["episode"][e]), g, p["T"])
            left = (1 << p["T"]) - 1
            for t in range(m):
                block = block_of(rows[t], p["shapes"])
                after = reach(left, targets, block)
                inside = sum(1 << k for k in range(p["T"]) if (left >> k) & 1 and block.aabb_contains(targets[k]))
                seen |= {"quirk"} if after & inside else set()
                left = after
                if left == 0:
                    seen |= {"early"} if t < m - 1 else set()
                    break
    return seen


@functools.lru_cache(maxsize=4096)
def _device_task(targets):
    return DeviceTask(targets)


def cached_device_task(targets):
    """DeviceTask(targets), built once per set of targets (a loop test meets every episode's task in each of its rows)."""
    return _device_task(tuple(tuple(float(v) for v in t) for t in targets))
