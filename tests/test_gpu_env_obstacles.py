"""GPU: per-env obstacles of the lock-step env -- every env owns its obstacles (an [E, O, 3] array / set_obstacles) or redraws
them on the device whenever it starts an episode (RandomObstacles, the reference's connecting_setup per env.reset(**setup_fct())).
Bit-exact: obstacles and episode counters against the restated draw, obstacle rasters against render_blocks_2d, candidate
masks / counts / flags / rewards / states against one oracle per env built on that env's own obstacle list; 1e-5: linear
rewards against the numpy oracle (the tolerance of tests/test_gpu_env_parity.py -- they do not depend on obstacles, and are
compared exactly with a device env that has none)."""
import ctypes as C

import numpy as np
import pytest
import torch

from obstacle_draw import draw_obstacles
from oracle import raster as R
from oracle.env import OracleGym, OracleLockstep, policy_draw
from oracle.geometry import Block
from oracle.shapes import get_shape
from task_draw import draw_targets
from test_gpu_env_parity import canvas_equals, run_lockstep_parity
from test_gpu_env_tasks import snapshots_equal

pytestmark = pytest.mark.gpu

RANGES = [((-3.0, 3.0), (0.3, 2.5))] * 2          # two obstacles, both x in [-3, 3), z in [0.3, 2.5)
TARGETS = [(0.5, 0.0, 1.2)]                       # the shared target list of the envs that only differ in obstacles
MAX_STEPS = 6


def make_vec(E, obstacles, targets=TARGETS, shape="trapezoid", max_steps=MAX_STEPS, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    kw.setdefault("f32_rasters", False)
    return VecAssemblyGym(E, [load_urdf(f"shapes/{shape}.urdf")], obstacles, targets, max_steps=max_steps, seed=seed, **kw)


def random_obstacles():
    from bridges_hip.vec_env import RandomObstacles
    return RandomObstacles(ranges=RANGES)


def oracle_gym(obstacles, targets=TARGETS, shape="trapezoid", max_steps=MAX_STEPS, **kw):
    return OracleGym([get_shape(shape)], [tuple(o) for o in obstacles], [tuple(t) for t in targets], max_steps=max_steps, **kw)


def drawn(seed, E, episode=0, base=0):
    return np.array([draw_obstacles(seed, base + e, episode, RANGES) for e in range(E)])


class EpisodeSetupGym(OracleGym):
    """OracleGym whose reset() installs the obstacles (and, with ``targets_of_episode``, the targets) of the episode that begins,
    as env.reset(**setup_fct()) does in the reference (successor_dqn.py:371).  Episodes are numbered as the device numbers them:
    0 is the episode after bridges_env_reset; the reset() calls of the constructors belong to it (start_counting() follows)."""

    def __init__(self, obstacles_of_episode, targets_of_episode=None, **kw):
        self.obstacles_of_episode, self.targets_of_episode = obstacles_of_episode, targets_of_episode
        self.episode, self.counting = 0, False
        targets = targets_of_episode(0) if targets_of_episode else TARGETS
        super().__init__(obstacles=obstacles_of_episode(0), targets=targets, **kw)

    def start_counting(self):
        self.counting = True

    def reset(self):
        if self.counting:
            self.episode += 1
            cube06 = get_shape("cube06")
            self.obstacles = [tuple(float(v) for v in o) for o in self.obstacles_of_episode(self.episode)]
            self.obstacle_blocks = [Block(cube06, (o[0], o[2])) for o in self.obstacles]
            self.obstacle_raster = R.render_blocks_2d(self.obstacle_blocks, self.xlim, self.ylim, self.img_size)
            if self.targets_of_episode:
                self.targets = [tuple(float(v) for v in t) for t in self.targets_of_episode(self.episode)]
                self.target_blocks = [Block(cube06, (t[0], t[2])) for t in self.targets]
                tr = R.render_blocks_2d(self.target_blocks, self.xlim, self.ylim, self.img_size).astype(np.float32)
                self.reward_map = R.convolve_with_gaussian(tr, 101, 16)
        super().reset()


def episode_oracles(E, seed, shape="trapezoid", random_targets=False, lockstep_cls=OracleLockstep, **kw):
    gyms = [EpisodeSetupGym(lambda k, e=e: draw_obstacles(seed, e, k, RANGES),
                            (lambda k, e=e: draw_targets(seed, e, k)) if random_targets else None,
                            shapes=[get_shape(shape)], max_steps=MAX_STEPS, **kw) for e in range(E)]
    oracles = [lockstep_cls(g) for g in gyms]
    for g in gyms:
        g.start_counting()
    return oracles


def assert_obstacles_follow_the_draw(vec, oracles, it=None):
    ob, ep, bits = vec.env_obstacles.cpu().numpy(), vec.task_episode.cpu().numpy(), vec.env_obstacle_bits.cpu().numpy()
    for e, o in enumerate(oracles):
        assert ep[e] == o.gym.episode, (it, e, ep[e], o.gym.episode)
        assert np.array_equal(ob[e], np.array(o.gym.obstacles)), (it, e)
        assert canvas_equals(bits[e], o.gym.obstacle_raster), (it, e)


# ------------------------------------------------------------------------------------------------- draw and raster
@pytest.mark.parametrize("img_size", [(64, 64), (32, 32)])
def test_drawn_obstacles_and_their_rasters(img_size):
    from bridges_hip import abi
    E, seed, S = 32, 0, img_size[0]
    vec = make_vec(E, random_obstacles(), seed=seed, img_size=img_size)
    assert vec.per_env_obstacles and vec.per_env_tasks and vec.n_obstacles == 2 and vec.random_targets is None
    assert tuple(vec.env_obstacles.shape) == (E, 2, 3) and tuple(vec.env_obstacle_bits.shape) == (E, 64)
    ref = drawn(seed, E)
    assert np.array_equal(vec.env_obstacles.cpu().numpy(), ref)
    assert int(vec.task_episode.abs().sum()) == 0
    bits = vec.env_obstacle_bits.cpu().numpy()
    rasters = vec.obstacle_rasters
    assert tuple(rasters.shape) == (E, S, S) and rasters.dtype == torch.float32
    nonzero = 0
    for e in range(E):
        g = oracle_gym(ref[e], img_size=img_size)
        assert canvas_equals(bits[e], g.obstacle_raster), e
        assert np.array_equal(rasters[e].cpu().numpy(), g.obstacle_raster.astype(np.float32)), e
        nonzero += int(g.obstacle_raster.any())
    assert nonzero == E                                         # every drawn obstacle pair lies inside the image
    # the shared target list was replicated; its tables are those of a fixed-task env; the shared obstacle raster is empty
    fixed = make_vec(1, [], img_size=img_size)
    assert torch.equal(vec.env_targets.cpu(), torch.tensor(TARGETS, dtype=torch.float64).expand(E, 1, 3))
    assert torch.equal(vec.reward_maps, fixed.reward_map.expand(E, 64, 64))
    assert torch.equal(vec.reward_prefix, fixed.reward_prefix.expand(E, 64, 65))
    assert int(vec.buf["obstacle_bits"].abs().sum()) == 0
    with pytest.raises(abi.BridgesHipError, match="obstacle_rasters"):
        vec.obstacle_raster
    assert tuple(fixed.obstacle_raster.shape) == (1, S, S) and not fixed.per_env_obstacles
    with pytest.raises(abi.BridgesHipError):
        fixed.obstacle_rasters


# ------------------------------------------------------------------------------------------------- fresh-state masks
@pytest.mark.parametrize("shape,n_hit,n_blocked", [("trapezoid", 24, 0), ("hexagon", 23, 4)])
def test_fresh_state_masks_against_the_oracle(shape, n_hit, n_blocked):
    """The same 32 envs on their fresh states.  Worked out on the numpy oracle alone: an obstacle masks a candidate that is
    valid without obstacles in 24 of the 32 envs (trapezoid) / 23 (hexagon); 4 hexagon envs have no valid candidate at all."""
    E, seed = 32, 0
    vec = make_vec(E, random_obstacles(), shape=shape, seed=seed)
    free = make_vec(1, [], shape=shape, seed=seed)              # the device's own cand_lin of the fresh state: obstacle-free
    ref = drawn(seed, E)
    no_obst = oracle_gym([], shape=shape).candidates()
    off, n_cand = vec.cand_offset.cpu().numpy(), vec.n_cand.cpu().numpy()
    mask, nvalid, lin = vec.cand_mask.cpu().numpy().astype(bool), vec.n_valid.cpu().numpy(), vec.cand_lin.cpu().numpy()
    needs_reset, free_lin = vec.needs_reset.cpu().numpy(), free.cand_lin.cpu().numpy()
    hit = blocked = 0
    for e in range(E):
        c = oracle_gym(ref[e], shape=shape).candidates()
        A = len(c["actions"])
        assert n_cand[e] == A and A == len(no_obst["actions"]), e
        sl = slice(off[e], off[e] + A)
        assert np.array_equal(mask[sl], c["mask"]), e
        assert nvalid[e] == int(c["mask"].sum()), e
        assert bool(needs_reset[e]) == (not c["mask"].any()), e
        print(shape, e, "max |cand_lin - oracle|", float(np.abs(lin[sl] - c["lin_reward"]).max()))
        np.testing.assert_allclose(lin[sl], c["lin_reward"], rtol=1e-5, atol=1e-6)
        assert np.array_equal(lin[sl], free_lin[:A]), e        # exactly what a device env without obstacles computes
        hit += int((no_obst["mask"] & ~c["mask"]).any())
        blocked += int(not c["mask"].any())
    assert hit == n_hit and hit >= E // 2, hit                  # not vacuous: obstacles decide masks in most of the envs
    assert blocked == n_blocked, blocked


# ------------------------------------------------------------------------------------------------- lock-step parity
@pytest.mark.parametrize("shape", ["trapezoid", "hexagon"])
def test_lockstep_parity_with_fixed_per_env_obstacles(shape):
    E, seed, n_lock = 8, 4, 12
    obstacles = drawn(31, E)                                   # any 8 obstacle pairs; they stay over episode boundaries
    vec = make_vec(E, obstacles, shape=shape, seed=seed, f32_rasters=True)
    assert vec.per_env_obstacles and vec.random_obstacles is None
    oracles = [OracleLockstep(oracle_gym(obstacles[e], shape=shape)) for e in range(E)]
    n = run_lockstep_parity(vec, oracles, seed, n_lock=n_lock)
    assert n > E * (n_lock - 3)
    assert torch.equal(vec.env_obstacles.cpu(), torch.from_numpy(obstacles)) and int(vec.task_episode.abs().sum()) == 0
    for e, o in enumerate(oracles):
        assert canvas_equals(vec.env_obstacle_bits[e].cpu().numpy(), o.gym.obstacle_raster), e
    st = vec.read_stats()
    assert st["lp_errors"] == 0 and st["if_overflow"] == 0 and st["env_steps"] == n


@pytest.mark.parametrize("shape,random_targets", [("trapezoid", False), ("trapezoid", True), ("hexagon", False)])
def test_lockstep_parity_across_episode_boundaries_with_random_obstacles(shape, random_targets):
    from bridges_hip.vec_env import RandomTargets
    E, seed, n_lock = 8, 7, 12
    targets = RandomTargets() if random_targets else TARGETS
    vec = make_vec(E, random_obstacles(), targets=targets, shape=shape, seed=seed)
    oracles = episode_oracles(E, seed, shape=shape, random_targets=random_targets)
    assert_obstacles_follow_the_draw(vec, oracles)
    maps0 = vec.reward_maps.clone()
    counters, n_real = [0] * E, 0
    for it in range(n_lock):
        n_real += run_lockstep_parity(vec, oracles, seed, 1, counters)       # one lock-step: results, then the new candidates
        assert_obstacles_follow_the_draw(vec, oracles, it)
        if random_targets:
            tg = vec.env_targets.cpu().numpy()
            for e, o in enumerate(oracles):
                assert np.array_equal(tg[e], np.array(o.gym.targets)), (it, e)
    episodes = [o.gym.episode for o in oracles]
    assert min(episodes) >= 1 and n_real > E * (n_lock - 4), (episodes, n_real)   # every env crossed a boundary
    if not random_targets:      # the obstacle sampler alone leaves the target tables bit for bit what they were
        assert torch.equal(vec.reward_maps, maps0)
        assert torch.equal(vec.env_targets.cpu(), torch.tensor(TARGETS, dtype=torch.float64).expand(E, 1, 3))


# env 10 of the 32 hexagon envs of seed 0 starts fully blocked by its obstacles (worked out on the numpy oracle); envs 8..11
RESET_ONLY_CASE = dict(E=4, env_id_base=8, seed=0, blocked=2, n_lock=3)


@pytest.mark.parametrize("stable_actions_only", [False, True])
def test_reset_only_lockstep_draws_the_next_obstacles(stable_actions_only):
    """An env whose fresh state is fully blocked by its obstacles resets in a reset-only lock-step and takes the obstacles of
    its next episode there (with stable_actions_only: bridges_env_restrict_to_stable runs behind the task launch)."""
    from test_gpu_stable_actions import StableOracleLockstep
    c = RESET_ONLY_CASE
    E, base, seed = c["E"], c["env_id_base"], c["seed"]
    vec = make_vec(E, random_obstacles(), shape="hexagon", seed=seed, env_id_base=base, stable_actions_only=stable_actions_only)
    cls = StableOracleLockstep if stable_actions_only else OracleLockstep
    gyms = [EpisodeSetupGym(lambda k, e=e: draw_obstacles(seed, base + e, k, RANGES), shapes=[get_shape("hexagon")],
                            max_steps=MAX_STEPS) for e in range(E)]
    oracles = [cls(g) for g in gyms]
    for g in gyms:
        g.start_counting()
    assert oracles[c["blocked"]].needs_reset and bool(vec.needs_reset[c["blocked"]])
    counters, reset_only = [0] * E, 0

    def compare():
        off, n_cand = vec.cand_offset.cpu().numpy(), vec.n_cand.cpu().numpy()
        mask, nvalid = vec.cand_mask.cpu().numpy().astype(bool), vec.n_valid.cpu().numpy()
        for e, o in enumerate(oracles):
            A = len(o.cand["actions"])
            assert n_cand[e] == A, e
            assert np.array_equal(mask[off[e]:off[e] + A], o.cand["mask"]), e
            assert nvalid[e] == int(o.cand["mask"].sum()), e
    compare()
    assert_obstacles_follow_the_draw(vec, oracles)
    for it in range(c["n_lock"]):
        before_ep, before_ob = vec.task_episode.cpu().numpy().copy(), vec.env_obstacles.cpu().numpy().copy()
        vec.select_random()
        sel = vec.sel_index.cpu().numpy()
        outs = []
        for e, o in enumerate(oracles):
            def pick(nv, e=e):
                r = policy_draw(seed, base + e, counters[e]) % nv
                counters[e] += 1
                return r
            outs.append(o.lockstep(pick))
        vec.step()
        fl = {k: v.cpu().numpy() for k, v in vec.flags().items()}
        reward, ep, ob = vec.reward.cpu().numpy(), vec.task_episode.cpu().numpy(), vec.env_obstacles.cpu().numpy()
        for e, out in enumerate(outs):
            assert bool(fl["valid_step"][e]) == out["valid_step"], (it, e)
            assert bool(fl["no_actions"][e]) == out["no_actions"], (it, e)
            if out["valid_step"]:
                assert sel[e] == out["action_index"] and bool(fl["done"][e]) == out["done"] and reward[e] == out["reward"], (it, e)
                assert ep[e] == before_ep[e] + int(out["done"]), (it, e)
            else:                                               # reset-only lock-step: the env drew its next obstacles here
                reset_only += 1
                assert ep[e] == before_ep[e] + 1 and not np.array_equal(ob[e], before_ob[e]), (it, e)
        compare()
        assert_obstacles_follow_the_draw(vec, oracles, it)
    assert reset_only >= 1 and vec.read_stats()["reset_only"] == reset_only


# ------------------------------------------------------------------------------------------------- other
def test_equal_obstacles_in_every_env_equal_the_fixed_task_env():
    from bridges_hip import abi
    E, seed, max_steps = 16, 6, 8
    obst = [(1.2, 0.0, 0.3), (-0.9, 0.0, 0.9)]
    fixed = make_vec(E, obst, max_steps=max_steps, seed=seed, f32_rasters=True)
    per_env = make_vec(E, torch.tensor(obst, dtype=torch.float64).expand(E, 2, 3).contiguous(), max_steps=max_steps, seed=seed,
                       f32_rasters=True)
    assert per_env.per_env_obstacles and not fixed.per_env_obstacles and fixed.obstacle_buf is None
    assert torch.equal(per_env.env_obstacle_bits, fixed.buf["obstacle_bits"].expand(E, 64))
    assert int(fixed.buf["obstacle_bits"].abs().sum()) > 0 and int(per_env.buf["obstacle_bits"].abs().sum()) == 0
    assert torch.equal(per_env.obstacle_rasters, fixed.obstacle_raster.expand(E, 64, 64))
    task_fields = ("obstacle_bits", "reward_map", "reward_prefix")
    names = [n for n, _, _ in abi.ENV_BUFFER_FIELDS + abi.ENV_BUFFER_FIELDS_TAIL if n not in task_fields]

    def same(it):
        total = int(fixed.cand_offset[E])
        assert total == int(per_env.cand_offset[E])
        for n in names:
            a, b = fixed.buf[n], per_env.buf[n]
            if a is None:
                assert b is None
                continue
            if a.shape[:1] == (E * fixed.a_max,):               # candidate arrays: the live prefix
                a, b = a[:total], b[:total]
            assert torch.equal(a, b), (it, n)
        assert torch.equal(fixed.stats - stats0[0], per_env.stats - stats0[1]), it
        snapshots_equal(fixed.lp_snap, per_env.lp_snap, it)
    stats0 = (fixed.stats.clone(), per_env.stats.clone())
    same(-1)
    masked = 0
    for it in range(10):
        for env in (fixed, per_env):
            env.select_random()
            env.step()
        same(it)
        total = int(fixed.cand_offset[E])
        masked += int((fixed.cand_inb[:total].bool() & ~fixed.cand_mask[:total].bool()).sum())
    assert masked > 0 and fixed.read_stats()["env_steps"] > E * 7


def test_two_groups_draw_what_one_env_of_all_ids_draws():
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym, VecAssemblyGymGroups
    E, seed = 32, 21
    geoms = [load_urdf("shapes/trapezoid.urdf")]
    one = VecAssemblyGym(E, geoms, random_obstacles(), TARGETS, max_steps=MAX_STEPS, seed=seed, f32_rasters=False)
    two = VecAssemblyGymGroups(E, geoms, random_obstacles(), TARGETS, groups=2, max_steps=MAX_STEPS, seed=seed, f32_rasters=False)
    assert [env.env_id_base for env in two.envs] == [0, 16] and all(env.per_env_obstacles for env in two.envs)

    def same():
        two.sync()
        torch.cuda.synchronize()
        for name in ("env_obstacles", "env_obstacle_bits", "task_episode", "n_valid", "n_blocks", "state_bits"):
            assert torch.equal(getattr(one, name), torch.cat([getattr(env, name) for env in two.envs])), name
        ref = np.array([draw_obstacles(seed, e, int(k), RANGES) for e, k in enumerate(one.task_episode.cpu().numpy())])
        assert np.array_equal(one.env_obstacles.cpu().numpy(), ref)
    same()
    assert int(one.task_episode.sum()) == 0
    for _ in range(8):
        one.select_random()
        one.step()
        two.lockstep_random()
    same()
    assert int(one.task_episode.min()) >= 1
    # explicit per-env arrays are cut into the groups' slices
    arr = drawn(3, E)
    cut = VecAssemblyGymGroups(E, geoms, arr, TARGETS, groups=2, max_steps=MAX_STEPS, seed=seed, f32_rasters=False)
    cut.sync()
    assert np.array_equal(torch.cat([env.env_obstacles for env in cut.envs]).cpu().numpy(), arr)


def candidate_view(vec):
    total = int(vec.cand_offset[vec.E])
    return [vec.cand_offset.clone(), vec.n_valid.clone(), vec.cand_mask[:total].clone(), vec.cand_lin[:total].clone(),
            vec.cand_bits[:total].clone(), vec.env_obstacle_bits.clone()]


def test_load_obstacles_then_refresh_equals_an_env_created_with_them():
    E, seed = 8, 2
    a, b = drawn(40, E), drawn(41, E)
    made = make_vec(E, b, seed=seed)
    vec = make_vec(E, a, seed=seed)
    assert not all(torch.equal(x, y) for x, y in zip(candidate_view(vec), candidate_view(made)))
    vec.load_obstacles(torch.from_numpy(b).to(vec.device))
    vec.refresh()
    assert all(torch.equal(x, y) for x, y in zip(candidate_view(vec), candidate_view(made)))
    assert torch.equal(vec.reward_prefix, made.reward_prefix) and int(vec.task_episode.abs().sum()) == 0
    # set_obstacles: the same through a reset, on an env that began with a shared list
    plain = make_vec(E, [(1.0, 0.0, 0.3), (2.0, 0.0, 0.3)], seed=seed)
    assert not plain.per_env_obstacles and not plain.per_env_tasks
    plain.set_obstacles(torch.from_numpy(b))
    assert plain.per_env_obstacles and plain.per_env_tasks
    assert all(torch.equal(x, y) for x, y in zip(candidate_view(plain), candidate_view(made)))
    sampled = make_vec(E, random_obstacles(), seed=seed)
    with pytest.raises(ValueError):
        sampled.load_obstacles(torch.from_numpy(b).to(vec.device))     # a sampler owns env_obstacles
    with pytest.raises(ValueError):
        vec.set_obstacles(torch.zeros((E, 3, 3), dtype=torch.float64))  # built for two obstacles per env


def test_state_groups_keys_on_the_obstacles():
    E = 8
    obst = drawn(50, 4)[[0, 1, 0, 2, 1, 0, 3, 2]]              # fresh states everywhere: envs differ in obstacles alone
    vec = make_vec(E, obst)
    assert vec.state_groups(task=False).tolist() == [0] * E
    assert vec.state_groups(task=True).tolist() == [0, 1, 0, 3, 1, 0, 6, 3]


def test_an_env_without_the_option_attaches_no_obstacle_buffer():
    """Plain obstacle list + per-env targets: env_obstacle_bits stays NULL, the shared raster is what the rasteriser reads, and
    every output equals the fixed-task env's; the library refuses a half-given pair and names the field."""
    from bridges_hip import abi
    E, seed = 16, 6
    obst, task = [(1.2, 0.0, 0.3), (-0.9, 0.0, 0.9)], [(0.5, 0.0, 1.2), (1.5, 0.0, 2.0), (-0.5, 0.0, 0.4)]
    fixed = make_vec(E, obst, targets=task, seed=seed)
    vec = make_vec(E, obst, targets=task, seed=seed)
    vec.set_targets(torch.tensor(task, dtype=torch.float64).expand(E, 3, 3).contiguous())
    assert vec.per_env_tasks and not vec.per_env_obstacles and vec.obstacle_buf is None and vec.n_obstacles == 0
    assert torch.equal(vec.buf["obstacle_bits"], fixed.buf["obstacle_bits"]) and torch.equal(vec.obstacle_raster, fixed.obstacle_raster)
    for it in range(8):
        total = int(fixed.cand_offset[E])
        assert total == int(vec.cand_offset[E])
        for n in ("cand_mask", "cand_lin", "cand_bits"):
            assert torch.equal(fixed.buf[n][:total], vec.buf[n][:total]), (it, n)
        for n in ("n_valid", "n_blocks", "state_bits", "step_flags", "reward", "lin_reward", "sel_index"):
            assert torch.equal(fixed.buf[n], vec.buf[n]), (it, n)
        for env in (fixed, vec):
            env.select_random()
            env.step()
    # the C ABI: the buffer without a count, a count without the buffer
    scratch = torch.zeros((E, 64), dtype=torch.int64, device=vec.device)
    coords = torch.zeros((E, 2, 3), dtype=torch.float64, device=vec.device)

    def attach(**fields):
        tb = abi.TaskBuffers()
        for name, _, _ in abi.TASK_BUFFER_FIELDS:
            setattr(tb, name, vec.task_buf[name].data_ptr())
        tb.gauss_k, tb.target_shape = vec._gauss_k.data_ptr(), len(vec.table_geoms) - 1
        for k, v in fields.items():
            setattr(tb, k, v)
        abi.check(vec.L.bridges_env_set_task_buffers(vec._env, C.byref(tb)), "bridges_env_set_task_buffers")
    with pytest.raises(abi.BridgesHipError, match="n_obstacles"):
        attach(env_obstacle_bits=scratch.data_ptr())
    with pytest.raises(abi.BridgesHipError, match="env_obstacle_bits"):
        attach(n_obstacles=2, env_obstacles=coords.data_ptr())
    with pytest.raises(abi.BridgesHipError, match="env_obstacles"):
        attach(n_obstacles=2, env_obstacle_bits=scratch.data_ptr())
    with pytest.raises(abi.BridgesHipError, match="n_obstacles"):
        attach(n_obstacles=5, env_obstacle_bits=scratch.data_ptr(), env_obstacles=coords.data_ptr())
    attach()                                                    # what the env had attached: still accepted
