"""GPU: per-env tasks of the lock-step env -- every env owns its targets (set_targets / a [E, T, 3] array) or redraws them on
the device whenever it starts an episode (RandomTargets, the reference's tower_setup per env.reset(**setup_fct())).
Bit-exact: the per-env task features against the host path of a fixed-task env, targets and episode counters against the
restated draw, candidates / masks / rasters / stability / rewards against the oracles; 1e-5: linear rewards and the reward
map against the numpy oracle (the tolerances of tests/test_gpu_env_parity.py)."""
import numpy as np
import pytest
import torch

from oracle import raster as R
from oracle.env import OracleGym, OracleLockstep, policy_draw
from oracle.geometry import Block
from oracle.shapes import get_shape
from task_draw import draw_targets
from test_gpu_env_parity import canvas_equals, run_lockstep_parity

pytestmark = pytest.mark.gpu


def tower_targets(rng, n, T=3):
    """n target sets from tower_setup's distribution (gym_env.py:64-79): x ~ U[-4, 4], z ~ U[0, 4], y = 0."""
    t = np.zeros((n, T, 3))
    t[:, :, 0] = rng.uniform(-4, 4, (n, T))
    t[:, :, 2] = rng.uniform(0, 4, (n, T))
    return t


def make_vec(E, targets, shape="trapezoid", max_steps=6, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    return VecAssemblyGym(E, [load_urdf(f"shapes/{shape}.urdf")], [], targets, max_steps=max_steps, seed=seed, **kw)


def oracle_gym(targets, shape="trapezoid", max_steps=6, **kw):
    return OracleGym([get_shape(shape)], [], [tuple(t) for t in targets], max_steps=max_steps, **kw)


class EpisodeTaskGym(OracleGym):
    """OracleGym whose reset() installs the task of the episode that begins, as env.reset(**setup_fct()) does in the reference
    (successor_dqn.py:371).  Episodes are numbered as the device numbers them: 0 is the episode after bridges_env_reset; the
    reset() calls of OracleGym.__init__ / OracleLockstep.__init__ belong to it (start_counting() comes after them)."""

    def __init__(self, task_of_episode, **kw):
        self.task_of_episode, self.episode, self.counting = task_of_episode, 0, False
        super().__init__(targets=task_of_episode(0), **kw)

    def start_counting(self):
        self.counting = True

    def reset(self):
        if self.counting:
            self.episode += 1
            self.targets = [tuple(float(v) for v in t) for t in self.task_of_episode(self.episode)]
            cube06 = get_shape("cube06")
            self.target_blocks = [Block(cube06, (t[0], t[2])) for t in self.targets]
            tr = R.render_blocks_2d(self.target_blocks, self.xlim, self.ylim, self.img_size).astype(np.float32)
            self.reward_map = R.convolve_with_gaussian(tr, 101, 16)
        super().reset()


def episode_oracles(E, seed, lockstep_cls=OracleLockstep, env_id_base=0, **kw):
    gyms = [EpisodeTaskGym(lambda k, e=e: draw_targets(seed, env_id_base + e, k), shapes=[get_shape("trapezoid")], obstacles=[], **kw)
            for e in range(E)]
    oracles = [lockstep_cls(g) for g in gyms]
    for g in gyms:
        g.start_counting()
    return oracles


def assert_tasks_follow_the_draw(vec, oracles, it=None):
    tg, ep = vec.env_targets.cpu().numpy(), vec.task_episode.cpu().numpy()
    for e, o in enumerate(oracles):
        assert ep[e] == o.gym.episode, (it, e, ep[e], o.gym.episode)
        assert np.array_equal(tg[e], np.array(o.gym.targets)), (it, e)


# ---------------------------------------------------------------------------------------------------------------- 1
HAND_SETS = [
    [(-3.9, 0.0, 2.0), (1.0, 0.0, 1.0), (2.0, 0.0, 3.0)],       # one target left of the image (x < -3): no pixel
    [(-3.0, 0.0, 2.0), (7.0, 0.0, 1.0), (0.0, 0.0, 10.0)],      # on the image border: left, right, top
    [(1.0, 0.0, 1.0), (1.3, 0.0, 1.2), (4.0, 0.0, 2.0)],        # two overlapping cubes
    [(0.5, 0.0, 1.5), (0.5, 0.0, 1.5), (3.0, 0.0, 0.5)],        # the same target twice
    [(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (-2.0, 0.0, 0.0)],       # z = 0: cube half below the floor
]


def check_task_features(sets, img_size):
    """set_targets(sets) on one env of len(sets) envs against a fixed-task env per set (host path) and the numpy oracle."""
    sets = np.asarray(sets, dtype=np.float64)
    n, T = sets.shape[:2]
    vec = make_vec(n, [(0.0, 0.0, 0.0)] * T, img_size=img_size, f32_rasters=False)
    assert not vec.per_env_tasks and vec.task_buf is None          # a plain target list allocates none of the new buffers
    vec.set_targets(torch.from_numpy(sets))
    assert vec.per_env_tasks and torch.equal(vec.env_targets.cpu(), torch.from_numpy(sets))
    S = img_size[0]
    assert tuple(vec.reward_maps.shape) == (n, 64, 64) and tuple(vec.reward_maps_img.shape) == (n, S, S)
    assert tuple(vec.reward_prefix.shape) == (n, 64, 65) and tuple(vec.target_bits.shape) == (n, 64)
    nonzero = 0
    for e in range(n):
        fixed = make_vec(1, [tuple(t) for t in sets[e]], img_size=img_size, f32_rasters=False)
        assert torch.equal(vec.target_bits[e], fixed.target_bits), e
        assert torch.equal(vec.reward_maps[e], fixed.reward_map), e
        assert torch.equal(vec.reward_prefix[e], fixed.reward_prefix), e
        g = oracle_gym(sets[e], img_size=img_size)
        tr = R.render_blocks_2d(g.target_blocks, g.xlim, g.ylim, img_size)
        assert canvas_equals(vec.target_bits[e].cpu().numpy(), tr), e
        np.testing.assert_allclose(vec.reward_maps_img[e].cpu().numpy(), g.reward_map, rtol=1e-5, atol=1e-7)
        nonzero += int(tr.any())
    assert int(vec.task_episode.abs().sum()) == 0
    return nonzero


@pytest.mark.parametrize("img_size", [(64, 64), (32, 32)])
def test_task_features_equal_the_host_path_bit_for_bit(img_size):
    rng = np.random.default_rng(20)
    sets3 = np.concatenate([np.array(HAND_SETS), tower_targets(rng, 27)])
    assert len(sets3) == 32
    assert check_task_features(sets3, img_size) >= 30
    check_task_features(tower_targets(rng, 2, T=1), img_size)
    check_task_features(tower_targets(rng, 2, T=8), img_size)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("shape", ["trapezoid", "hexagon"])
def test_lockstep_parity_with_fixed_per_env_targets(shape):
    E, seed, max_steps = 48, 9, 8
    targets = tower_targets(np.random.default_rng(4), E)
    vec = make_vec(E, targets, shape=shape, max_steps=max_steps, seed=seed)
    oracles = [OracleLockstep(oracle_gym(targets[e], shape=shape, max_steps=max_steps)) for e in range(E)]
    n = run_lockstep_parity(vec, oracles, seed, n_lock=25)
    assert n > E * 20
    assert torch.equal(vec.env_targets.cpu(), torch.from_numpy(targets)) and int(vec.task_episode.abs().sum()) == 0
    st = vec.read_stats()
    assert st["lp_errors"] == 0 and st["if_overflow"] == 0 and st["env_steps"] == n


# ---------------------------------------------------------------------------------------------------------------- 3
def test_lockstep_parity_across_episode_boundaries_with_the_sampler_on():
    from bridges_hip.vec_env import RandomTargets
    E, seed, max_steps, n_lock = 48, 13, 6, 40
    vec = make_vec(E, RandomTargets(), max_steps=max_steps, seed=seed, f32_rasters=False)
    oracles = episode_oracles(E, seed, max_steps=max_steps)
    assert_tasks_follow_the_draw(vec, oracles)
    counters, n_real, reached = [0] * E, 0, 0
    for it in range(n_lock):
        n_real += run_lockstep_parity(vec, oracles, seed, 1, counters)       # one lock-step: results, then the new candidates
        assert_tasks_follow_the_draw(vec, oracles, it)
        reached += int((vec.n_reached > 0).sum())
    episodes = [o.gym.episode for o in oracles]
    assert min(episodes) >= 2, episodes                                        # every env crossed at least two boundaries
    assert n_real > E * 30 and reached > 0
    # the tables of the tasks the envs hold now are those of fixed-task envs on the same targets
    for e in (0, E - 1):
        fixed = make_vec(1, oracles[e].gym.targets, max_steps=max_steps, f32_rasters=False)
        assert torch.equal(vec.reward_maps[e], fixed.reward_map) and torch.equal(vec.reward_prefix[e], fixed.reward_prefix)


# seed and sizes picked with the numpy oracle alone (this draw formula): 12 reset-only lock-steps and 36 `done` among 288,
# every env past its fourth episode; the test asserts that both kinds of boundary occurred, so the case cannot drop out silently
RESET_ONLY_CASE = dict(E=12, seed=3, max_steps=6, n_lock=24, mu=0.3)


def test_reset_only_lockstep_draws_a_new_task_stable_actions_only():
    """The other kind of episode boundary: an env left without a (stable) candidate resets in a reset-only lock-step and takes
    its next task there.  Narrowed oracle protocol of tests/test_gpu_stable_actions.py; bridges_env_restrict_to_stable runs
    behind the task launch."""
    from bridges_hip.vec_env import RandomTargets
    from test_gpu_stable_actions import StableOracleLockstep
    c = RESET_ONLY_CASE
    E, seed = c["E"], c["seed"]
    vec = make_vec(E, RandomTargets(), max_steps=c["max_steps"], seed=seed, mu=c["mu"], f32_rasters=False, stable_actions_only=True)
    oracles = episode_oracles(E, seed, lockstep_cls=StableOracleLockstep, max_steps=c["max_steps"], mu=c["mu"])
    counters = [0] * E
    reset_only = dones = 0

    def compare():
        off, n_cand = vec.cand_offset.cpu().numpy(), vec.n_cand.cpu().numpy()
        mask, nvalid, lin = vec.cand_mask.cpu().numpy().astype(bool), vec.n_valid.cpu().numpy(), vec.cand_lin.cpu().numpy()
        for e, o in enumerate(oracles):
            A = len(o.cand["actions"])
            assert n_cand[e] == A, (e, n_cand[e], A)
            assert np.array_equal(mask[off[e]:off[e] + A], o.cand["mask"]), e
            assert nvalid[e] == int(o.cand["mask"].sum()), e
            np.testing.assert_allclose(lin[off[e]:off[e] + A], o.cand["lin_reward"], rtol=1e-5, atol=1e-6)
    compare()
    assert_tasks_follow_the_draw(vec, oracles)
    for it in range(c["n_lock"]):
        before_ep = vec.task_episode.cpu().numpy().copy()
        before_tg = vec.env_targets.cpu().numpy().copy()
        vec.select_random()
        sel = vec.sel_index.cpu().numpy()
        outs = []
        for e, o in enumerate(oracles):
            def pick(nv, e=e):
                r = policy_draw(seed, e, counters[e]) % nv
                counters[e] += 1
                return r
            outs.append(o.lockstep(pick))
        vec.step()
        fl = {k: v.cpu().numpy() for k, v in vec.flags().items()}
        reward, ep, tg = vec.reward.cpu().numpy(), vec.task_episode.cpu().numpy(), vec.env_targets.cpu().numpy()
        for e, out in enumerate(outs):
            assert bool(fl["valid_step"][e]) == out["valid_step"], (it, e)
            assert bool(fl["no_actions"][e]) == out["no_actions"], (it, e)
            if out["valid_step"]:
                assert sel[e] == out["action_index"], (it, e)
                assert bool(fl["done"][e]) == out["done"], (it, e)
                assert reward[e] == out["reward"], (it, e)
                dones += int(out["done"])
                assert ep[e] == before_ep[e] + int(out["done"]), (it, e)
            else:                                               # reset-only lock-step: the env drew its next task here
                reset_only += 1
                assert ep[e] == before_ep[e] + 1 and not np.array_equal(tg[e], before_tg[e]), (it, e)
        compare()
        assert_tasks_follow_the_draw(vec, oracles, it)
    assert reset_only >= 1 and dones >= 1, (reset_only, dones)
    st = vec.read_stats()
    assert st["lp_errors"] == 0 and st["if_overflow"] == 0 and st["reset_only"] == reset_only


# ---------------------------------------------------------------------------------------------------------------- 4
def test_fixed_per_env_targets_at_size_against_the_c_oracle():
    """1024 envs, each with its own three targets, each against its own C oracle built on them: selected action, stability
    booleans, reward, termination, candidate / valid counts, state raster."""
    from oracle.c_env import CEnv
    E, seed, max_steps, n_lock = 1024, 29, 10, 25
    targets = tower_targets(np.random.default_rng(11), E)
    vec = make_vec(E, targets, max_steps=max_steps, seed=seed, f32_rasters=False)
    cenvs = [CEnv(oracle_gym(targets[e], max_steps=max_steps)) for e in range(E)]
    steps = mism = reached = 0
    for it in range(n_lock):
        vec.select_random()
        sel = vec.sel_index.cpu().numpy()
        vec.step()
        fl, rew, ncand = vec.step_flags.cpu().numpy(), vec.reward.cpu().numpy(), vec.n_cand.cpu().numpy()
        nval, nre = vec.n_valid.cpu().numpy(), vec.n_reached.cpu().numpy()
        sb = vec.state_bits.cpu().numpy().astype(np.uint64)
        lin = vec.lin_reward.cpu().numpy()
        for e, ce in enumerate(cenvs):
            o = ce.lockstep(seed, e)
            ok = bool(fl[e, 0]) == bool(o.valid_step) and bool(fl[e, 6]) == bool(o.no_actions)
            if o.valid_step:
                steps += 1
                reached += int(o.n_reached > 0)
                ok = ok and sel[e] == o.action_index and fl[e, 1] == o.stable_frozen and fl[e, 2] == o.stable_unfrozen \
                    and fl[e, 3] == o.terminated and fl[e, 4] == o.truncated and rew[e] == o.reward and (fl[e, 7] & 3) == 0 \
                    and nre[e] == o.n_reached and bool(np.isclose(lin[e], o.lin_reward, rtol=1e-5, atol=1e-7))
            if it % 6 == 0:
                cands, n_v = ce.candidates()
                ok = ok and len(cands) == ncand[e] and n_v == nval[e] and list(sb[e]) == ce.state_bits()
            mism += int(not ok)
    assert mism == 0 and steps > E * 20 and reached > 100, (mism, steps, reached)


# ---------------------------------------------------------------------------------------------------------------- 5
def snapshots_equal(a, b, it):
    """lp_snap of two envs where k_step defines it (rbe_device.h: WarmHdr, lp_warm_store): the six header words; for a live
    snapshot (magic set) the basis of its m rows and rows 0..m x the 4 n_if + 2 + m columns of the tableau.  The rest of a
    slot is never written by the step that made the snapshot."""
    a, b = a.cpu(), b.cpu()
    ha, hb = a[:, :64].contiguous().view(torch.int32), b[:, :64].contiguous().view(torch.int32)
    assert torch.equal(ha[:, :6], hb[:, :6]), it
    live = 0
    for e in range(a.shape[0]):
        magic, _nb, n_if, stride, _half, m = (int(v) for v in ha[e, :6])
        if magic == 0:
            continue
        live += 1
        ncols = 4 * n_if + 2 + m
        assert torch.equal(ha[e, 16:16 + m], hb[e, 16:16 + m]), (it, e)
        ta, tb = (t[e, 64:64 + (m + 1) * stride].reshape(m + 1, stride)[:, :ncols] for t in (a, b))
        assert torch.equal(ta, tb), (it, e)
    return live


def test_one_task_for_all_envs_equals_the_fixed_task_env():
    from bridges_hip import abi
    E, seed, max_steps = 64, 6, 8
    task = [(0.5, 0.0, 1.2), (1.5, 0.0, 2.0), (-0.5, 0.0, 0.4)]
    fixed = make_vec(E, task, max_steps=max_steps, seed=seed)
    per_env = make_vec(E, task, max_steps=max_steps, seed=seed)
    per_env.set_targets(torch.tensor(task, dtype=torch.float64).expand(E, 3, 3).contiguous())
    task_fields = ("obstacle_bits", "reward_map", "reward_prefix")
    names = [n for n, _, _ in abi.ENV_BUFFER_FIELDS + abi.ENV_BUFFER_FIELDS_TAIL if n not in task_fields]
    assert torch.equal(per_env.buf["obstacle_bits"], fixed.buf["obstacle_bits"])
    assert torch.equal(per_env.reward_maps, fixed.reward_map.expand(E, 64, 64))
    assert torch.equal(per_env.reward_prefix, fixed.reward_prefix.expand(E, 64, 65))

    def same(it):
        total = int(fixed.cand_offset[E])
        assert total == int(per_env.cand_offset[E])
        for n in names:
            a, b = fixed.buf[n], per_env.buf[n]
            if a is None:                                       # sparse-update masks: not allocated
                assert b is None
                continue
            if a.shape[:1] == (E * fixed.a_max,):               # candidate arrays: the live prefix
                a, b = a[:total], b[:total]
            assert torch.equal(a, b), (it, n)
        assert torch.equal(fixed.stats - stats0[0], per_env.stats - stats0[1]), it       # (set_targets was a second reset)
        snapshots_equal(fixed.lp_snap, per_env.lp_snap, it)
    stats0 = (fixed.stats.clone(), per_env.stats.clone())
    same(-1)
    for it in range(20):
        for env in (fixed, per_env):
            env.select_random()
            env.step()
        same(it)
    assert int(fixed.n_reached.max()) >= 1 and fixed.read_stats()["env_steps"] > E * 15


# ---------------------------------------------------------------------------------------------------------------- 6
def test_two_groups_draw_what_one_env_of_all_ids_draws():
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomTargets, VecAssemblyGym, VecAssemblyGymGroups
    E, seed = 128, 21
    geoms = [load_urdf("shapes/trapezoid.urdf")]
    one = VecAssemblyGym(E, geoms, [], RandomTargets(), max_steps=6, seed=seed, f32_rasters=False)
    two = VecAssemblyGymGroups(E, geoms, [], RandomTargets(), groups=2, max_steps=6, seed=seed, f32_rasters=False)
    assert [env.env_id_base for env in two.envs] == [0, 64] and all(env.per_env_tasks for env in two.envs)

    def same():
        two.sync()
        torch.cuda.synchronize()
        for name in ("env_targets", "task_episode", "target_bits", "reward_maps", "reward_prefix"):
            assert torch.equal(getattr(one, name), torch.cat([getattr(env, name) for env in two.envs])), name
        ref = np.array([draw_targets(seed, e, int(k)) for e, k in enumerate(one.task_episode.cpu().numpy())])
        assert np.array_equal(one.env_targets.cpu().numpy(), ref)
    same()
    assert int(one.task_episode.sum()) == 0
    for _ in range(10):
        one.select_random()
        one.step()
        two.lockstep_random()
    same()
    assert int(one.task_episode.min()) >= 1


# ---------------------------------------------------------------------------------------------------------------- 7
def test_vec_dqn_refuses_per_env_tasks_and_single_task_attributes_raise():
    from bridges_hip import abi
    from bridges_hip.vec_env import RandomTargets
    from robotoddler.training.vec_dqn import VecDQN
    for vec in (make_vec(4, RandomTargets(), f32_rasters=False),
                make_vec(4, tower_targets(np.random.default_rng(0), 4), f32_rasters=False)):
        with pytest.raises(ValueError, match="per-env tasks"):
            VecDQN(None, None, None, vec, 64, 8, 0.9, 0.05, "q")
        for name, per_env in (("reward_map", "reward_maps"), ("reward_features", "reward_maps_img"),
                              ("_reward_obstacle_flat", "reward_maps_img")):
            with pytest.raises(abi.BridgesHipError, match=per_env):
                getattr(vec, name)
    plain = make_vec(4, [(0.5, 0.0, 1.0)], f32_rasters=False)
    assert tuple(plain.reward_map.shape) == (64, 64) and tuple(plain.reward_features.shape) == (1, 64, 64)
    assert plain._reward_obstacle_flat is None and not plain.per_env_tasks
    with pytest.raises(ValueError):
        plain.set_targets(torch.zeros((4, 3, 3), dtype=torch.float64))       # built for one target per env
