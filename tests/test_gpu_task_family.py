"""GPU: task families of the lock-step env (RandomBridges / bridges_env_set_task_family) -- every env draws ONE integer n whenever
it starts an episode and holds the target and obstacles of horizontal_bridge_setup(num_obstacles=n) / bridge_setup(num_stories=n),
unused obstacle slots parked -- and the per-class episode statistics (bridges_episode_stats_by_class).
Bit-exact: coordinates, classes and episode counters against the restated draw (tests/family_draw.py), rasters against
render_blocks_2d, the degenerate family against explicit per-env arrays and the fixed task, masks / counts / flags / rewards /
states against one oracle per env that installs the episode's task at reset(), one class of the by-class fold against
bridges_episode_stats.  1e-5: linear rewards against the numpy oracle (the tolerance of tests/test_gpu_env_parity.py); the float
sums of the fold against the float64 restatement as tests/test_gpu_episode_stats.py compares them."""
import ctypes as C

import numpy as np
import pytest
import torch

from class_stats_ref import RestatedByClass
from family_draw import PARK_Z, draw_family, family_draw, family_task
from oracle import raster as R
from oracle.env import OracleLockstep
from oracle.geometry import Block
from oracle.shapes import get_shape
from test_gpu_env_obstacles import EpisodeSetupGym
from test_gpu_env_parity import canvas_equals, run_lockstep_parity
from test_gpu_episode_stats import _synthetic_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1                                          # BRIDGES_E_ARG


def make_vec(E, obstacles, targets, shape="trapezoid", max_steps=6, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    kw.setdefault("f32_rasters", False)
    return VecAssemblyGym(E, [load_urdf(f"shapes/{shape}.urdf")], obstacles, targets, max_steps=max_steps, seed=seed, **kw)


def family_env(E, kind, sizes, **kw):
    from bridges_hip.vec_env import RandomBridges
    return make_vec(E, [], RandomBridges(kind, sizes=sizes), **kw)


def render(points, size):
    from oracle.env import XLIM, YLIM
    cube06 = get_shape("cube06")
    return R.render_blocks_2d([Block(cube06, (p[0], p[2])) for p in points], XLIM, YLIM, (size, size))


def assert_follows_the_draw(vec, kind, seed, lo, hi, episodes, tag=None):
    """env_targets, env_obstacles, task_class and task_episode of every env are those of (seed, env, episodes[e])."""
    tg, ob = vec.env_targets.cpu().numpy(), vec.env_obstacles.cpu().numpy()
    cls, ep = vec.task_class.cpu().numpy(), vec.task_episode.cpu().numpy()
    for e in range(vec.E):
        n, targets, obstacles = draw_family(kind, seed, e, episodes[e], lo, hi)
        assert ep[e] == episodes[e] and cls[e] == n, (tag, e, ep[e], episodes[e], cls[e], n)
        assert np.array_equal(tg[e], np.array(targets)) and np.array_equal(ob[e], np.array(obstacles)), (tag, e)
    return cls


# ------------------------------------------------------------------------------------------------- draw and rasters
@pytest.mark.parametrize("img_size", [(64, 64), (32, 32)])
@pytest.mark.parametrize("kind", ["span", "tower"])
def test_drawn_tasks_and_their_rasters(kind, img_size):
    E, seed, S, lo, hi = 32, 0, img_size[0], 1, 4
    vec = family_env(E, kind, (lo, hi), seed=seed, img_size=img_size)
    assert vec.per_env_tasks and vec.per_env_obstacles and vec.n_targets == 1 and vec.n_obstacles == hi
    assert vec.random_targets is None and vec.random_obstacles is None
    assert vec.task_family.kind == kind and vec.task_class.dtype == torch.int32 and tuple(vec.task_class.shape) == (E,)
    assert tuple(vec.env_targets.shape) == (E, 1, 3) and tuple(vec.env_obstacles.shape) == (E, hi, 3)
    cls = assert_follows_the_draw(vec, kind, seed, lo, hi, [0] * E)
    assert sorted(set(cls.tolist())) == [1, 2, 3, 4]                       # all four classes occur
    assert cls.tolist() == [int(v) for v in "2 4 1 1 1 1 3 1 3 4 1 2 3 1 1 2 1 3 4 2 3 3 4 1 3 4 2 1 1 4 4 2".split()]
    tbits, obits = vec.target_bits.cpu().numpy(), vec.env_obstacle_bits.cpu().numpy()
    parked = 0
    for e in range(E):
        targets, obstacles = family_task(kind, int(cls[e]), hi)
        assert canvas_equals(tbits[e], render(targets, S)) and render(targets, S).any(), e
        live = render(obstacles[:cls[e]], S)
        assert canvas_equals(obits[e], live) and live.any(), e             # parked slots add nothing to the live obstacles
        assert np.array_equal(live, render(obstacles, S)), e
        parked += sum(1 for o in obstacles if o[2] == PARK_Z)
    assert parked == sum(hi - int(n) for n in cls) > 0


# ------------------------------------------------------------------------------------------------- degenerate family
def cli_task(kind, n):
    """The numbers run_vectorised builds for --bridge_length n / --tower_height n."""
    if kind == "tower":
        H = 0.8
        return [(0.5, 0, n * H + H / 2)], [(0.5, 0., i * H + H / 2) for i in range(n)]
    sq = 0.6
    return [(n * sq + 2.5 * sq, 0, sq / 2)], [(i * sq, 0, sq / 2) for i in range(1, n + 1)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", ["span", "tower"])
def test_a_family_of_one_size_is_the_fixed_task(kind, n):
    E, seed = 8, 2
    fam = family_env(E, kind, (n, n), seed=seed)
    targets, obstacles = cli_task(kind, n)
    arrays = make_vec(E, np.array([obstacles] * E, dtype=np.float64), np.array([targets] * E, dtype=np.float64), seed=seed)
    fixed = make_vec(E, obstacles, targets, seed=seed)
    assert fam.n_obstacles == arrays.n_obstacles == n and int(fam.task_class.min()) == int(fam.task_class.max()) == n

    def same():
        assert torch.equal(fam.env_targets, arrays.env_targets) and torch.equal(fam.env_obstacles, arrays.env_obstacles)
        for name in ("target_bits", "reward_maps", "reward_prefix", "env_obstacle_bits"):
            assert torch.equal(getattr(fam, name), getattr(arrays, name)), name
        assert torch.equal(fam.env_obstacle_bits, fixed.buf["obstacle_bits"].expand(E, 64))
        assert torch.equal(fam.reward_maps, fixed.reward_map.expand(E, 64, 64))
        total = fam.total_candidates()
        assert torch.equal(fam.cand_offset, arrays.cand_offset) and torch.equal(fam.n_valid, arrays.n_valid)
        assert torch.equal(fam.state_bits, arrays.state_bits)
        for name in ("cand_mask", "cand_lin"):
            assert torch.equal(getattr(fam, name)[:total], getattr(arrays, name)[:total]), name
    same()
    for _ in range(8):                                                     # across episode boundaries: the redraw changes nothing
        for v in (fam, arrays, fixed):
            v.select_random()
            v.step()
        same()
        assert torch.equal(fam.reward, fixed.reward) and torch.equal(fam.step_flags, fixed.step_flags)
    assert int(fam.task_episode.min()) >= 1


# ------------------------------------------------------------------------------------------------- lock-step parity
@pytest.mark.parametrize("shape,kind,sizes", [("trapezoid", "span", (1, 4)), ("hexagon", "tower", (1, 3))])
def test_lockstep_parity_across_episode_boundaries(shape, kind, sizes):
    E, seed, n_lock, max_steps = 32, 5, 20, 6
    lo, hi = sizes
    vec = family_env(E, kind, sizes, shape=shape, seed=seed, max_steps=max_steps)
    # one oracle per env: reset() installs the task of the episode that begins, the live obstacles alone
    live = lambda e, k: (lambda n, t, o: o[:n])(*draw_family(kind, seed, e, k, lo, hi))
    gyms = [EpisodeSetupGym(lambda k, e=e: live(e, k), lambda k, e=e: draw_family(kind, seed, e, k, lo, hi)[1],
                            shapes=[get_shape(shape)], max_steps=max_steps) for e in range(E)]
    oracles = [OracleLockstep(g) for g in gyms]
    for g in gyms:
        g.start_counting()
    assert_follows_the_draw(vec, kind, seed, lo, hi, [0] * E)
    counters, n_real, seen = [0] * E, 0, set()
    for it in range(n_lock):
        n_real += run_lockstep_parity(vec, oracles, seed, 1, counters)     # one lock-step: results, then the new candidates
        cls = assert_follows_the_draw(vec, kind, seed, lo, hi, [g.episode for g in gyms], it)
        seen |= set(cls.tolist())
        obits, tbits = vec.env_obstacle_bits.cpu().numpy(), vec.target_bits.cpu().numpy()
        for e, g in enumerate(gyms):
            assert canvas_equals(obits[e], g.obstacle_raster), (it, e)
            assert len(g.obstacles) == cls[e], (it, e)
    episodes = [g.episode for g in gyms]
    assert min(episodes) >= 2, episodes                                    # every env redrew its task at least twice
    assert seen == set(range(lo, hi + 1)) and n_real > E * (n_lock - 6)
    st = vec.read_stats()
    assert st["lp_errors"] == 0 and st["if_overflow"] == 0 and st["env_steps"] == n_real


# ------------------------------------------------------------------------------------------------- refusals, a later attach
def _set_family(vec, n_lo, n_hi, family=1, size=0.6, task_class="own"):
    from bridges_hip import abi
    cls = torch.zeros(vec.E, dtype=torch.int32, device=vec.device)
    fam = abi.TaskFamily()
    fam.family, fam.n_lo, fam.n_hi, fam.size, fam.x = family, n_lo, n_hi, size, 0.5
    fam.task_class = cls.data_ptr() if task_class == "own" else None
    rc = vec.L.bridges_env_set_task_family(vec._env, C.byref(fam))
    return rc, vec.L.bridges_last_error().decode(), cls


def test_set_task_family_refuses_what_it_cannot_draw_into():
    E = 4
    fixed = make_vec(E, [(0.6, 0, 0.3)], [(2.1, 0, 0.3)])                   # no task buffers
    rc, msg, _ = _set_family(fixed, 1, 1)
    assert rc == E_ARG and "no task buffers" in msg
    two = make_vec(E, np.zeros((E, 2, 3)), np.zeros((E, 2, 3)))             # n_targets == 2
    rc, msg, _ = _set_family(two, 1, 2)
    assert rc == E_ARG and "n_targets == 1" in msg
    slots = make_vec(E, np.zeros((E, 2, 3)), np.zeros((E, 1, 3)))           # n_obstacles == 2
    for n_hi in (1, 3):
        rc, msg, _ = _set_family(slots, 1, n_hi)
        assert rc == E_ARG and "n_obstacles == n_hi" in msg
    shared = make_vec(E, [], np.zeros((E, 1, 3)))                           # per-env targets, obstacles shared: n_obstacles == 0
    assert _set_family(shared, 1, 1)[0] == E_ARG
    for kw in (dict(n_lo=-1, n_hi=2), dict(n_lo=3, n_hi=2), dict(n_lo=0, n_hi=2, size=0.0), dict(n_lo=0, n_hi=2, family=3),
               dict(n_lo=0, n_hi=2, task_class=None)):
        assert _set_family(slots, **kw)[0] == E_ARG, kw
    assert _set_family(slots, 0, 5)[0] == E_ARG and _set_family(slots, 0, 0)[0] == E_ARG
    # what is allowed: set, then cleared by family 0 and by NULL
    rc, _, cls = _set_family(slots, 0, 2)
    assert rc == 0
    slots.reset()
    assert [int(v) for v in cls.cpu()] == [family_draw(0, e, 0, 0, 2) for e in range(E)]
    assert _set_family(slots, 0, 2, family=0)[0] == 0 and slots.L.bridges_env_set_task_family(slots._env, None) == 0
    before = slots.env_obstacles.clone()
    slots.reset()
    assert torch.equal(slots.env_obstacles, before)                          # cleared: the coordinates stay as written


def test_a_later_attach_returns_the_env_to_the_uniform_samplers():
    from bridges_hip.vec_env import RandomObstacles, RandomTargets
    E, seed, ranges = 16, 9, [((-3.0, 3.0), (0.3, 2.5))] * 2
    vec = family_env(E, "span", (1, 2), seed=seed)
    plain = make_vec(E, RandomObstacles(ranges), RandomTargets(1), seed=seed)
    for _ in range(3):
        vec.select_random()
        vec.step()
    vec._init_obstacles(RandomObstacles(ranges))
    vec._attach_task_buffers(RandomTargets(1))                              # bridges_env_set_task_buffers: the family is gone
    assert vec.task_family is None
    vec.reset()
    cls_before = vec.task_class.clone()
    for it in range(8):
        for name in ("env_targets", "env_obstacles", "task_episode", "target_bits", "reward_maps", "reward_prefix",
                     "env_obstacle_bits", "cand_offset", "n_valid", "state_bits"):
            assert torch.equal(getattr(vec, name), getattr(plain, name)), (it, name)
        total = vec.total_candidates()                                      # rows beyond it are left over from earlier states
        for name in ("cand_mask", "cand_lin"):
            assert torch.equal(getattr(vec, name)[:total], getattr(plain, name)[:total]), (it, name)
        for v in (vec, plain):
            v.select_random()
            v.step()
    assert int(vec.task_episode.max()) >= 1 and torch.equal(vec.task_class, cls_before)
    # set_targets on a family env detaches the family as it replaces a sampler
    fam = family_env(E, "tower", (1, 2), seed=seed)
    held = fam.env_targets.clone()
    fam.set_targets(held)
    assert fam.task_family is None and fam.per_env_tasks and fam.per_env_obstacles
    for _ in range(8):
        fam.select_random()
        fam.step()
    assert int(fam.task_episode.max()) == 0 and torch.equal(fam.env_targets, held)


# ------------------------------------------------------------------------------------------------- statistics by class
@pytest.mark.parametrize("count_first_only", [False, True])
def test_episode_stats_by_class_against_the_restatement(count_first_only):
    from robotoddler.training.episode_stats import EpisodeStats
    E, K, gamma, n_targets, n_classes = 300, 6, 0.95, 1, 5
    calls = _synthetic_calls(E, K, 24, seed=31 + count_first_only, n_targets=n_targets)
    rng = np.random.default_rng(77)
    cls = rng.choice([0, 1, 2, 4], E).astype(np.int32)                      # class 3 stays empty
    cls[17] = 9                                                            # one class out of range
    cls[255], cls[256], cls[299] = 4, 0, 2                                  # both sides of the 256-thread pass
    dev = torch.device(DEV)
    cls_d = torch.from_numpy(cls).to(dev)
    outs = []
    for _repeat in range(2):
        st = EpisodeStats(E, K, gamma, n_targets, dev, count_first_only=count_first_only, n_classes=n_classes)
        for rec, valid in calls:                                           # consecutive folds into the same sums
            st.fold(torch.from_numpy(rec).to(dev), torch.from_numpy(valid).to(dev), cls=cls_d)
        outs.append(st.out_by_class.cpu().numpy())
    ref = RestatedByClass(E, K, gamma, n_targets, n_classes, count_first_only)
    for rec, valid in calls:
        ref.fold(rec, valid, cls)
    for c in range(n_classes):
        print("class", c, "episodes", outs[0][c, 0], "sum reward", outs[0][c, 1], "restated", ref.sums()[c, 1])
    ref.check(outs[0])
    assert outs[0].tobytes() == outs[1].tobytes()                           # no atomics: the same bits every run
    assert outs[0][3, 0] == 0 and not outs[0][3].any() and all(outs[0][c, 0] > 0 for c in (0, 1, 2, 4))
    assert np.array_equal(st.counted.cpu().numpy(), ref.counted) and np.array_equal(st.run.cpu().numpy(), ref.run)
    assert ref.counted[17] > 0                                             # the env of no class still advances
    vals = st.take().get()
    assert vals["episodes"] == sum(len(e) for e in ref.episodes) and [c["episodes"] for c in vals["by_class"]] == [len(e) for e in ref.episodes]
    assert vals["by_class"][3]["success_rate"] is None and float(st.out_by_class.abs().sum()) == 0.0
    # one class, cls all zero: bridges_episode_stats bit for bit
    # (both sides are k_episode_stats<MAX_CLASSES> now; the independent evidence is test_gpu_twin_kernels_golden.py)
    from bridges_hip import ops
    one = EpisodeStats(E, K, gamma, n_targets, dev, count_first_only=count_first_only)
    out1, run1 = torch.zeros((1, 8), dtype=torch.float64, device=dev), torch.zeros((E, 2), dtype=torch.float32, device=dev)
    counted1, zero = torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
    for rec, valid in calls:
        r, v = torch.from_numpy(rec).to(dev), torch.from_numpy(valid).to(dev)
        one.fold(r, v)
        ops.episode_stats_by_class_(out1, r, v, one.gpow, n_targets, run1, counted1, zero, count_first_only)
    assert one.out.cpu().numpy().tobytes() == out1[0].cpu().numpy().tobytes() and float(one.out[0]) > 0
    assert torch.equal(one.run, run1) and torch.equal(one.counted, counted1)


# ------------------------------------------------------------------------------------------------- the loop
def make_agent(env, model, **kw):
    from robotoddler.training.vec_dqn import VecDQN
    if model == "SuccessorMLP":
        from test_gpu_vec_dqn_tasks import make_mlp
        pol, tgt = make_mlp(seed=4), make_mlp(seed=4)
        opt = torch.optim.Adam(pol.parameters(), lr=1e-4)
        return VecDQN(pol, tgt, opt, env, 4096, 16, 0.95, 0.01, "mse_q_values+mse_block_features", seed=3, per_env_tasks=True,
                      per_env_obstacles=True, episode_stats=True, **kw)
    from test_gpu_vec_dqn_conv_tasks import make_agent as conv_agent
    return conv_agent(env, model, capacity=4096, episode_stats=True, **kw)


def run_loop(model, kind, sizes, E=64, seed=21):
    from robotoddler.training import records as R
    env = family_env(E, kind, sizes, seed=seed, max_steps=4)
    agent = make_agent(env, model)
    hi = sizes[1]
    assert agent.episode_stats.n_classes == hi + 1 and agent.ring.width == R.RECORD_WIDTH + 3 + 3 * hi
    before = torch.cat([p.detach().flatten().clone() for p in agent.policy_net.parameters()])
    cap, inner_step, inner_act = {}, env.step, agent.act

    def step(sel_index=None):
        cap.update(targets=env.env_targets.clone(), obstacles=env.env_obstacles.clone(), cls=env.task_class.clone())
        inner_step(sel_index)

    def act(*a, **k):
        rec, valid = inner_act(*a, **k)
        cap["valid"] = valid
        return rec, valid

    env.step, agent.act = step, act
    losses, finished = [], np.zeros(hi + 1, dtype=np.int64)
    for _ in range(3):
        l, allrec = agent.lockstep(2)
        losses += l
        v = cap["valid"]
        assert allrec.shape[0] == int(v.sum())
        assert torch.equal(allrec[:, R.RECORD_WIDTH:R.RECORD_WIDTH + 3], cap["targets"].reshape(E, -1)[v])      # the pre-step task
        assert torch.equal(allrec[:, R.RECORD_WIDTH + 3:], cap["obstacles"].reshape(E, -1)[v])
        assert torch.equal(env._task_class, cap["cls"])
        done = (allrec[:, R.O_DONE] > 0.5).cpu().numpy()
        finished += np.bincount(cap["cls"][v].cpu().numpy()[done], minlength=hi + 1)
    stats = agent.episode_stats.take().get()
    assert [c["episodes"] for c in stats["by_class"]] == finished.tolist() and stats["episodes"] == int(finished.sum())
    after = torch.cat([p.detach().flatten() for p in agent.policy_net.parameters()])
    assert len(losses) == 6 and all(np.isfinite(losses)) and bool(torch.isfinite(after).all()) and not torch.equal(after, before)
    return agent, after


@pytest.mark.parametrize("model,kind,sizes", [("SuccessorMLP", "span", (1, 3)), ("ConvNet", "tower", (1, 2))])
def test_vec_dqn_trains_on_a_family_env(model, kind, sizes, monkeypatch):
    from robotoddler.training.vec_dqn import VecDQN
    lo, hi = sizes
    agent, weights = run_loop(model, kind, sizes)
    eval_seed, n_eval = 77, 16
    eval_env = family_env(n_eval, kind, sizes, seed=eval_seed, max_steps=4)
    ev = agent.evaluate(eval_env)
    want = np.bincount([family_draw(eval_seed, e, 0, lo, hi) for e in range(n_eval)], minlength=hi + 1)
    assert ev["episodes"] == n_eval == sum(ev["episodes_by_class"]) and ev["episodes_by_class"] == want.tolist()
    assert len(ev["success_by_class"]) == hi + 1 and ev["success_by_class"][0] is None
    assert all(s is None or 0.0 <= s <= 1.0 for s in ev["success_by_class"])
    # rows shared by (state, task) against every env's own rows: the same run
    monkeypatch.setattr(VecDQN, "DEDUP_STATES", False)
    _, own_rows = run_loop(model, kind, sizes)
    print(model, "max |w shared - w own rows|", float((weights - own_rows).abs().max()))
    assert torch.allclose(weights, own_rows, rtol=1e-5, atol=1e-5)


class _FakeAim:
    def __init__(self):
        self.calls = []

    def track(self, value, name=None, step=None, context=None):
        self.calls.append((name, value, step, context["context"]))


def test_the_cli_loop_trains_on_a_family_and_logs_success_per_span():
    from robotoddler.training import successor_dqn as S
    from robotoddler.training.vec_dqn import run_vectorised
    argv = ["--model", "SuccessorMLP", "--loss_function", "mse_q_values+mse_block_features", "--num_envs", "32", "--max_steps", "4",
            "--random_bridge_length", "1:2", "--num_episodes", "120", "--num_training_steps", "2", "--batch_size", "16", "--seed", "2",
            "--eval_envs", "8", "--evaluate_every", "50", "--shapes", "hexagon"]
    args = vars(S.build_parser().parse_args(argv))
    S.check_random_targets(args)
    aim = _FakeAim()
    hist, agent = run_vectorised(args, torch.device("cuda", 0), aim_run=aim, return_agent=True)
    env = agent.env
    assert env.task_family.kind == "span" and (env.task_family.lo, env.task_family.hi) == (1, 2) and env.n_obstacles == 2
    assert agent.per_env_tasks and agent.per_env_obstacles and agent.episode_stats.n_classes == 3
    assert agent.episodes_done >= 120 and all(np.isfinite(h["avg_loss"]) for h in hist if h["avg_loss"] is not None)
    by_class = np.array([h["episodes_by_class"] for h in hist])
    assert by_class[:, 0].sum() == 0 and (by_class[:, 1:].sum(axis=0) > 0).all()          # n = 0 is never drawn, 1 and 2 are
    assert by_class.sum() == sum(h["episodes_finished"] for h in hist) == agent.episodes_done
    for h in hist:
        assert len(h["success_by_class"]) == 3 and h["class_lo"] == 1
    evals = [h["evaluation"] for h in hist if "evaluation" in h]
    assert evals and all(sum(ev["episodes_by_class"]) == 8 and ev["episodes_by_class"][0] == 0 for ev in evals)
    assert evals[0]["episodes_by_class"] == evals[-1]["episodes_by_class"]                # the same held-out tasks every time
    for context in ("training", "evaluation"):
        names = {c[0] for c in aim.calls if c[3] == context}
        assert {"success_rate", "success_rate_n1", "success_rate_n2"} <= names and "success_rate_n0" not in names, (context, names)
        assert not any(n.endswith("_by_class") for n in names)
