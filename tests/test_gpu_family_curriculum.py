"""GPU: weighted class draws of a task family and the curriculum that adapts them on the device (bridges_family_draw,
bridges_family_thresholds, bridges_env_set_family_thresholds, bridges_family_curriculum; RandomBridges(weights=...),
VecAssemblyGym.set_family_weights, VecDQN(curriculum=...)).  Everything here is exact: classes, tables and weights are integers, and
the update's float64 steps are rounded one by one on both sides (tests/weighted_family_draw.py)."""
import numpy as np
import pytest
import torch

from family_draw import family_draw, family_task, family_word
from weighted_family_draw import curriculum_update, thresholds, weighted_family_draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev_thr(thr):
    return torch.tensor(thr, dtype=torch.int64, device=DEV)


def episodes_grid(E, n_ep):
    """(env ids, episodes) of E envs x episodes 0..n_ep-1 as one batch per episode."""
    return [(torch.full((E,), k, dtype=torch.int32, device=DEV), k) for k in range(n_ep)]


def make_vec(E, targets, max_steps=6, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    kw.setdefault("f32_rasters", False)
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [], targets, max_steps=max_steps, seed=seed, **kw)


# ------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("seed,counts", [(0, {1: 52, 3: 100, 4: 232}), (3, {1: 49, 3: 77, 4: 258})])
def test_family_draw_operator_is_the_restatement(seed, counts):
    from bridges_hip import ops
    E, lo, hi, weights = 64, 1, 4, (1, 0, 2, 5)
    thr = thresholds(weights)
    want = np.array([[weighted_family_draw(seed, e, k, lo, hi, thr) for e in range(E)] for k in range(6)])
    got_counts = {int(n): int((want == n).sum()) for n in np.unique(want)}
    print("classes of the restatement:", got_counts)
    assert got_counts == counts                          # every positive-weight class occurs, the zero-weight one never
    w_dev = torch.tensor(weights, dtype=torch.int32, device=DEV)
    thr_dev = ops.family_thresholds_(torch.zeros(3, dtype=torch.int64, device=DEV), w_dev)
    assert thr_dev.tolist() == thr                       # the table built on the device
    for ep, k in episodes_grid(E, 6):
        got = ops.family_draw(seed, 0, ep, lo, hi, thr_dev)
        assert got.dtype == torch.int32 and got.tolist() == want[k].tolist(), k
    # a batch that starts at another env id and mixes episodes; more than one workgroup and a ragged last one
    ep = torch.arange(300, dtype=torch.int32, device=DEV) % 7
    got = ops.family_draw(seed, 40, ep, lo, hi, thr_dev).tolist()
    assert got == [weighted_family_draw(seed, 40 + i, i % 7, lo, hi, thr) for i in range(300)]
    # no table: the uniform draw of tests/family_draw.py
    got = ops.family_draw(seed, 40, ep, lo, hi).tolist()
    assert got == [family_draw(seed, 40 + i, i % 7, lo, hi) for i in range(300)]


def test_threshold_comparison_direction():
    """u >= thr[k] counts: a threshold equal to an env's own u puts the env above it, u + 1 below."""
    from bridges_hip import ops
    seed, lo, hi = 0, 1, 4
    ep = torch.zeros(3, dtype=torch.int32, device=DEV)
    for e in range(3):
        u = family_word(seed, e, 0) >> 32
        at = ops.family_draw(seed, 0, ep, lo, hi, dev_thr([0, u, 1 << 32])).tolist()[e]
        above = ops.family_draw(seed, 0, ep, lo, hi, dev_thr([0, u + 1, 1 << 32])).tolist()[e]
        assert (at, above) == (3, 2), (e, u, at, above)


def test_extreme_thresholds():
    from bridges_hip import ops
    weights = (0, 0, 0, 0, 0, 0, 1, 0)
    thr = thresholds(weights)
    assert thr == [0] * 6 + [1 << 32]
    w_dev = torch.tensor(weights, dtype=torch.int32, device=DEV)
    thr_dev = ops.family_thresholds_(torch.zeros(7, dtype=torch.int64, device=DEV), w_dev)
    assert thr_dev.tolist() == thr
    for ep, _k in episodes_grid(64, 3):
        assert ops.family_draw(5, 0, ep, 0, 7, thr_dev).tolist() == [6] * 64


@pytest.mark.parametrize("weights", [(3, 3, 3), (1 << 20,) * 8, (0, 0, 0), (5,), (1 << 20, 0, 1), (7, 1, 0, 0, 65536)])
def test_thresholds_operator(weights):
    """Equal weights, the largest weights, the zero sum (the device's fall-back: equal weights), one class, zeros at the end."""
    from bridges_hip import ops
    w_dev = torch.tensor(weights, dtype=torch.int32, device=DEV)
    thr_dev = ops.family_thresholds_(torch.full((len(weights) - 1,), -1, dtype=torch.int64, device=DEV), w_dev)
    assert thr_dev.tolist() == thresholds(weights)


# ------------------------------------------------------------------------------------------------- the env
TASK_TENSORS = ("task_class", "env_targets", "env_obstacles", "target_bits", "env_obstacle_bits")


@pytest.mark.parametrize("kind,sizes", [("span", (1, 4)), ("tower", (0, 3))])
def test_equal_weights_are_a_no_op(kind, sizes):
    from bridges_hip.vec_env import RandomBridges
    E = 8
    plain = make_vec(E, RandomBridges(kind, sizes=sizes))
    equal = make_vec(E, RandomBridges(kind, sizes=sizes, weights=(5, 5, 5, 5)))
    assert plain.family_weights is None and plain.family_thresholds is None
    assert equal.family_weights.tolist() == [5, 5, 5, 5] and equal.family_thresholds.tolist() == [1 << 30, 1 << 31, 3 << 30]

    def same(tag):
        for name in TASK_TENSORS + ("task_episode", "reward", "step_flags"):
            assert torch.equal(getattr(plain, name), getattr(equal, name)), (tag, name)
    same("reset")
    for it in range(12):                                 # one selection for both: the policy stream of (seed, env)
        for v in (plain, equal):
            v.select_random()
            v.step()
        same(it)
    assert int(plain.task_episode.min()) >= 1


def test_weighted_env_follows_the_restatement():
    from bridges_hip.vec_env import RandomBridges
    E, seed, lo, hi, kind = 8, 0, 1, 4, "span"
    first, second = (1, 0, 2, 5), (0, 4, 0, 1)
    vec = make_vec(E, RandomBridges(kind, sizes=(lo, hi), weights=first), seed=seed)
    assert vec.family_weights.tolist() == list(first) and vec.family_thresholds.tolist() == thresholds(first)
    table = [thresholds(first)] * E                      # the table every env's CURRENT episode was drawn under
    episode = [0] * E

    def check(tag):
        ep, cls = vec.task_episode.tolist(), vec.task_class.tolist()
        tg, ob = vec.env_targets.cpu().numpy(), vec.env_obstacles.cpu().numpy()
        for e in range(E):
            if ep[e] != episode[e]:                      # the env began an episode in this lock-step: under the table of now
                assert ep[e] == episode[e] + 1, (tag, e)
                episode[e], table[e] = ep[e], current[0]
            n = weighted_family_draw(seed, e, ep[e], lo, hi, table[e])
            assert cls[e] == n, (tag, e, ep[e], cls[e], n)
            targets, obstacles = family_task(kind, n, hi)
            assert np.array_equal(tg[e], np.array(targets)) and np.array_equal(ob[e], np.array(obstacles)), (tag, e)
        return cls

    current = [thresholds(first)]
    seen = set(check("reset"))
    for it in range(10):
        vec.select_random()
        vec.step()
        seen |= set(check(it))
    assert 2 not in seen and max(episode) >= 1
    vec.set_family_weights(second)                       # mid-run: no reset, only episodes that begin afterwards change
    current[0] = thresholds(second)
    assert vec.family_thresholds.tolist() == current[0]
    before = list(episode)
    check("after set_family_weights")                    # nothing moved: every env still holds the task it had
    assert episode == before
    late = set()
    for it in range(14):
        vec.select_random()
        vec.step()
        cls = check(("second", it))
        late |= {cls[e] for e in range(E) if table[e] is current[0]}
    assert late and late <= {2, 4}
    vec.set_family_weights(None)                         # back to the uniform draw
    assert vec.family_weights is None and vec.family_thresholds is None
    current[0] = None
    for it in range(8):
        vec.select_random()
        vec.step()
        check(("uniform", it))
    assert any(t is None for t in table)


def test_thresholds_need_a_family():
    from bridges_hip import abi
    from bridges_hip.vec_env import RandomBridges, RandomTargets
    vec = make_vec(4, RandomTargets(1))
    buf = torch.zeros(3, dtype=torch.int64, device=DEV)
    assert vec.L.bridges_env_set_family_thresholds(vec._env, buf.data_ptr()) == -1       # BRIDGES_E_ARG
    assert b"no task family" in vec.L.bridges_last_error()
    with pytest.raises(ValueError):
        vec.set_family_weights((1, 1))
    fam = make_vec(4, RandomBridges("span", sizes=(1, 2), weights=(1, 3)))
    assert fam.family_thresholds.tolist() == [1 << 30]
    fam.set_targets(fam.env_targets.clone())             # explicit targets drop the family, and its table with it
    assert fam.task_family is None and fam.family_weights is None and fam.family_thresholds is None
    assert fam.L.bridges_env_set_family_thresholds(fam._env, buf.data_ptr()) == -1
    assert abi.FAMILY_MAX_CLASSES == 8


# ------------------------------------------------------------------------------------------------- the update kernel
def run_update(sums, state, lo, hi, beta, w_min, min_episodes):
    """One update on the device and in the restatement, on copies -> ((sums, state, w, thr) of the device, the same restated)."""
    from bridges_hip import ops
    C_ = hi - lo + 1
    s_dev = torch.tensor(sums, dtype=torch.float64, device=DEV)
    st_dev = torch.tensor(state, dtype=torch.float64, device=DEV)
    w_dev = torch.full((C_,), -1, dtype=torch.int32, device=DEV)
    thr_dev = torch.full((C_ - 1,), -1, dtype=torch.int64, device=DEV)
    ops.family_curriculum_(s_dev, st_dev, lo, hi, beta, w_min, min_episodes, w_dev, thr_dev)
    s_ref, st_ref = [list(r) for r in sums], [list(r) for r in state]
    w_ref, thr_ref = curriculum_update(s_ref, st_ref, lo, hi, beta, w_min, min_episodes)
    return (s_dev.tolist(), st_dev.tolist(), w_dev.tolist(), thr_dev.tolist()), (s_ref, st_ref, w_ref, thr_ref)


def test_curriculum_update_bit_for_bit():
    lo, hi, beta, w_min, min_ep = 1, 4, 0.3, 6554, 4
    row = lambda e, s: [float(e), 1.25, 2.5, 3.0 * e, float(e), float(s), 0.0, 0.0]
    sums = [row(9, 7),              # class 0: outside the family -- rubbish that must be ignored and kept
            [0.0] * 8,              # class 1: never seen
            row(12, 12),            # class 2: all success
            row(7, 0),              # class 3: all fail
            row(3, 1)]              # class 4: below min_episodes, the row survives
    state = [[0.77, 1.0]] + [[0.0, 0.0]] * 4
    got, want = run_update(sums, state, lo, hi, beta, w_min, min_ep)
    assert got == want
    g_sums, g_state, g_w, _ = got
    assert g_sums[0] == sums[0] and g_state[0] == state[0]
    assert g_sums[2] == [0.0] * 8 and g_sums[3] == [0.0] * 8 and g_sums[4] == sums[4]
    assert g_w == [w_min + 65536, w_min, w_min + 65536, w_min + 65536]
    assert g_state[1:] == [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]]
    # a second call on the output of the first: the EMA branch, with rates that are no short binary fractions
    sums2 = [list(r) for r in g_sums]
    sums2[1], sums2[2], sums2[3], sums2[4][0], sums2[4][5] = row(7, 3), row(9, 2), row(11, 4), sums2[4][0] + 4.0, sums2[4][5] + 2.0
    got2, want2 = run_update(sums2, g_state, lo, hi, beta, w_min, min_ep)
    assert got2 == want2
    ema2 = 1.0 + 0.3 * (2.0 / 9.0 - 1.0)
    assert got2[1][2] == [ema2, 1.0] and got2[1][1] == [3.0 / 7.0, 1.0] and got2[1][4] == [3.0 / 7.0, 1.0]
    assert got2[0][1:] == [[0.0] * 8] * 4                # every consumed row zeroed
    # a third, with nothing new: the table stays what the state says
    got3, want3 = run_update(got2[0], got2[1], lo, hi, beta, w_min, min_ep)
    assert got3 == want3 and got3[2] == got2[2] and got3[3] == got2[3]


def test_curriculum_update_of_one_class():
    got, want = run_update([[0.0] * 8, [0.0] * 8, [5.0, 0, 0, 0, 0, 2.0, 0, 0]], [[0.0, 0.0]] * 3, 2, 2, 0.25, 1, 1)
    assert got == want and got[2] == [1 + int((1.0 - 0.4) * 65536.0 + 0.5)] and got[3] == []


# ------------------------------------------------------------------------------------------------- the loop
LOOP = dict(E=64, sizes=(1, 3), env_seed=21, every=2, min_episodes=1, beta=0.25, floor=0.1)


def make_loop(curriculum="on", episode_stats=True):
    """SuccessorMLP agent on RandomBridges("span", (1, 3)); curriculum "on" | None | "absent" (the argument not given at all)."""
    from bridges_hip.vec_env import RandomBridges
    from robotoddler.training.vec_dqn import Curriculum, VecDQN
    from test_gpu_vec_dqn_tasks import make_mlp
    env = make_vec(LOOP["E"], RandomBridges("span", sizes=LOOP["sizes"]), max_steps=4, seed=LOOP["env_seed"])
    pol, tgt = make_mlp(seed=4), make_mlp(seed=4)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-4)
    kw = {}
    if curriculum == "on":
        kw["curriculum"] = Curriculum(beta=LOOP["beta"], floor=LOOP["floor"], every=LOOP["every"], min_episodes=LOOP["min_episodes"])
    elif curriculum is None:
        kw["curriculum"] = None
    agent = VecDQN(pol, tgt, opt, env, 4096, 16, 0.95, 0.01, "mse_q_values+mse_block_features", seed=3, per_env_tasks=True,
                   per_env_obstacles=True, episode_stats=episode_stats, **kw)
    return env, agent, opt


def table_of(agent):
    c = agent.curriculum
    return c.w.tolist(), c.thr.tolist(), c.state.tolist(), c.sums.tolist()


@pytest.fixture(scope="module")
def curriculum_run(tmp_path_factory):
    """ONE run of 8 lock-steps with the curriculum on, shared by the tests below: the class history, the table after every
    lock-step, the table restated from an independent fold of the same records, and a checkpoint taken after lock-step 4."""
    from robotoddler.training import train_step as T
    from robotoddler.training.episode_stats import EpisodeStats
    from robotoddler.utils.utils import save_checkpoint
    env, agent, opt = make_loop()
    lo, hi = LOOP["sizes"]
    w0 = 6554 + 65536
    assert agent.curriculum.settings.w_min == 6554 and env.family_weights.tolist() == [w0] * 3
    assert env.family_thresholds.tolist() == thresholds([1, 1, 1])
    own = EpisodeStats(env.E, env.K, 0.95, env.n_targets, env.device, across_ranks=False, n_classes=hi + 1)
    inner_act = agent.act

    def act(*a, **k):
        rec, valid = inner_act(*a, **k)
        own.fold(rec, valid, cls=env._task_class)
        return rec, valid
    agent.act = act
    sums, state = [[0.0] * 8 for _ in range(hi + 1)], [[0.0, 0.0] for _ in range(hi + 1)]
    want_w, want_thr = [w0] * 3, thresholds([1, 1, 1])
    classes, tables, restated, ckpt = [], [], [], str(tmp_path_factory.mktemp("curriculum_ckpt"))
    for it in range(1, 9):
        agent.lockstep(2)
        if it == 3:
            agent.episode_stats.take()                   # the logging statistics' cadence is none of the curriculum's business
        if it % LOOP["every"] == 0:
            new = own.out_by_class.tolist()
            own.out_by_class.zero_()
            sums = [[a + b for a, b in zip(r, n)] for r, n in zip(sums, new)]
            want_w, want_thr = curriculum_update(sums, state, lo, hi, LOOP["beta"], 6554, LOOP["min_episodes"])
        classes.append(env.task_class.tolist())
        tables.append(table_of(agent))
        restated.append((list(want_w), list(want_thr), [list(r) for r in state], [list(r) for r in sums]))
        if it == 4:
            T.sync_optimizer(agent.policy_net)
            save_checkpoint(ckpt, agent.policy_net, agent.target_net, agent.ring, opt, agent.episodes_done, {})
            agent.save_extra(ckpt + "/latest/agent.pt", lockstep=it)
            env.reset()                                  # as run_vectorised: a resumed run starts from fresh environments
    return dict(classes=classes, tables=tables, restated=restated, ckpt=ckpt + "/latest")


def test_loop_table_is_the_restatement_of_an_independent_fold(curriculum_run):
    for it, (got, want) in enumerate(zip(curriculum_run["tables"], curriculum_run["restated"]), 1):
        assert got == want, it
    w_last = curriculum_run["tables"][-1][0]
    assert any(w != 6554 + 65536 for w in w_last)        # episodes ended and moved the weights
    assert all(6554 <= w <= 6554 + 65536 for w in w_last)


def test_loop_is_reproducible(curriculum_run):
    env, agent, _ = make_loop()
    for it in range(1, 5):
        agent.lockstep(2)
        assert env.task_class.tolist() == curriculum_run["classes"][it - 1], it
        assert table_of(agent) == curriculum_run["tables"][it - 1], it


def test_loop_resumes_from_a_checkpoint(curriculum_run):
    from robotoddler.utils.utils import load_checkpoint
    env, agent, opt = make_loop()
    load_checkpoint(curriculum_run["ckpt"], agent.policy_net, agent.target_net, agent.ring, opt)
    assert agent.load_extra(curriculum_run["ckpt"] + "/agent.pt") == dict(lockstep=4)
    assert table_of(agent) == curriculum_run["tables"][3]
    env.reset()
    for it in range(5, 9):
        agent.lockstep(2)
        assert env.task_class.tolist() == curriculum_run["classes"][it - 1], it
        assert table_of(agent) == curriculum_run["tables"][it - 1], it


def test_no_curriculum_is_the_loop_as_it_was():
    runs = []
    for mode in (None, "absent"):
        env, agent, _ = make_loop(curriculum=mode)
        assert agent.curriculum is None and env.family_weights is None and env.family_thresholds is None
        for _ in range(4):
            agent.lockstep(2)
        runs.append((torch.cat([p.detach().flatten() for p in agent.policy_net.parameters()]), env.task_class.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_curriculum_needs_a_family():
    from bridges_hip.vec_env import RandomTargets
    from robotoddler.training.curriculum import Curriculum, CurriculumRun
    with pytest.raises(ValueError, match="task family"):
        CurriculumRun(Curriculum(), make_vec(4, RandomTargets(1)), 0.95)
