"""GPU: VecDQN.particle_search and the search in training with search_sampler="particles", on the small SuccessorMLP (hidden [8])
of tests/test_gpu_vec_dqn_beam.py, a beam env of 4 tasks, max_steps 6.  Width 1 with the elite is beam_search(width=1); equal
generator states give equal searches; the returned structures replay to what the search reports; without resampling no live
particle is lost or moved; the traced rows are those of tests/beam_trace_ref.py fed what the search kept; the loop pushes the traced
rows behind its own; the particle search waits for the device where the beam search waits; and with the option off nothing moves."""
import numpy as np
import pytest
import torch

import beam_trace_ref as TR
import test_gpu_vec_dqn_beam as BT
import test_gpu_vec_dqn_search as ST

pytestmark = pytest.mark.gpu
DEV = "cuda"
TASKS, INF = 4, float("inf")
NEW_KEYS = ("particles", "ess_by_depth", "p_sel_mean_by_depth")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _envs(width, seed=77):
    from robotoddler.training.vec_dqn import beam_env_like
    eval_env = BT.random_env(TASKS, seed=seed)
    return eval_env, beam_env_like(eval_env, width)


def _same_numbers(a, b):
    assert {k: v for k, v in a.items() if k not in NEW_KEYS and k != "beam_width"} == \
           {k: v for k, v in b.items() if k not in NEW_KEYS and k != "beam_width"}
    for x, y in zip(a["structures"], b["structures"]):
        assert np.float64(x["lin_reward"]).tobytes() == np.float64(y["lin_reward"]).tobytes()
        assert np.float64(x["reward"]).tobytes() == np.float64(y["reward"]).tobytes()


def test_width_1_with_the_elite_is_the_beam_search_of_width_1():
    agent = BT.make_agent()
    _eval_env, env = _envs(1)
    want = agent.beam_search(env, 1)
    got = agent.particle_search(env, 1, 0.5, elite=True)
    assert set(got) - set(want) == set(NEW_KEYS) and got["particles"] == 1 and got["beam_width"] == want["beam_width"] == 1
    _same_numbers(got, want)
    n = len(got["ess_by_depth"])
    # one particle, the elite: ess 1 and p_sel 1 wherever a task is still open (0: a depth at which every task had ended)
    assert 1 <= n <= env.K and got["ess_by_depth"][0] == 1.0 and set(got["ess_by_depth"]) <= {0.0, 1.0}
    assert got["p_sel_mean_by_depth"] == got["ess_by_depth"]


def test_equal_generator_states_give_equal_searches_and_another_seed_differs():
    agent = BT.make_agent()
    _eval_env, env = _envs(4)
    kw = dict(temperature=1.0, resample_temperature=2.0, elite=False)
    a = agent.particle_search(env, 4, generator=_gen(5), **kw)
    b = agent.particle_search(env, 4, generator=_gen(5), **kw)
    assert a == b
    others = [agent.particle_search(env, 4, generator=_gen(s), **kw) for s in (6, 7, 8)]
    assert any([s["actions"] for s in o["structures"]] != [s["actions"] for s in a["structures"]] for o in others)
    # the stream of the agent's own: made by the first search that needs it, moved by every search, nobody else's
    assert agent.search_gen is None
    before = (agent.sample_gen.get_state().clone(), agent.explore_gen.get_state().clone())
    c = agent.particle_search(env, 4, **kw)
    state = agent.search_gen.get_state().clone()
    d = agent.particle_search(env, 4, **kw)
    assert not torch.equal(agent.search_gen.get_state(), state)
    assert torch.equal(agent.sample_gen.get_state(), before[0]) and torch.equal(agent.explore_gen.get_state(), before[1])
    agent.search_gen.set_state(state)
    assert agent.particle_search(env, 4, **kw) == d and c["particles"] == 4
    open_depths = [d for d, e in enumerate(c["ess_by_depth"]) if e > 0.0]       # (0: every task had ended before that depth)
    assert open_depths[0] == 0 and c["ess_by_depth"][0] == 1.0                  # depth 0: one parent per group
    assert all(1.0 <= c["ess_by_depth"][d] <= 4.0 and 0.0 < c["p_sel_mean_by_depth"][d] <= 1.0 for d in open_depths)


@pytest.mark.parametrize("kw", [dict(temperature=0.5), dict(temperature=1.0, resample_temperature=INF, elite=False),
                                dict(temperature=0.25, resample_temperature=0.05, merge=True)])
def test_structures_replay_to_what_the_search_reports(kw):
    agent = BT.make_agent()
    eval_env, env = _envs(4)
    res = agent.particle_search(env, 4, generator=_gen(11), **kw)
    BT.check_replay(eval_env, res)
    assert res["episodes"] == TASKS and res["particles"] == 4


def test_without_resampling_no_live_particle_is_lost_or_moved():
    """T_r = inf and no elite: the weights are all 1, so every live env of a group is the parent of at least one slot, and in a
    group whose B envs are all live the parents are the identity (the exact property of the rule); only the slots of closed envs
    are refilled."""
    agent = BT.make_agent()
    _eval_env, env = _envs(4)
    E, B = env.E, 4
    parent_buf = agent._trace_buffers(E, env.K)[2]
    lives, parents = [], []

    def on_depth(d, live):
        lives.append(live.clone())
        parents.append(parent_buf[d].clone())
    agent.particle_search(env, B, 1.0, INF, elite=False, on_depth=on_depth, trace=True, generator=_gen(3))
    assert len(lives) >= 2
    own = np.arange(E)
    assert (parents[0].cpu().numpy() == own // B * B).all()                     # depth 0: slot 0 of every group fans out
    full = kept = 0
    for d in range(1, len(lives)):
        live, src = lives[d - 1].cpu().numpy().astype(bool), parents[d].cpu().numpy()
        for g in range(E // B):
            sl = slice(g * B, (g + 1) * B)
            if not live[sl].any():
                continue
            assert set(own[sl][live[sl]]) == set(src[sl]), (d, g)               # every live env continues, nothing else does
            kept += 1
            if live[sl].all():
                assert (src[sl] == own[sl]).all(), (d, g)
                full += 1
    assert full > 0 and kept > full                                             # both kinds of group were seen


@pytest.mark.parametrize("n_step", [1, 3])
def test_traced_rows_are_the_reference_fed_what_the_search_kept(n_step):
    agent = BT.make_agent()
    eval_env, env = _envs(4)
    res = agent.particle_search(env, 4, 0.5, 0.2, elite=False, trace=True, trace_n_step=n_step, trace_priority=0.25, generator=_gen(21))
    rec, valid, parent = (t.cpu().numpy().copy() for t in agent._trace_buffers(env.E, env.K))
    steps = [s["num_steps"] for s in res["structures"]]
    case = dict(B=4, n_step=n_step, gamma=BT.GAMMA, priority=0.25, rec=rec, valid=valid, parent=parent,
                end_env=res["trace_end_env"].cpu().numpy(), end_depth=np.asarray(steps, np.int32) - 1,
                tail=np.ascontiguousarray(env.env_targets.reshape(env.E, -1).cpu().numpy()))
    want = TR.reference(case)
    n = sum(steps)
    assert res["trace_count"] == n == int(want["offset"][-1]) and not want["status"].any()
    got = res["trace_rows"].cpu().numpy()
    assert got.shape == (n, agent.ring.width + (n_step > 1)) and got.tobytes() == want["rows"][:n].tobytes()
    assert res["trace_offset"].cpu().numpy().tobytes() == want["offset"].tobytes() and not res["trace_status"].any().item()
    # the premise: some best path changes slot, or a trace by slot would pass
    paths = ST._best_path_slots(agent, env, res)
    assert any(a != b for p in paths for a, b in zip(p, p[1:])), paths
    # ... and an untraced search returns the same numbers
    plain = agent.particle_search(env, 4, 0.5, 0.2, elite=False, generator=_gen(21))
    assert {k: v for k, v in res.items() if k not in ST.TRACE_KEYS} == plain


def test_the_loop_pushes_the_particle_rows_behind_its_own():
    agent = ST.make_loop_agent(search_every=2, search_tasks=4, search_width=4, search_sampler="particles", search_temperature=0.5,
                               search_resample_temperature=1.0)
    inner, seen, log = agent.particle_search, [], []

    def recording(*a, **kw):
        assert kw["trace"] and a[2:] == (0.5, 1.0)
        res = inner(*a, **kw)
        seen.append((agent.ring.head, res["trace_count"], res["trace_rows"].clone()))
        return res
    agent.particle_search = recording
    agent.beam_search = None                                                    # (the option replaces it)
    for _ in range(4):
        head = agent.ring.head
        _losses, own = agent.lockstep(1)
        log.append((head, len(own), agent.ring.head, agent.last_search))
    assert [s is not None for *_x, s in log] == [False, True, False, True] and len(seen) == 2
    data = agent.ring.data
    for (head, n_own, head_after, last), (head_at_search, count, rows) in zip(log[1::2], seen):
        assert head_at_search == head + n_own and count > 0 and head_after == head_at_search + count
        assert last["search_rows"] == count and torch.equal(data[head_at_search:head_after], rows)
    for head, n_own, head_after, last in log[0::2]:
        assert head_after == head + n_own
    assert agent.search_rows == sum(c for _h, c, _r in seen)


def test_the_particle_search_waits_where_the_beam_search_waits():
    agent = BT.make_agent()
    _eval_env, env = _envs(4)
    for _ in range(2):
        agent.beam_search(env, 4)
        agent.particle_search(env, 4, 0.5)
    BT._waits(lambda: agent.beam_search(env, 4))                                # (the first call under the debug mode reports one more)
    w_beam = sorted(BT._waits(lambda: agent.beam_search(env, 4)))
    w_part = sorted(BT._waits(lambda: agent.particle_search(env, 4, 0.5)))
    print("waits: beam", w_beam, "particles", w_part)
    # both run env.K depths (a closed slot resets and holds candidates again): acting's wait for the row count per depth, one
    # read-back at the end, and the particle search nothing beyond
    assert w_part == w_beam, (w_part, w_beam)
    assert w_part.count("stream") == env.K and w_part.count("event") == w_part.count("device") == 0


def test_with_the_option_off_nothing_moves(monkeypatch):
    """Ring, losses and parameters after 6 lock-steps: an agent given the new arguments as None against one built without them,
    and the plain loop against the hash test_gpu_vec_dqn_search.py keeps of the loop before any search existed."""
    from bridges_hip import ops

    def refuse(*a, **k):
        raise AssertionError("an agent without search_sampler launched bridges_particle_select")
    monkeypatch.setattr(ops, "particle_select", refuse)
    plain = ST.make_loop_agent()
    assert plain.search_sampler is None and plain.search_gen is None
    assert ST._ring_hash(plain) == ST.RING_BEFORE and plain.search_gen is None

    def run(**kw):
        agent = ST.make_loop_agent(search_every=2, search_tasks=4, search_width=4, **kw)
        losses = [agent.lockstep(1)[0] for _ in range(6)]
        torch.cuda.synchronize()
        params = torch.cat([p.detach().flatten() for p in agent.policy_net.parameters()]).cpu().numpy().tobytes()
        return agent.ring.data.cpu().numpy().tobytes(), agent.ring.head, np.asarray(losses, np.float64).tobytes(), params, agent.search_rows
    assert run() == run(search_sampler=None, search_temperature=None, search_resample_temperature=None)
