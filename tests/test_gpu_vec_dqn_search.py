"""GPU: VecDQN.beam_search(trace=True) and the search in training (VecDQN(search_every=N)) on the small SuccessorMLP (hidden [8]) of
tests/test_gpu_vec_dqn_beam.py, max_steps 6.  A traced search returns what an untraced one returns; its rows are the records of
every task's returned actions replayed in a fresh env (one-step: bit for bit; three-step: through bridges_nstep_fold, O_LIN within
the window's bound) -- after the premise that a best path changes slot, without which a trace by slot would pass; the same with
merging, per-env obstacles and a ConvNet on task channels.  The loop pushes exactly the traced rows behind its own, leaves every
other piece of training state alone, trains on them under n_step = 3, gives them search_priority under prioritised replay, adds the
host waits of one search and nothing else, checkpoints its phase; and an agent without the option fills the ring it always filled."""
import hashlib
import math

import numpy as np
import pytest
import torch

import test_gpu_vec_dqn_beam as BT

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAMMA = BT.GAMMA
TRACE_KEYS = ("trace_rows", "trace_count", "trace_offset", "trace_status", "trace_end_env")


def _tail(agent, env):
    E = env.E
    if not agent.per_env_tasks:
        return np.zeros((E, 0))
    t = env.env_targets.reshape(E, -1)
    if agent.per_env_obstacles:
        t = torch.cat([t, env.env_obstacles.reshape(E, -1)], dim=1)
    return t.cpu().numpy()


def replay_records(agent, eval_env, structures):
    """Every task's returned actions in a fresh env of one env per task, recorded with the two launches acting uses -> per task
    the list of its records, each followed by the task tail."""
    from robotoddler.training import records as R
    from robotoddler.training.vec_dqn import beam_env_like
    env = beam_env_like(eval_env, 1)
    E = env.E
    env.reset()
    tail = _tail(agent, env)
    recs = [[] for _ in range(E)]
    for d in range(env.K):
        off, mask = env.cand_offset.cpu().numpy(), env.cand_mask.cpu().numpy()
        first_valid = [int(np.argmax(mask[off[e]:off[e + 1]])) if off[e + 1] > off[e] else 0 for e in range(E)]
        a = torch.tensor([s["actions"][d] if d < s["num_steps"] else first_valid[e] for e, s in enumerate(structures)],
                         dtype=torch.int32, device=DEV)
        rec = R.pack_state(env, env.cand_offset[:E].long() + a.long())
        env.step(a)
        valid = R.pack_result(env, rec).cpu().numpy()
        rec = rec.cpu().numpy()
        for e, s in enumerate(structures):
            if d < s["num_steps"]:
                assert valid[e] and (rec[e, R.O_DONE] > 0.5) == (d == s["num_steps"] - 1), (e, d)
                recs[e].append(np.concatenate([rec[e], tail[e]]))
    return recs


def expected_rows(recs, n_step, priority):
    """-> (rows, g_bound per row).  n_step = 1: the records with the priority in O_TD.  n_step > 1: the records through
    bridges_nstep_fold, one env per task, in the order the fold emits them, task after task."""
    from bridges_hip import dqn_ops
    from robotoddler.training import records as R
    M, W = len(recs), len(recs[0][0])
    if n_step == 1:
        rows = np.array([r for task in recs for r in task])
        rows[:, R.O_TD] = priority
        return rows, np.zeros(len(rows))
    depth = max(len(t) for t in recs)
    window = (torch.zeros(M, dtype=torch.int32, device=DEV), *(torch.zeros((M, n_step), dtype=torch.float64, device=DEV) for _ in range(4)))
    emitted = [[] for _ in range(M)]
    for d in range(depth):
        rec = np.array([t[d] if d < len(t) else np.zeros(W) for t in recs])
        rec[:, R.O_TD] = priority
        valid = torch.tensor([d < len(t) for t in recs], device=DEV)
        out, out_valid = dqn_ops.nstep_fold(torch.from_numpy(rec).to(DEV), valid, GAMMA, n_step, *window)
        out, out_valid = out.cpu().numpy(), out_valid.cpu().numpy()
        for e in range(M):
            emitted[e] += [out[e * n_step + r] for r in range(n_step) if out_valid[e * n_step + r]]
    bounds = []
    for e, task in enumerate(recs):
        assert len(emitted[e]) == len(task)
        for t in range(len(task)):
            h = min(n_step, len(task) - t)
            bounds.append(2 * h * 2.0 ** -53 * math.fsum(abs(GAMMA ** k * task[t + k][R.O_LIN]) for k in range(h)))
    return np.array([r for task in emitted for r in task]), np.array(bounds)


def check_rows(res, want, g_bound, what):
    from robotoddler.training import records as R
    n = res["trace_count"]
    got = res["trace_rows"].cpu().numpy()
    assert n == sum(s["num_steps"] for s in res["structures"]) == int(res["trace_offset"][-1]) == len(want), what
    assert got.shape == want.shape and int(res["trace_status"].sum()) == 0, (what, got.shape, want.shape)
    cols = np.ones(got.shape[1], dtype=bool)
    cols[R.O_LIN] = bool(np.all(g_bound == 0))
    g, w = np.ascontiguousarray(got[:, cols]).view(np.uint64), np.ascontiguousarray(want[:, cols]).view(np.uint64)
    bad = np.argwhere(g != w)
    assert not len(bad), (what, "rows differ first at (row, kept column)", bad[0].tolist())
    assert np.all(np.abs(got[:, R.O_LIN] - want[:, R.O_LIN]) <= g_bound), what


def test_a_traced_search_returns_what_an_untraced_one_returns():
    from robotoddler.training.vec_dqn import beam_env_like
    agent = BT.make_agent()
    beam_env = beam_env_like(BT.random_env(BT.M, seed=77), 4)
    for merge in (False, True):
        plain = agent.beam_search(beam_env, 4, merge=merge)
        traced = agent.beam_search(beam_env, 4, merge=merge, trace=True, trace_n_step=3, trace_priority=0.5)
        assert set(traced) - set(plain) == set(TRACE_KEYS)
        assert {k: v for k, v in traced.items() if k not in TRACE_KEYS} == plain
        for a, b in zip(plain["structures"], traced["structures"]):
            assert np.float64(a["lin_reward"]).tobytes() == np.float64(b["lin_reward"]).tobytes()
            assert np.float64(a["reward"]).tobytes() == np.float64(b["reward"]).tobytes()
    with pytest.raises(ValueError, match="trace_n_step"):
        agent.beam_search(beam_env, 4, trace=True, trace_n_step=9)


def _best_path_slots(agent, beam_env, res):
    """The slots every task's best path went through: the parents the search kept, walked back from the end it named."""
    parent = agent._trace_buffers(beam_env.E, beam_env.K)[2].cpu().numpy()
    ends = res["trace_end_env"].cpu().numpy()
    paths = []
    for m, s in enumerate(res["structures"]):
        e, path = int(ends[m]), []
        for t in range(s["num_steps"] - 1, -1, -1):
            path.append(e)
            if t:
                e = int(parent[t, e])
        paths.append(path[::-1])
    return paths


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("n_step", [1, 3])
def test_traced_rows_are_the_replayed_records(n_step, merge):
    from robotoddler.training.vec_dqn import beam_env_like
    agent = BT.make_agent()
    eval_env = BT.random_env(BT.M, seed=77)
    beam_env = beam_env_like(eval_env, 4)
    res = agent.beam_search(beam_env, 4, merge=merge, trace=True, trace_n_step=n_step, trace_priority=0.25)
    # the premise: a best path changes slot between two depths (or a trace by slot would pass)
    paths = _best_path_slots(agent, beam_env, res)
    assert any(a != b for p in paths for a, b in zip(p, p[1:])), paths
    BT.check_replay(eval_env, res)
    want, g_bound = expected_rows(replay_records(agent, eval_env, res["structures"]), n_step, 0.25)
    check_rows(res, want, g_bound, (n_step, merge))
    assert res["trace_rows"].shape[1] == agent.ring.width + (n_step > 1)


def test_traced_rows_on_per_env_obstacles():
    from robotoddler.training.vec_dqn import beam_env_like
    agent = BT.make_agent(O=1)
    eval_env = BT.random_env(BT.M, O=1, seed=78)
    res = agent.beam_search(beam_env_like(eval_env, 2), 2, trace=True)
    want, g_bound = expected_rows(replay_records(agent, eval_env, res["structures"]), 1, 0.0)
    check_rows(res, want, g_bound, "obstacles")
    assert res["trace_rows"].shape[1] == agent.ring.width == 111 + 6 + 3


def test_traced_rows_of_a_convnet_on_task_channels():
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN, beam_env_like
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    env = BT.random_env(16, O=1, seed=2)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 64, 8, GAMMA, 0.01, "mse_q_values", seed=3,
                   per_env_tasks=True, per_env_obstacles=True, task_channels=True)
    eval_env = BT.random_env(4, O=1, seed=79, max_steps=3)
    res = agent.beam_search(beam_env_like(eval_env, 2), 2, trace=True, trace_n_step=2)
    want, g_bound = expected_rows(replay_records(agent, eval_env, res["structures"]), 2, 0.0)
    check_rows(res, want, g_bound, "convnet")


# ---- the loop -----------------------------------------------------------------------------------------------------------------------
def make_loop_agent(E=64, batch=16, **kw):
    from robotoddler.training.vec_dqn import VecDQN
    env = BT.random_env(E, seed=2)
    pol, tgt = BT.make_mlp(1), BT.make_mlp(1)
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 4096, batch, GAMMA, 0.01, "mse_q_values+mse_block_features",
                  seed=3, per_env_tasks=True, **kw)


def _tensors(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            yield from _tensors(obj[k])
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v)


def left_alone(agent):
    """What a search must not touch: the rollout env (every buffer), the count images, the exploration stream, epsilon and the
    temperature, the n-step windows, the hindsight buffer, the episode statistics, the curriculum and the counters."""
    env = agent.env
    h = hashlib.sha256()
    parts = [env.buf, getattr(env, "task_buf", None), env.env_targets, env.task_episode, agent.step_images, agent.explore_gen.get_state(),
             agent._window, vars(agent.hindsight_buffer) if agent.hindsight_buffer is not None else None,
             vars(agent.episode_stats) if agent.episode_stats is not None else None,
             vars(agent.curriculum) if agent.curriculum is not None else None]
    for t in _tensors(parts):
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return (h.hexdigest(), agent.epsilon, agent.temperature, agent.env_steps, agent.episodes_done, env._cand_version)


def run_loop(agent, locksteps, n_train=1):
    """-> per lock-step (ring head before, own rows, searched?, the stand-alone search's rows or None).  Every search of the loop is
    preceded by a stand-alone traced search on the same tasks with the same net, in an env of its own, and checked to leave the
    training state alone."""
    from robotoddler.training.vec_dqn import search_env_like
    log, inner = [], agent._search
    alone_env = search_env_like(agent.env, agent.search_tasks, agent.search_width) if agent.search_every else None

    def searching():
        M, B = agent.search_tasks, agent.search_width
        alone_env.load_targets(agent.env.env_targets[:M].repeat_interleave(B, dim=0))
        alone = agent.beam_search(alone_env, B, merge=agent.search_merge, trace=True, trace_n_step=agent.n_step,
                                  trace_priority=agent.search_priority)
        torch.cuda.synchronize()
        before, head = left_alone(agent), agent.ring.head
        inner()
        torch.cuda.synchronize()
        assert left_alone(agent) == before, "the search touched training state"
        log[-1].update(searched=True, alone=alone["trace_rows"].cpu().numpy(), head_at_search=head, count=agent.last_search["search_rows"])
    agent._search = searching
    try:
        for _ in range(locksteps):
            log.append(dict(head=agent.ring.head, searched=False))
            losses, allrec = agent.lockstep(n_train)
            log[-1].update(own=allrec.cpu().numpy(), head_after=agent.ring.head, losses=losses, last_search=agent.last_search)
    finally:
        del agent._search
    return log


def check_ring(agent, log):
    data = agent.ring.data.cpu().numpy()
    for i, step in enumerate(log):
        own = step["own"]
        assert data[step["head"]:step["head"] + len(own)].tobytes() == own.tobytes(), i
        if step["searched"]:
            assert step["head_at_search"] == step["head"] + len(own)
            assert step["count"] == len(step["alone"]) > 0 and step["head_after"] == step["head_at_search"] + step["count"]
            assert data[step["head_at_search"]:step["head_after"]].tobytes() == step["alone"].tobytes(), i
            assert step["last_search"]["search_rows"] == step["count"]
        else:
            assert step["head_after"] == step["head"] + len(own) and step["last_search"] is None


def test_the_loop_pushes_the_traced_rows_behind_its_own_and_touches_nothing_else():
    agent = make_loop_agent(search_every=2, search_tasks=4, search_width=4, episode_stats=True)
    log = run_loop(agent, 6)
    assert [s["searched"] for s in log] == [False, True] * 3
    check_ring(agent, log)
    assert agent.search_rows == sum(s["count"] for s in log if s["searched"]) and agent.search_env_steps == 3 * 16 * agent.env.K
    assert 0.0 <= agent.search_success_rate <= 1.0 and agent.ring.width == 111 + 6
    from robotoddler.training import records as R
    rows = agent.ring.data[log[1]["head_at_search"]:log[1]["head_after"]]
    assert bool((rows[:, R.O_TD] == 0.0).all())                                 # a uniform loop stores no priorities
    # the tasks are the rollout's own: the tails of the searched rows are the targets of rollout envs 0 .. 3 at that moment -- of which
    # the last search's still stand unless the env finished an episode since, which the last lock-step's train step does not do
    last = agent.ring.data[log[5]["head_at_search"]:log[5]["head_after"], R.RECORD_WIDTH:].cpu().numpy()
    tasks = {t.tobytes() for t in agent.env.env_targets[:4].reshape(4, -1).cpu().numpy()}
    assert {t.tobytes() for t in last} == tasks


def test_the_loop_with_three_step_returns_trains_on_search_rows():
    agent = make_loop_agent(batch=4, n_step=3, search_every=1, search_tasks=4, search_width=4)
    log = run_loop(agent, 3)
    check_ring(agent, log)
    assert log[0]["count"] >= 4 > len(log[0]["own"])                            # the windows are filling: the ring holds search rows first of all
    assert len(log[0]["losses"]) == 1 and np.isfinite(log[0]["losses"][0])      # ... and the train step ran on a batch of them
    assert agent.ring.width == 111 + 6 + 1
    h = agent.ring.data[log[0]["head_at_search"]:log[0]["head_after"], -1].cpu().numpy()
    assert set(h.tolist()) <= {1.0, 2.0, 3.0} and h[-1] == 1.0 and (log[0]["count"] < 3 * 4 or 3.0 in h)
    assert len(log[2]["own"]) > 0                                               # by now the fold emits rows of its own in front


def test_prioritised_rows_carry_the_search_priority():
    from robotoddler.training import records as R
    agent = make_loop_agent(prioritized=True, priority_refresh=True, search_every=1, search_tasks=4, search_width=2, search_priority=2.5)
    log = run_loop(agent, 1, n_train=0)
    rows = agent.ring.data[log[0]["head_at_search"]:log[0]["head_after"]]
    assert len(rows) > 0 and bool((rows[:, R.O_TD] == 2.5).all())
    assert make_loop_agent(prioritized=True, search_every=1).search_priority == 1.0


def _ring_hash(agent, locksteps=6):
    for _ in range(locksteps):
        agent.lockstep(1)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    h.update(agent.ring.data.cpu().numpy().tobytes())
    for p in agent.policy_net.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest(), agent.ring.size, agent.ring.head


# sha256 over the ring and the policy net's parameters after 6 lock-steps of make_loop_agent() as the loop stood BEFORE the option
# existed (the same function run on that tree), the ring's size and head
RING_BEFORE = ("e919e89b11071c98a40952c5113ef0fa0f9b93724b95227aa3fb609be669c45d", 384, 384)


def test_without_the_option_the_ring_is_the_one_it_always_was(monkeypatch):
    from bridges_hip import ops

    def refuse(*a, **k):
        raise AssertionError("an agent without search_every launched bridges_beam_trace")
    monkeypatch.setattr(ops, "beam_trace", refuse)
    agent = make_loop_agent()
    assert agent.search_every == 0 and agent.last_search is None
    assert _ring_hash(agent) == RING_BEFORE
    assert agent.search_env is None and agent.search_rows == 0 and not agent._trace_state


def _lockstep_waits(agent):
    """One lockstep(0) -> (the host waits outside the search, those inside it, [] without a search): BT._waits' counting, split at
    the entry and the exit of VecDQN._search."""
    import warnings
    seen, marks, inner = [], [], agent._search
    saved = (torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize)

    def counting(name, fn):
        def f(*a, **k):
            seen.append(name)
            return fn(*a, **k)
        return f
    torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize = counting("stream", saved[0]), counting("event", saved[1])
    torch.cuda.synchronize = counting("device", saved[2])
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")

            def ops_so_far():
                return sum("synchroniz" in str(x.message) for x in w)

            def searching():
                marks.append((len(seen), ops_so_far()))
                inner()
                marks.append((len(seen), ops_so_far()))
            agent._search = searching
            torch.cuda.set_sync_debug_mode("warn")
            try:
                agent.lockstep(0)
            finally:
                torch.cuda.set_sync_debug_mode("default")
                del agent._search
            n_ops = ops_so_far()
    finally:
        torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize = saved
    if not marks:
        return sorted(seen + ["op"] * n_ops), []
    (s0, o0), (s1, o1) = marks
    return sorted(seen[:s0] + seen[s1:] + ["op"] * (n_ops - (o1 - o0))), sorted(seen[s0:s1] + ["op"] * (o1 - o0))


def test_a_search_adds_the_waits_of_one_search_and_nothing_else():
    plain, agent = make_loop_agent(), make_loop_agent(search_every=2, search_tasks=4, search_width=4)
    for a in (plain, agent):
        for _ in range(3):                                                      # (allocations and caches of the first calls are behind us,
            a.lockstep(0)
        _lockstep_waits(a)                                                      # and so is the first call under the debug mode)
    w_plain, _none = _lockstep_waits(plain)
    w_quiet, inside = _lockstep_waits(agent)                                    # lock-step 5: no search
    assert agent.last_search is None and inside == [] and _none == []
    w_outside, w_inside = _lockstep_waits(agent)                                # lock-step 6: a search
    assert agent.last_search is not None
    # the search of the loop once more, alone: the same env, the same tasks, the same net (lockstep(0) trains nothing)
    w_alone = sorted(BT._waits(lambda: agent.beam_search(agent.search_env, 4, trace=True, trace_n_step=agent.n_step)))
    w_untraced = sorted(BT._waits(lambda: agent.beam_search(agent.search_env, 4)))
    print("waits: plain", w_plain, "quiet", w_quiet, "searching, outside the search", w_outside, "inside", w_inside, "one search", w_alone,
          "untraced", w_untraced)
    assert w_quiet == w_plain == w_outside                                      # a lock-step has the waits it had, searching or not
    assert w_inside == w_alone                                                  # the search adds those of one beam_search, nothing else
    assert w_alone == w_untraced                                                # and tracing adds none to a search
    assert w_alone.count("stream") <= agent.search_env.K and w_alone.count("event") == w_alone.count("device") == 0


def test_the_phase_is_checkpointed(tmp_path):
    agent = make_loop_agent(search_every=3, search_tasks=2, search_width=2)
    for _ in range(2):
        agent.lockstep(0)
    assert agent.search_calls == 2 and agent.last_search is None
    path = str(tmp_path / "extra.pt")
    agent.save_extra(path, lockstep=2)
    other = make_loop_agent(search_every=3, search_tasks=2, search_width=2)
    assert other.load_extra(path)["lockstep"] == 2 and other.search_calls == 2
    other.lockstep(0)
    assert other.last_search is not None and other.search_calls == 0           # the resumed run searches on the same lock-step
    # a checkpoint without the entry loads with phase 0
    blob = torch.load(path, weights_only=False)
    del blob["search_phase"]
    torch.save(blob, path)
    third = make_loop_agent(search_every=3, search_tasks=2, search_width=2)
    third.search_calls = 1
    third.load_extra(path)
    assert third.search_calls == 0


def test_refusals_at_construction_come_in_words():
    for kw, word in ((dict(search_every=2, search_width=17), "search_width"), (dict(search_every=2, search_width=0), "search_width"),
                     (dict(search_every=2, search_tasks=65), "search_tasks"), (dict(search_every=-1), "search_every"),
                     (dict(search_tasks=4), "need search_every"), (dict(search_merge=True), "need search_every"),
                     (dict(search_every=2, search_priority=1.0), "prioritized")):
        with pytest.raises(ValueError) as e:
            make_loop_agent(**kw)
        assert word in str(e.value), (kw, str(e.value))
    # a fixed task: every group would find the same episode, so one task is searched
    from robotoddler.training.vec_dqn import VecDQN
    H = 0.8
    env = BT.make_vec(8, [(0.5, 0., H / 2)], [(0.5, 0, H + H / 2)])
    pol, tgt = BT.make_mlp(1), BT.make_mlp(1)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 256, 8, GAMMA, 0.01, "mse_q_values", seed=3,
                   search_every=1, search_tasks=8, search_width=2)
    assert agent.search_tasks == 1
    agent.lockstep(0)
    assert agent.search_env.E == 2 and agent.last_search["search_rows"] >= 1 and agent.ring.width == 111
