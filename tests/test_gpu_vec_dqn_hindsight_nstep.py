"""GPU: the vectorised DQN loop with hindsight relabelling under n-step returns (VecDQN(hindsight="final", hindsight_fold=True,
n_step=3)).  The ring after every lock-step is the ring of a host-side loop that takes the same buffer writes and appends, behind
the loop's own emitted rows, the rows of tests/hindsight_nstep_ref.py, bit for bit; with n_step = 1 the option is
hindsight="final" alone; the counts that ride to the host are those of the two parent options; the targets of a batch of
relabelled rows are finite; the running episodes survive a checkpoint."""
import numpy as np
import pytest
import torch

import hindsight_nstep_ref as HN
import hindsight_ref as H
from oracle.shapes import get_shape
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, T, MAX_STEPS, LOCKSTEPS, N, G, GAMMA = 16, 3, 6, 10, 3, 2, 0.95
LOSS = "mse_q_values+mse_block_features"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make_agent(B=16, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomTargets, VecAssemblyGym
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    env = VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [], RandomTargets(T), max_steps=MAX_STEPS, seed=11,
                         f32_rasters=False, device=DEV)
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "SuccessorMLP"])), torch.device(DEV))
    opt = torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True)
    return VecDQN(pol, tgt, opt, env, 8192, B, GAMMA, 0.01, LOSS, seed=3, per_env_tasks=True, **kw)


class HostLoop:
    """The ring of a loop that appends the reference's folded relabelled rows behind every lock-step's own emitted rows."""

    def __init__(self, agent):
        env = agent.env
        self.shapes = [get_shape("trapezoid"), get_shape("cube06")]
        self.seed, self.base = env.seed, env.env_id_base
        W = agent.ring.width - 1                                 # the buffer's: one-step records
        self.buf, self.flags = np.zeros((E, env.K, W)), np.zeros((E, env.K, 8), dtype=np.uint8)
        self.length, self.episode = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
        self.ring, self.relabelled, self.open_tail_rows = [np.zeros((0, W + 1))], 0, 0

    def lockstep(self, own, rec, flags, valid, episode):
        for e in np.flatnonzero(valid):
            self.buf[e, self.length[e]], self.flags[e, self.length[e]], self.episode[e] = rec[e], flags[e], episode[e]
            self.length[e] += 1
        ended = valid & (rec[:, R.O_DONE] > 0.5)
        rows = HN.relabel_nstep(self.buf, self.flags, self.length, ended, self.episode, self.shapes, self.seed, self.base, G, T, N, GAMMA,
                                task_cls=H.cached_device_task)
        self.length[ended] = 0
        self.ring += [own, rows]
        self.relabelled = len(rows)
        self.open_tail_rows += int(((rows[:, -1] < N) & ~(rows[:, R.O_DONE] > 0.5)).sum())


def spy_on(agent):
    """What every lock-step hands to the agent's hindsight buffer, as numpy copies."""
    calls, write = [], agent.hindsight_buffer.write

    def spy(rec, flags, valid, episode):
        calls.append(tuple(t.cpu().numpy().copy() for t in (rec, flags, valid, episode)))
        return write(rec, flags, valid, episode)
    agent.hindsight_buffer.write = spy
    return calls


def test_the_ring_is_the_emitted_rows_plus_the_reference_rows():
    agent = make_agent(hindsight="final", hindsight_goals=G, hindsight_fold=True, n_step=N)
    assert agent.ring.width == R.RECORD_WIDTH + 3 * T + 1
    # the counts that ride to the host: those of the two parent options and no more
    assert agent._count_names == ("valid", "done", "emitted", "hindsight") and agent._counts_host.numel() == 4
    host, calls = HostLoop(agent), spy_on(agent)
    trained = total = 0
    for it in range(LOCKSTEPS):
        losses, own = agent.lockstep(1)
        assert len(calls) == it + 1 and calls[-1][0].shape[1] == agent.ring.width - 1        # one-step records go into the buffer
        host.lockstep(own.cpu().numpy(), *calls[-1])
        want = np.concatenate(host.ring)
        got = agent.ring.data[:agent.ring.size].cpu().numpy()
        assert agent.hindsight_rows == host.relabelled and agent.ring.size == len(want), (it, agent.hindsight_rows, host.relabelled)
        assert np.array_equal(bits(got), bits(want)), it
        total += host.relabelled
        if losses:
            assert all(np.isfinite(l) for l in losses), (it, losses)
            trained += 1
    print(f"{agent.ring.size} ring rows, {total} relabelled, {host.open_tail_rows} of them flushed at an open end")
    assert trained >= LOCKSTEPS - 3 and total >= E               # episodes of at most 6 steps: every env ended one
    h = agent.ring.data[:agent.ring.size, -1].cpu().numpy()
    assert set(np.unique(h)) == {1.0, 2.0, 3.0}


def test_with_one_step_returns_the_option_is_hindsight_alone():
    def run(**kw):
        agent = make_agent(hindsight="final", hindsight_goals=G, **kw)
        log = []
        for _ in range(6):
            losses, own = agent.lockstep(1)
            log.append((losses, own.cpu().numpy().copy(), agent.hindsight_rows, agent.env_steps, agent.episodes_done))
        return agent, log
    a, log_a = run()
    b, log_b = run(hindsight_fold=True)
    assert b.hindsight_buffer.fold is False and a.ring.width == b.ring.width == R.RECORD_WIDTH + 3 * T
    assert a._count_names == b._count_names == ("valid", "done", "hindsight")
    assert a.ring.size == b.ring.size > 0 and torch.equal(a.ring.data, b.ring.data)
    for pa, pb in zip(a.policy_net.parameters(), b.policy_net.parameters()):
        assert torch.equal(pa, pb)
    for (la, ra, *ca), (lb, rb, *cb) in zip(log_a, log_b):
        assert la == lb and np.array_equal(bits(ra), bits(rb)) and ca == cb


def test_targets_of_a_batch_of_relabelled_rows_are_finite():
    agent = make_agent(hindsight="final", hindsight_goals=G, hindsight_fold=True, n_step=N)
    relabelled = []
    for _ in range(MAX_STEPS + 2):
        agent.lockstep(0)
        if agent.hindsight_rows:
            relabelled.append(agent.hindsight_buffer.out[:agent.hindsight_rows].clone())
    rows = torch.cat(relabelled)
    assert rows.shape[0] >= agent.B and rows.shape[1] == agent.ring.width
    # a batch that holds every horizon, the open-ended tails among them
    pick = torch.cat([torch.nonzero(rows[:, -1] == h).flatten()[:agent.B // 2] for h in (1.0, 2.0, 3.0)])[:agent.B]
    pick = torch.cat([pick, torch.arange(agent.B - pick.numel(), device=DEV)])
    batch = rows[pick].contiguous()
    out = agent._targets(batch)
    leaves = []

    def collect(v):
        if torch.is_tensor(v):
            leaves.append(v)
        elif isinstance(v, dict):
            [collect(x) for x in v.values()]
        elif isinstance(v, (tuple, list)):
            [collect(x) for x in v]
        elif hasattr(v, "__dict__"):
            [collect(x) for x in vars(v).values()]
    collect(out)
    floats = [v for v in leaves if v.is_floating_point()]
    assert floats and all(bool(torch.isfinite(v).all()) for v in floats)
    losses = agent.train_steps(1)
    assert all(np.isfinite(l) for l in losses)


def test_checkpoint_round_trip_in_the_middle_of_episodes(tmp_path):
    """Two identical loops run four lock-steps; one writes its checkpoint, the other loses its running episodes and reads them
    back from that file: both go on to the same rings."""
    a, b = (make_agent(hindsight="final", hindsight_goals=G, hindsight_fold=True, n_step=N) for _ in range(2))
    for agent in (a, b):
        for _ in range(4):
            agent.lockstep(1)
    assert int(a.hindsight_buffer.length.sum()) > 0               # episodes are running
    assert torch.equal(a.ring.data, b.ring.data)
    path = str(tmp_path / "agent.pt")
    a.save_extra(path, lockstep=4)
    assert torch.load(path, weights_only=True)["hindsight_fold"] is True
    hb = b.hindsight_buffer
    want = {n: getattr(hb, n).clone() for n in ("rows", "flags", "length", "episode")}
    hb.rows.zero_(); hb.flags.zero_(); hb.length.zero_(); hb.episode.zero_()
    assert b.load_extra(path) == dict(lockstep=4)
    for n, v in want.items():
        assert torch.equal(getattr(hb, n), v), n
    for it in range(4):
        a.lockstep(1); b.lockstep(1)
        assert a.hindsight_rows == b.hindsight_rows and a.ring.size == b.ring.size and torch.equal(a.ring.data, b.ring.data), it
    plain = make_agent(hindsight="final", hindsight_goals=G)
    with pytest.raises(ValueError, match="hindsight|n_step"):
        plain.load_extra(path)
