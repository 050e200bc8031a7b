"""GPU: the vectorised DQN loop with hindsight relabelling (VecDQN(hindsight="final")).  The ring after every lock-step is the
ring of a host-side loop that takes the same rollout records and appends the rows of tests/hindsight_ref.py, bit for bit; every
ring row's stored linear reward is reproduced from the reward map its own tail rebuilds; the optimiser steps run on it; without the
option the loop is the loop it was; the running episodes survive a checkpoint; another setting's checkpoint is refused."""
import numpy as np
import pytest
import torch

import hindsight_ref as H
from oracle.shapes import get_shape
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, T, MAX_STEPS, LOCKSTEPS = 64, 3, 6, 12
RANGE = ((-3.0, 3.0), (0.3, 2.5))
LOSS = dict(ConvNet="mse_q_values", SuccessorMLP="mse_q_values+mse_block_features")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make_env(O=0, seed=11):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomObstacles, RandomTargets, VecAssemblyGym
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], RandomObstacles([RANGE] * O) if O else [], RandomTargets(T),
                          max_steps=MAX_STEPS, seed=seed, f32_rasters=False, device=DEV)


def make_agent(model="SuccessorMLP", O=0, B=16, **kw):
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    env = make_env(O)
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", model])), torch.device(DEV))
    opt = torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True)
    return VecDQN(pol, tgt, opt, env, 8192, B, 0.95, 0.01, LOSS[model], seed=3, per_env_tasks=True, per_env_obstacles=bool(O),
                  task_channels=model != "SuccessorMLP", **kw)


class HostLoop:
    """The ring of a loop that appends the reference's relabelled rows behind every lock-step's own records."""

    def __init__(self, agent, G):
        env = agent.env
        self.shapes, self.G = [get_shape("trapezoid"), get_shape("cube06")], G
        self.seed, self.base = env.seed, env.env_id_base
        W = agent.ring.width
        self.buf, self.flags = np.zeros((E, env.K, W)), np.zeros((E, env.K, 8), dtype=np.uint8)
        self.length, self.episode = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
        self.ring, self.relabelled = [np.zeros((0, W))], 0

    def lockstep(self, rec, flags, valid, episode):
        for e in np.flatnonzero(valid):
            self.buf[e, self.length[e]], self.flags[e, self.length[e]], self.episode[e] = rec[e], flags[e], episode[e]
            self.length[e] += 1
        ended = valid & (rec[:, R.O_DONE] > 0.5)
        rows = H.relabel(self.buf, self.flags, self.length, ended, self.episode, self.shapes, self.seed, self.base, self.G, T,
                         task_cls=H.cached_device_task)
        self.length[ended] = 0
        self.ring += [rec[valid], rows]
        self.relabelled = len(rows)


def spy_on(agent):
    """What every lock-step hands to the agent's hindsight buffer, as numpy copies."""
    calls, write = [], agent.hindsight_buffer.write

    def spy(rec, flags, valid, episode):
        calls.append(tuple(t.cpu().numpy().copy() for t in (rec, flags, valid, episode)))
        return write(rec, flags, valid, episode)
    agent.hindsight_buffer.write = spy
    return calls


@pytest.mark.parametrize("model,O,G", [("SuccessorMLP", 0, 2), ("ConvNet", 2, 1)])
def test_the_ring_is_the_rollout_plus_the_reference_rows(model, O, G):
    agent = make_agent(model, O, hindsight="final", hindsight_goals=G)
    assert agent.ring.width == R.RECORD_WIDTH + 3 * T + 3 * O
    host, calls = HostLoop(agent, G), spy_on(agent)
    trained = total = 0
    for it in range(LOCKSTEPS):
        losses, _own = agent.lockstep(1)
        host.lockstep(*calls[-1])
        want = np.concatenate(host.ring)
        got = agent.ring.data[:agent.ring.size].cpu().numpy()
        assert agent.hindsight_rows == host.relabelled and agent.ring.size == len(want), (it, agent.hindsight_rows, host.relabelled)
        assert np.array_equal(bits(got), bits(want)), it
        total += host.relabelled
        if losses:
            assert all(np.isfinite(l) for l in losses), (it, losses)
            trained += 1
    assert trained >= LOCKSTEPS - 2 and total >= E                # episodes of at most 6 steps: every env ended one, most two
    # every ring row -- rolled out or relabelled -- stores the linear reward of its block under the map its own tail rebuilds
    rows = agent.ring.data[:agent.ring.size].cpu().numpy()
    by_base = by_hundredth = zeros = 0
    for row in rows:
        task = H.cached_device_task(row[R.RECORD_WIDTH:R.RECORD_WIDTH + 3 * T].reshape(T, 3))
        base = task.base(H.block_of(row, host.shapes))
        lin, frozen = np.float32(row[R.O_LIN]), row[R.O_STABLE_N] > 0.5
        assert float(lin) == row[R.O_LIN]
        allowed = (base, base / np.float32(100)) if frozen else (base, np.float32(0))
        assert any(lin.tobytes() == a.tobytes() for a in allowed), (row[R.O_NB], lin, base, frozen)
        by_base += lin.tobytes() == base.tobytes()
        by_hundredth += frozen and lin.tobytes() == (base / np.float32(100)).tobytes()
        zeros += (not frozen) and lin == 0
    print(f"{model}: {len(rows)} ring rows, {total} relabelled; lin = base {by_base}, base / 100 {by_hundredth}, 0 {zeros}")
    assert by_base >= len(rows) // 4


def test_without_the_option_the_loop_is_the_loop_it_was():
    def run(**kw):
        agent = make_agent(**kw)
        log = []
        for _ in range(6):
            losses, own = agent.lockstep(1)
            log.append((losses, own.cpu().numpy().copy(), agent.epsilon, agent.env_steps, agent.episodes_done))
        return agent, log
    a, log_a = run()
    b, log_b = run(hindsight=None, hindsight_goals=1)
    assert b.hindsight_buffer is None and a._counts_host.numel() == b._counts_host.numel() == 2
    assert a.ring.size == b.ring.size and torch.equal(a.ring.data, b.ring.data)
    for pa, pb in zip(a.policy_net.parameters(), b.policy_net.parameters()):
        assert torch.equal(pa, pb)
    for (la, ra, *ca), (lb, rb, *cb) in zip(log_a, log_b):
        assert la == lb and np.array_equal(bits(ra), bits(rb)) and ca == cb


def test_checkpoint_round_trip_in_the_middle_of_episodes(tmp_path):
    """Two identical loops run five lock-steps; one writes its checkpoint, the other loses its running episodes and reads them
    back from that file: both go on to the same rings."""
    a, b = (make_agent(hindsight="final", hindsight_goals=2) for _ in range(2))
    for agent in (a, b):
        for _ in range(5):
            agent.lockstep(1)
    assert int(a.hindsight_buffer.length.sum()) > 0               # episodes are running
    assert torch.equal(a.ring.data, b.ring.data)
    path = str(tmp_path / "agent.pt")
    a.save_extra(path, lockstep=5)
    hb = b.hindsight_buffer
    want = {n: getattr(hb, n).clone() for n in ("rows", "flags", "length", "episode")}
    hb.rows.zero_(); hb.flags.zero_(); hb.length.zero_(); hb.episode.zero_()
    assert b.load_extra(path) == dict(lockstep=5)
    for n, v in want.items():
        assert torch.equal(getattr(hb, n), v), n
    for it in range(4):
        a.lockstep(1); b.lockstep(1)
        assert a.hindsight_rows == b.hindsight_rows and a.ring.size == b.ring.size and torch.equal(a.ring.data, b.ring.data), it
    assert a.ring.size > 9 * E


def test_a_checkpoint_of_another_setting_is_refused(tmp_path):
    one, two, none = make_agent(hindsight="final"), make_agent(hindsight="final", hindsight_goals=2), make_agent()
    p1, p0 = str(tmp_path / "one.pt"), str(tmp_path / "none.pt")
    one.save_extra(p1, lockstep=1)
    none.save_extra(p0, lockstep=1)
    for agent, path in ((two, p1), (none, p1), (one, p0)):
        with pytest.raises(ValueError, match="hindsight"):
            agent.load_extra(path)
    assert one.load_extra(p1) == dict(lockstep=1) and none.load_extra(p0) == dict(lockstep=1)
