"""GPU: the vectorised DQN loop with per-step hindsight goals (VecDQN(hindsight="per_step")).  The ring after every lock-step is
the ring of a host-side loop that takes the same buffer writes and appends the rows of tests/hindsight_step_ref.py, bit for bit
-- under one-step returns and folded under n-step returns; every ring row's stored linear reward is reproduced from the reward
map its own tail rebuilds; the optimiser steps run on it; the running episodes survive a checkpoint; and without the option, or
with hindsight="final", a seeded run is the run it was."""
import numpy as np
import pytest
import torch

import hindsight_ref as H
import hindsight_step_ref as S
from oracle.shapes import get_shape
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, T, MAX_STEPS, LOCKSTEPS, GAMMA = 64, 3, 6, 8, 0.95
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
    """The ring of a loop that appends a reference's relabelled rows behind every lock-step's own emitted rows.  ``strategy``:
    "per_step" (tests/hindsight_step_ref.py; n: the window of the fold or None) or "final" (tests/hindsight_ref.py)."""

    def __init__(self, agent, G, n=None, strategy="per_step"):
        env = agent.env
        self.shapes, self.G, self.n, self.strategy = [get_shape("trapezoid"), get_shape("cube06")], G, n, strategy
        self.seed, self.base = env.seed, env.env_id_base
        W = agent.ring.width - (n is not None)                   # the buffer's: one-step records
        self.buf, self.flags = np.zeros((E, env.K, W)), np.zeros((E, env.K, 8), dtype=np.uint8)
        self.length, self.episode = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
        self.ring, self.relabelled = [np.zeros((0, agent.ring.width))], 0

    def lockstep(self, own, rec, flags, valid, episode):
        for e in np.flatnonzero(valid):
            self.buf[e, self.length[e]], self.flags[e, self.length[e]], self.episode[e] = rec[e], flags[e], episode[e]
            self.length[e] += 1
        ended = valid & (rec[:, R.O_DONE] > 0.5)
        args = (self.buf, self.flags, self.length, ended, self.episode, self.shapes, self.seed, self.base, self.G, T)
        if self.strategy == "final":
            rows = H.relabel(*args, task_cls=H.cached_device_task)
        else:                                                    # (the device-arithmetic task is cached per target set)
            rows = S.relabel(*args, n_step=self.n, gamma=None if self.n is None else GAMMA)
        self.length[ended] = 0
        self.ring += [own, rows]
        self.relabelled = len(rows)


def spy_on(agent):
    """What every lock-step hands to the agent's hindsight buffer, as numpy copies."""
    calls, write = [], agent.hindsight_buffer.write

    def spy(rec, flags, valid, episode):
        calls.append(tuple(t.cpu().numpy().copy() for t in (rec, flags, valid, episode)))
        return write(rec, flags, valid, episode)
    agent.hindsight_buffer.write = spy
    return calls


@pytest.mark.parametrize("G,n", [(2, None), (1, 3)])
def test_the_ring_is_the_emitted_rows_plus_the_reference_rows(G, n, tmp_path):
    kw = dict(hindsight="per_step", hindsight_goals=G, **({} if n is None else dict(n_step=n, hindsight_fold=True)))
    agent = make_agent(**kw)
    assert agent.ring.width == R.RECORD_WIDTH + 3 * T + (n is not None)
    assert agent._count_names == (("valid", "done") + (("emitted",) if n else ()) + ("hindsight",))   # "final"'s host waits, no more
    host, calls = HostLoop(agent, G, n), spy_on(agent)
    trained = total = 0
    for it in range(LOCKSTEPS):
        losses, own = agent.lockstep(1)
        rec, _flags, valid, _episode = calls[-1]
        host.lockstep(own.cpu().numpy() if n else rec[valid], *calls[-1])
        want = np.concatenate(host.ring)
        got = agent.ring.data[:agent.ring.size].cpu().numpy()
        assert agent.hindsight_rows == host.relabelled and agent.ring.size == len(want), (it, agent.hindsight_rows, host.relabelled)
        assert np.array_equal(bits(got), bits(want)), it
        total += host.relabelled
        if losses:
            assert all(np.isfinite(l) for l in losses), (it, losses)
            trained += 1
    assert trained >= LOCKSTEPS - 2 and total >= E * G            # episodes of at most 6 steps: every env ended one
    rows = agent.ring.data[:agent.ring.size].cpu().numpy()
    if n is None:
        # every ring row -- rolled out or relabelled -- stores the linear reward of its block under the map its own tail rebuilds
        by_base = 0
        for row in rows:
            task = H.cached_device_task(row[R.RECORD_WIDTH:R.RECORD_WIDTH + 3 * T].reshape(T, 3))
            base = task.base(H.block_of(row, host.shapes))
            lin, frozen = np.float32(row[R.O_LIN]), row[R.O_STABLE_N] > 0.5
            assert float(lin) == row[R.O_LIN]
            allowed = (base, base / np.float32(100)) if frozen else (base, np.float32(0))
            assert any(lin.tobytes() == a.tobytes() for a in allowed), (row[R.O_NB], lin, base, frozen)
            by_base += lin.tobytes() == base.tobytes()
        assert by_base >= len(rows) // 4
    else:
        assert set(np.unique(rows[:, -1])) == {1.0, 2.0, 3.0}
    print(f"G={G} n={n}: {len(rows)} ring rows, {total} relabelled")
    # a save / load round trip in the middle of episodes continues with the same ring
    assert int(agent.hindsight_buffer.length.sum()) > 0
    path = str(tmp_path / "agent.pt")
    agent.save_extra(path, lockstep=LOCKSTEPS)
    assert tuple(torch.load(path, weights_only=True)["hindsight"]) == ("per_step", G)
    hb = agent.hindsight_buffer
    kept = {name: getattr(hb, name).clone() for name in ("rows", "flags", "length", "episode")}
    hb.rows.zero_(); hb.flags.zero_(); hb.length.zero_(); hb.episode.zero_()
    assert agent.load_extra(path) == dict(lockstep=LOCKSTEPS)
    for name, v in kept.items():
        assert torch.equal(getattr(hb, name), v), name
    for it in range(2):
        _losses, own = agent.lockstep(1)
        rec, _flags, valid, _episode = calls[-1]
        host.lockstep(own.cpu().numpy() if n else rec[valid], *calls[-1])
        got = agent.ring.data[:agent.ring.size].cpu().numpy()
        assert np.array_equal(bits(got), bits(np.concatenate(host.ring))), it
    with pytest.raises(ValueError, match="hindsight"):            # the other strategy refuses the file
        make_agent(**dict(kw, hindsight="final")).load_extra(path)


def test_without_the_option_and_with_final_the_seeded_run_is_the_run_it_was():
    """No optimiser step, so the three loops act alike: the plain loop's ring is the rollout records of the other two, the
    "final" loop's ring is those records plus the rows of the "final" reference, and its buffer asks for "final"'s scratch."""
    from bridges_hip import dqn_ops
    plain, final, step = make_agent(), make_agent(hindsight="final", hindsight_goals=2), make_agent(hindsight="per_step", hindsight_goals=2)
    assert plain.hindsight_buffer is None and plain._count_names == ("valid", "done")
    assert final.hindsight_buffer.strategy == "final"
    assert final.hindsight_buffer._scratch.numel() == dqn_ops.hindsight_relabel_scratch(E, 2) == 4 * E * 2
    host, calls, calls_step = HostLoop(final, 2, strategy="final"), spy_on(final), spy_on(step)
    records = [np.zeros((0, plain.ring.width))]
    for it in range(LOCKSTEPS):
        for agent in (plain, final, step):
            agent.lockstep(0)
        rec, _flags, valid, _episode = calls[-1]
        for a, b in zip(calls[-1], calls_step[-1]):
            assert np.array_equal(a, b), it                       # the rollout does not depend on the strategy
        records.append(rec[valid])
        host.lockstep(rec[valid], *calls[-1])
        assert np.array_equal(bits(plain.ring.data[:plain.ring.size].cpu().numpy()), bits(np.concatenate(records))), it
        assert final.hindsight_rows == host.relabelled
        assert np.array_equal(bits(final.ring.data[:final.ring.size].cpu().numpy()), bits(np.concatenate(host.ring))), it
    assert final.ring.size > plain.ring.size > 0 and step.ring.size > plain.ring.size
