"""CPU-only: the reference of prioritised replay on the device (tests/priority_ref.py) -- the probe, the acceptance rule of the
sampler and the twins it must reject, the reference of the refresh and its twin -- and the host side of
VecDQN(prioritized=True, priority_alpha=..., priority_refresh=...): the constructor, the command line, the entry points in the
header and their ctypes mirror, and the default loop, which never reaches the new ring methods."""
import os
import re

import numpy as np
import pytest
import torch

import priority_ref as P
from robotoddler.training import records as R
from test_cpu_nstep import host_agent, stand_in_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the sampler's rule
@pytest.mark.parametrize("N", P.PROBE_N)
def test_reference_decides_every_draw_of_the_probe_and_the_plain_statement_passes(N):
    """On every probe case the reference alone leaves 0 undecided draws, returns its own index inside its range, and the
    float64 cumsum + searchsorted(right=True) statement -- the torch path's formulation -- passes the rule."""
    for alpha in P.PROBE_ALPHA:
        for n in P.PROBE_DRAWS:
            td, u = P.probe(N, n)
            ref = P.probe_ref(N, alpha, n)
            assert P.undecided(ref) == 0, (N, alpha, n, P.undecided(ref))
            assert P.accept(ref[0], ref) is None
            assert P.accept(P.sample_plain(td, alpha, u), ref) is None, (N, alpha, n)
            assert ref[0].min() >= 0 and ref[0].max() <= N - 1


def test_probe_holds_the_rows_it_names():
    td, u = P.probe(4099, 800)
    assert td[4099 // 3] == 1e6 and np.isnan(td[4099 // 2]) and td[-1] == -1.0
    assert 0.15 < float((td == 0).mean()) < 0.25 and u.shape == (800,) and 0.0 <= u.min() and u.max() < 1.0
    m = P.masses(td, 1.0)
    assert m[4099 // 2] == P.FLOOR and m[-1] == P.FLOOR and np.isfinite(m).all()            # NaN and negative: the floor
    assert m[4099 // 3] / m.sum() > 0.99                                                    # one outlier holds nearly all of it
    assert (P.masses(td, 0.0) == 1.0).all() and np.isfinite(P.masses(td, 0.6)).all()
    assert P.masses(np.array([np.inf, 1e300]), 1.0).tolist() == [P.CEIL + P.FLOOR] * 2
    td1, _ = P.probe(2, 1)
    assert np.isfinite(td1).all() and (td1 >= 0).all()                                      # N <= 3: no planted rows


@pytest.mark.parametrize("name", sorted(P.TWINS))
def test_every_defective_twin_is_rejected(name):
    twin = P.TWINS[name]
    if name == "side_left":
        # the two rules differ on exact ties only, which a tolerance always allows: the exact case (integer masses) has none
        td, u = P.tie_probe()
        ref = P.sample_ref(td, 0.0, u, tol=0.0)
        assert P.undecided(ref) == 0 and ref[0].tolist() == list(range(256))
        assert P.accept(P.sample_plain(td, 0.0, u), ref) is None
        assert "outside" in P.accept(twin(td, 0.0, u), ref)
        return
    rejected = []
    for N, alpha, n in P.PROBE_CASES:
        td, u = P.probe(N, n)
        if P.accept(twin(td, alpha, u), P.probe_ref(N, alpha, n)) is not None:
            rejected.append((N, alpha, n))
    assert rejected, name
    print(name, "rejected on", len(rejected), "of", len(P.PROBE_CASES), "cases")


def test_acceptance_rule_itself():
    td, u = P.probe(257, 65)
    ref = P.sample_ref(td, 0.6, u)
    off = ref[0].copy()
    off[7] = min(off[7] + 1, 256) if off[7] < 256 else off[7] - 1
    assert "draw 7" in P.accept(off, ref)
    assert "draws" in P.accept(ref[0][:-1], ref)
    # undecided draws: a neighbour passes, and the cap counts them
    wide = (ref[0], ref[0] - (ref[0] > 0), ref[0])
    assert P.undecided(wide) > 1 and "cap" in P.accept(ref[0], wide) and P.accept(ref[0], wide, cap=None) is None
    assert P.accept(wide[1], wide, cap=None) is None


# ------------------------------------------------------------------------------------------------------------ the refresh
@pytest.mark.parametrize("n", P.UPDATE_N)
def test_update_reference_and_its_twin(n):
    rec, idx, q_sa, q_target = P.update_probe(n)
    out = P.update_ref(rec, R.O_TD, idx, q_sa, q_target)
    other = np.ones(rec.shape, dtype=bool)
    other[:, R.O_TD] = False
    assert np.array_equal(out[other], rec[other])                                           # no other column
    live = [(j, i) for j, i in enumerate(idx.tolist()) if 0 <= i < rec.shape[0]]
    last = {i: j for j, i in live}
    for i in range(rec.shape[0]):
        want = float(np.abs(q_sa[last[i]] - q_target[last[i]])) if i in last else rec[i, R.O_TD]
        assert out[i, R.O_TD] == want
    first = P.twin_update_first_wins(rec, R.O_TD, idx, q_sa, q_target)
    if n > 1:
        assert len(last) < len(live) and not np.array_equal(first, out)                     # rows repeat: the twin differs
        assert any(i < 0 or i >= rec.shape[0] for i in idx.tolist()) == (n >= 64)
    else:
        assert np.array_equal(first, out)


# ------------------------------------------------------------------------------------------------------------ host side
def test_new_entry_points_are_declared_and_mirrored():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, n_args in (("bridges_priority_sample_scratch", 2), ("bridges_priority_sample", 11), ("bridges_priority_update", 9)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(abi.SIGNATURES[name]), name
    with open(os.path.join(ROOT, "bridges-with-reinforcement-learning_amd", "csrc", "api.hip")) as fh:
        assert '#include "replay_kernels.hip"' in fh.read()


def test_scratch_sizing_call_needs_no_gpu():
    from bridges_hip import abi, dqn_ops
    assert dqn_ops.priority_sample_scratch(0) == 0
    assert dqn_ops.priority_sample_scratch(1) == 256 + 2 and dqn_ops.priority_sample_scratch(256) == 256 + 2
    assert dqn_ops.priority_sample_scratch(257) == 512 + 4 and dqn_ops.priority_sample_scratch(131072) == 131072 + 1024
    with pytest.raises(abi.BridgesHipError):
        dqn_ops.priority_sample_scratch(-1)


def test_constructor_takes_the_options_and_refuses_in_words(monkeypatch):
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True)
    assert a.priority_alpha == 1.0 and a.priority_refresh is False
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=0.6, priority_refresh=True)
    assert a.priority_alpha == 0.6 and a.priority_refresh is True and a.ring.width == R.RECORD_WIDTH
    assert host_agent(monkeypatch, stand_in_env(), priority_alpha=1.0, priority_refresh=False).prioritized is False
    for kw in (dict(priority_alpha=0.5), dict(priority_refresh=True), dict(priority_alpha=0.0, priority_refresh=True)):
        with pytest.raises(ValueError, match="prioritized=True"):
            host_agent(monkeypatch, stand_in_env(), **kw)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=bad)
    # several ranks: the sampler alone is allowed, the refresh is not
    from robotoddler.training import distributed as D
    monkeypatch.setattr(D, "active", lambda: True)
    assert host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=0.5).priority_alpha == 0.5
    with pytest.raises(ValueError, match="one rank"):
        host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_refresh=True)


class _Reached(Exception):
    pass


def _raising(*a, **k):
    raise AssertionError("a new ring method was reached")


def test_default_prioritized_loop_never_reaches_the_new_ring_methods(monkeypatch):
    """VecDQN(prioritized=True) samples through ReplayRing.sample as it always did: with a ring whose new methods raise,
    train_steps gets as far as _targets, handing it what ring.sample drew from the same stream."""
    def agent(**kw):
        a = host_agent(monkeypatch, stand_in_env(), prioritized=True, **kw)
        g = torch.Generator().manual_seed(5)
        rec = torch.rand((12, R.RECORD_WIDTH), generator=g, dtype=torch.float64)
        a.ring.push(rec)
        a.ring.sample_prioritized = a.ring.update_priorities = _raising
        seen = []

        def targets(rec):
            seen.append(rec.clone())
            raise _Reached
        a._targets = targets
        return a, seen
    for kw in ({}, dict(priority_alpha=1.0, priority_refresh=False)):
        a, seen = agent(**kw)
        want = a.ring.sample(8, torch.Generator().manual_seed(1234567), True)                # sample_gen's seed (seed = 0)
        with pytest.raises(_Reached):
            a.train_steps(2)
        assert len(seen) == 1 and torch.equal(seen[0], want)
    for kw in (dict(priority_alpha=0.5), dict(priority_refresh=True)):
        a, seen = agent(**kw)
        with pytest.raises(AssertionError, match="new ring method"):
            a.train_steps(2)
        assert not seen


def test_checkpoint_extra_has_no_key_for_the_options(monkeypatch, tmp_path):
    """The priorities live in the ring: save_extra writes the same keys with and without the options, and either file loads
    into an agent with the other settings."""
    plain = host_agent(monkeypatch, stand_in_env(), prioritized=True)
    fresh = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=0.6, priority_refresh=True)
    plain.save_extra(str(tmp_path / "a.pt"), lockstep=3)
    fresh.save_extra(str(tmp_path / "b.pt"), lockstep=3)
    a, b = (torch.load(str(tmp_path / f), weights_only=True) for f in ("a.pt", "b.pt"))
    assert sorted(a) == sorted(b) and not any("priority" in k for k in a)
    assert fresh.load_extra(str(tmp_path / "a.pt")) == {"lockstep": 3} and plain.load_extra(str(tmp_path / "b.pt")) == {"lockstep": 3}


# ------------------------------------------------------------------------------------------------------------ command line
def test_cli_options_are_opt_in_and_reach_the_agent():
    from robotoddler.training.successor_dqn import build_parser, check_priority, priority_from_args
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--prioritized_replay"]))
    assert "priority_alpha" not in plain and "priority_refresh" not in plain                # a plain parse keeps the keys it had
    check_priority(plain)
    assert priority_from_args(plain) == dict(prioritized=True, priority_alpha=1.0, priority_refresh=False)
    a = vars(build_parser().parse_args(["--num_envs", "64", "--prioritized_replay", "--priority_alpha", "0.6", "--priority_refresh"]))
    check_priority(a)
    assert priority_from_args(a) == dict(prioritized=True, priority_alpha=0.6, priority_refresh=True)


@pytest.mark.parametrize("argv, word", [
    (["--prioritized_replay", "--priority_alpha", "0.6"], "--num_envs"),
    (["--num_envs", "1", "--prioritized_replay", "--priority_refresh"], "--num_envs"),
    (["--num_envs", "64", "--priority_alpha", "0.6"], "--prioritized_replay"),
    (["--num_envs", "64", "--priority_refresh"], "--prioritized_replay"),
    (["--num_envs", "64", "--prioritized_replay", "--priority_alpha", "1.5"], "[0, 1]"),
    (["--num_envs", "64", "--prioritized_replay", "--priority_alpha", "-0.5"], "[0, 1]"),
])
def test_cli_refuses_in_words_before_anything_touches_the_gpu(argv, word):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(["--model", "SuccessorMLP", *argv])
    assert word in str(e.value) and "priority" in str(e.value)
