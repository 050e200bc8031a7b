"""CPU-only: the reference of the importance-sampling weights (tests/is_weight_ref.py) -- the defining and the cancelled form, the
normalisation, the twins the GPU test's bounds must reject -- and the host side of VecDQN(prioritized=True, priority_beta=...,
priority_beta_anneal=...): the constructor, the annealing schedule, the checkpoint key, the command line, the entry points in the
header and their ctypes mirror, and the loop without the option, which never reaches the weights."""
import os
import re

import numpy as np
import pytest
import torch

import is_weight_ref as W
import mlp_conformance as M
from robotoddler.training import records as R
from test_cpu_nstep import host_agent, stand_in_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    for N, alpha, beta, B, n in W.W_CASES:
        m, idx = W.reference_draws(N, alpha, B * n)
        yield (N, alpha, beta, B, n), m, idx


# ------------------------------------------------------------------------------------------------------------ the weights
def test_defining_form_and_cancelled_form_agree():
    worst = 0.0
    for case, m, idx in cases():
        a, b = W.weights_ref(m, idx, case[3], case[2]), W.weights_cancelled(m, idx, case[3], case[2])
        rel = np.abs(a - b) / a
        assert rel.max() <= 1e-13, (case, rel.max())
        worst = max(worst, rel.max())
        assert W.accept_weights(b.astype(np.float32), a) is None, case        # rounded once to float32: inside the GPU test's bound
    print(f"largest relative difference of the two forms: {worst:.3e}")


def test_every_batch_holds_a_weight_of_exactly_one_and_none_above():
    for case, m, idx in cases():
        for form in (W.weights_ref, W.weights_cancelled):
            w = form(m, idx, case[3], case[2]).reshape(case[4], case[3])
            assert (w.max(axis=1) == 1.0).all() and (w > 0).all() and np.isfinite(w).all(), case
            if case[2] == 0.0 or case[1] == 0.0:
                assert (w == 1.0).all(), case


def test_an_index_outside_the_ring_has_weight_zero_and_no_part_in_the_maximum():
    m, idx = W.reference_draws(257, 0.6, 64)
    planted = idx.copy()
    planted[3], planted[40] = -1, 257
    w = W.weights_cancelled(m, planted, 32, 0.4)
    assert w[3] == 0.0 and w[40] == 0.0
    keep = np.ones(64, dtype=bool)
    keep[[3, 40]] = False
    for lo in (0, 32):
        sel = np.nonzero(keep[lo:lo + 32])[0] + lo
        assert np.array_equal(w[sel], W.weights_cancelled(m, idx[sel], sel.size, 0.4))


@pytest.mark.parametrize("name", sorted(W.WEIGHT_TWINS))
def test_every_twin_of_the_weights_is_rejected(name):
    rejected = []
    for case, m, idx in cases():
        ref = W.weights_ref(m, idx, case[3], case[2])
        if W.accept_weights(W.WEIGHT_TWINS[name](m, idx, case[3], case[2]).astype(np.float32), ref) is not None:
            rejected.append(case)
    assert rejected, name
    print(name, "rejected on", len(rejected), "of", len(W.W_CASES), "cases")


def test_acceptance_bound_itself():
    ref = np.array([1.0, 0.5, 0.0, 1e-30])
    assert W.accept_weights(ref, ref) is None
    assert W.accept_weights(ref * (1 + 2.0 ** -24), ref) is None
    assert "draw 1" in W.accept_weights(ref * np.array([1, 1 + 2.0 ** -22, 1, 1]), ref)
    assert "draw 2" in W.accept_weights(ref + np.array([0, 0, 1e-40, 0]), ref)            # a zero weight is exactly zero
    assert "draw 0" in W.accept_weights(np.array([np.nan, 0.5, 0.0, 1e-30]), ref)
    assert "weights for" in W.accept_weights(ref[:-1], ref)


# ------------------------------------------------------------------------------------------------------------ the weighted loss
@pytest.mark.parametrize("shape", W.LOSS_ROWS)
def test_weighted_loss_reference_accepts_float32_and_rejects_the_twin(shape):
    batch, px, nf, use_q, use_sf, per_row = shape
    pr = M.loss_probe(batch, px, nf, per_row, "cpu")
    w_all = W.loss_weights(batch, "cpu")
    for c in W.LOSS_COUNTERS:
        w = w_all[c * batch:(c + 1) * batch]
        # one row exactly 1 and one exactly 0 (batch 1: the tested batches 0 and 2 are the 1 and the 0)
        assert (float(w.max()), float(w.min())) == ((1.0, 0.0) if batch > 1 else ((1.0, 1.0), None, (0.0, 0.0))[c])
        args = (w, pr["y"], *M.loss_batch(pr, batch, px, c), batch, px, nf, use_q, use_sf)
        refs, lib = W.weighted_loss_ref(*args), W.weighted_loss_lib(*args)
        for k in ("q", "loss_rows", "dy"):
            W.inside(f"weighted_loss.{k}.c{c}", lib[k], *refs[k], shape)
        plain = M.loss_ref(*args[1:])
        assert torch.equal(refs["q"][0], plain["q"][0])                                       # q is not weighted
        zero = torch.nonzero(w == 0).flatten().tolist()
        for b in zero:
            assert float(refs["dy"][0][b].abs().max()) == 0.0 and float(refs["dy"][1][b].abs().max()) == 0.0
        twin = W.twin_loss_sf_gradient_unweighted(*args)
        if use_sf and bool((w != 1).any()):
            with pytest.raises(AssertionError, match="outside the bound"):
                W.inside("twin.dy", twin["dy"], *refs["dy"], shape)
        else:                                                                                 # nothing to forget: the twin is right
            W.inside("twin.dy", twin["dy"], *refs["dy"], shape)


def test_weights_of_one_give_the_unweighted_reference():
    batch, px, nf, use_q, use_sf, per_row = M.LOSS_SHAPES[5]
    pr = M.loss_probe(batch, px, nf, per_row, "cpu")
    args = (pr["y"], *M.loss_batch(pr, batch, px, 0), batch, px, nf, use_q, use_sf)
    a, b = W.weighted_loss_ref(torch.ones(batch), *args), M.loss_ref(*args)
    for k in ("q", "loss_rows", "dy"):
        assert torch.equal(a[k][0], b[k][0]) and bool((a[k][1] >= b[k][1]).all())


# ------------------------------------------------------------------------------------------------------------ host side
def test_new_entry_points_are_declared_and_mirrored():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, n_args in (("bridges_priority_weights", 9), ("bridges_successor_loss_weighted", 22)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(abi.SIGNATURES[name]), name
        assert name in abi.EXPORTED_SYMBOLS
    # the weighted form is the _rows argument list plus the weights, in front of the stream
    assert abi.SIGNATURES["bridges_successor_loss_weighted"][:20] == abi.SIGNATURES["bridges_successor_loss_rows"][:20]


def test_constructor_takes_the_options_and_refuses_in_words(monkeypatch):
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True)
    assert a.priority_beta is None and a.priority_beta_anneal == 0
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=0.6, priority_beta=0.4, priority_beta_anneal=100)
    assert a.priority_beta == 0.4 and a.priority_beta_anneal == 100 and a.ring.width == R.RECORD_WIDTH
    for ok in (0.0, 1.0, 0):
        assert host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=ok).priority_beta == float(ok)
    for kw in (dict(priority_beta=0.5), dict(priority_beta=0.0), dict(priority_beta=0.5, priority_beta_anneal=3)):
        with pytest.raises(ValueError, match="prioritized=True"):
            host_agent(monkeypatch, stand_in_env(), **kw)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=bad)
    with pytest.raises(ValueError, match="priority_beta_anneal"):
        host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=0.4, priority_beta_anneal=-1)
    with pytest.raises(ValueError, match="priority_beta as well"):
        host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta_anneal=5)
    # several ranks: the weights are allowed without the refresh, the refresh stays refused
    from robotoddler.training import distributed as D
    monkeypatch.setattr(D, "active", lambda: True)
    assert host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=0.4).priority_beta == 0.4
    with pytest.raises(ValueError, match="one rank"):
        host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=0.4, priority_refresh=True)


class _Reached(Exception):
    pass


def _raising(*a, **k):
    raise AssertionError("the weights were reached")


def _loaded(agent, targets):
    agent.env.reward_features = agent.env.obstacle_raster = torch.zeros(1, 64, 64)          # what _train_step hands the driver
    g = torch.Generator().manual_seed(5)
    agent.ring.push(torch.rand((12, R.RECORD_WIDTH), generator=g, dtype=torch.float64))
    agent._targets = targets


def test_loop_without_the_option_never_reaches_the_weights(monkeypatch):
    """priority_beta=None: train_steps never calls ReplayRing.sample_weights and asks for a driver without weights; the plain
    prioritised loop still samples through ReplayRing.sample, handing _targets what it drew from the same stream."""
    from robotoddler.training import train_step as T
    asked = []

    def of(cls, *a, **config):
        asked.append(config.get("weights"))
        raise _Reached
    monkeypatch.setattr(T.CapturedTrainStep, "of", classmethod(of))
    from robotoddler.training.vec_dqn import TargetBatch
    blank = TargetBatch(*(torch.zeros(1) for _ in range(5)))
    for kw in ({}, dict(priority_beta=None, priority_beta_anneal=0), dict(priority_alpha=0.5, priority_beta=None)):
        a = host_agent(monkeypatch, stand_in_env(), prioritized=True, **kw)
        seen = []
        _loaded(a, lambda rec: seen.append(rec.clone()) or blank)
        a.ring.sample_weights = _raising
        if "priority_alpha" in kw:
            a.ring.sample_prioritized = lambda n, gen, alpha: (a.ring.sample(n, gen, True), torch.zeros(n, dtype=torch.int64))
        else:
            a.ring.sample_prioritized = _raising
        want = a.ring.sample(8, torch.Generator().manual_seed(1234567), True)                # sample_gen's seed (seed = 0)
        with pytest.raises(_Reached):
            a.train_steps(2)
        assert len(seen) == 1 and torch.equal(seen[0], want) and a.priority_beta_calls == 0
    assert asked == [False, False, False]


def test_loop_with_the_option_draws_through_the_kernel_and_hands_the_weights_on(monkeypatch):
    """priority_beta set, also at priority_alpha = 1 without refresh: sample_prioritized, then sample_weights on its idx with the
    batch size and beta_now, before _targets; the driver is asked for with weights=True and run with the weights."""
    from robotoddler.training import train_step as T
    events = []

    class Driver:
        def run(self, n, *a, weights=None):
            events.append(("run", n, weights))
            raise _Reached
    monkeypatch.setattr(T.CapturedTrainStep, "of", classmethod(lambda cls, *a, **config: events.append(("of", config["weights"])) or Driver()))
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=0.25, priority_beta_anneal=3)
    from robotoddler.training.vec_dqn import TargetBatch
    _loaded(a, lambda rec: events.append(("targets",)) or TargetBatch(*(torch.zeros(1) for _ in range(5))))
    idx, w = torch.arange(8), torch.linspace(0.1, 1.0, 8)
    a.ring.sample_prioritized = lambda n, gen, alpha: (events.append(("draw", n, alpha)) or a.ring.data[:n], idx)
    a.ring.sample_weights = lambda i, batch, beta: events.append(("weights", i is idx, batch, beta)) or w
    for k in range(2):
        with pytest.raises(_Reached):
            a.train_steps(2)
    one = [("draw", 8, 1.0), ("weights", True, 4, 0.25), ("targets",), ("of", True), ("run", 2, w)]
    assert events[:5] == one and events[6] == ("weights", True, 4, 0.5) and a.priority_beta_calls == 2
    # a call that does not train (fewer rows than a batch, or no steps) does not advance the schedule
    assert a.train_steps(0) == [] and a.priority_beta_calls == 2


def test_annealing_schedule(monkeypatch):
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=0.4)
    for k in (0, 1, 10 ** 6):
        a.priority_beta_calls = k
        assert a.beta_now() == 0.4                                                          # anneal == 0: constant
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=0.4, priority_beta_anneal=600)
    got = []
    for k in (0, 1, 300, 599, 600, 601, 10 ** 6):
        a.priority_beta_calls = k
        got.append(a.beta_now())
    assert got[0] == 0.4 and got[1] == 0.4 + 0.6 * 1 / 600 and got[2] == 0.4 + 0.6 * 300 / 600 and got[3] < 1.0
    assert got[4:] == [1.0, 1.0, 1.0] and all(x <= y for x, y in zip(got, got[1:]))
    a = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_beta=1.0, priority_beta_anneal=5)
    assert a.beta_now() == 1.0


def test_checkpoint_key_is_there_only_with_the_option(monkeypatch, tmp_path):
    plain = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=0.6)
    weighted = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=0.6, priority_beta=0.4, priority_beta_anneal=10)
    weighted.priority_beta_calls = 7
    plain.save_extra(str(tmp_path / "a.pt"), lockstep=3)
    weighted.save_extra(str(tmp_path / "b.pt"), lockstep=3)
    a, b = (torch.load(str(tmp_path / f), weights_only=True) for f in ("a.pt", "b.pt"))
    assert sorted(set(b) - set(a)) == ["priority_beta_calls"] and set(a) <= set(b) and b["priority_beta_calls"] == 7
    assert not any("priority" in k for k in a)
    # resumed mid-anneal: the clock and with it beta_now continue; a file without the key means 0; a plain agent ignores the key
    fresh = host_agent(monkeypatch, stand_in_env(), prioritized=True, priority_alpha=0.6, priority_beta=0.4, priority_beta_anneal=10)
    assert fresh.load_extra(str(tmp_path / "b.pt")) == {"lockstep": 3}
    assert fresh.priority_beta_calls == 7 and fresh.beta_now() == weighted.beta_now() == 0.4 + 0.6 * 7 / 10
    assert fresh.load_extra(str(tmp_path / "a.pt")) == {"lockstep": 3} and fresh.priority_beta_calls == 0 and fresh.beta_now() == 0.4
    assert plain.load_extra(str(tmp_path / "b.pt")) == {"lockstep": 3} and plain.priority_beta_calls == 0


def test_ring_refuses_weights_before_a_draw():
    ring = R.ReplayRing(16, "cpu")
    with pytest.raises(RuntimeError, match="sample_prioritized has not run"):
        ring.sample_weights(torch.zeros(4, dtype=torch.int64), 4, 0.4)


def test_driver_key_holds_the_flag_and_run_refuses_a_mismatch():
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training import train_step as T
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8])
    parts = ["mse_q_values"]
    plain = T.CapturedTrainStep(net, None, 8, parts, (64, 64), True)
    weighted = T.CapturedTrainStep(net, None, 8, parts, (64, 64), True, weights=True)
    assert plain.key[:4] == weighted.key[:4] and plain.key != weighted.key and plain.key[4] is False and weighted.key[4] is True
    with pytest.raises(ValueError, match="weights"):
        plain.run(1, *[None] * 7, weights=torch.ones(8))
    with pytest.raises(ValueError, match="weights"):
        weighted.run(1, *[None] * 7)


# ------------------------------------------------------------------------------------------------------------ command line
def test_cli_options_are_opt_in_and_reach_the_agent():
    from robotoddler.training.successor_dqn import build_parser, check_priority, priority_from_args
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--prioritized_replay", "--priority_alpha", "0.6"]))
    assert "priority_beta" not in plain and "priority_beta_anneal" not in plain             # a plain parse keeps the keys it had
    assert priority_from_args(plain) == dict(prioritized=True, priority_alpha=0.6, priority_refresh=False)
    a = vars(build_parser().parse_args(["--num_envs", "64", "--prioritized_replay", "--priority_beta", "0.4", "--priority_beta_anneal", "600"]))
    check_priority(a)
    assert priority_from_args(a) == dict(prioritized=True, priority_alpha=1.0, priority_refresh=False, priority_beta=0.4,
                                         priority_beta_anneal=600)
    b = vars(build_parser().parse_args(["--num_envs", "64", "--prioritized_replay", "--priority_beta", "0"]))
    assert priority_from_args(b)["priority_beta"] == 0.0 and priority_from_args(b)["priority_beta_anneal"] == 0


@pytest.mark.parametrize("argv, word", [
    (["--prioritized_replay", "--priority_beta", "0.4"], "--num_envs"),
    (["--num_envs", "64", "--priority_beta", "0.4"], "--prioritized_replay"),
    (["--num_envs", "64", "--prioritized_replay", "--priority_beta", "1.5"], "[0, 1]"),
    (["--num_envs", "64", "--prioritized_replay", "--priority_beta", "-0.5"], "[0, 1]"),
    (["--num_envs", "64", "--prioritized_replay", "--priority_beta", "nan"], "[0, 1]"),
    (["--num_envs", "64", "--prioritized_replay", "--priority_beta_anneal", "10"], "--priority_beta as well"),
])
def test_cli_refuses_in_words_before_anything_touches_the_gpu(argv, word):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(["--model", "SuccessorMLP", *argv])
    assert word in str(e.value) and "priority" in str(e.value)
