"""GPU: relative temperatures in the vectorised DQN (VecDQN(temp_relative=, target_temp_relative=, spread_floor=)).  With both
options off the loop is the loop it was, bit for bit; with temp_relative a lock-step's selections are the reference's at the q the
loop computed and at the operator's own temp_out, which lies within the derived bound of the exact spread; with
target_temp_relative _targets equals next_targets of the reference on the captured rows (tests/relative_temperature_ref.py on
top of the recomputation of tests/test_gpu_vec_dqn_soft_target.py); checkpoints round-trip and are refused in both directions."""
import numpy as np
import pytest
import torch

import boltzmann_ref as B
import relative_temperature_ref as RT
import soft_target_ref as S
import test_gpu_vec_dqn_soft_target as ST
from test_gpu_boltzmann import KEYS, TEMPS, check
from test_gpu_double_q import conv_agent as small_conv_agent, mlp_agent as small_mlp_agent, tower_env as small_tower_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-5                                                  # far below the spread of an untrained net's q: the spread decides


# ------------------------------------------------------------------------------------------------------------ options off
def test_both_options_off_is_the_loop_it_was(monkeypatch):
    from bridges_hip import dqn_ops, ops
    seen = []
    for mod, name in ((ops, "boltzmann_select"), (dqn_ops, "soft_expect")):
        inner = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _f=inner, _n=name, **kw: (seen.append((_n, sorted(kw))), _f(*a, **kw))[1])

    def run(**kw):
        agent = ST.mlp_agent(ST.tower_env(f32_rasters=False), exploration="boltzmann", target_temperature=0.5, **TEMPS, **kw)
        losses = []
        for _ in range(3):
            losses += agent.lockstep(ST.TRAIN_STEPS)[0]
        torch.cuda.synchronize()
        return agent, [float(l).hex() for l in losses]
    a, la = run()
    b, lb = run(temp_relative=False, target_temp_relative=False, spread_floor=1e-3)
    assert seen and not any("relative" in kw or "spread_floor" in kw for _, kw in seen)          # the calls the loop made before
    assert la == lb and len(la) >= 2 * ST.TRAIN_STEPS and a.ring.size == b.ring.size and torch.equal(a.ring.data, b.ring.data)
    for p, q in zip([*a.policy_net.parameters(), *a.target_net.parameters()], [*b.policy_net.parameters(), *b.target_net.parameters()]):
        assert torch.equal(p, q)
    assert b.temperature_effective is None and b.target_temperature_effective is None and b._count_names == a._count_names
    seen.clear()
    c, lc = run(temp_relative=True, target_temp_relative=True, spread_floor=FLOOR)
    assert {n for n, kw in seen if "relative" in kw} == {"boltzmann_select", "soft_expect"}
    assert lc != la and all(np.isfinite(float.fromhex(x)) for x in lc)
    assert c.temperature_effective > 0 and c.target_temperature_effective > 0 and c.target_entropy > 0


# ------------------------------------------------------------------------------------------------------------ temp_relative
def recorded_relative_loop(monkeypatch, agent, locksteps):
    from bridges_hip import ops
    calls, valids, inner, inner_act = [], [], ops.boltzmann_select, agent.act

    def recording(seg, q, u, temperature, greedy, idx, cand_offset, rep=None, **kw):
        out = inner(seg, q, u, temperature, greedy, idx, cand_offset, rep=rep, **kw)
        lo, hi = seg if isinstance(seg, (tuple, list)) else (seg[:-1], seg[1:])
        E = lo.numel()
        case = dict(seg_lo=lo.cpu().numpy().copy(), seg_hi=hi.cpu().numpy().copy(), q=q.float().cpu().numpy(), u=u.cpu().numpy(),
                    T=temperature, idx=idx.cpu().numpy(), cand_offset=cand_offset.cpu().numpy()[:E],
                    rep=None if rep is None else rep.cpu().numpy())
        calls.append((case, bool(greedy), kw, {k: v.cpu().numpy() for k, v in zip(KEYS + ("temp_out",), out)}))
        return out
    monkeypatch.setattr(ops, "boltzmann_select", recording)

    def act(*a, **k):
        rec, valid = inner_act(*a, **k)
        valids.append(valid.clone())
        return rec, valid
    agent.act = act
    effective = []
    for _ in range(locksteps):
        agent.lockstep(0)
        effective.append(agent.temperature_effective)
    return calls, valids, effective


def relative_loop_case(monkeypatch, agent, locksteps):
    calls, valids, effective = recorded_relative_loop(monkeypatch, agent, locksteps)
    assert len(calls) == locksteps
    t, explored = TEMPS["temp_start"], 0
    for (case, greedy, kw, got), valid, eff in zip(calls, valids, effective):
        assert not greedy and kw == dict(relative=True, spread_floor=FLOOR)
        assert case["T"] == t                                                                       # the schedule is the multiple's
        t = (t - TEMPS["temp_end"]) * TEMPS["temp_decay"] + TEMPS["temp_end"]
        want, bound = RT.select_temperatures(case, floor=FLOOR)
        assert (np.abs(got["temp_out"] - want) <= bound).all()
        for temps in (got["temp_out"], want - bound, want + bound):                                 # no draw of the run lies in the band
            assert float(RT.select_reference(case, temps)["margin"].min()) > B.MARGIN
        check({k: got[k] for k in KEYS}, RT.select_reference(case, got["temp_out"]), f"lock-step at multiple {case['T']}")
        v = valid.cpu().numpy().astype(bool)
        assert eff == pytest.approx(float(got["temp_out"][v].sum()) / max(int(v.sum()), 1), rel=1e-12)
        explored += int((got["explore_w"] * v).sum())
    assert agent.temperature == t and explored > 0
    spreads = np.concatenate([c[3]["temp_out"] / c[0]["T"] for c in calls])
    print("spreads of the run: min", float(spreads.min()), "max", float(spreads.max()), "distinct", len(np.unique(spreads)))
    assert len(np.unique(spreads)) > 2 and spreads.max() > FLOOR                                    # states do differ in their spread
    return calls


def test_temp_relative_successor_mlp_draws_the_reference_choice_every_lockstep(monkeypatch):
    agent = small_mlp_agent(small_tower_env(64, f32_rasters=False), exploration="boltzmann", temp_relative=True, spread_floor=FLOOR, **TEMPS)
    calls = relative_loop_case(monkeypatch, agent, 6)
    assert any(c[0]["rep"] is not None and (c[0]["rep"] != np.arange(64)).any() for c in calls)
    # evaluation and act(greedy=True) stay greedy
    monkeypatch.undo()
    a = small_mlp_agent(small_tower_env(64, f32_rasters=False), exploration="boltzmann", temp_relative=True)
    b = small_mlp_agent(small_tower_env(64, f32_rasters=False))
    for _ in range(2):
        (rec_a, valid_a), (rec_b, valid_b) = a.act(greedy=True), b.act(greedy=True)
        assert torch.equal(valid_a, valid_b) and torch.equal(rec_a, rec_b)
    assert bool((a._temp_out == 0).all())


def test_temp_relative_conv_net(monkeypatch):
    agent = small_conv_agent(small_tower_env(8, f32_rasters=True), exploration="boltzmann", temp_relative=True, spread_floor=FLOOR, **TEMPS)
    relative_loop_case(monkeypatch, agent, 4)


# ------------------------------------------------------------------------------------------------------------ target_temp_relative
def recompute_relative(monkeypatch, agent, batch, seen, n, factored):
    """test_gpu_vec_dqn_soft_target.recompute with stage one's reference taken per transition at the operator's own temp_out,
    which is first held to the derived bound of the exact spread of the captured select_q."""
    assert seen["relative"] is True and seen["spread_floor"] == agent.spread_floor == FLOOR
    temps = seen["stats"]["temp_out"].cpu().numpy()
    scalar, checked = S.reference, []

    def reference(case, twin=None):
        want, bound = RT.expect_temperatures(case, floor=FLOOR)
        err = np.abs(temps - want)
        print("temp_out: largest |error| / bound", float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        assert (err <= bound).all()
        checked.append(len(want))
        with monkeypatch.context() as m:
            m.setattr(S, "reference", scalar)
            return RT.expect_reference(case, temps)
    with monkeypatch.context() as m:
        m.setattr(S, "reference", reference)
        out = ST.recompute(agent, batch, seen, n, factored)
    assert checked == [len(temps)]
    live = ~seen["done"].cpu().numpy().astype(bool)[:n]
    assert len(np.unique(temps[:n][live])) > 2                                                      # a temperature per transition
    return out


def finished(agent, batch):
    """One train_steps call: the third mean rides with the losses."""
    agent.train_steps(ST.TRAIN_STEPS)
    assert agent.target_temperature_effective is not None and agent.target_temperature_effective > 0
    assert np.isfinite(agent.target_entropy) and agent.soft_value_gap >= -1e-6


def test_target_relative_factored_mlp_on_the_fixed_tower(monkeypatch):
    agent = ST.mlp_agent(ST.tower_env(f32_rasters=False), target_temperature=0.5, target_temp_relative=True, spread_floor=FLOOR)
    batch, seen, n = ST.captured_targets(agent)
    recompute_relative(monkeypatch, agent, batch, seen, n, factored=True)
    assert seen.get("select_q") is None
    # the log's third mean, formed on the device behind the two of the scalar option: over the transitions that are not done
    live = ~seen["done"][:n]
    mean = float(seen["stats"]["temp_out"][:n][live].sum() / live.sum())
    assert agent._soft_stats.shape == (3,) and float(agent._soft_stats[2]) == pytest.approx(mean, rel=1e-5)
    finished(agent, batch)


def test_target_relative_factored_mlp_with_three_step_double_q(monkeypatch):
    agent = ST.mlp_agent(ST.random_env(3, 2), per_env_tasks=True, per_env_obstacles=True, n_step=3, double_q=True, target_temperature=0.5,
                         target_temp_relative=True, spread_floor=FLOOR)
    ST.perturb_last_layer(agent.policy_net)
    batch, seen, n = ST.captured_targets(agent)
    recompute_relative(monkeypatch, agent, batch, seen, n, factored=True)
    assert seen["select_q"] is not None and not torch.equal(seen["select_q"], seen["next_q"])
    # the spread is the policy net's q's, the values that weigh the rows: next_q's would lie outside the bound
    lo, hi = (t.cpu().numpy() for t in seen["seg"])
    case = dict(seg_lo=lo, seg_hi=hi, select_q=seen["select_q"].float().cpu().numpy(), next_q=seen["next_q"].float().cpu().numpy(), T=0.5)
    temps = seen["stats"]["temp_out"].cpu().numpy()
    other, _ = RT.expect_temperatures(case, floor=FLOOR, twin="spread_of_next_q")
    _, bound = RT.expect_temperatures(case, floor=FLOOR)
    assert (np.abs(temps - other) > bound)[bound > 0].any()
    assert seen["discount"] is not None and len(set(seen["discount"].tolist())) > 1


def test_target_relative_module_forward_mlp(monkeypatch):
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "FACTORED_ACTING", False)
    agent = ST.mlp_agent(ST.tower_env(f32_rasters=True), target_temperature=0.5, target_temp_relative=True, spread_floor=FLOOR)
    batch, seen, n = ST.captured_targets(agent)
    recompute_relative(monkeypatch, agent, batch, seen, n, factored=False)
    assert seen["feat_row"] is not None and seen["next_feat"].shape[1] == 4096


# ------------------------------------------------------------------------------------------------------------ log and checkpoints
def test_deferred_losses_carry_the_third_mean_and_the_counts_carry_the_sum():
    agent = ST.mlp_agent(ST.tower_env(f32_rasters=False), exploration="boltzmann", temp_relative=True, target_temperature=0.5,
                         target_temp_relative=True, spread_floor=FLOOR, **TEMPS)
    for _ in range(2):
        agent.lockstep(0)
    d = agent.lockstep(ST.TRAIN_STEPS, defer_losses=True)[0]
    losses = d.get()
    assert len(losses) == ST.TRAIN_STEPS and set(d.soft) == {"target_entropy", "soft_value_gap", "target_temperature_effective"}
    assert d.soft["target_temperature_effective"] == agent.target_temperature_effective > 0
    assert agent._count_names[-1] == "temp_sum" and agent.temperature_effective > 0


def test_checkpoint_round_trip_and_refusal_in_both_directions(tmp_path):
    def agent(**kw):
        return ST.mlp_agent(ST.tower_env(f32_rasters=False), target_temperature=0.5, **kw)
    rel, plain = agent(target_temp_relative=True, spread_floor=FLOOR), agent()
    for a in (rel, plain):
        a.lockstep(0)
    paths = dict(rel=str(tmp_path / "rel.pt"), plain=str(tmp_path / "plain.pt"))
    rel.save_extra(paths["rel"], lockstep=1)
    plain.save_extra(paths["plain"], lockstep=1)
    blob = torch.load(paths["rel"], weights_only=True)
    assert blob["target_temp_relative"] == FLOOR and "target_temp_relative" not in torch.load(paths["plain"], weights_only=True)
    again = agent(target_temp_relative=True, spread_floor=FLOOR)
    assert again.load_extra(paths["rel"]) == dict(lockstep=1) and again.env_steps == rel.env_steps
    assert agent().load_extra(paths["plain"]) == dict(lockstep=1)
    for who, path in ((plain, paths["rel"]), (rel, paths["plain"]), (agent(target_temp_relative=True, spread_floor=0.5), paths["rel"])):
        with pytest.raises(ValueError, match="target_temp_relative, spread_floor"):
            who.load_extra(path)
    # temp_relative: an entry when set, resumed with or without it as the exploration setting itself is
    act = ST.mlp_agent(ST.tower_env(f32_rasters=False), exploration="boltzmann", temp_relative=True, spread_floor=FLOOR, **TEMPS)
    act.lockstep(0)
    path = str(tmp_path / "act.pt")
    act.save_extra(path, lockstep=1)
    assert torch.load(path, weights_only=True)["temp_relative"] == FLOOR
    other = ST.mlp_agent(ST.tower_env(f32_rasters=False), exploration="boltzmann", **TEMPS)
    assert other.load_extra(path) == dict(lockstep=1) and other.temperature == act.temperature
