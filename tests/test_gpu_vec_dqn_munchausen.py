"""GPU: Munchausen targets in the vectorised DQN (VecDQN(munchausen_alpha=A)); 64 envs, six lock-steps, batches of 16.  What
_targets fed the operators is captured and q_target is recomputed from it in float64 (tests/munchausen_ref.py: the rule and its
bound); sf_target is the soft-target loop's, bit for bit; every sampled record's action is found among the rebuilt candidates of
its state, in every mode the option composes with; the options unset are the loop it was, bit for bit; the refusals."""
import numpy as np
import pytest
import torch

import munchausen_ref as M
import soft_target_ref as S
from gpu_helpers import U32
from test_gpu_vec_dqn_soft_target import (BATCH, DEV, MAX_STEPS, TRAIN_STEPS, captured_targets, conv_agent, mlp_agent,
                                           perturb_last_layer, random_env, tower_env)

pytestmark = pytest.mark.gpu
LOCKSTEPS = 6
ALPHA, CLIP, TEMP = 0.9, -1.0, 0.5
OPTION = dict(target_temperature=TEMP, munchausen_alpha=ALPHA)


def recompute_q(agent, batch, seen, n):
    """q_target from the captured inputs in float64, every element under its bound.  Stage one-b under the reference's bounds;
    stage two is float32 arithmetic on it, a = lin + bonus (one rounding), t = a + d * V' (two):
    |t - ref| <= bound(bonus) + u |a| + d * bound(V') + 2 u (|a| + |d V'|), u = 2^-24; done: the V' term is 0."""
    assert seen["munchausen"] == (ALPHA, CLIP) == agent.munchausen and seen["temperature"] == TEMP
    st = seen["stats"]
    lo, hi = (t.cpu().numpy() for t in seen["seg"])
    nxt = dict(seg_lo=lo, seg_hi=hi, q=seen["next_q"].float().cpu().numpy(), T=TEMP)
    clo, chi = (t.cpu().numpy() for t in seen["cur_seg"])
    cur = dict(seg_lo=clo, seg_hi=chi, q=seen["cur_q"].cpu().numpy(), T=TEMP, taken_row=seen["taken_row"].cpu().numpy(), alpha=ALPHA, clip_lo=CLIP)
    temps_n = temps_c = None
    if agent.target_temp_relative:                           # each state at its own spread: the temperatures the device formed
        from bridges_hip import dqn_ops
        kw = dict(relative=True, spread_floor=agent.spread_floor)
        temps_n = dqn_ops.soft_value(seen["seg"], seen["next_q"].float().contiguous(), TEMP, **kw)[4].cpu().numpy()
        temps_c = dqn_ops.soft_value(seen["cur_seg"], seen["cur_q"], TEMP, **kw)[4].cpu().numpy()
        # (stage one sums its spread over four waves, the value operator over one: the same T_e but for the order of the sums)
        assert np.allclose(temps_n, st["temp_out"].cpu().numpy(), rtol=1e-12, atol=0) and len(set(temps_c.tolist())) > 1
    ref_n, ref_c = M.reference(nxt, temps=temps_n), M.reference(cur, temps=temps_c)
    figures = {}
    bad = M.violations(dict(value=st["soft_value"].cpu().numpy()), ref_n, figures, taken=False)
    got_c = {k: st[k].cpu().numpy() for k in ("tlogp", "bonus", "miss")}
    got_c["value"] = ref_c["value"].astype(np.float32)       # (the value over s is not handed on)
    bad += M.violations(got_c, ref_c, figures)
    print("stage one-b, largest |error| / bound:", figures)
    assert not bad, bad[:5]
    assert not ref_c["miss"][:n].any()                       # every taken action was found
    done = seen["done"].cpu().numpy().astype(bool)
    lin = seen["lin"].double().cpu().numpy()
    d = float(np.float32(agent.gamma))
    assert (done | ~ref_n["nothing"]).all()
    a = lin + ref_c["bonus"]
    v = np.where(done, 0.0, ref_n["value"])
    want = a + d * v
    bound = (S.half_ulp32(ref_c["bonus"]) + ref_c["bonus_bound"] + U32 * np.abs(a)
             + np.where(done, 0.0, d * (S.half_ulp32(ref_n["value"]) + ref_n["value_bound"])) + 2 * U32 * (np.abs(a) + np.abs(d * v)))
    got = batch.q_target.double().cpu().numpy()
    err = np.abs(got - want[:n])
    print("q_target: largest error", float(err.max()), "largest error / bound", float((err / bound[:n]).max()))
    assert (err <= bound[:n]).all()
    assert (ref_c["bonus"][:n] < 0).any() and not done[:n].all()
    return ref_n, ref_c


def rollout(agent):
    for _ in range(LOCKSTEPS):
        agent.lockstep(0)


# ------------------------------------------------------------------------------------------------------------ q_target and sf_target
def test_factored_mlp_q_target_recomputed_and_sf_target_the_soft_loops():
    agent = mlp_agent(tower_env(f32_rasters=False), **OPTION)
    perturb_last_layer(agent.target_net, scale=3.0)
    batch, seen, n = captured_targets(agent, locksteps=LOCKSTEPS)
    ref_n, ref_c = recompute_q(agent, batch, seen, n)
    # the same records and nets through the soft-target loop: its sf_target, bit for bit, and another q_target
    soft = mlp_agent(tower_env(f32_rasters=False), target_temperature=TEMP)
    perturb_last_layer(soft.target_net, scale=3.0)           # (the same seeded noise; every lock-step then moves both alike)
    rollout(soft)
    assert torch.equal(soft.ring.data, agent.ring.data)
    for p, q in zip(soft.target_net.parameters(), agent.target_net.parameters()):
        assert torch.equal(p, q)
    rec = soft.ring.sample(n, soft.sample_gen, False)
    want = soft._targets(rec)
    assert torch.equal(want.sf_target, batch.sf_target) and torch.equal(want.state_bits, batch.state_bits)
    assert not torch.equal(want.q_target, batch.q_target)
    # V_T >= E[q]: the entropy bonus of the bootstrap
    live = ~seen["done"].cpu().numpy().astype(bool)
    assert (seen["stats"]["soft_value"].cpu().numpy()[live] >= seen["stats"]["value"].cpu().numpy()[live] - 1e-5).all()


def test_relative_temperatures_give_each_state_its_own_spread():
    agent = mlp_agent(tower_env(f32_rasters=False), target_temp_relative=True, spread_floor=1e-6, **OPTION)
    perturb_last_layer(agent.target_net)
    batch, seen, n = captured_targets(agent, locksteps=LOCKSTEPS)
    recompute_q(agent, batch, seen, n)
    assert seen["relative"] is True and seen["spread_floor"] == 1e-6


def missed_on(agent, n=TRAIN_STEPS * BATCH):
    batch, seen, n = captured_targets(agent, n=n, locksteps=LOCKSTEPS)
    st = seen["stats"]
    assert bool(torch.isfinite(batch.q_target).all())
    rows = seen["cur_q"].numel()
    taken = seen["taken_row"][:n]
    lo, hi = seen["cur_seg"]
    assert bool(((taken >= lo[:n]) & (taken < hi[:n]) & (taken < rows)).all())
    assert bool((st["tlogp"][:n] <= 0).all()) and bool((st["bonus"][:n] >= ALPHA * CLIP - 1e-6).all())
    return int(st["miss"][:n].sum()), seen


def test_every_action_is_found_mlp_on_per_env_tasks_and_obstacles():
    missed, seen = missed_on(mlp_agent(random_env(3, 2), per_env_tasks=True, per_env_obstacles=True, **OPTION))
    assert missed == 0


def test_every_action_is_found_convnet_with_task_channels():
    from robotoddler.training.successor_dqn import build_parser, make_nets
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    tgt.load_state_dict(pol.state_dict())
    agent = conv_agent(random_env(3, 0), nets=(pol, tgt), per_env_tasks=True, task_channels=True, **OPTION)
    missed, seen = missed_on(agent, n=BATCH)
    assert missed == 0


def test_every_action_is_found_with_stable_actions_only():
    agent = mlp_agent(tower_env(f32_rasters=False, stable_actions_only=True), stable_actions_only=True, **OPTION)
    missed, seen = missed_on(agent)
    assert missed == 0 and agent.replay_env_s.stable_actions_only


def test_every_action_is_found_with_hindsight_rows_in_the_ring():
    agent = mlp_agent(random_env(3, 0), per_env_tasks=True, hindsight="final", **OPTION)
    pushed = 0
    for _ in range(LOCKSTEPS + MAX_STEPS):                   # (long enough for episodes to end and be relabelled)
        agent.lockstep(0)
        pushed += agent.hindsight_rows
    assert pushed > 0
    missed, seen = missed_on(agent)
    assert missed == 0


# ------------------------------------------------------------------------------------------------------------ it trains; the log keys
def test_the_loop_trains_and_logs_its_three_keys():
    agent = mlp_agent(tower_env(f32_rasters=False), **OPTION)
    losses = []
    for _ in range(LOCKSTEPS):
        losses += agent.lockstep(TRAIN_STEPS)[0]
    assert len(losses) >= 2 * TRAIN_STEPS and all(np.isfinite(losses))
    assert agent.munchausen_missed == 0.0 and ALPHA * CLIP - 1e-6 <= agent.munchausen_bonus <= 0.0
    assert 0.0 <= agent.munchausen_clipped <= 1.0 and agent.target_entropy > 0
    deferred = agent.lockstep(TRAIN_STEPS, defer_losses=True)[0]
    assert len(deferred.get()) == TRAIN_STEPS and deferred.soft["munchausen_missed"] == 0.0
    assert set(deferred.soft) == {"target_entropy", "soft_value_gap", "munchausen_bonus", "munchausen_clipped", "munchausen_missed"}


def test_deferred_and_immediate_losses_decode_the_longest_tail_alike():
    """Two agents of one seed side by side, the losses of one deferred: the same losses and the same six means behind them."""
    from robotoddler.training.vec_dqn import MUNCHAUSEN_KEYS, RELATIVE_TARGET_KEYS, SOFT_TARGET_KEYS
    keys = SOFT_TARGET_KEYS + RELATIVE_TARGET_KEYS + MUNCHAUSEN_KEYS
    now, later = (mlp_agent(tower_env(f32_rasters=False), target_temp_relative=True, **OPTION) for _ in range(2))
    losses = {now: [], later: []}
    for _ in range(LOCKSTEPS):
        losses[now] += now.lockstep(TRAIN_STEPS)[0]
        deferred = later.lockstep(TRAIN_STEPS, defer_losses=True)[0]
        losses[later] += deferred.get()
        assert deferred.soft is None or tuple(deferred.soft) == keys
        assert [getattr(now, k) for k in keys] == [getattr(later, k) for k in keys]
    assert len(losses[now]) >= 2 * TRAIN_STEPS and losses[now] == losses[later]
    assert len(keys) == 6 and all(isinstance(getattr(now, k), float) for k in keys) and later.soft_value_gap == deferred.soft["soft_value_gap"]


# ------------------------------------------------------------------------------------------------------------ option off
def test_the_options_unset_are_the_loop_it_was(monkeypatch):
    from bridges_hip import dqn_ops
    launches = []
    for name in ("soft_value", "action_row"):
        inner = getattr(dqn_ops, name)
        monkeypatch.setattr(dqn_ops, name, lambda *a, _inner=inner, **kw: launches.append(1) or _inner(*a, **kw))

    def run(**kw):
        agent = mlp_agent(tower_env(f32_rasters=False), **kw)
        losses = []
        for _ in range(LOCKSTEPS):
            losses += agent.lockstep(TRAIN_STEPS)[0]
        torch.cuda.synchronize()
        return agent, [float(l).hex() for l in losses]
    a, la = run(target_temperature=TEMP)
    b, lb = run(target_temperature=TEMP, munchausen_alpha=None, munchausen_clip=None)
    assert not launches and b.munchausen is None and b.replay_env_s is None and b.munchausen_bonus is None
    assert la == lb and len(la) >= 2 * TRAIN_STEPS and a.ring.size == b.ring.size and torch.equal(a.ring.data, b.ring.data)
    for p, q in zip(list(a.policy_net.parameters()) + list(a.target_net.parameters()),
                    list(b.policy_net.parameters()) + list(b.target_net.parameters())):
        assert torch.equal(p, q)
    c, lc = run(**OPTION)
    assert launches and lc != la and all(np.isfinite(float.fromhex(x)) for x in lc)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_construction_refusals():
    env = tower_env(f32_rasters=False)
    for kw, word in ((dict(munchausen_alpha=ALPHA), "target_temperature"),
                     (dict(munchausen_alpha=ALPHA, target_temperature=TEMP, double_q=True), "double_q"),
                     (dict(munchausen_alpha=ALPHA, target_temperature=TEMP, n_step=2), "n_step"),
                     (dict(munchausen_clip=CLIP, target_temperature=TEMP), "munchausen_alpha"),
                     (dict(munchausen_alpha=1.5, target_temperature=TEMP), "munchausen_alpha"),
                     (dict(munchausen_alpha=ALPHA, munchausen_clip=0.5, target_temperature=TEMP), "munchausen_clip")):
        with pytest.raises(ValueError, match=word):
            mlp_agent(env, **kw)


def test_checkpoint_is_refused_under_another_setting(tmp_path):
    env = tower_env(f32_rasters=False)
    with_option, soft = mlp_agent(env, **OPTION), mlp_agent(env, target_temperature=TEMP)
    other = mlp_agent(env, target_temperature=TEMP, munchausen_alpha=ALPHA, munchausen_clip=-0.5)
    paths = {}
    for name, agent in (("option", with_option), ("soft", soft), ("other", other)):
        paths[name] = str(tmp_path / f"{name}.pt")
        agent.save_extra(paths[name], lockstep=2)
    assert tuple(torch.load(paths["option"], weights_only=True)["munchausen"]) == (ALPHA, CLIP)
    assert "munchausen" not in torch.load(paths["soft"], weights_only=True)
    assert with_option.load_extra(paths["option"]) == soft.load_extra(paths["soft"]) == dict(lockstep=2)
    for agent, path in ((with_option, "soft"), (soft, "option"), (with_option, "other"), (other, "option")):
        with pytest.raises(ValueError, match="munchausen"):
            agent.load_extra(paths[path])
