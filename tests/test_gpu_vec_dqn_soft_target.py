"""GPU: expected-value targets in the vectorised DQN (VecDQN(target_temperature=T)).  What _targets fed the operator is captured
and the targets are recomputed from it in float64 (tests/soft_target_ref.py: the rule and its bound); the option off is the loop
it was, bit for bit; the loop trains with it; its checkpoint is refused under another setting; no new host wait."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_conformance as M
import soft_target_ref as S
from gpu_helpers import U32
from test_gpu_vec_dqn_tasks import ROOT, make_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.8
H = 0.8
RANGE = ((-3.0, 3.0), (0.3, 2.5))
E, BATCH, TRAIN_STEPS, MAX_STEPS = 64, 16, 3, 8
LOSS = "mse_q_values+mse_block_features"


def tower_env(**kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)], [(0.5, 0, 2 * H + H / 2)],
                          max_steps=MAX_STEPS, seed=0, **kw)


def random_env(T=3, O=2):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomObstacles, RandomTargets, VecAssemblyGym
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], RandomObstacles([RANGE] * O) if O else [], RandomTargets(T),
                          max_steps=MAX_STEPS, seed=0, f32_rasters=False)


def mlp_agent(env, loss=LOSS, **kw):
    from robotoddler.training.vec_dqn import VecDQN
    pol, tgt = make_mlp(seed=0), make_mlp(seed=0)
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 8192, BATCH, GAMMA, 0.01, loss, seed=3, **kw)


def conv_agent(env, nets=None, **kw):
    from robotoddler.models.cv import ConvNet
    from robotoddler.training.vec_dqn import VecDQN
    from robotoddler.utils.utils import init_weights
    if nets is None:
        nets = []
        for _ in range(2):
            torch.manual_seed(0)
            net = ConvNet(img_size=(64, 64)).to(DEV)
            net.apply(init_weights)
            nets.append(net)
    return VecDQN(nets[0], nets[1], torch.optim.Adam(nets[0].parameters(), lr=1e-4, fused=True), env, 8192, BATCH, GAMMA, 0.01,
                  "mse_q_values", seed=3, **kw)


def perturb_last_layer(net, seed=1, scale=30.0):
    """Seeded noise on the last layer, far above its weights, so that the net orders a state's candidates on its own."""
    last = [m for m in net.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))][-1]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        last.weight.add_((torch.randn(last.weight.shape, generator=g) * scale * float(last.weight.abs().mean())).to(DEV))


def captured_targets(agent, n=TRAIN_STEPS * BATCH, locksteps=4):
    """A few lock-steps without optimiser steps, one sample of n records, _targets on it -> (batch, what next_targets was given)."""
    from bridges_hip import dqn_ops
    for _ in range(locksteps):
        agent.lockstep(0)
    rec = agent.ring.sample(n, agent.sample_gen, False)
    seen, inner = {}, dqn_ops.next_targets

    def next_targets(seg, next_q, done, gamma, **kw):
        seen.update(seg=seg, next_q=next_q.clone(), done=done.clone(), gamma=gamma,
                    **{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items() if k != "stats"})
        out = inner(seg, next_q, done, gamma, **kw)
        seen["stats"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw["stats"].items()}
        return out
    dqn_ops.next_targets = next_targets
    try:
        batch = agent._targets(rec)
    finally:
        dqn_ops.next_targets = inner
    torch.cuda.synchronize()
    return batch, seen, n


def recompute(agent, batch, seen, n, factored):
    """q_target and sf_target from the captured inputs in float64, every element under its bound:
    stage one under the reference's bound (tests/soft_target_ref.py); stage two is two float32 operations on it,
    t = a + d * s:  |t - ref| <= d * bound(s) + 2 u (|a| + |d s|), exact where done.
    The factored path: the captured last-hidden rows averaged in float64 and put through the psi' head in float64; the head's own
    float32 error is granted the bound of mlp_conformance.lin_forward_ref (the forward-error bound of the linear layer kernels'
    conformance test, K = the hidden width), taken at the float32 mean the head was given."""
    lo, hi = (t.cpu().numpy() for t in seen["seg"])
    sel = seen["select_q"] if seen.get("select_q") is not None else seen["next_q"]
    feat = seen.get("next_feat")
    feat_np = None
    if feat is not None:
        feat_np = feat.cpu().numpy()                                             # (the values; a strided view arrives contiguous here)
    nq_np = seen["next_q"].float().cpu().numpy()
    case = dict(seg_lo=lo, seg_hi=hi, select_q=nq_np if seen.get("select_q") is None else sel.float().cpu().numpy(), next_q=nq_np,
                T=seen["temperature"], feat=feat_np, feat_row=seen["feat_row"].cpu().numpy() if seen.get("feat_row") is not None else None)
    assert seen["temperature"] == agent.target_temperature
    ref = S.reference(case)
    st = seen["stats"]
    got = dict(value=st["value"].cpu().numpy(), entropy=st["entropy"].cpu().numpy(), argmax_row=st["argmax_row"].cpu().numpy(),
               feat_mean=st["feat_mean"].cpu().numpy() if st["feat_mean"] is not None else np.zeros((len(lo), 0), np.float32))
    figures = {}
    bad = S.violations(got, ref, figures)
    print("stage one, largest |error| / bound:", figures)
    assert not bad, bad[:5]
    EE = len(lo)
    done = seen["done"].cpu().numpy().astype(bool)
    lin = seen["lin"].double().cpu().numpy()
    d = (seen["discount"].double().cpu().numpy() if seen.get("discount") is not None
         else np.full(EE, float(np.float32(agent.gamma))))
    assert (done | ~ref["nothing"]).all()                                        # a transition that is not done has a next row
    v = np.where(done, 0.0, ref["value"])
    want_q = lin + d * v
    bound_q = np.where(done, 0.0, d * (S.half_ulp32(ref["value"]) + ref["value_bound"]) + 2 * U32 * (np.abs(lin) + np.abs(d * v)))
    got_q = batch.q_target.double().cpu().numpy()
    err = np.abs(got_q - want_q[:n])
    print("q_target: largest error", float(err.max()), "largest error / bound", float((err / np.maximum(bound_q[:n], 1e-300)).max()))
    assert (err <= bound_q[:n]).all()
    assert not done[:n].all() and (np.abs(want_q[:n][~done[:n]] - lin[:n][~done[:n]]) > 0).any()   # something was bootstrapped
    if batch.sf_target is None:
        assert feat is None
        return ref, seen
    act = seen["action_raster"].reshape(EE, -1).double().cpu().numpy()
    mean64 = ref["feat_mean"]
    mean_bound = S.half_ulp32(mean64) + ref["feat_mean_bound"]
    if factored:
        net = agent.target_net
        last = [m for m in net.mlp.layers if isinstance(m, torch.nn.Linear)][-1]
        px = 64 * 64
        W, b = last.weight[:px].detach(), last.bias[:px].detach()
        assert seen["feat_head"] is not None and feat.shape[1] == W.shape[1]
        psi = mean64 @ W.double().cpu().numpy().T + b.double().cpu().numpy()
        _, head_bound = M.lin_forward_ref(st["feat_mean"], W, b, False)
        psi_bound = head_bound.double().cpu().numpy() + mean_bound @ np.abs(W.double().cpu().numpy()).T
    else:
        assert seen["feat_head"] is None
        psi, psi_bound = mean64, mean_bound
    live = ~done
    want_sf = act + d[:, None] * np.where(live[:, None], psi, 0.0)
    bound_sf = np.where(live[:, None], d[:, None] * psi_bound + 2 * U32 * (np.abs(act) + np.abs(d[:, None] * psi)), 0.0)
    got_sf = batch.sf_target.double().cpu().numpy().reshape(n, -1)
    err = np.abs(got_sf - want_sf[:n])
    print("sf_target: largest error", float(err.max()), "largest error / bound", float((err / np.maximum(bound_sf[:n], 1e-300)).max()))
    assert (err <= bound_sf[:n]).all()
    return ref, seen


# ------------------------------------------------------------------------------------------------------------ the four cases
def test_factored_mlp_on_the_fixed_tower():
    agent = mlp_agent(tower_env(f32_rasters=False), target_temperature=0.5)
    batch, seen, n = captured_targets(agent)
    ref, seen = recompute(agent, batch, seen, n, factored=True)
    assert seen.get("select_q") is None and seen["next_feat"].shape[0] == seen["next_q"].numel()     # h_last of ALL next-state rows
    assert float(ref["entropy"].max()) > 0.1                                     # the policy is not the arg-max: rows were averaged


def test_factored_mlp_on_random_tasks_and_obstacles_with_three_step_double_q():
    agent = mlp_agent(random_env(3, 2), per_env_tasks=True, per_env_obstacles=True, n_step=3, double_q=True, target_temperature=0.5)
    perturb_last_layer(agent.policy_net)
    batch, seen, n = captured_targets(agent)
    recompute(agent, batch, seen, n, factored=True)
    assert seen["select_q"] is not None and not torch.equal(seen["select_q"], seen["next_q"])        # the policy net weighs the rows
    assert seen["discount"] is not None and len(set(seen["discount"].tolist())) > 1                   # gamma^h per row, unchanged


def test_convnet_on_f32_rasters():
    agent = conv_agent(tower_env(f32_rasters=True), target_temperature=0.5)
    batch, seen, n = captured_targets(agent)
    recompute(agent, batch, seen, n, factored=False)
    assert batch.sf_target is None


def test_convnet_with_task_channels_finds_the_distinct_rows_once(monkeypatch):
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    tgt.load_state_dict(pol.state_dict())
    agent = conv_agent(random_env(3, 0), nets=(pol, tgt), per_env_tasks=True, task_channels=True, double_q=True, target_temperature=0.5)
    calls, inner = [], VecDQN._distinct_rows
    batch, seen, n = captured_targets(agent)
    recompute(agent, batch, seen, n, factored=False)
    monkeypatch.setattr(VecDQN, "_distinct_rows", lambda self, *a: calls.append(1) or inner(self, *a))
    agent._targets(agent.ring.sample(n, agent.sample_gen, False))
    assert len(calls) == 1                                                       # hashed and grouped once for both forwards


def test_module_forward_mlp_averages_the_distinct_rows_through_the_inverse_map(monkeypatch):
    """A SuccessorMLP fed through _forward_rows (the path of the U-Net and of other image sizes): feat = channel 0 of the DISTINCT
    rows' outputs (a strided view, 4096 wide), feat_row = the inverse map of the de-duplication."""
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "FACTORED_ACTING", False)
    agent = mlp_agent(tower_env(f32_rasters=True), target_temperature=0.5)
    batch, seen, n = captured_targets(agent)
    recompute(agent, batch, seen, n, factored=False)
    assert seen["feat_row"] is not None and seen["next_feat"].shape == (int(seen["feat_row"].max()) + 1, 4096)
    assert seen["next_feat"].shape[0] < seen["next_q"].numel()                   # rows were shared


# ------------------------------------------------------------------------------------------------------------ option off
def test_target_temperature_none_is_the_loop_it_was(monkeypatch):
    from bridges_hip import dqn_ops
    launches, inner = [], dqn_ops.soft_expect
    monkeypatch.setattr(dqn_ops, "soft_expect", lambda *a, **kw: launches.append(1) or inner(*a, **kw))

    def run(**kw):
        agent = mlp_agent(tower_env(f32_rasters=False), **kw)
        losses = []
        for _ in range(3):
            losses += agent.lockstep(TRAIN_STEPS)[0]
        torch.cuda.synchronize()
        return agent, [float(l).hex() for l in losses]
    a, la = run()
    b, lb = run(target_temperature=None)
    assert not launches
    assert la == lb and len(la) >= 2 * TRAIN_STEPS and a.ring.size == b.ring.size and torch.equal(a.ring.data, b.ring.data)
    for p, q in zip(a.policy_net.parameters(), b.policy_net.parameters()):
        assert torch.equal(p, q)
    for p, q in zip(a.target_net.parameters(), b.target_net.parameters()):
        assert torch.equal(p, q)
    assert b.target_entropy is None and b.soft_value_gap is None
    c, lc = run(target_temperature=0.5)
    assert launches and lc != la and all(np.isfinite(float.fromhex(x)) for x in lc)
    assert c.target_entropy is not None and c.target_entropy > 0 and c.soft_value_gap >= -1e-6           # E[q] <= max q


# ------------------------------------------------------------------------------------------------------------ it trains
LOOP = ["--model", "SuccessorMLP", "--loss_function", LOSS, "--tower_height", "2", "--max_steps", "8",
        "--num_envs", "64", "--num_training_steps", "3", "--batch_size", "16", "--seed", "3", "--learning_rate", "1e-4", "--gamma", "0.8",
        "--checkpoint_every", "200", "--replay_buffer_capacity", "30000"]


def test_the_loop_trains_with_the_option_and_its_checkpoint_is_refused_without(tmp_path):
    from robotoddler.training.successor_dqn import build_parser, main
    from robotoddler.training.vec_dqn import run_vectorised
    args = vars(build_parser().parse_args([*LOOP, "--target_temperature", "0.5", "--num_episodes", "300", "--save_checkpoint", str(tmp_path)]))
    hist, agent = run_vectorised(args, torch.device(DEV), return_agent=True)
    assert agent.target_temperature == 0.5 and len(hist) >= 4
    losses = [h["avg_loss"] for h in hist if h["avg_loss"] is not None]
    assert len(losses) >= 3 and all(np.isfinite(losses)) and min(losses) >= 0
    logged = [h for h in hist if "target_entropy" in h]
    assert len(logged) == len(losses) and all(np.isfinite(h["target_entropy"]) and np.isfinite(h["soft_value_gap"]) for h in logged)
    assert all(h["target_entropy"] >= 0 and h["soft_value_gap"] >= -1e-6 for h in logged)
    ckpts = sorted(int(d) for d in os.listdir(tmp_path) if d.isdigit())
    assert ckpts
    first = os.path.join(str(tmp_path), str(ckpts[0]))
    with pytest.raises(ValueError, match="target_temperature"):                  # resumed with the option off
        main([*LOOP, "--num_episodes", str(ckpts[0] + 64), "--load_checkpoint", first])
    with pytest.raises(ValueError, match="target_temperature"):                  # ... and under another temperature
        main([*LOOP, "--target_temperature", "0.25", "--num_episodes", str(ckpts[0] + 64), "--load_checkpoint", first])
    # the other way round: a plain agent's file is refused by the agent with the option
    plain = mlp_agent(tower_env(f32_rasters=False))
    path = str(tmp_path / "plain_agent.pt")
    plain.save_extra(path, lockstep=1)
    assert "target_temperature" not in torch.load(path, weights_only=True)
    with pytest.raises(ValueError, match="target_temperature"):
        agent.load_extra(path)
    assert plain.load_extra(path) == dict(lockstep=1)
    more = main([*LOOP, "--target_temperature", "0.5", "--num_episodes", str(ckpts[0] + 64), "--load_checkpoint", first])
    assert more and more[-1]["episodes"] >= ckpts[0] + 64


# ------------------------------------------------------------------------------------------------------------ no new wait
def test_find_syncs_counts_no_new_host_wait():
    """tools/find_syncs.py reports the same number of host waits per lock-step with --target_temperature as without.  One child
    process runs at a time."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "BRIDGES_DIST_BACKEND")}
    counts = {}
    for name, extra in (("plain", []), ("soft", ["--target_temperature", "1.0"])):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "find_syncs.py"), "--envs", "64", *extra], env=env,
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        m = re.search(r"^(\d+) synchronising calls in one lock-step", out.stdout, flags=re.M)
        assert m, out.stdout[-2000:]
        counts[name] = int(m.group(1))
        print(name, counts[name], "host waits per lock-step")
    assert counts["soft"] == counts["plain"], counts
