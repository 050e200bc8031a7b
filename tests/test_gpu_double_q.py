"""GPU: double Q-learning targets of the vectorised DQN (VecDQN(double_q=True)) -- the target kernel that selects a transition's
next row by one value vector and values it by another (bridges_td_target_select), the operator layer, and the loop that feeds it
the policy net's q.  Probe, float64 reference, bound and the plain float32 statement come from tests/double_q_ref.py (checked
without a GPU by tests/test_cpu_double_q.py, which also shows that the defective twins are rejected)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import double_q_ref as Q
from gpu_helpers import U32
from mlp_conformance import NO_ROW
from nstep_ref import row_discounts
from robotoddler.training import records as R
from test_gpu_vec_dqn_tasks import ROOT, make_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.8
H = 0.8
RANGE = ((-3.0, 3.0), (0.3, 2.5))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def segments(pr):
    return (torch.tensor(pr["lo"], dtype=torch.int32, device=DEV), torch.tensor(pr["hi"], dtype=torch.int32, device=DEV))


def run_select(pr, d, select_q, seg=None, n=None):
    """dqn_ops.td_target on the probe (the first n transitions); d a scalar gamma or a per-row discount -> (q, sf, rows list)."""
    from bridges_hip import dqn_ops
    n = len(pr["lo"]) if n is None else n
    rows_form = torch.is_tensor(d)
    q, sf, rows = dqn_ops.td_target(seg if seg is not None else segments(pr), pr["next_q"], pr["lin"][:n], torch.tensor(pr["done"][:n], device=DEV),
                                    123.0 if rows_form else d, next_sf=pr["next_sf"], action_raster=None if pr["act"] is None else pr["act"][:n],
                                    discount=d[:n] if rows_form else None, select_q=select_q)
    return q, sf, rows.cpu().tolist()


# ------------------------------------------------------------------------------------------------------------ 1: the kernel
@pytest.mark.parametrize("form", ["scalar", "rows"])
@pytest.mark.parametrize("strided", [True, False])
@pytest.mark.parametrize("sf_dim", Q.SELECT_SF_DIMS)
def test_kernel_on_the_probe(sf_dim, strided, form):
    """Rows exact, q and sf within 2 u (|a| + |d s|) of the float64 statement (exact where done and where the target is infinite),
    for sf_dim 0, 4, 6 (rows of 24 bytes: the element-wise epilogue), 64 and 4096, next_sf strided and contiguous, the scalar gamma
    and a per-row discount with more than two distinct values, (lo, hi) pairs with shared ranges and the prefix-sum form."""
    pr = Q.select_probe(sf_dim, DEV, strided=strided)
    B = len(pr["lo"])
    d = GAMMA if form == "scalar" else row_discounts(B, GAMMA).to(DEV)
    assert form == "scalar" or len(set(d.tolist())) > 2
    ref, rows = Q.td_select_ref(pr, d)
    got = run_select(pr, d, pr["select_q"])
    Q.select_conform("td_select", got, Q.td_select_plain(pr, d), ref, rows, (sf_dim, strided, form))
    dn = torch.tensor(pr["done"], device=DEV)
    assert torch.equal(got[0][dn], pr["lin"][dn]) and rows[7] == NO_ROW
    if sf_dim:
        assert torch.equal(got[1][dn], pr["act"].reshape(B, -1)[dn])
    # the prefix-sum form over the back-to-back transitions 0..7: what the pairs gave for them
    seg = torch.tensor(pr["lo"][:8] + [pr["hi"][7]], dtype=torch.int32, device=DEV)
    again = run_select(pr, d, pr["select_q"], seg=seg, n=8)
    assert again[2] == got[2][:8] and torch.equal(again[0], got[0][:8]) and (sf_dim == 0 or torch.equal(again[1], got[1][:8]))


# ------------------------------------------------------------------------------------------------------------ 2: identity
@pytest.mark.parametrize("form", ["scalar", "rows"])
@pytest.mark.parametrize("sf_dim", [0, 4, 64, 4096])
def test_select_q_equal_to_next_q_is_the_plain_target_bit_for_bit(sf_dim, form):
    # both sides launch one kernel (k_td_target<PER_ROW>) now; the independent evidence is test_gpu_twin_kernels_golden.py
    for strided in (True, False):
        pr = Q.select_probe(sf_dim, DEV, strided=strided)
        d = GAMMA if form == "scalar" else row_discounts(len(pr["lo"]), GAMMA).to(DEV)
        want = run_select(pr, d, None)                                    # bridges_td_target / bridges_td_target_rows
        for select_q in (pr["next_q"].clone(), pr["next_q"]):             # equal values, and the same pointer
            got = run_select(pr, d, select_q)
            assert got[2] == want[2] and torch.equal(got[0], want[0]) and (sf_dim == 0 or torch.equal(got[1], want[1]))


def test_next_targets_selects_in_the_call_that_finds_the_rows():
    from bridges_hip import dqn_ops
    pr = Q.select_probe(4096, DEV)
    B = len(pr["lo"])
    done = torch.tensor(pr["done"], device=DEV)
    for d in (None, row_discounts(B, GAMMA).to(DEV)):
        want = run_select(pr, GAMMA if d is None else d, pr["select_q"])
        for next_sf in (lambda best: pr["next_sf"][best].contiguous(), pr["next_sf"]):       # psi' of the arg-max rows, or of every row
            q, sf = dqn_ops.next_targets(segments(pr), pr["next_q"], done, GAMMA, next_sf=next_sf, action_raster=pr["act"], lin=pr["lin"],
                                         discount=d, select_q=pr["select_q"])
            assert torch.equal(q, want[0]) and torch.equal(sf, want[1])
    with pytest.raises(ValueError, match="lin"):
        dqn_ops.next_targets(segments(pr), pr["next_q"], done, GAMMA, select_q=pr["select_q"])


# ------------------------------------------------------------------------------------------------------------ 3: refusals
def test_entry_point_refuses_what_the_header_says_it_refuses():
    from bridges_hip import abi
    L = abi.require_gpu()
    pr = Q.select_probe(4, DEV, strided=False)
    B, D = len(pr["lo"]), 4
    lo, hi = segments(pr)
    done = torch.tensor(pr["done"], device=DEV).to(torch.uint8)
    act = pr["act"].reshape(B, D).contiguous()
    q = torch.full((B,), 7.0, device=DEV)
    sf = torch.full((B, D), 7.0, device=DEV)
    rows = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    disc = torch.full((B,), GAMMA, device=DEV)
    base = dict(n=B, lo=_ptr(lo), hi=_ptr(hi), sel=_ptr(pr["select_q"]), nq=_ptr(pr["next_q"]), nsf=_ptr(pr["next_sf"]), act=_ptr(act),
                lin=_ptr(pr["lin"]), done=_ptr(done), disc=_ptr(disc), D=D, q=_ptr(q), sf=_ptr(sf), rows=_ptr(rows),
                stride=pr["next_sf"].stride(0))

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_td_target_select(a["n"], a["lo"], a["hi"], a["sel"], a["nq"], a["nsf"], a["stride"], a["act"], a["lin"],
                                          a["done"], a["disc"], GAMMA, a["D"], a["q"], a["sf"], a["rows"], abi.current_stream())
    null = C.c_void_p(0)
    bad = [dict(n=-1), dict(D=-1), dict(lo=null), dict(hi=null), dict(sel=null), dict(nq=null), dict(lin=null), dict(done=null),
           dict(q=null), dict(rows=null), dict(nsf=null), dict(act=null), dict(sf=null), dict(stride=-4),
           dict(sel=C.c_void_p(pr["select_q"].data_ptr() + 2))]
    for kw in bad:
        with pytest.raises(abi.BridgesHipError):
            abi.check(call(**kw), "bridges_td_target_select")
        assert "td_target_select" in L.bridges_last_error().decode(), kw
    torch.cuda.synchronize()
    assert bool((q == 7.0).all()) and bool((sf == 7.0).all()) and bool((rows == 7).all())       # a refusal launches nothing
    abi.check(call(n=0), "bridges_td_target_select")                                          # nothing to do is not an error
    abi.check(call(D=0, nsf=null, act=null, sf=null), "bridges_td_target_select")             # sf_dim = 0 needs none of the three
    abi.check(call(disc=null), "bridges_td_target_select")                                    # no discount: the scalar gamma
    torch.cuda.synchronize()
    assert rows.cpu().tolist() == Q.td_select_ref(pr, GAMMA)[1]


# ------------------------------------------------------------------------------------------------------------ 4, 5: the loop
MAX_STEPS = 4
HIDDEN = (16, 8, 16)


def tower_env(E, seed=0, **kw):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)], [(0.5, 0, 2 * H + H / 2)],
                          max_steps=MAX_STEPS, seed=seed, **kw)


def random_env(E, T=3, O=1, seed=0):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomObstacles, RandomTargets, VecAssemblyGym
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], RandomObstacles([RANGE] * O) if O else [], RandomTargets(T),
                          max_steps=MAX_STEPS, seed=seed, f32_rasters=False)


def mlp_agent(env, **kw):
    from robotoddler.training.vec_dqn import VecDQN
    pol, tgt = make_mlp(HIDDEN, seed=0), make_mlp(HIDDEN, seed=0)             # the same state dict
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 4096, 8, GAMMA, 0.01,
                  "mse_q_values+mse_block_features", seed=3, **kw)


def conv_agent(env, **kw):
    from robotoddler.models.cv import ConvNet
    from robotoddler.training.vec_dqn import VecDQN
    from robotoddler.utils.utils import init_weights
    nets = []
    for _ in range(2):
        torch.manual_seed(0)
        net = ConvNet(img_size=(64, 64)).to(DEV)
        net.apply(init_weights)
        nets.append(net)
    return VecDQN(nets[0], nets[1], torch.optim.Adam(nets[0].parameters(), lr=1e-4, fused=True), env, 4096, 8, GAMMA, 0.01, "mse_q_values",
                  seed=3, **kw)


def filled(agent, locksteps=6, n=24):
    """A few lock-steps without optimiser steps, then one sample of n records."""
    for _ in range(locksteps):
        agent.lockstep(0)
    assert len(agent.ring) >= n
    return agent.ring.sample(n, agent.sample_gen, False)


def targets_of(agent, rec, double_q):
    """_targets(rec) with the option set -> (q_target, sf_target or None, what next_targets was called with, rows fed)."""
    from bridges_hip import dqn_ops
    seen, inner_nt, inner_rows = {}, dqn_ops.next_targets, agent._rows

    def next_targets(seg, next_q, done, gamma, **kw):
        seen.update(seg=seg, next_q=next_q.clone(), done=done.clone(), gamma=gamma, **{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()})
        return inner_nt(seg, next_q, done, gamma, **kw)

    def rows(env, stable):
        seen["stable"] = stable.clone()
        return inner_rows(env, stable)
    agent.double_q, agent.rows_fed = double_q, 0
    dqn_ops.next_targets, agent._rows = next_targets, rows
    try:
        out = agent._targets(rec)
    finally:
        dqn_ops.next_targets = inner_nt
        del agent._rows
    torch.cuda.synchronize()
    return out[3].clone(), (out[4].clone() if out[4] is not None else None), seen, agent.rows_fed


def perturb_last_layer(net, seed=1, scale=30.0):
    """Seeded noise on the last layer, ``scale`` times its mean |weight|: far above the weights, so that the perturbed net orders
    the candidates of a state on its own (noise of the weights' size leaves the order of q largely as it was: the candidates of
    one state differ in a few dozen input pixels)."""
    last = [m for m in net.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))][-1]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        last.weight.add_((torch.randn(last.weight.shape, generator=g) * scale * float(last.weight.abs().mean())).to(DEV))


def check_against_torch(agent, rec, q_t, sf_t, seen):
    """(c) the targets against a formulation built here from _net_q of both nets over _rows of the scratch env: the segment
    arg-max (first maximum) of the policy net's q, the target net's q and successor features gathered at it.  Rows exact; values
    within 2 u (|a| + |d s|), zero where done -- a, d and done are what the loop handed to next_targets."""
    renv, n = agent.replay_env, rec.shape[0]
    E = renv.E
    stable = seen["stable"]
    idx, row_env, (lo, hi), _rep = agent._rows(renv, stable)                     # (the cache of the call under test)
    factored = agent._factored(agent.target_net)
    pol_q = agent._net_q(agent.policy_net, renv, idx, row_env, stable).float()
    tgt = agent._net_q(agent.target_net, renv, idx, row_env, stable, return_h=factored)
    tgt_q, h_pre = (tgt if factored else (tgt, None))
    assert torch.equal(seen["select_q"], pol_q) and torch.equal(seen["next_q"], tgt_q.float())
    rows = Q.segment_first_max(pol_q, lo, hi)
    plain_rows = Q.segment_first_max(tgt_q, lo, hi)
    done = seen["done"].cpu().tolist()
    lin = seen["lin"].double().cpu()
    d = seen["discount"].double().cpu() if seen.get("discount") is not None else torch.full((E,), float(np.float32(agent.gamma)), dtype=torch.float64)
    assert all(dn or r != NO_ROW for dn, r in zip(done, rows))
    nq = tgt_q.double().cpu()
    want = torch.tensor([lin[i] if done[i] else lin[i] + d[i] * nq[rows[i]] for i in range(E)], dtype=torch.float64)
    bound = torch.tensor([0.0 if done[i] else 2 * U32 * (abs(float(lin[i])) + abs(float(d[i] * nq[rows[i]]))) for i in range(E)], dtype=torch.float64)
    got = q_t.double().cpu()
    assert bool(((got - want[:n]).abs() <= bound[:n]).all()), float(((got - want[:n]).abs() - bound[:n]).max())
    # the rows: the kernel's own argmax_row for the same inputs, against the host's first maximum
    from bridges_hip import dqn_ops
    _, _, arg = dqn_ops.td_target((lo, hi), seen["next_q"], seen["lin"], seen["done"], agent.gamma, discount=seen.get("discount"),
                                  select_q=seen["select_q"])
    assert arg.cpu().tolist() == rows
    if sf_t is not None:
        live = [i for i in range(n) if not done[i]]
        # psi' as the SAME float32 numbers the loop hands the kernel: one call on the selected rows of all E transitions, the
        # shape of the loop's own call (a GEMM of another shape may round differently, which no bound in u |d s| covers)
        best = torch.tensor(rows, device=DEV).clamp_(0, pol_q.numel() - 1)
        psi = agent.target_net.sf0_from_first_layer(h_pre.index_select(0, best)).double().cpu()[live]
        act = seen["action_raster"].reshape(E, -1).double().cpu()
        got_sf = sf_t.double().cpu().reshape(n, -1)
        for k, i in enumerate(live):
            w = act[i] + d[i] * psi[k]
            b = 2 * U32 * (act[i].abs() + (d[i] * psi[k]).abs())
            assert bool(((got_sf[i] - w).abs() <= b).all()), (i, float(((got_sf[i] - w).abs() - b).max()))
        for i in set(range(n)) - set(live):
            assert torch.equal(got_sf[i], act[i])
    return rows, plain_rows


def loop_case(agent, sf):
    rec = filled(agent)
    agent.target_net.load_state_dict(agent.policy_net.state_dict())          # (the soft updates of the lock-steps round: t = p tau + t (1 - tau))
    # (a) policy net == target net: the option changes nothing, bit for bit; and it feeds the rows twice
    q0, sf0, _, fed0 = targets_of(agent, rec, False)
    q1, sf1, seen, fed1 = targets_of(agent, rec, True)
    assert torch.equal(q0, q1) and (not sf or torch.equal(sf0, sf1)) and (sf0 is not None) == sf
    assert seen["select_q"] is not None and fed0 > 0 and fed1 == 2 * fed0
    # (b) a policy net of its own: some transition's next row, and with it its q target, is another
    perturb_last_layer(agent.policy_net)
    q2, sf2, seen, _ = targets_of(agent, rec, True)
    q3, sf3, plain_seen, _ = targets_of(agent, rec, False)
    assert plain_seen.get("select_q") is None and torch.equal(q3, q0)          # the plain target does not read the policy net
    rows, plain_rows = check_against_torch(agent, rec, q2, sf2, seen)        # (c)
    assert rows != plain_rows and not torch.equal(q2, q0)
    return rows


def test_loop_factored_mlp_on_the_fixed_tower():
    loop_case(mlp_agent(tower_env(16, f32_rasters=False)), sf=True)


def test_loop_factored_mlp_on_per_env_tasks_and_obstacles():
    loop_case(mlp_agent(random_env(16), per_env_tasks=True, per_env_obstacles=True), sf=True)


def test_loop_factored_mlp_with_three_step_returns():
    agent = mlp_agent(tower_env(16, f32_rasters=False), n_step=3)
    loop_case(agent, sf=True)
    assert agent.ring.width == R.RECORD_WIDTH + 1


def test_loop_convnet_on_f32_rasters():
    loop_case(conv_agent(tower_env(8, f32_rasters=True)), sf=False)


def test_loop_convnet_with_task_channels_finds_the_distinct_rows_once(monkeypatch):
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    torch.manual_seed(5)
    pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "ConvNet"])), torch.device(DEV))
    tgt.load_state_dict(pol.state_dict())
    env = random_env(8, T=3, O=0)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 4096, 8, GAMMA, 0.01, "mse_q_values", seed=3,
                   per_env_tasks=True, task_channels=True)
    calls, inner = [], VecDQN._distinct_rows
    monkeypatch.setattr(VecDQN, "_distinct_rows", lambda self, *a: calls.append(1) or inner(self, *a))
    loop_case(agent, sf=False)
    rec = agent.ring.sample(24, agent.sample_gen, False)
    for flag in (False, True):
        del calls[:]
        targets_of(agent, rec, flag)
        assert len(calls) == 1, (flag, len(calls))                           # hashed and grouped once for both forwards


# ------------------------------------------------------------------------------------------------------------ 6: opt-in
def test_double_q_false_is_the_loop_it_was():
    def run(**kw):
        agent = mlp_agent(tower_env(16, f32_rasters=False), **kw)
        losses = []
        for _ in range(4):
            losses += agent.lockstep(2)[0]
        torch.cuda.synchronize()
        return agent, losses
    a, la = run()
    b, lb = run(double_q=False)
    assert la == lb and len(la) >= 4 and a.ring.size == b.ring.size and torch.equal(a.ring.data, b.ring.data)
    for p, q in zip(a.policy_net.parameters(), b.policy_net.parameters()):
        assert torch.equal(p, q)
    for p, q in zip(a.target_net.parameters(), b.target_net.parameters()):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------------------ 7: it trains
LOOP = ["--model", "SuccessorMLP", "--loss_function", "mse_q_values+mse_block_features", "--tower_height", "2", "--max_steps", "4",
        "--num_envs", "64", "--num_training_steps", "2", "--batch_size", "8", "--seed", "3", "--learning_rate", "1e-4", "--gamma", "0.8",
        "--checkpoint_every", "200", "--replay_buffer_capacity", "30000"]


def test_the_loop_trains_with_double_q_and_its_checkpoint_loads_without(tmp_path):
    from robotoddler.training.successor_dqn import build_parser, main
    from robotoddler.training.vec_dqn import run_vectorised
    args = vars(build_parser().parse_args([*LOOP, "--double_q", "--num_episodes", "400", "--save_checkpoint", str(tmp_path)]))
    hist, agent = run_vectorised(args, torch.device(DEV), return_agent=True)
    assert agent.double_q and len(hist) >= 6                                  # at most 64 episodes end per lock-step
    losses = [h["avg_loss"] for h in hist if h["avg_loss"] is not None]
    assert len(losses) >= 3 and all(np.isfinite(losses)) and min(losses) >= 0
    assert agent._graph_state is not None                                     # the captured step, as by default
    ckpts = sorted(int(d) for d in os.listdir(tmp_path) if d.isdigit())
    assert ckpts
    first = os.path.join(str(tmp_path), str(ckpts[0]))
    more = main([*LOOP, "--num_episodes", str(ckpts[0] + 64), "--load_checkpoint", first])        # resumed with the option off
    assert more and more[-1]["episodes"] >= ckpts[0] + 64
    assert all(np.isfinite(h["avg_loss"]) for h in more if h["avg_loss"] is not None)


def test_learning_curve_tool_prints_the_forecast_beside_the_realised_return():
    """tools/learning_curve.py --double_q at a toy size, one child process: every block's line holds the greedy evaluation with
    eval_q_first (the mean q of the rows chosen in the episodes' first step) beside eval_lin_reward, both finite."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "BRIDGES_DIST_BACKEND")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "learning_curve.py"), "--envs", "64", "--locksteps", "4", "--block", "2",
                          "--train_steps", "2", "--max_steps", "4", "--eval_envs", "8", "--double_q", "--n_step", "2"], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [l["lockstep"] for l in lines] == [2, 4]
    for l in lines:
        assert np.isfinite(l["eval_q_first"]) and np.isfinite(l["eval_lin_reward"]) and 0.0 <= l["eval_success_rate"] <= 1.0
        assert l["mean_loss"] is None or np.isfinite(l["mean_loss"])


# ------------------------------------------------------------------------------------------------------------ 8: no new wait
def test_find_syncs_counts_no_new_host_wait():
    """tools/find_syncs.py reports the same number of host waits per lock-step with --double_q as without.  One child process
    runs at a time."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "BRIDGES_DIST_BACKEND")}
    counts = {}
    for name, extra in (("plain", []), ("double_q", ["--double_q"])):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "find_syncs.py"), "--envs", "64", *extra], env=env,
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        m = re.search(r"^(\d+) synchronising calls in one lock-step", out.stdout, flags=re.M)
        assert m, out.stdout[-2000:]
        counts[name] = int(m.group(1))
        print(name, counts[name], "host waits per lock-step")
    assert counts["double_q"] == counts["plain"], counts
