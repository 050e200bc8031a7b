"""GPU: Boltzmann exploration on the device -- the selection kernel (bridges_boltzmann_select) against the float64 statement of
its rule, the operator layer, and the vectorised loop that draws with it (VecDQN(exploration="boltzmann")).  Rule, probe tables
and the probe condition come from tests/boltzmann_ref.py (checked without a GPU by tests/test_cpu_boltzmann.py, which also shows
that the defective twins are rejected and that no random draw lies within the band where the rule has no single answer)."""
import ctypes as C

import numpy as np
import pytest
import torch

import boltzmann_ref as B
from robotoddler.training import records as R
from test_gpu_double_q import conv_agent, mlp_agent, tower_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("sel_compact", "sel_index", "q_sel", "explore_w", "p_sel")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(case, greedy=False):
    from bridges_hip import ops
    out = ops.boltzmann_select((dev(case["seg_lo"]), dev(case["seg_hi"])), dev(case["q"]), dev(case["u"]), case["T"], greedy,
                               dev(case["idx"]), dev(case["cand_offset"]), rep=dev(case.get("rep")))
    return {k: v.cpu().numpy() for k, v in zip(KEYS, out)}


def check(got, ref, what=""):
    """sel_compact, sel_index, explore_w equal; q_sel the same bits; |p_sel - ref| <= 2^-22 ref (one float32 rounding and the
    ulp or two of the device's exp)."""
    for k in ("sel_compact", "sel_index", "explore_w"):
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, (what, k, bad[:8], got[k][bad[:8]], ref[k][bad[:8]])
    assert np.array_equal(got["q_sel"].view(np.int32), ref["q_sel"].view(np.int32)), what
    err = np.abs(got["p_sel"].astype(np.float64) - ref["p_sel"])
    print(what, "envs", len(ref["p_sel"]), "max |p_sel - ref| / ref", float(np.max(err / np.maximum(ref["p_sel"], 1e-300), initial=0.0)))
    assert (err <= 2.0 ** -22 * ref["p_sel"]).all(), (what, float(err.max()))


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("T", B.TEMPERATURES)
def test_random_probes(T):
    case = B.random_probe(T)
    check(run(case), B.reference(case), f"T={T}")


def test_exact_probes_every_boundary_of_the_strict_rule():
    case, want = B.exact_probe()
    got = run(case)
    assert np.array_equal(got["sel_compact"], case["idx"][want])                                   # row lo + k for u = k / n
    check(got, B.reference(case), "exact")
    assert np.array_equal(got["p_sel"], (1.0 / (case["seg_hi"] - case["seg_lo"])).astype(np.float32))


@pytest.mark.parametrize("i", range(len(B.NONFINITE) + len(B.NONFINITE_EXACT)))
def test_non_finite_probes(i):
    case = (B.nonfinite_probe() + B.nonfinite_probe(B.NONFINITE_EXACT))[i]
    check(run(case), B.reference(case), f"non-finite {i}")


def test_shared_rows_every_env_draws_with_its_own_u_and_the_call_is_deterministic():
    case = B.shared_probe()
    ref = B.reference(case)
    got, again = run(case), run(case)
    check(got, ref, "shared")
    assert len(case["u"]) == 4096 and len(set(got["sel_compact"].tolist())) > 64
    assert (got["sel_index"] == got["sel_compact"] - case["cand_offset"][5]).all()                 # the REPRESENTATIVE's offset
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k                   # the same bits


@pytest.mark.parametrize("T", (0.1, 1e30))
def test_greedy_is_the_greedy_branch_of_eps_greedy_select(T):
    from bridges_hip import ops
    for case in (B.random_probe(T), B.shared_probe(E=256), B.nonfinite_probe()[0]):
        got = run(case, greedy=True)
        seg = (dev(case["seg_lo"]), dev(case["seg_hi"]))
        q = dev(case["q"])
        want = ops.eps_greedy_select(seg, q, torch.zeros_like(q), dev(case["u"]), 0.5, True, dev(case["idx"]), dev(case["cand_offset"]),
                                     rep=dev(case.get("rep")))
        for k, w in zip(KEYS[:3], want[:3]):
            assert np.array_equal(got[k].view(np.uint8), w.cpu().numpy().view(np.uint8)), k
        has = case["seg_hi"] > case["seg_lo"]
        assert (got["explore_w"] == 0).all() and np.array_equal(got["p_sel"], has.astype(np.float32))


def test_refusals_launch_nothing():
    from bridges_hip import abi, ops
    L = abi.require_gpu()
    case = B.random_probe(1.0)
    E, n = len(case["u"]), len(case["q"])
    t = {k: dev(case[k]) for k in ("seg_lo", "seg_hi", "q", "u", "idx", "cand_offset")}
    outs = dict(sel_compact=torch.full((E,), 7, dtype=torch.int64, device=DEV), sel_index=torch.full((E,), 7, dtype=torch.int32, device=DEV),
                **{k: torch.full((E,), 7.0, device=DEV) for k in ("q_sel", "explore_w", "p_sel")})
    ptr = lambda x: C.c_void_p(x.data_ptr())
    base = dict(E=E, n=n, T=1.0, **{k: ptr(v) for k, v in t.items()}, **{k: ptr(v) for k, v in outs.items()})

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_boltzmann_select(a["E"], a["n"], a["seg_lo"], a["seg_hi"], a["q"], a["u"], a["T"], 0, a["idx"], a["cand_offset"],
                                          None, a["sel_compact"], a["sel_index"], a["q_sel"], a["explore_w"], a["p_sel"],
                                          abi.current_stream())
    null = C.c_void_p(0)
    bad = [dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(T=-float("inf")), dict(n=0), dict(n=-3),
           dict(E=-1)] + [{k: null} for k in list(t) + list(outs)]
    for kw in bad:
        with pytest.raises(abi.BridgesHipError):
            abi.check(call(**kw), "bridges_boltzmann_select")
        assert "boltzmann_select" in L.bridges_last_error().decode(), kw
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())                                        # a refusal launches nothing
    abi.check(call(E=0), "bridges_boltzmann_select")                                               # nothing to do is not an error
    abi.check(call(E=0, T=0.0, n=0), "bridges_boltzmann_select")                                   # ... and is answered first
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())
    for T in (0.0, -2.0, float("nan"), float("inf")):                                              # the operator layer hands it on
        with pytest.raises(abi.BridgesHipError, match="temperature"):
            ops.boltzmann_select((t["seg_lo"], t["seg_hi"]), t["q"], t["u"], T, False, t["idx"], t["cand_offset"])
    with pytest.raises(abi.BridgesHipError, match="n_rows"):
        ops.boltzmann_select((t["seg_lo"], t["seg_hi"]), t["q"][:0], t["u"], 1.0, False, t["idx"][:0], t["cand_offset"])
    abi.check(call(), "bridges_boltzmann_select")                                                  # the same arguments, accepted
    torch.cuda.synchronize()
    check({k: v.cpu().numpy() for k, v in outs.items()}, B.reference(case), "after the refusals")


def test_segment_array_form_equals_the_pair_form():
    from bridges_hip import ops
    case = B.random_probe(0.1)
    order = np.argsort(case["seg_lo"], kind="stable")
    assert np.array_equal(order, np.arange(len(order)))                                            # laid end to end: a prefix array
    seg = np.concatenate([case["seg_lo"], case["seg_hi"][-1:]]).astype(np.int32)
    out = ops.boltzmann_select(dev(seg), dev(case["q"]), dev(case["u"]), case["T"], False, dev(case["idx"]), dev(case["cand_offset"]))
    check({k: v.cpu().numpy() for k, v in zip(KEYS, out)}, B.reference(case), "seg [E + 1]")


# -------------------------------------------------------------------------------------------------------------------- the loop
TEMPS = dict(temp_start=2.0, temp_end=0.25, temp_decay=0.5)


def recorded_loop(monkeypatch, agent, locksteps):
    """``locksteps`` lock-steps without optimiser steps, ops.boltzmann_select wrapped to keep what it was given and what it
    returned, ops.bits_dot / ops.bits_accumulate_ counted.  -> (calls, counts, pushed rows per lock-step, valid per lock-step)."""
    from bridges_hip import ops
    calls, counts, inner = [], dict(bits_dot=0, bits_accumulate_=0), ops.boltzmann_select

    def recording(seg, q, u, temperature, greedy, idx, cand_offset, rep=None):
        out = inner(seg, q, u, temperature, greedy, idx, cand_offset, rep=rep)
        lo, hi = seg if isinstance(seg, (tuple, list)) else (seg[:-1], seg[1:])
        E = lo.numel()
        case = dict(seg_lo=lo.cpu().numpy().copy(), seg_hi=hi.cpu().numpy().copy(), q=q.float().cpu().numpy(), u=u.cpu().numpy(),
                    T=temperature, idx=idx.cpu().numpy(), cand_offset=cand_offset.cpu().numpy()[:E],
                    rep=None if rep is None else rep.cpu().numpy())
        calls.append((case, bool(greedy), {k: v.cpu().numpy() for k, v in zip(KEYS, out)}))
        return out
    monkeypatch.setattr(ops, "boltzmann_select", recording)
    for name in counts:
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=fn, **k: (counts.__setitem__(_n, counts[_n] + 1), _f(*a, **k))[1])
    pushed, valids = [], []
    inner_act = agent.act

    def act(*a, **k):
        rec, valid = inner_act(*a, **k)
        valids.append(valid.clone())
        return rec, valid
    agent.act = act
    for _ in range(locksteps):
        _losses, allrec = agent.lockstep(0)
        pushed.append(allrec)
    return calls, counts, pushed, valids


def loop_case(monkeypatch, agent, locksteps=6):
    E = agent.env.E
    images_before = agent.step_images.clone()
    eps_before = agent.epsilon
    calls, counts, pushed, valids = recorded_loop(monkeypatch, agent, locksteps)
    assert len(calls) == locksteps and counts == dict(bits_dot=0, bits_accumulate_=0)
    t, explored_any = TEMPS["temp_start"], 0
    for (case, greedy, got), allrec, valid in zip(calls, pushed, valids):
        assert not greedy and case["T"] == t                                                       # the schedule, per lock-step
        t = (t - TEMPS["temp_end"]) * TEMPS["temp_decay"] + TEMPS["temp_end"]
        ref = B.reference(case)
        assert float(ref["margin"].min()) > B.MARGIN                                               # no draw of the run lies in the band
        check(got, ref, f"lock-step at T={case['T']}")
        # records and ring: one finite row per valid env, in env order, whose candidate is the drawn one
        v = valid.cpu().numpy().astype(bool)
        assert allrec.shape == (int(v.sum()), agent.ring.width) and bool(torch.isfinite(allrec).all())
        done = allrec[:, R.O_DONE].cpu().numpy()
        assert set(np.unique(done).tolist()) <= {0.0, 1.0}
        explored_any += int((got["explore_w"] * v).sum())
    assert agent.temperature == t and agent.epsilon == eps_before                                   # epsilon is left alone
    last_case, _, last = calls[-1]
    v = valids[-1].cpu().numpy().astype(bool)
    assert agent.explored_fraction == pytest.approx(float((last["explore_w"] * v).sum()) / max(int(v.sum()), 1), abs=1e-12)
    assert explored_any > 0                                                                        # at T = 2 some env leaves the arg-max
    assert len(agent.ring) == sum(int(p.shape[0]) for p in pushed)
    assert torch.equal(agent.step_images, images_before) and not bool(agent.step_images.any())     # the count images stay zero
    assert bool((agent._counts_host >= 0).all()) and agent.env_steps == sum(int(x.sum()) for x in valids)
    return calls


def test_loop_successor_mlp_draws_the_reference_choice_every_lockstep(monkeypatch):
    agent = mlp_agent(tower_env(64, f32_rasters=False), exploration="boltzmann", **TEMPS)
    calls = loop_case(monkeypatch, agent)
    assert any(c[0]["rep"] is not None and (c[0]["rep"] != np.arange(64)).any() for c in calls)     # envs shared rows, drew apart
    # act(greedy=True) is the greedy act of an epsilon-greedy agent with the same seed and weights
    monkeypatch.undo()
    a, b = mlp_agent(tower_env(64, f32_rasters=False), exploration="boltzmann"), mlp_agent(tower_env(64, f32_rasters=False))
    for _ in range(3):
        (rec_a, valid_a), (rec_b, valid_b) = a.act(greedy=True), b.act(greedy=True)
        assert torch.equal(valid_a, valid_b) and torch.equal(rec_a, rec_b) and torch.equal(a._q_sel, b._q_sel)
    assert not bool(a.step_images.any())


def test_loop_conv_net(monkeypatch):
    loop_case(monkeypatch, conv_agent(tower_env(8, f32_rasters=True), exploration="boltzmann", **TEMPS), locksteps=4)


def test_evaluate_stays_greedy_and_refuses_epsilon():
    agent = mlp_agent(tower_env(16, f32_rasters=False), exploration="boltzmann")
    plain = mlp_agent(tower_env(16, f32_rasters=False))
    ev, want = agent.evaluate(tower_env(8, seed=9, f32_rasters=False)), plain.evaluate(tower_env(8, seed=9, f32_rasters=False))
    assert ev == want and ev["episodes"] == 8
    with pytest.raises(ValueError, match="exploration='boltzmann'"):
        agent.evaluate(tower_env(8, seed=9, f32_rasters=False), epsilon=0.1)


def test_checkpoint_resumes_the_schedule_and_the_draws(tmp_path):
    """An agent stopped after 3 lock-steps and a NEW agent resumed from its files (ring and extras) leave the ring the
    uninterrupted agent leaves after 6 -- which, as the run loop does at a checkpoint, resets its envs there.  The new agent
    gets an env that went through the same 3 lock-steps and the reset (a twin's): a reset env keeps the stale poses of the
    block slots beyond n_blocks, which the records copy, so a never-used env would differ in columns no consumer reads."""
    order = lambda r: r.data[(r.head - r.size + torch.arange(r.size, device=r.data.device)) % r.capacity]     # oldest first
    whole = mlp_agent(tower_env(16, f32_rasters=False), exploration="boltzmann", **TEMPS)
    twin = mlp_agent(tower_env(16, f32_rasters=False), exploration="boltzmann", **TEMPS)
    for _ in range(3):
        whole.lockstep(0)
        twin.lockstep(0)
    whole.ring.save(str(tmp_path / "ring.pt"))
    whole.save_extra(str(tmp_path / "agent.pt"), lockstep=3)
    assert torch.load(str(tmp_path / "agent.pt"), weights_only=True)["temperature"] == whole.temperature != TEMPS["temp_start"]
    whole.env.reset()
    twin.env.reset()
    resumed = mlp_agent(twin.env, exploration="boltzmann", **TEMPS)     # a new agent: temp_start, fresh streams, empty ring
    assert resumed.temperature == TEMPS["temp_start"] and len(resumed.ring) == 0
    resumed.ring.load(str(tmp_path / "ring.pt"))
    assert resumed.load_extra(str(tmp_path / "agent.pt")) == dict(lockstep=3)
    assert resumed.temperature == whole.temperature and resumed.env_steps == whole.env_steps
    for _ in range(3):
        whole.lockstep(0)
        resumed.lockstep(0)
    assert resumed.temperature == whole.temperature and len(resumed.ring) == len(whole.ring)
    a, b = order(resumed.ring), order(whole.ring)
    diff = (a != b).nonzero()
    print("rows that differ", diff[:, 0].unique().tolist()[:16], "columns", diff[:, 1].unique().tolist())
    assert torch.equal(a, b)
