"""CPU-only: the rule of bridges_beam_trace in numpy (tests/beam_trace_ref.py) against the n-step window of tests/nstep_ref.py fed
with every chain step by step, what the probe tables hold, the defective twins each rejected by a probe, the argument checks of
ops.beam_trace that need no device, the header / abi.py mirror of the new symbol, and the search in training as far as it runs
without a device: its command line, the construction refusals of VecDQN(search_every=N) and the checkpointed phase."""
import os
import re

import numpy as np
import pytest
import torch

import beam_trace_ref as TR
from nstep_ref import RefWindow
from robotoddler.training import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDED = [(G, B, D, n, nt) for G in (1, 5) for B in (1, 4, 16) for D in (1, 6, 16) for n, nt in ((1, 0), (3, 9), (8, 2))]


def _cases():
    out = dict(TR.probe_tables())
    for G, B, D, n, nt in SEEDED:
        out[f"seeded_{G}_{B}_{D}_{n}_{nt}"] = TR.random_case(G, B, D, n, nt, seed=1000 * G + 100 * B + 10 * D + n)
    return out


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def _window_rows(case, envs, g):
    """The chain of one group as ONE env of the n-step window: its steps in order, the task tail joined on, TD = the priority and
    DONE at the last step alone (the window flushes at DONE) -> rows [L, W + n_tail + 1], g_bound [L]."""
    n, n_tail = case["n_step"], TR.dims(case)["n_tail"]
    win = RefWindow(1, n, case["gamma"])
    rows, bounds = [], []
    for t, e in enumerate(envs):
        rec = case["rec"][t, e].copy()
        rec[R.O_TD] = case["priority"]
        if n_tail:
            rec = np.concatenate([rec, case["tail"][case["end_env"][g]]])
        out, out_valid, g_bound = win.fold(rec[None], np.ones(1, dtype=bool))
        rows += [out[i] for i in np.nonzero(out_valid)[0]]
        bounds += [g_bound[i] for i in np.nonzero(out_valid)[0]]
    return np.array(rows), np.array(bounds)


def _window_can_replay(case, envs):
    """The window tells the end of an episode by DONE and folds LIN by arithmetic: chains whose records are raw bits are not its."""
    done = [case["rec"][t, e, R.O_DONE] > 0.5 for t, e in enumerate(envs)]
    return done == [False] * (len(envs) - 1) + [True] and all(np.isfinite(case["rec"][t, e, R.O_LIN]) for t, e in enumerate(envs))


@pytest.mark.parametrize("name", sorted(_cases()))
def test_rows_are_those_of_the_nstep_window_fed_the_chain(name):
    case = _cases()[name]
    d, ref = TR.dims(case), TR.reference(case)
    W_in = TR.W + d["n_tail"]
    other = np.ones(W_in + 1, dtype=bool)
    other[R.O_LIN] = False
    total = 0
    for g in range(d["G"]):
        envs, status = TR.chain(case, g)
        assert ref["status"][g] == status and ref["offset"][g] == total
        if envs is None:
            continue
        got = ref["rows"][total:total + len(envs)]
        total += len(envs)
        if not _window_can_replay(case, envs):
            continue
        want, g_bound = _window_rows(case, envs, g)
        assert want.shape[0] == len(envs), "the window emits one row per start"
        if case["n_step"] == 1:                                              # no h column in the ring's one-step rows
            assert np.all(want[:, W_in] == 1.0)
            want, cols = want[:, :W_in], other[:W_in]
        else:
            cols = other
        assert got[:, cols].view(np.uint64).tobytes() == np.ascontiguousarray(want[:, cols]).view(np.uint64).tobytes(), (name, g)
        err = np.abs(got[:, R.O_LIN] - want[:, R.O_LIN])                     # the window's LIN is the fsum
        assert np.all(err <= g_bound), (name, g, err, g_bound)
        assert np.all(np.abs(got[:, R.O_LIN] - ref["g_exact"][total - len(envs):total]) <= ref["g_bound"][total - len(envs):total])
    assert ref["offset"][d["G"]] == total
    assert np.all(ref["rows"][total:].view(np.uint64) == TR.ROW_SENTINEL)


def test_the_probes_hold_what_they_are_named_for():
    P = TR.probe_tables()
    c = P["lengths"]
    n, D = c["n_step"], TR.dims(c)["D"]
    assert sorted(int(v) + 1 for v in c["end_depth"]) == sorted([1, D, n, n + 1, 0])
    for t in range(1, D):                                                    # the parents permute the slots at every depth
        for g in range(TR.dims(c)["G"]):
            p = c["parent"][t, g * 4:g * 4 + 4]
            assert sorted(p) == list(range(g * 4, g * 4 + 4)) and np.all(p != np.arange(g * 4, g * 4 + 4))
    assert TR.reference(P["invalid_step"])["status"].tolist() == [1, 1, 1, 0, 0]
    assert TR.reference(P["parent_outside"])["status"].tolist() == [0, 1, 1, 1, 1, 1]
    assert TR.reference(P["end_env_outside"])["status"].tolist() == [1, 1, 1]
    assert TR.reference(P["end_depth_beyond"])["status"].tolist() == [1, 0, 1, 0]
    assert TR.reference(P["nothing_ended_anywhere"])["offset"].tolist() == [0, 0, 0, 0]
    bits = P["bits_one_step"]["rec"].view(np.uint64)
    assert np.isnan(P["bits_one_step"]["rec"]).sum() >= 64 and np.any(bits == np.uint64(0x8000000000000000))
    ref = TR.reference(P["bits_one_step"])
    assert np.isnan(ref["rows"][:int(ref["offset"][-1])]).any()              # NaN payloads travel into the rows
    w = P["widest"]
    assert (w["B"], TR.dims(w)["D"], w["n_step"]) == (16, 16, 8)
    odd_even = {TR.dims(c)["W_out"] % 2 for c in P.values()}
    assert odd_even == {0, 1}


@pytest.mark.parametrize("twin", TR.TWINS)
def test_every_twin_is_rejected_by_a_probe(twin):
    hits = [name for name, case in TR.probe_tables().items() if not TR.same(TR.reference(case, twin), TR.reference(case))]
    assert hits, f"no probe table tells the twin {twin!r} from the rule"


def test_the_return_is_summed_in_the_order_of_the_fold():
    lins, gamma = [0.1, 0.7, -0.3, 1e-9], 0.95
    acc, disc = 0.0, 1.0
    for lin in lins:
        acc += disc * lin
        disc *= gamma
    assert TR.returns(lins, gamma).tobytes() == np.float64(acc).tobytes()
    assert TR.returns(lins, gamma) != TR.returns(lins, gamma, "undiscounted")
    assert np.signbit(np.float64(-0.0)) and not np.signbit(TR.returns([-0.0, -0.0], gamma))     # 0 + 1 * -0.0 = +0.0: h > 1 sums


# ---- ops.beam_trace: the checks that need no device ---------------------------------------------------------------------------------
def _torch_case(case):
    t = {k: torch.from_numpy(case[k]) for k in ("rec", "valid", "parent", "end_env", "end_depth")}
    t["tail"] = None if case["tail"] is None else torch.from_numpy(case["tail"])
    return t


def test_argument_checks_that_need_no_device():
    from bridges_hip import ops
    case = TR.make_case(3, 4, 6, 3, 5, seed=1)
    t = _torch_case(case)

    def check(B=4, gamma=0.9, n_step=3, **swap):
        a = dict(t, **swap)
        return ops.beam_trace_args(a["rec"], a["valid"], a["parent"], a["end_env"], a["end_depth"], B, gamma, n_step, a["tail"])
    assert check() == (12, 4, 6, 3, 5, TR.W + 5 + 1)
    assert check(n_step=1, tail=None) == (12, 4, 6, 1, 0, TR.W)
    for bad, word in ((dict(B=0), "width"), (dict(B=17), "width"), (dict(B=5), "multiple"), (dict(n_step=0), "n_step"),
                      (dict(n_step=9), "n_step"), (dict(gamma=float("nan")), "finite"), (dict(gamma=float("inf")), "finite"),
                      (dict(rec=t["rec"].float()), "rec"), (dict(rec=t["rec"][:, :, :110]), "rec"),
                      (dict(rec=torch.zeros((17, 12, TR.W), dtype=torch.float64)), "depths"),
                      (dict(valid=t["valid"][:5]), "valid"), (dict(valid=t["valid"].int()), "valid"),
                      (dict(parent=t["parent"].long()), "parent"), (dict(parent=t["parent"][:, :8]), "parent"),
                      (dict(end_env=t["end_env"][:2]), "end_env"), (dict(end_depth=t["end_depth"].long()), "end_depth"),
                      (dict(tail=t["tail"].float()), "tail"), (dict(tail=t["tail"][:8]), "tail"),
                      (dict(tail=t["tail"][:, ::2]), "contiguous"), (dict(rec=t["rec"].transpose(0, 1).contiguous().transpose(0, 1)), "contiguous")):
        with pytest.raises(ValueError) as e:
            check(**bad)
        assert word in str(e.value), (bad.keys(), str(e.value))


# ---- header / abi.py ------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_and_mirrored():
    import ctypes as C
    from bridges_hip import abi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bridges_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bridges_beam_trace\s*\(([^;]*)\)\s*;", text)
    assert m, "bridges_beam_trace is not declared in include/bridges_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = abi.SIGNATURES["bridges_beam_trace"]
    assert len(params) == len(sig) == 17
    for p, ct in zip(params, sig):
        want = abi.vp if "*" in p else (abi.f64 if p.startswith("double") else abi.i32)
        assert ct is want, p
    assert [p.split()[-1].lstrip("*") for p in params] == ["E", "B", "D", "n_step", "n_tail", "rec", "valid", "parent", "end_env",
                                                           "end_depth", "tail", "gamma", "priority", "out", "offset", "status", "stream"]
    assert "bridges_beam_trace" in abi.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(abi.LIB_PATH), "bridges_beam_trace")
    assert abi.REC_WIDTH == R.RECORD_WIDTH == 111 and abi.BEAM_TRACE_MAX_DEPTH == R.K == 16 and abi.NSTEP_MAX == 8


# ---- search in training: command line and construction ------------------------------------------------------------------------------
def test_command_line_of_the_search():
    from robotoddler.training import successor_dqn as S
    parse = lambda *argv: vars(S.build_parser().parse_args(list(argv)))
    plain = parse()
    assert not {"search_every", "search_tasks", "search_width", "search_merge"} & set(plain)     # SUPPRESS: a plain parse is as it was
    S.check_search(plain)
    assert S.search_from_args(plain) == {}
    ok = parse("--num_envs", "64", "--search_every", "10")
    assert S.search_from_args(ok) == dict(search_every=10, search_width=8, search_merge=False)
    full = parse("--num_envs", "64", "--search_every", "10", "--search_tasks", "16", "--search_width", "4", "--search_merge")
    assert S.search_from_args(full) == dict(search_every=10, search_tasks=16, search_width=4, search_merge=True)
    for flag, value in (("--search_tasks", "4"), ("--search_width", "4"), ("--search_merge", None)):
        with pytest.raises(SystemExit, match="--search_every N"):
            S.check_search(parse("--num_envs", "64", flag, *([value] if value else [])))
    with pytest.raises(SystemExit, match="--num_envs"):
        S.check_search(parse("--search_every", "10"))
    with pytest.raises(SystemExit, match=">= 1"):
        S.check_search(dict(ok, search_every=0))
    with pytest.raises(SystemExit, match="1..16"):
        S.check_search(dict(ok, search_width=17))
    with pytest.raises(SystemExit, match="--search_tasks"):
        S.check_search(dict(ok, search_tasks=65))
    with pytest.raises(SystemExit, match="--num_envs"):
        S.main(["--search_every", "10"])                                                          # refused before the GPU is asked for
    assert "search_success_rate" in S.build_parser().format_help()


def test_command_line_refuses_several_ranks(monkeypatch):
    from robotoddler.training import successor_dqn as S
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank"):
        S.check_search(dict(num_envs=64, search_every=10))


def _stand_in_env(cls=None, **kw):
    from bridges_hip.vec_env import VecAssemblyGym
    env = (cls or VecAssemblyGym).__new__(cls or VecAssemblyGym)                                  # (no device behind it: nothing to free)
    env.__dict__.update(dict(per_env_tasks=True, per_env_obstacles=False, img=64, n_targets=3, n_obstacles=0, device="cpu", K=4, E=8,
                             stable_actions_only=False, max_steps=4), **kw)
    return env


def _host_agent(monkeypatch, env, **kw):
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "_make_replay_env", lambda self, n: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8])
    return VecDQN(net, net, torch.optim.Adam(net.parameters(), lr=1e-4), env, 16, 4, 0.9, 0.05, "mse_block_features", **kw)


def test_construction_of_the_search(monkeypatch, tmp_path):
    import types
    from bridges_hip.vec_env import VecAssemblyGymGroups
    from robotoddler.training import distributed as D
    plain = _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True)
    assert plain.search_every == 0 and plain.search_env is None and plain.last_search is None
    a = _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True, search_every=5)
    assert (a.search_every, a.search_tasks, a.search_width, a.search_merge, a.search_priority) == (5, 8, 8, False, 0.0)
    b = _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True, n_step=3, prioritized=True, search_every=2, search_tasks=4,
                    search_width=16, search_merge=True)
    assert (b.search_tasks, b.search_width, b.search_merge, b.search_priority) == (4, 16, True, 1.0)
    assert b.ring.width == R.RECORD_WIDTH + 9 + 1                                                  # what a traced search of n_step 3 writes
    fixed = _host_agent(monkeypatch, _stand_in_env(per_env_tasks=False), search_every=2, search_tasks=8)
    assert fixed.search_tasks == 1                                                                 # one task: one group
    for kw, word in ((dict(search_every=2, search_width=0), "search_width"), (dict(search_every=2, search_width=17), "search_width"),
                     (dict(search_every=2, search_tasks=9), "search_tasks"), (dict(search_every=2, search_tasks=0), "search_tasks"),
                     (dict(search_every=-1), "search_every"), (dict(search_tasks=2), "need search_every"),
                     (dict(search_width=2), "need search_every"), (dict(search_merge=True), "need search_every"),
                     (dict(search_priority=1.0), "need search_every"), (dict(search_every=2, search_priority=1.0), "prioritized=True"),
                     (dict(search_every=2, prioritized=True, search_priority=-1.0), ">= 0")):
        with pytest.raises(ValueError) as e:
            _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True, **kw)
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError, match="block slots"):
        _host_agent(monkeypatch, _stand_in_env(K=65), per_env_tasks=True, search_every=2, search_merge=True)
    with pytest.raises(ValueError, match="VecAssemblyGymGroups"):
        _host_agent(monkeypatch, _stand_in_env(VecAssemblyGymGroups), per_env_tasks=True, search_every=2)
    with pytest.raises(ValueError, match="SimpleNamespace"):
        _host_agent(monkeypatch, types.SimpleNamespace(**vars(_stand_in_env())), per_env_tasks=True, search_every=2)
    # the phase rides in save_extra; a file without it loads with phase 0, a plain run's file is as it was
    p0, p1 = str(tmp_path / "plain.pt"), str(tmp_path / "search.pt")
    plain.save_extra(p0, lockstep=1)
    assert "search_phase" not in torch.load(p0, weights_only=True)
    a.search_calls = 3
    a.save_extra(p1, lockstep=8)
    assert torch.load(p1, weights_only=True)["search_phase"] == 3
    again = _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True, search_every=5)
    assert again.load_extra(p1) == dict(lockstep=8) and again.search_calls == 3
    again.load_extra(p0)
    assert again.search_calls == 0
    monkeypatch.setattr(D, "active", lambda: True)
    with pytest.raises(ValueError, match="one rank"):
        _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True, search_every=2)
