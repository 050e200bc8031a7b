"""CPU: the reference of the relative-temperature operators (tests/relative_temperature_ref.py) -- the spread against exact
rational arithmetic, the derived bound against every defective twin, the draw condition on the seeded probes -- and the host
side of VecDQN(temp_relative=, target_temp_relative=, spread_floor=): the header and its ctypes mirror, the operator layer's
unchanged calls, the constructor, the command line, the checkpoint entries and the log keys."""
import os
import re

import numpy as np
import pytest
import torch

import boltzmann_ref as B
import relative_temperature_ref as RT
import soft_target_ref as S
from test_cpu_nstep import host_agent, stand_in_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def segments(case, key):
    for lo, hi in zip(case["seg_lo"], case["seg_hi"]):
        yield case[key][lo:hi] if hi > lo else case[key][:0]


# ------------------------------------------------------------------------------------------------------------ the references
def test_spread_against_exact_rational_arithmetic_on_every_probe_segment():
    worst, seen = 0.0, 0
    for case, key in [(c, "q") for c in RT.select_cases() + RT.select_exact_cases()] + [(c, "select_q") for c in RT.expect_cases()]:
        done = set()
        for q in segments(case, key):
            if q.tobytes() in done or len(q) > 300:                  # (the rational sums of the longest segments take seconds)
                continue
            done.add(q.tobytes())
            s, n, _ = RT.spread(q)
            want = RT.spread_brute_force(q)
            if n < 2:
                assert s == 0.0 == want
                continue
            _, bound = RT.effective_temperature(q, 1.0, 1e-30)
            assert abs(s - want) <= 8 * RT.U * want, (s, want)          # the module's own roundings: 3.5 u of the derivation, and the brute force's two
            assert bound >= 8 * RT.U * want or want == 0.0
            worst, seen = max(worst, abs(s - want) / max(want, 1e-300)), seen + 1
    assert seen > 100
    print("segments", seen, "largest |spread - exact| / exact", worst)


def test_spread_of_the_plain_cases():
    assert RT.spread(np.asarray([], np.float32))[0] == 0.0
    assert RT.spread(np.asarray([3.0], np.float32))[0] == 0.0
    assert RT.spread(np.asarray([np.nan, 2.0, np.inf, -np.inf], np.float32))[:2] == (0.0, 1)           # one finite row
    assert RT.spread(np.asarray([1.0, 3.0], np.float32))[0] == 1.0                                      # population, not sample (sqrt 2)
    assert RT.spread(np.asarray([1.0, np.nan, 3.0, np.inf, -np.inf], np.float32))[:2] == (1.0, 2)       # non-finite rows left out
    assert RT.spread(np.full(300, 0.375, np.float32))[0] == 0.0                                         # exact ties: exactly 0
    rng = np.random.default_rng(0)
    for n in RT.UNIT_LENGTHS:
        for a in (-3.0, 0.0, 2.0, 17.0):
            assert RT.spread(RT.unit_spread_rows(n, a, rng))[0] == 1.0


def test_effective_temperature_floor_and_exact_cases():
    f32 = lambda x: float(np.float32(x))
    tied = np.full(65, -7.25, np.float32)
    assert RT.effective_temperature(tied, 0.3, 1e-3) == (f32(0.3) * f32(1e-3), 0.0)                     # the floor binds, exactly
    assert RT.effective_temperature(tied[:0], 0.3, 1e-3) == (f32(0.3) * f32(1e-3), 0.0)                 # an empty segment
    assert RT.effective_temperature(np.asarray([np.nan, -np.inf], np.float32), 2.0, 0.5) == (1.0, 0.0)  # no finite row
    te, bound = RT.effective_temperature(np.asarray([1.0, 3.0], np.float32), 0.5, 1e-3)
    assert te == 0.5 and 0.0 < bound < 1e-14
    te, _ = RT.effective_temperature(np.asarray([1.0, 3.0], np.float32), 0.5, 4.0)                      # fmax, not a sum
    assert te == 2.0
    # a large common offset: the mean's error D enters at second order (D^2 / 2 s) while s >> D, and at first order where the rows
    # all but tie
    q = np.float32(1e4) + np.float32(1e-2) * np.arange(300, dtype=np.float32)
    te, bound = RT.effective_temperature(q, 1.0, 1e-3)
    assert 0.8 < te < 0.9 and 150 * RT.U * te < bound < 1e-12 * te
    near = np.asarray([1e4, 1e4 + 2.0 ** -10] * 150, dtype=np.float32)                                  # s = 2^-11 at |q| = 1e4
    te, bound = RT.effective_temperature(near, 1.0, 1e-6)
    assert te == 2.0 ** -11 and bound > 150 * RT.U * te + 0.5 * (300 * RT.U * 1e4) ** 2 / te


@pytest.mark.parametrize("twin", RT.TWINS + ("spread_of_next_q",))
def test_the_bound_rejects_every_twin(twin):
    assert RT.rejected(twin)


def test_no_twin_is_rejected_for_the_wrong_reason():
    """The rule itself is not rejected, and each twin is told apart on the probe it was made for."""
    assert not RT.rejected(None)
    offset = [RT.select_offset_probe()]
    assert RT.rejected("single_pass", select=offset, expect=[]) and RT.rejected("float32_accumulation", select=offset, expect=[])
    tied = [RT.select_tied_probe()]
    assert RT.rejected("floor_ignored", select=tied, expect=[])                   # T_e = 0 where the rows tie
    assert not RT.rejected("floor_added", select=tied, expect=[])                 # (s = 0: the sum IS the maximum there)
    assert RT.rejected("floor_added", select=offset, expect=[])                   # s > floor: off by floor / s = 1e-3 relative
    nonfinite = B.nonfinite_probe()
    for twin in ("inf_counted", "nan_counted", "ineligible_in_mean"):
        assert RT.rejected(twin, select=nonfinite, expect=[]), twin
    assert RT.rejected("sample_variance", select=[B.random_probe(1.0)], expect=[])
    assert RT.rejected("spread_of_next_q", select=[], expect=[S.random_probe(1.0, 0, double=True)])
    assert not RT.rejected("spread_of_next_q", select=[], expect=[S.random_probe(1.0, 0, double=False)])  # one array: the same spread


def test_the_probe_sets_hold_what_they_promise():
    lengths = set()
    for c in RT.select_cases():
        lengths |= set((c["seg_hi"].astype(int) - c["seg_lo"]).tolist())
    assert set(B.SEG_LENGTHS) <= lengths
    lengths, dims = set(), set()
    for c in RT.expect_cases():
        lengths |= set((c["seg_hi"].astype(int) - c["seg_lo"]).tolist())
        dims.add(0 if c["feat"] is None else c["feat"].shape[1])
    assert set(S.SEG_LENGTHS) <= lengths and set(RT.EXPECT_DIMS) <= dims
    assert any(c.get("rep") is not None for c in RT.select_cases())                                     # shared rows and rep
    c = RT.select_offset_probe()
    assert all(q.min() >= 1e4 and RT.spread(q)[0] < 1.0 for q in segments(c, "q") if len(q))            # a large offset, a small spread
    te, _ = RT.select_temperatures(RT.select_tied_probe())
    assert (te == float(np.float32(1.0)) * float(np.float32(RT.FLOOR))).all()                           # the floor binds in every segment
    te, _ = RT.expect_temperatures(RT.expect_offset_probe(5, tied=True))
    assert (te[:2 * len(S.SEG_LENGTHS)] == float(np.float32(RT.FLOOR))).all()


def test_references_at_a_given_temperature_are_the_scalar_references():
    """At one float32 temperature for every segment the two references ARE boltzmann_ref.reference / soft_target_ref.reference."""
    case = B.random_probe(0.1)
    T = float(np.float32(0.1))
    got, want = RT.select_reference(case, np.full(len(case["u"]), T)), B.reference(case)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    case = S.random_probe(0.1, 5)
    got, want = RT.expect_reference(case, np.full(len(case["seg_lo"]), T)), S.reference(case)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert S.temperature_of(dict(T=0.1)) == T                                                           # (the patch was undone)
    # ... and against boltzmann_ref's brute force at a temperature of each env's own
    case = RT.select_offset_probe()
    te, _ = RT.select_temperatures(case)
    ref = RT.select_reference(case, te)
    for e, q in enumerate(segments(case, "q")):
        if len(q):
            row, p, ex = B.brute_force(q, case["u"][e], te[e])
            assert ref["row"][e] == case["seg_lo"][e] + row and ref["explore_w"][e] == ex and abs(ref["p_sel"][e] - p) <= 1e-12 * p


def test_the_draw_condition_at_the_perturbed_temperatures():
    """At the reference's T_e and at T_e -+ its bound no probe draw lies within boltzmann_ref.MARGIN of a CDF boundary, and the
    drawn row is the same at all three: the device's T_e (anywhere inside the bound) decides no draw.  A condition on the seeded
    inputs; no case is left out on the GPU."""
    for k, case in enumerate(RT.select_cases()):
        te, bound = RT.select_temperatures(case)
        mid = RT.select_reference(case, te)
        for t in (te - bound, te + bound):
            ref = RT.select_reference(case, t)
            assert np.array_equal(ref["row"], mid["row"]), k
            assert (ref["margin"] >= B.MARGIN).all(), (k, float(ref["margin"].min()))
        assert (mid["margin"] >= B.MARGIN).all(), (k, float(mid["margin"].min()))
    floored = B.reference(dict(RT.select_offset_probe(), T=2.0))      # the GPU test's case under a floor that binds: T_e = 2 exactly
    assert (floored["margin"] >= B.MARGIN).all()
    for case in RT.select_exact_cases():                               # weights exactly 0 or 1 at ANY temperature: no margin needed
        te, bound = RT.select_temperatures(case)
        a, b = RT.select_reference(case, te), RT.select_reference(case, 1e3 * te + 1.0)
        assert np.array_equal(a["row"], b["row"]) and np.array_equal(a["p_sel"], b["p_sel"])


# ------------------------------------------------------------------------------------------------------------ header and bindings
def test_entry_points_are_declared_with_their_rule_and_mirrored():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        full = fh.read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    C = abi.C
    want = {"bridges_boltzmann_select_rel": [C.c_int32, C.c_int32, *[C.c_void_p] * 4, C.c_float, C.c_float, C.c_int32, *[C.c_void_p] * 10],
            "bridges_soft_expect_rel": [C.c_int32, *[C.c_void_p] * 4, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                        *[C.c_void_p] * 6]}
    for name, sig in want.items():
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M).group(1)
        assert name in abi.EXPORTED_SYMBOLS and decl.count(",") + 1 == len(abi.SIGNATURES[name]) == len(sig)
        assert abi.SIGNATURES[name] == sig
        for arg in (r"float\s+temperature\s*,\s*float\s+spread_floor", r"double\s*\*\s*temp_out\s*,\s*void\s*\*\s*stream"):
            assert re.search(arg, decl), (name, arg)
        sibling = re.search(r"^int\s+" + name[:-4] + r"\s*\(([^;]*)\);", text, flags=re.M).group(1)
        strip = lambda d: re.sub(r"\s+", " ", d).strip()
        assert strip(decl).replace("float spread_floor, ", "").replace("double* temp_out, ", "") == strip(sibling)
    comment = full[:full.index("int bridges_boltzmann_select_rel(")].rsplit("/*", 1)[1]
    for word in ("SPREAD", "FINITE", "n_f < 2", "population standard", "two passes", "never E[x^2] - mean^2", "float64", "EFFECTIVE TEMPERATURE",
                 "fmax(s, (double)spread_floor)", "temp_out", "word for word", "greedy != 0", "temp_out[e] = 0", "8-byte aligned"):
        assert word in comment, word
    comment = full[:full.index("int bridges_soft_expect_rel(")].rsplit("/*", 1)[1]
    for word in ("bridges_boltzmann_select_rel", "select_q", "never next_q", "temp_out[i]"):
        assert word in comment, word


class _CountingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, len(args)))
            return 0
        return fn


def test_operator_layer_calls_the_new_entry_points_only_when_asked(monkeypatch):
    from bridges_hip import abi, dqn_ops, ops
    lib = _CountingLib()
    monkeypatch.setattr(abi, "require_gpu", lambda: lib)
    monkeypatch.setattr(dqn_ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    seg = torch.tensor([0, 2, 5], dtype=torch.int32)
    q, u, idx, off = torch.randn(5), torch.rand(2), torch.arange(5), torch.zeros(2, dtype=torch.int32)
    assert len(ops.boltzmann_select(seg, q, u, 1.0, False, idx, off)) == 5
    out = ops.boltzmann_select(seg, q, u, 1.0, False, idx, off, relative=True, spread_floor=0.5)
    assert len(out) == 6 and out[5].dtype == torch.float64 and tuple(out[5].shape) == (2,)
    assert lib.calls == [("bridges_boltzmann_select", 17), ("bridges_boltzmann_select_rel", 19)]
    lib.calls.clear()
    nq, done, lin = torch.randn(5), torch.zeros(2, dtype=torch.bool), torch.zeros(2)
    assert len(dqn_ops.soft_expect(seg, nq, nq, 0.5)) == 4
    out = dqn_ops.soft_expect(seg, nq, nq, 0.5, relative=True)
    assert len(out) == 5 and out[4].dtype == torch.float64 and tuple(out[4].shape) == (2,)
    assert lib.calls == [("bridges_soft_expect", 15), ("bridges_soft_expect_rel", 17)]
    lib.calls.clear()
    stats = {}
    dqn_ops.next_targets(seg, nq, done, 0.9, lin=lin, temperature=0.5, stats=stats)
    assert [c[0] for c in lib.calls] == ["bridges_soft_expect", "bridges_td_target_select"] and "temp_out" not in stats
    lib.calls.clear()
    dqn_ops.next_targets(seg, nq, done, 0.9, lin=lin, temperature=0.5, stats=stats, relative=True, spread_floor=0.25)
    assert [c[0] for c in lib.calls] == ["bridges_soft_expect_rel", "bridges_td_target_select"]         # stage two is unchanged
    assert stats["temp_out"].dtype == torch.float64


# ------------------------------------------------------------------------------------------------------------ VecDQN, CLI, files
def test_constructor_takes_the_options_and_refuses_them_without_their_parent(monkeypatch):
    a = host_agent(monkeypatch, stand_in_env())
    assert a.temp_relative is False and a.target_temp_relative is False and a.spread_floor == 1e-3
    assert a._count_names == host_agent(monkeypatch, stand_in_env(), temp_relative=False, target_temp_relative=False)._count_names
    b = host_agent(monkeypatch, stand_in_env(), exploration="boltzmann", temp_relative=True, spread_floor=0.01)
    assert b.temp_relative and not b.target_temp_relative and b.spread_floor == 0.01 and b._count_names[-1] == "temp_sum"
    assert b.temperature == b.temp_start and b.temperature_effective is None
    c = host_agent(monkeypatch, stand_in_env(), target_temperature=0.5, target_temp_relative=True, double_q=True, n_step=3, prioritized=True)
    assert c.target_temp_relative and not c.temp_relative and c.target_temperature == 0.5 and "temp_sum" not in c._count_names
    with pytest.raises(ValueError, match="temp_relative.*exploration='boltzmann'"):
        host_agent(monkeypatch, stand_in_env(), temp_relative=True)
    with pytest.raises(ValueError, match="target_temp_relative.*target_temperature"):
        host_agent(monkeypatch, stand_in_env(), target_temp_relative=True)
    with pytest.raises(ValueError, match="target_temp_relative.*target_temperature"):
        host_agent(monkeypatch, stand_in_env(), exploration="boltzmann", temp_relative=True, target_temp_relative=True)
    with pytest.raises(ValueError, match="spread_floor.*temp_relative"):
        host_agent(monkeypatch, stand_in_env(), exploration="boltzmann", spread_floor=0.01)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1.0", True):
        with pytest.raises(ValueError, match="spread_floor"):
            host_agent(monkeypatch, stand_in_env(), exploration="boltzmann", temp_relative=True, spread_floor=bad)


def test_cli_options_are_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_relative_temperature, relative_temperature_from_args
    base = ["--model", "SuccessorMLP", "--num_envs", "64"]
    plain = vars(build_parser().parse_args(base))
    assert not {"temp_relative", "target_temp_relative", "spread_floor"} & set(plain) and relative_temperature_from_args(plain) == {}
    check_relative_temperature(plain)
    args = vars(build_parser().parse_args(base + ["--exploration", "boltzmann", "--temp_relative"]))
    check_relative_temperature(args)
    assert relative_temperature_from_args(args) == dict(temp_relative=True)
    args = vars(build_parser().parse_args(base + ["--target_temperature", "1.0", "--target_temp_relative", "--spread_floor", "0.01"]))
    check_relative_temperature(args)
    assert relative_temperature_from_args(args) == dict(target_temp_relative=True, spread_floor=0.01)
    for flag in ("--temp_relative", "--target_temp_relative", "--spread_floor"):
        assert flag in build_parser().format_help()
    refused = [(["--temp_relative"], "--exploration boltzmann"), (["--target_temp_relative"], "--target_temperature"),
               (["--spread_floor", "0.01"], "--temp_relative"),
               (["--exploration", "boltzmann", "--temp_relative", "--target_temp_relative"], "--target_temperature"),
               (["--target_temperature", "1.0", "--target_temp_relative", "--temp_relative"], "--exploration boltzmann")]
    refused += [(["--exploration", "boltzmann", "--temp_relative", "--spread_floor", bad], "--spread_floor") for bad in ("0", "-1", "inf", "nan")]
    for argv, word in refused:
        with pytest.raises(SystemExit) as e:
            check_relative_temperature(vars(build_parser().parse_args(base + argv)))
        assert isinstance(e.value.code, str) and word in e.value.code, (argv, e.value.code)


@pytest.mark.parametrize("argv", [["--exploration", "boltzmann", "--temp_relative"],
                                  ["--num_envs", "1", "--exploration", "boltzmann", "--temp_relative"],
                                  ["--exploration", "boltzmann", "--temp_relative", "--spread_floor", "0.01"]])
def test_cli_refuses_the_single_env_loop_in_words(argv):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(["--model", "SuccessorMLP"] + argv)
    assert isinstance(e.value.code, str) and "--temp_relative" in e.value.code and "--num_envs" in e.value.code, e.value.code


def test_checkpoint_entries_only_with_the_options_and_refused_under_another_setting(tmp_path):
    from robotoddler.training.vec_dqn import VecDQN

    def agent(rel=None, act=None, T=0.5):
        a = VecDQN.__new__(VecDQN)
        a.n_task_targets, a.n_task_obstacles, a.n_step, a.double_q = 0, 0, 1, False
        a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
        a.step_images = torch.zeros((3, 4, 4))
        a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        a.target_temperature = T
        if rel is not None:
            a.target_temp_relative, a.spread_floor = True, rel
        if act is not None:
            a.exploration, a.temperature, a.temp_start, a.temp_relative, a.spread_floor = "boltzmann", 0.7, 1.0, True, act
        return a
    paths = {}
    for rel in (None, 1e-3, 0.5):
        paths[rel] = str(tmp_path / f"agent_{rel}.pt")
        agent(rel).save_extra(paths[rel], lockstep=5)
    keys = {rel: sorted(torch.load(paths[rel], weights_only=True)) for rel in paths}
    assert "target_temp_relative" not in keys[None] and keys[1e-3] == sorted(keys[None] + ["target_temp_relative"])
    assert torch.load(paths[0.5], weights_only=True)["target_temp_relative"] == 0.5
    assert agent(None).load_extra(paths[None]) == agent(1e-3).load_extra(paths[1e-3]) == dict(lockstep=5)
    for have, want in ((None, 1e-3), (1e-3, None), (1e-3, 0.5)):                        # both directions, and another floor
        with pytest.raises(ValueError, match="target_temp_relative, spread_floor"):
            agent(have).load_extra(paths[want])
    # temp_relative goes the way of the exploration setting itself: an entry only when set, no refusal either way
    acting = str(tmp_path / "acting.pt")
    agent(act=0.01).save_extra(acting, lockstep=5)
    blob = torch.load(acting, weights_only=True)
    assert blob["temp_relative"] == 0.01 and blob["temperature"] == 0.7 and "temp_relative" not in keys[None]
    assert agent().load_extra(acting) == agent(act=0.01).load_extra(paths[None]) == dict(lockstep=5)


def test_log_values_carry_the_keys_only_with_the_options():
    from robotoddler.training.vec_dqn import EPISODE_KEYS, DeferredLosses, lockstep_log_values
    info = dict(mean_reward=0., mean_lin_reward=0., avg_loss=0., lockstep_env_steps=1, epsilon=0.1, env_steps=1, steps_per_s=1.,
                **{k: None for k in EPISODE_KEYS})
    plain = lockstep_log_values(info)
    assert "temperature_effective" not in plain and "target_temperature_effective" not in plain
    vals = lockstep_log_values(dict(info, temperature_effective=0.75, target_temperature_effective=1.5))
    assert vals["temperature_effective"] == 0.75 and vals["target_temperature_effective"] == 1.5

    class Ready:
        def synchronize(self):
            pass
    owner = type("A", (), dict(target_temp_relative=True))()
    d = DeferredLosses(torch.tensor([1.0, 2.0, 0.5, 0.125, 3.0]), Ready(), None,
                       names=("target_entropy", "soft_value_gap", "target_temperature_effective"), owner=owner)
    assert d.get() == [1.0, 2.0] and d.soft == dict(target_entropy=0.5, soft_value_gap=0.125, target_temperature_effective=3.0)
    assert owner.target_temperature_effective == 3.0 and owner.soft_value_gap == 0.125
    # the float64 sum of the effective temperatures rides among the int64 counts as its bits
    s = torch.tensor([0.3, 1e-9, 7.0], dtype=torch.float64).sum()
    host = torch.stack([torch.tensor(5), s.view(torch.int64)])
    assert float(host[1:2].view(torch.float64)) == float(s)
