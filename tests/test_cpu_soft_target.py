"""CPU: the reference of the expected-value target operator (tests/soft_target_ref.py) -- its bound rejects every defective twin,
its limits are the arg-max row (T -> 0) and the mean (T -> inf) -- and the host side of VecDQN(target_temperature=T): the header
and its ctypes mirror, next_targets' unchanged path, the constructor, the command line and the checkpoint entry."""
import os
import re

import numpy as np
import pytest
import torch

import soft_target_ref as S
from test_cpu_nstep import host_agent, stand_in_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_reference_conforms_to_itself_on_every_case():
    for case in S.cpu_cases():
        ref = S.reference(case)
        assert S.violations(S.as_device(ref), ref) == []
        assert ref["value"].shape == (len(case["seg_lo"]),) and (ref["nothing"] == (ref["argmax_row"] == S.NONE_ROW)).all()
        assert (ref["value"][ref["nothing"]] == -np.inf).all() and not ref["feat_mean"][ref["nothing"]].any()


@pytest.mark.parametrize("twin", S.TWINS)
def test_the_bound_rejects_every_twin(twin):
    assert S.rejected(twin)


def test_the_probe_set_holds_what_it_promises():
    cases = S.cpu_cases()
    lengths = set()
    for c in cases:
        lengths |= set((c["seg_hi"].astype(int) - c["seg_lo"]).tolist())
    assert set(S.SEG_LENGTHS) <= lengths
    assert {S.temperature_of(c) for c in cases} >= {float(np.float32(T)) for T in S.TEMPERATURES}
    c = S.random_probe(1.0, 5)
    pairs = list(zip(c["seg_lo"].tolist(), c["seg_hi"].tolist()))
    assert len(set(pairs)) < len(pairs)                                                       # shared ranges
    assert any(a < d and c_ < b and (a, b) != (c_, d) for a, b in pairs for c_, d in pairs if (a, b) < (c_, d))   # overlapping ones
    m = S.random_probe(1.0, 7, mapped=True)
    assert len(np.unique(m["feat_row"])) < len(m["feat_row"]) and m["feat"].shape[0] < len(m["select_q"])
    assert any(c["select_q"] is c["next_q"] for c in cases) and any(c["select_q"] is not c["next_q"] for c in cases)
    for c in S.nonfinite_probe():                                        # NaN / inf in next_q and feat only where select_q is ineligible
        bad = np.isnan(c["select_q"]) | (c["select_q"] == -np.inf)
        if c["select_q"] is not c["next_q"]:
            assert np.isfinite(c["next_q"][~bad]).all() and np.isfinite(c["feat"][~bad]).all()
            assert not np.isfinite(c["next_q"][bad]).any() and not np.isfinite(c["feat"][bad]).any()
    assert any((S.reference(c)["value"] == np.inf).any() for c in S.nonfinite_probe())        # m = +inf through one array


def test_small_temperature_gives_the_argmax_row():
    rng = np.random.default_rng(5)
    sel = rng.permutation(np.arange(40, dtype=np.float32))                                   # unique maxima, gaps of 1 >> T
    case = dict(seg_lo=np.asarray([0, 10, 17], np.int32), seg_hi=np.asarray([10, 40, 18], np.int32), select_q=sel,
                next_q=rng.standard_normal(40).astype(np.float32), T=1e-6, feat=rng.standard_normal((40, 6)).astype(np.float32), feat_row=None)
    ref = S.reference(case)
    for i, (a, b) in enumerate(zip(case["seg_lo"], case["seg_hi"])):
        j = a + int(np.argmax(sel[a:b]))
        assert ref["argmax_row"][i] == j and ref["value"][i] == case["next_q"][j] and (ref["feat_mean"][i] == case["feat"][j]).all()
        assert ref["entropy"][i] == 0.0


def test_large_temperature_gives_the_mean_over_the_eligible_rows():
    sel = np.asarray([1.0, S.NAN, -2.0, -S.INF, 0.5, 3.0], dtype=np.float32)
    nq = np.asarray([2.0, S.NAN, 4.0, S.INF, -1.0, 7.0], dtype=np.float32)
    feat = np.arange(12, dtype=np.float32).reshape(6, 2)
    ref = S.reference(dict(seg_lo=np.asarray([0], np.int32), seg_hi=np.asarray([6], np.int32), select_q=sel, next_q=nq, T=1e30,
                           feat=feat, feat_row=None))
    ok = [0, 2, 4, 5]
    assert abs(ref["value"][0] - nq[ok].astype(np.float64).mean()) < 1e-12
    assert np.allclose(ref["feat_mean"][0], feat[ok].astype(np.float64).mean(axis=0), rtol=1e-12)
    assert abs(ref["entropy"][0] - np.log(4.0)) < 1e-12


def test_a_constant_added_to_select_q_changes_nothing():
    case = S.random_probe(1.0, 3)
    ref = S.reference(case)
    shifted = dict(case, select_q=(case["select_q"].astype(np.float64) + 4.0).astype(np.float32))
    exact = np.array_equal(shifted["select_q"].astype(np.float64) - 4.0, case["select_q"].astype(np.float64))
    got = S.reference(shifted)
    assert np.array_equal(got["argmax_row"], ref["argmax_row"])
    if exact:                                                            # (the shift itself rounded nothing: the weights are the same)
        assert np.array_equal(got["value"], ref["value"])
    assert np.allclose(got["value"][~ref["nothing"]], ref["value"][~ref["nothing"]], rtol=0, atol=1e-4)
    assert np.allclose(got["feat_mean"], ref["feat_mean"], rtol=0, atol=1e-4)


def test_new_entry_point_is_declared_with_its_rule_and_mirrored():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        full = fh.read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    name = "bridges_soft_expect"
    decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M).group(1)
    assert name in abi.EXPORTED_SYMBOLS and decl.count(",") + 1 == len(abi.SIGNATURES[name]) == 15
    C = abi.C
    assert abi.SIGNATURES[name] == [C.c_int32, *[C.c_void_p] * 4, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                    *[C.c_void_p] * 5]
    for arg in (r"const\s+float\s*\*\s*select_q", r"const\s+float\s*\*\s*next_q", r"float\s+temperature", r"int64_t\s+feat_row_stride",
                r"const\s+int64_t\s*\*\s*feat_row", r"int32_t\s+dim", r"float\s*\*\s*entropy", r"int32_t\s*\*\s*argmax_row"):
        assert re.search(arg, decl), arg
    comment = full[:full.index("int bridges_soft_expect(")].rsplit("/*", 1)[1]
    for word in ("ELIGIBLE", "bridges_boltzmann_select", "VALUE", "FEATURE MEAN", "ENTROPY", "ARG-MAX ROW", "NOTHING ELIGIBLE",
                 "0x7fffffff", "ascending row order", "No atomics"):
        assert word in comment, word


class _CountingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def test_next_targets_without_a_temperature_makes_the_calls_it_made(monkeypatch):
    from bridges_hip import abi, dqn_ops
    lib = _CountingLib()
    monkeypatch.setattr(abi, "require_gpu", lambda: lib)
    monkeypatch.setattr(dqn_ops, "_stream", lambda: None)
    seg = torch.tensor([0, 2, 5], dtype=torch.int32)
    nq, done, lin = torch.randn(5), torch.zeros(2, dtype=torch.bool), torch.zeros(2)
    sf, ar = torch.randn(5, 8), torch.zeros(2, 8)
    dqn_ops.next_targets(seg, nq, done, 0.9, lin=lin)
    assert lib.calls == ["bridges_td_target"]
    lib.calls.clear()
    dqn_ops.next_targets(seg, nq, done, 0.9, next_sf=sf, action_raster=ar, lin=lin, temperature=None)
    assert lib.calls == ["bridges_td_target", "bridges_td_target"]
    lib.calls.clear()
    dqn_ops.next_targets(seg, nq, done, 0.9, next_sf=lambda best: sf[best], action_raster=ar, lin=lin, discount=torch.ones(2), select_q=nq.clone())
    assert lib.calls == ["bridges_td_target_select", "bridges_td_target_rows"]
    lib.calls.clear()
    heads = []
    dqn_ops.next_targets(seg, nq, done, 0.9, action_raster=ar, lin=lin, temperature=0.5, next_feat=sf,
                         feat_head=lambda mean: heads.append(tuple(mean.shape)) or mean)
    assert lib.calls == ["bridges_soft_expect", "bridges_td_target_select"] and heads == [(2, 8)]
    with pytest.raises(ValueError, match="lin"):
        dqn_ops.next_targets(seg, nq, done, 0.9, temperature=0.5)


def test_constructor_takes_the_temperature_and_refuses_what_is_none(monkeypatch):
    a = host_agent(monkeypatch, stand_in_env())
    assert a.target_temperature is None and a._soft_stats is None
    b = host_agent(monkeypatch, stand_in_env(), target_temperature=0.5, double_q=True, n_step=3, prioritized=True)
    assert b.target_temperature == 0.5 and b.ring.width == host_agent(monkeypatch, stand_in_env(), n_step=3).ring.width
    assert host_agent(monkeypatch, stand_in_env(), target_temperature=2).target_temperature == 2.0
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1.0", True):
        with pytest.raises(ValueError, match="target_temperature"):
            host_agent(monkeypatch, stand_in_env(), target_temperature=bad)


def test_cli_option_is_opt_in():
    from robotoddler.training.successor_dqn import (build_parser, check_target_temperature, target_temperature_from_args)
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64"]))
    assert "target_temperature" not in plain and target_temperature_from_args(plain) == {}
    check_target_temperature(plain)
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--target_temperature", "0.25", "--double_q"]))
    assert args["target_temperature"] == 0.25 and target_temperature_from_args(args) == dict(target_temperature=0.25)
    check_target_temperature(args)
    assert "--target_temperature" in build_parser().format_help()
    for bad in ("0", "-1", "inf", "nan"):
        with pytest.raises(SystemExit) as e:
            check_target_temperature(vars(build_parser().parse_args(["--num_envs", "64", "--target_temperature", bad])))
        assert isinstance(e.value.code, str) and "--target_temperature" in e.value.code


@pytest.mark.parametrize("argv", [["--model", "SuccessorMLP", "--target_temperature", "1.0"],
                                  ["--model", "SuccessorMLP", "--num_envs", "1", "--target_temperature", "1.0"]])
def test_cli_refuses_the_single_env_loop_in_words(argv):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and "--target_temperature" in e.value.code and "--num_envs" in e.value.code, e.value.code


def test_checkpoint_entry_only_with_the_option_and_refused_under_another_setting(tmp_path):
    from robotoddler.training.vec_dqn import VecDQN

    def agent(T):
        a = VecDQN.__new__(VecDQN)
        a.n_task_targets, a.n_task_obstacles, a.n_step, a.double_q = 0, 0, 1, False
        a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
        a.step_images = torch.zeros((3, 4, 4))
        a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        if T is not None:
            a.target_temperature = T
        return a
    paths = {}
    for T in (None, 0.5, 2.0):
        paths[T] = str(tmp_path / f"agent_{T}.pt")
        agent(T).save_extra(paths[T], lockstep=5)
    keys = {T: sorted(torch.load(paths[T], weights_only=True)) for T in paths}
    assert "target_temperature" not in keys[None] and keys[0.5] == sorted(keys[None] + ["target_temperature"])
    assert torch.load(paths[0.5], weights_only=True)["target_temperature"] == 0.5
    assert agent(None).load_extra(paths[None]) == agent(0.5).load_extra(paths[0.5]) == dict(lockstep=5)
    for have, want in ((None, 0.5), (0.5, None), (0.5, 2.0)):
        with pytest.raises(ValueError, match="target_temperature"):
            agent(have).load_extra(paths[want])


def test_log_values_carry_the_keys_only_with_the_option():
    from robotoddler.training.vec_dqn import EPISODE_KEYS, DeferredLosses, lockstep_log_values
    info = dict(mean_reward=0., mean_lin_reward=0., avg_loss=0., lockstep_env_steps=1, epsilon=0.1, env_steps=1, steps_per_s=1.,
                **{k: None for k in EPISODE_KEYS})
    assert "target_entropy" not in lockstep_log_values(info)
    vals = lockstep_log_values(dict(info, target_entropy=1.5, soft_value_gap=0.25))
    assert vals["target_entropy"] == 1.5 and vals["soft_value_gap"] == 0.25

    class Ready:
        def synchronize(self):
            pass
    owner = type("A", (), {})()
    d = DeferredLosses(torch.tensor([1.0, 2.0, 0.5, 0.125]), Ready(), None, names=("target_entropy", "soft_value_gap"), owner=owner)
    assert d.get() == [1.0, 2.0] and d.soft == dict(target_entropy=0.5, soft_value_gap=0.125) and owner.soft_value_gap == 0.125
    plain = DeferredLosses(torch.tensor([1.0, 2.0]), Ready(), None)
    assert plain.get() == [1.0, 2.0] and plain.soft is None
    # no riders named: nothing is split off, whatever the values and with no owner to write to
    unsplit = DeferredLosses(torch.tensor([1.0, 2.0, 0.5, 0.125]), Ready(), None, names=())
    assert unsplit.get() == [1.0, 2.0, 0.5, 0.125] and unsplit.soft is None
