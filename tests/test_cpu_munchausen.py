"""CPU: the reference of the Munchausen operators (tests/munchausen_ref.py) -- it agrees with soft_target_ref where the two
overlap, is shift invariant, has the arg-max limit, and its probes reject every defective twin -- and the host side of
VecDQN(munchausen_alpha=A): the header and its ctypes mirror, next_targets' launches, the constructor, the command line, the log
keys and the checkpoint entry."""
import os
import re

import numpy as np
import pytest
import torch

import munchausen_ref as M
import soft_target_ref as S
from test_cpu_nstep import host_agent, stand_in_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_reference_conforms_to_itself_on_every_case():
    for case in M.cpu_cases():
        ref = M.reference(case)
        assert M.violations(M.as_device(ref), ref) == []
        assert (ref["value"][ref["nothing"]] == -np.inf).all() and (ref["miss"][ref["nothing"]] == 1).all()
        assert (ref["tlogp"] <= 0).all() and not np.signbit(ref["bonus"][ref["bonus"] == 0]).any()
        assert not ref["tlogp"][ref["miss"] == 1].any() and not ref["bonus"][ref["miss"] == 1].any()


def test_the_record_layout_is_the_loop_s():
    from robotoddler.training import records as R
    assert (M.O_ASHAPE, M.O_APOSE, M.O_ATB, M.O_ATF, M.O_AFACE, M.RECORD_WIDTH) == \
        (R.O_ASHAPE, R.O_APOSE, R.O_ATB, R.O_ATF, R.O_AFACE, R.RECORD_WIDTH)


def test_value_is_the_expectation_plus_t_times_the_entropy():
    """V_T = sum_j p_j q_j + T H(p): the log-sum-exp value against soft_target_ref's value and entropy on its seeded tables."""
    for T in S.TEMPERATURES[1:3]:
        soft = S.random_probe(T, 0, double=False)
        ref_s = S.reference(soft)
        ref_m = M.reference(dict(seg_lo=soft["seg_lo"], seg_hi=soft["seg_hi"], q=soft["select_q"], T=T))
        live = ~ref_s["nothing"]
        assert np.array_equal(ref_m["nothing"], ref_s["nothing"]) and live.sum() > 10
        t32 = M.f32(T)
        want = ref_s["value"][live] + t32 * ref_s["entropy"][live]
        # (both sides in float64: the expectation's own bound, T times the entropy's, and this module's, with room to spare)
        tol = ref_s["value_bound"][live] + t32 * ref_s["entropy_bound"][live] + ref_m["value_bound"][live] + 1e-13 * np.abs(want)
        assert (np.abs(ref_m["value"][live] - want) <= tol).all()


def test_a_constant_added_to_q_shifts_the_value_and_leaves_the_log_policy():
    case = M.random_probe(1.0)
    ref = M.reference(case)
    shifted = dict(case, q=(case["q"].astype(np.float64) + 4.0).astype(np.float32))
    exact = np.array_equal(shifted["q"].astype(np.float64) - 4.0, case["q"].astype(np.float64))
    got = M.reference(shifted)
    live, hit = ~ref["nothing"], ref["miss"] == 0
    assert np.array_equal(got["miss"], ref["miss"])
    assert np.allclose(got["value"][live], ref["value"][live] + 4.0, rtol=0, atol=1e-4)
    assert np.allclose(got["tlogp"][hit], ref["tlogp"][hit], rtol=0, atol=1e-4)
    if exact:                                                # (the shift itself rounded nothing: the weights are the same)
        assert np.array_equal(got["tlogp"], ref["tlogp"]) and np.array_equal(got["bonus"], ref["bonus"])


def test_small_temperature_gives_the_maximum_and_no_bonus_on_its_row():
    rng = np.random.default_rng(5)
    q = rng.permutation(np.arange(40, dtype=np.float32))     # unique maxima, gaps of 1 >> T
    lo, hi = np.asarray([0, 10, 17], np.int32), np.asarray([10, 40, 18], np.int32)
    best = np.asarray([a + int(np.argmax(q[a:b])) for a, b in zip(lo, hi)], np.int32)
    ref = M.reference(dict(seg_lo=lo, seg_hi=hi, q=q, T=1e-6, taken_row=best, alpha=1.0, clip_lo=-1.0))
    assert np.array_equal(ref["value"], q[best].astype(np.float64))
    assert not ref["tlogp"].any() and not ref["bonus"].any() and not ref["miss"].any()
    other = np.where(best == lo, lo + 1, lo).astype(np.int32)[:2]
    ref = M.reference(dict(seg_lo=lo[:2], seg_hi=hi[:2], q=q, T=1e-6, taken_row=other, alpha=1.0, clip_lo=-1.0))
    assert (ref["tlogp"] <= -1.0 + 1e-5).all() and (ref["bonus"] == -1.0).all()          # any other row: clipped


def test_tied_and_single_rows():
    tied = M.tied_probe()
    ref = M.reference(tied)
    n = (tied["seg_hi"] - tied["seg_lo"]).astype(np.float64)
    T = M.f32(tied["T"])
    assert np.allclose(ref["value"], tied["q"][tied["seg_lo"]] + T * np.log(n), rtol=1e-14, atol=0)
    assert np.allclose(ref["tlogp"], -T * np.log(n), rtol=1e-14, atol=0)
    one = M.single_probe()
    ref = M.reference(one)
    assert np.array_equal(ref["value"], one["q"].astype(np.float64)) and not ref["bonus"].any() and not np.signbit(ref["bonus"]).any()


@pytest.mark.parametrize("twin", M.TWINS)
def test_the_bound_rejects_every_twin(twin):
    assert M.rejected(twin)


def test_alpha_or_clip_zero_give_positive_zero():
    for kw in (dict(alpha=0.0), dict(clip_lo=0.0)):
        for case in [M.random_probe(0.1, **kw)] + M.nonfinite_probe(**kw):
            ref = M.reference(case)
            assert not ref["bonus"].any() and not np.signbit(ref["bonus"]).any()


@pytest.mark.parametrize("twin", M.ROW_TWINS)
def test_the_action_table_rejects_every_row_twin(twin):
    t = M.action_row_table()
    assert not np.array_equal(M.action_row(**t, twin=twin), M.action_row(**t))


def test_the_action_table_holds_what_it_promises():
    t = M.action_row_table()
    row = M.action_row(**t)
    cand = [int(t["idx"][j]) if j != M.NONE_ROW else None for j in row]
    pos = {int(c): j for j, c in enumerate(t["idx"])}
    assert cand[0] in (7, 40) and row[0] == min(pos[7], pos[40])                   # equal pose and descriptor: the first row wins
    assert cand[1] == 41 and (t["cand_desc"][41] == t["cand_desc"][7]).all()         # the descriptor again, told apart by the pose
    assert cand[2] == int(t["idx"][100]) and cand[3] == 90 and cand[4] == int(t["idx"][149]) and cand[7] == int(t["idx"][5])
    assert cand[5] is None and cand[8] is None                                      # an empty segment; a pose nobody has
    assert cand[6] is None and M.action_row(**t, twin="float_eq")[6] == pos[90]      # the sign of a zero
    lo, hi = t["seg_lo"], t["seg_hi"]
    assert (lo[0], hi[0]) == (lo[1], hi[1]) and lo[8] < hi[7]                        # shared and overlapping segments


def _declaration(name):
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        full = fh.read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M).group(1)
    comment = full[:full.index("int " + name + "(")].rsplit("/*", 1)[1]
    return decl, comment


def test_new_entry_points_are_declared_with_their_rule_and_mirrored():
    from bridges_hip import abi
    C = abi.C
    vp, i32, f32, i64 = C.c_void_p, C.c_int32, C.c_float, C.c_int64
    want = {"bridges_soft_value": [i32, vp, vp, vp, f32, vp, f32, f32, vp, vp, vp, vp, vp],
            "bridges_soft_value_rel": [i32, vp, vp, vp, f32, f32, vp, f32, f32, vp, vp, vp, vp, vp, vp],
            "bridges_action_row": [i32, vp, vp, vp, vp, vp, vp, i64, vp, vp],
            "bridges_replay_unpack_prev": abi.SIGNATURES["bridges_replay_unpack"]}
    for name, sig in want.items():
        decl, _ = _declaration(name)
        assert name in abi.EXPORTED_SYMBOLS and decl.count(",") + 1 == len(abi.SIGNATURES[name]) == len(sig)
        assert abi.SIGNATURES[name] == sig
    decl, comment = _declaration("bridges_soft_value")
    for arg in (r"const\s+int32_t\s*\*\s*taken_row", r"float\s+alpha", r"float\s+clip_lo", r"float\s*\*\s*tlogp", r"uint8_t\s*\*\s*miss"):
        assert re.search(arg, decl), arg
    for word in ("bridges_boltzmann_select", "ELIGIBILITY", "VALUE", "NOTHING ELIGIBLE", "TAKEN ROW", "0x7fffffff", "+0.0", "fmin",
                 "fmax", "no atomics"):
        assert word in comment, word
    decl, comment = _declaration("bridges_action_row")
    assert re.search(r"int64_t\s+rec_stride", decl) and "64-bit patterns" in comment and "0x7fffffff" in comment
    prev, _ = _declaration("bridges_replay_unpack_prev")
    assert re.sub(r"\s+", " ", prev) == re.sub(r"\s+", " ", _declaration("bridges_replay_unpack")[0])


class _CountingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def test_next_targets_launches_the_operator_only_with_the_option(monkeypatch):
    from bridges_hip import abi, dqn_ops
    lib = _CountingLib()
    monkeypatch.setattr(abi, "require_gpu", lambda: lib)
    monkeypatch.setattr(dqn_ops, "_stream", lambda: None)
    seg = torch.tensor([0, 2, 5], dtype=torch.int32)
    nq, done, lin = torch.randn(5), torch.zeros(2, dtype=torch.bool), torch.zeros(2)
    sf, ar = torch.randn(5, 8), torch.zeros(2, 8)
    dqn_ops.next_targets(seg, nq, done, 0.9, action_raster=ar, lin=lin, temperature=0.5, next_feat=sf)
    assert lib.calls == ["bridges_soft_expect", "bridges_td_target_select"]
    lib.calls.clear()
    cur = dict(cur_seg=torch.tensor([0, 3, 4], dtype=torch.int32), cur_q=torch.randn(4), taken_row=torch.tensor([1, 3], dtype=torch.int32))
    stats = {}
    dqn_ops.next_targets(seg, nq, done, 0.9, action_raster=ar, lin=lin, temperature=0.5, next_feat=sf, munchausen=(0.9, -1.0),
                         stats=stats, **cur)
    assert lib.calls == ["bridges_soft_expect", "bridges_td_target_select", "bridges_soft_value", "bridges_soft_value",
                         "bridges_td_target_select"]
    assert {"soft_value", "tlogp", "bonus", "miss", "entropy", "value"} <= set(stats)
    lib.calls.clear()
    dqn_ops.next_targets(seg, nq, done, 0.9, lin=lin, temperature=0.5, munchausen=(0.9, -1.0), relative=True, **cur)
    assert lib.calls == ["bridges_soft_expect_rel", "bridges_td_target_select", "bridges_soft_value_rel", "bridges_soft_value_rel",
                         "bridges_td_target_select"]
    with pytest.raises(ValueError, match="temperature"):
        dqn_ops.next_targets(seg, nq, done, 0.9, lin=lin, munchausen=(0.9, -1.0), **cur)


def test_constructor_takes_the_option_and_refuses_what_it_cannot_run(monkeypatch):
    a = host_agent(monkeypatch, stand_in_env())
    assert a.munchausen is None and a.replay_env_s is None
    b = host_agent(monkeypatch, stand_in_env(), target_temperature=0.5, munchausen_alpha=0.9)
    assert b.munchausen == (0.9, -1.0)
    c = host_agent(monkeypatch, stand_in_env(), target_temperature=0.5, munchausen_alpha=1, munchausen_clip=-0.25, target_temp_relative=True,
                   prioritized=True)
    assert c.munchausen == (1.0, -0.25)
    for kw, word in ((dict(munchausen_alpha=0.9), "target_temperature"),
                     (dict(munchausen_alpha=0.9, target_temperature=1.0, double_q=True), "double_q"),
                     (dict(munchausen_alpha=0.9, target_temperature=1.0, n_step=2), "n_step"),
                     (dict(munchausen_clip=-1.0, target_temperature=1.0), "munchausen_alpha"),
                     (dict(munchausen_alpha=1.5, target_temperature=1.0), "munchausen_alpha"),
                     (dict(munchausen_alpha=-0.1, target_temperature=1.0), "munchausen_alpha"),
                     (dict(munchausen_alpha=float("nan"), target_temperature=1.0), "munchausen_alpha"),
                     (dict(munchausen_alpha=True, target_temperature=1.0), "munchausen_alpha"),
                     (dict(munchausen_alpha=0.9, munchausen_clip=0.5, target_temperature=1.0), "munchausen_clip"),
                     (dict(munchausen_alpha=0.9, munchausen_clip=float("-inf"), target_temperature=1.0), "munchausen_clip"),
                     (dict(munchausen_alpha=0.9, munchausen_clip=float("nan"), target_temperature=1.0), "munchausen_clip")):
        with pytest.raises(ValueError, match=word):
            host_agent(monkeypatch, stand_in_env(), **kw)


def test_cli_options_are_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_munchausen, munchausen_from_args
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64"]))
    assert "munchausen_alpha" not in plain and "munchausen_clip" not in plain and munchausen_from_args(plain) == {}
    check_munchausen(plain)
    base = ["--model", "SuccessorMLP", "--num_envs", "64", "--target_temperature", "1.0"]
    args = vars(build_parser().parse_args(base + ["--munchausen_alpha", "0.9"]))
    assert args["munchausen_alpha"] == 0.9 and "munchausen_clip" not in args
    assert munchausen_from_args(args) == dict(munchausen_alpha=0.9, munchausen_clip=-1.0)
    check_munchausen(args)
    args = vars(build_parser().parse_args(base + ["--munchausen_alpha", "0.5", "--munchausen_clip", "-0.25", "--target_temp_relative"]))
    assert munchausen_from_args(args) == dict(munchausen_alpha=0.5, munchausen_clip=-0.25)
    help_text = build_parser().format_help()
    assert "--munchausen_alpha" in help_text and "--munchausen_clip" in help_text


@pytest.mark.parametrize("argv,words", [
    (["--munchausen_alpha", "0.9"], ("--munchausen_alpha", "--num_envs")),
    (["--num_envs", "1", "--munchausen_clip", "-1", "--munchausen_alpha", "0.9"], ("--munchausen_clip", "--num_envs")),
    (["--num_envs", "64", "--munchausen_alpha", "0.9"], ("--munchausen_alpha", "--target_temperature")),
    (["--num_envs", "64", "--munchausen_clip", "-0.5", "--munchausen_alpha", "0.9"], ("--munchausen_clip", "--target_temperature")),
    (["--num_envs", "64", "--munchausen_alpha", "0.9", "--target_temperature", "1.0", "--double_q"], ("--munchausen_alpha", "--double_q")),
    (["--num_envs", "64", "--munchausen_alpha", "0.9", "--target_temperature", "1.0", "--n_step", "3"], ("--munchausen_alpha", "--n_step")),
    (["--num_envs", "64", "--munchausen_clip", "-0.5", "--target_temperature", "1.0"], ("--munchausen_clip", "--munchausen_alpha")),
    (["--num_envs", "64", "--munchausen_alpha", "1.5", "--target_temperature", "1.0"], ("--munchausen_alpha", "[0, 1]")),
    (["--num_envs", "64", "--munchausen_alpha", "nan", "--target_temperature", "1.0"], ("--munchausen_alpha", "[0, 1]")),
    (["--num_envs", "64", "--munchausen_alpha", "0.9", "--munchausen_clip", "0.5", "--target_temperature", "1.0"], ("--munchausen_clip",)),
    (["--num_envs", "64", "--munchausen_alpha", "0.9", "--munchausen_clip=-inf", "--target_temperature", "1.0"], ("--munchausen_clip",)),
])
def test_cli_refuses_in_words(argv, words):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(["--model", "SuccessorMLP", "--max_steps", "10"] + argv)
    assert isinstance(e.value.code, str), e.value.code
    for w in words:
        assert w in e.value.code, e.value.code


def test_tools_take_the_flags():
    for tool in ("train_throughput.py", "learning_curve.py", "find_syncs.py"):
        with open(os.path.join(ROOT, "tools", tool)) as fh:
            text = fh.read()
        # the tools take every training option through the two shared functions, whose Munchausen group is checked below
        assert "add_training_arguments(ap" in text and "**agent_options_from_args(vars(a)" in text, tool
    import argparse
    from robotoddler.training.successor_dqn import add_training_arguments, agent_options_from_args
    ap = argparse.ArgumentParser()
    add_training_arguments(ap, prioritized_flag=True)
    a = ap.parse_args(["--target_temperature", "1.0", "--munchausen_alpha", "0.9", "--munchausen_clip", "-0.5"])
    kw = agent_options_from_args(vars(a), num_envs=64)
    assert (kw["munchausen_alpha"], kw["munchausen_clip"], kw["target_temperature"]) == (0.9, -0.5, 1.0)
    with open(os.path.join(ROOT, "tools", "soft_target_bench.py")) as fh:
        assert "--munchausen" in fh.read()


def test_checkpoint_entry_only_with_the_option_and_refused_under_another_setting(tmp_path):
    from robotoddler.training.vec_dqn import VecDQN

    def agent(m):
        a = VecDQN.__new__(VecDQN)
        a.n_task_targets, a.n_task_obstacles, a.n_step, a.double_q = 0, 0, 1, False
        a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
        a.step_images = torch.zeros((3, 4, 4))
        a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        a.target_temperature = 1.0
        if m is not None:
            a.munchausen = m
        return a
    settings = (None, (0.9, -1.0), (0.9, -0.5), (0.5, -1.0))
    paths = {}
    for m in settings:
        paths[m] = str(tmp_path / f"agent_{settings.index(m)}.pt")
        agent(m).save_extra(paths[m], lockstep=5)
    keys = {m: sorted(torch.load(paths[m], weights_only=True)) for m in paths}
    assert "munchausen" not in keys[None] and keys[(0.9, -1.0)] == sorted(keys[None] + ["munchausen"])
    assert tuple(torch.load(paths[(0.9, -1.0)], weights_only=True)["munchausen"]) == (0.9, -1.0)
    assert agent(None).load_extra(paths[None]) == agent((0.9, -1.0)).load_extra(paths[(0.9, -1.0)]) == dict(lockstep=5)
    for have, want in ((None, (0.9, -1.0)), ((0.9, -1.0), None), ((0.9, -1.0), (0.9, -0.5)), ((0.9, -1.0), (0.5, -1.0))):
        with pytest.raises(ValueError, match="munchausen"):
            agent(have).load_extra(paths[want])


def test_log_values_carry_the_keys_only_with_the_option():
    from robotoddler.training.vec_dqn import EPISODE_KEYS, DeferredLosses, lockstep_log_values
    info = dict(mean_reward=0., mean_lin_reward=0., avg_loss=0., lockstep_env_steps=1, epsilon=0.1, env_steps=1, steps_per_s=1.,
                **{k: None for k in EPISODE_KEYS})
    assert not any(k.startswith("munchausen") for k in lockstep_log_values(dict(info, target_entropy=1.5, soft_value_gap=0.25)))
    vals = lockstep_log_values(dict(info, target_entropy=1.5, soft_value_gap=0.25, munchausen_bonus=-0.5, munchausen_clipped=0.25,
                                    munchausen_missed=0.0))
    assert (vals["munchausen_bonus"], vals["munchausen_clipped"], vals["munchausen_missed"]) == (-0.5, 0.25, 0.0)

    class Ready:
        def synchronize(self):
            pass
    owner = type("A", (), {})()
    owner.munchausen = (0.9, -1.0)
    soft, munch = ("target_entropy", "soft_value_gap"), ("munchausen_bonus", "munchausen_clipped", "munchausen_missed")
    d = DeferredLosses(torch.tensor([1.0, 2.0, 0.5, 0.125, -0.75, 0.25, 0.0]), Ready(), None, names=soft + munch, owner=owner)
    assert d.get() == [1.0, 2.0]
    assert d.soft == dict(target_entropy=0.5, soft_value_gap=0.125, munchausen_bonus=-0.75, munchausen_clipped=0.25, munchausen_missed=0.0)
    assert owner.munchausen_bonus == -0.75 and owner.munchausen_missed == 0.0
    owner.target_temp_relative = True
    d = DeferredLosses(torch.tensor([1.0, 0.5, 0.125, 3.0, -0.75, 0.25, 0.0]), Ready(), None,
                       names=soft + ("target_temperature_effective",) + munch, owner=owner)
    assert d.get() == [1.0] and d.soft["target_temperature_effective"] == 3.0 and d.soft["munchausen_bonus"] == -0.75
