"""CPU: the reference of the double Q-learning target (tests/double_q_ref.py) checked against the plain float32 statement, its
defective twins and the reference of the plain target, and the host side of VecDQN(double_q=True) -- the constructor, the command
line, the operator layer's refusal, the new entry point in the header and its ctypes mirror."""
import os
import re

import pytest
import torch

import double_q_ref as Q
import mlp_conformance as M
from nstep_ref import row_discounts
from test_cpu_nstep import host_agent, stand_in_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.8


def rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def forms(B):
    disc = row_discounts(B, GAMMA)
    assert len(set(disc.tolist())) > 2
    return (("scalar", GAMMA), ("rows", disc))


@pytest.mark.parametrize("sf_dim", Q.SELECT_SF_DIMS)
def test_plain_float32_passes_and_every_twin_is_rejected(sf_dim):
    pr = Q.select_probe(sf_dim, "cpu")
    for name, d in forms(len(pr["lo"])):
        ref, rows = Q.td_select_ref(pr, d)
        plain = Q.td_select_plain(pr, d)
        Q.select_conform("select", plain, plain, ref, rows, (sf_dim, name))
        for twin in Q.TWINS:
            assert rejected(Q.select_conform, "select", Q.td_select_plain(pr, d, twin=twin), plain, ref, rows, (sf_dim, name)), twin
    # 'value_from_select_q' selects the right rows: it is the VALUES that give it away
    assert Q.td_select_plain(pr, GAMMA, twin="value_from_select_q")[2] == rows


@pytest.mark.parametrize("strided", [True, False])
def test_probe_holds_the_cases_it_names(strided):
    pr = Q.select_probe(6, "cpu", strided=strided)
    lo, hi, sel, nq = pr["lo"], pr["hi"], pr["select_q"], pr["next_q"]
    assert [h - l for l, h in zip(lo, hi)][:7] == list(M.TD_LENGTHS) + [3]
    assert torch.equal(sel * 4, torch.round(sel * 4))                                     # quarters
    ties = {5: (7, 7 + 256), 3: (100, 256), 4: (63, 64)}
    for seg, (a, b) in ties.items():
        assert sel[lo[seg] + a] == sel[lo[seg] + b] == M.TD_PEAK == sel[lo[seg]:hi[seg]].max()
        assert int((sel[lo[seg]:hi[seg]] == M.TD_PEAK).sum()) == 2
    assert (7 % 256 == (7 + 256) % 256) and (100 // 64 != 256 % 256 // 64) and (63 // 64, 64 // 64) == (0, 1)
    _, rows = Q.td_select_ref(pr, GAMMA)
    _, plain_rows = M.td_ref(pr, GAMMA)
    assert rows[:7] == [0, lo[1] + 130, plain_rows[2], lo[3] + 100, lo[4] + 63, lo[5] + 7, lo[6] + 1] and rows[7] == M.NO_ROW
    assert rows[8] == lo[3] + 100 and rows[9] == lo[5] + 7 + 256                          # the shared ranges
    # the selected rows differ from the plain target's wherever a maximum was planted
    assert all(rows[i] != plain_rows[i] for i in (1, 3, 4, 5, 6, 8, 9))
    s = Q.SAME_SEGMENT
    assert torch.equal(sel[lo[s]:hi[s]], nq[lo[s]:hi[s]])
    assert bool(torch.isinf(nq[lo[6]:hi[6]]).all()) and bool(torch.isfinite(sel).all())
    ref, _ = Q.td_select_ref(pr, GAMMA)
    assert ref["q"][0][6] == -float("inf") and ref["q"][1][6] == 0 and not pr["done"][6]   # the value taken is -inf, met exactly
    assert bool(torch.isfinite(ref["sf"][0][6]).all()) and bool((ref["sf"][1][6] > 0).any())
    # sf_dim = 6: rows of 24 bytes, strided or not
    assert pr["sf_dim"] == 6 and tuple(pr["next_sf"].shape) == (nq.numel(), 6) and pr["next_sf"].stride(0) == (12 if strided else 6)
    for sf_dim in (4, 64, 4096):
        p = Q.select_probe(sf_dim, "cpu", strided=strided)
        assert p["next_sf"][0].numel() == sf_dim and p["next_sf"].is_contiguous() != strided


@pytest.mark.parametrize("sf_dim", [0, 4, 64])
def test_with_select_q_equal_to_next_q_the_reference_is_td_ref(sf_dim):
    """td_ref's values are the oracle's float32 evaluation, this reference is float64 on the float32 gamma: the same rows, the
    same bounds, and values that differ by no more than the bound either reference grants a float32 evaluation."""
    pr = Q.select_probe(sf_dim, "cpu")
    pr["select_q"] = pr["next_q"].clone()
    for gamma in (1.0, GAMMA):
        ref, rows = Q.td_select_ref(pr, gamma)
        want, want_rows = M.td_ref(pr, gamma)
        assert rows == want_rows
        for k in ("q", "sf"):
            if want[k] is None:
                assert ref[k] is None
                continue
            assert torch.allclose(ref[k][1], want[k][1], rtol=1e-6, atol=0)
            a, b = ref[k][0], want[k][0].reshape(ref[k][0].shape)
            err = torch.where(a == b, torch.zeros_like(a), (a - b).abs())
            assert bool((err <= ref[k][1].reshape(a.shape)).all())
        plain = M.td_plain(pr, gamma)
        Q.select_conform("same", plain, plain, ref, rows, (sf_dim, gamma))                  # the plain target passes this reference


def test_new_entry_point_is_declared_and_mirrored():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    name = "bridges_td_target_select"
    decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M).group(1)
    assert name in abi.EXPORTED_SYMBOLS and decl.count(",") + 1 == len(abi.SIGNATURES[name])
    # the inputs of bridges_td_target_rows plus select_q and the scalar gamma
    assert len(abi.SIGNATURES[name]) == len(abi.SIGNATURES["bridges_td_target_rows"]) + 2
    assert re.search(r"const\s+float\s*\*\s*select_q", decl) and re.search(r"const\s+float\s*\*\s*discount", decl) and "float gamma" in decl


def test_vec_dqn_takes_double_q_and_defaults_to_false(monkeypatch):
    assert host_agent(monkeypatch, stand_in_env()).double_q is False
    assert host_agent(monkeypatch, stand_in_env(), double_q=False).double_q is False
    a = host_agent(monkeypatch, stand_in_env(), double_q=True)
    assert a.double_q is True and a.ring.width == host_agent(monkeypatch, stand_in_env()).ring.width      # no new column
    b = host_agent(monkeypatch, stand_in_env(), double_q=True, n_step=3, prioritized=True)
    assert b.double_q and b.n_step == 3 and b.prioritized


def test_checkpoint_extra_is_the_same_with_and_without_double_q(tmp_path):
    """The ring stores transitions, not targets: save_extra writes no key for the option and load_extra accepts either."""
    from robotoddler.training.vec_dqn import VecDQN

    def agent(double_q):
        a = VecDQN.__new__(VecDQN)
        a.n_task_targets, a.n_task_obstacles, a.n_step, a.double_q = 0, 0, 1, double_q
        a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
        a.step_images = torch.zeros((3, 4, 4))
        a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        return a
    paths = {}
    for flag in (False, True):
        paths[flag] = str(tmp_path / f"agent_{int(flag)}.pt")
        agent(flag).save_extra(paths[flag], lockstep=5)
    keys = [sorted(torch.load(paths[f], weights_only=True)) for f in (False, True)]
    assert keys[0] == keys[1] and not any("double" in k for k in keys[0])
    assert agent(False).load_extra(paths[True]) == agent(True).load_extra(paths[False]) == dict(lockstep=5)


def test_cli_option_is_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_double_q
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64"]))
    assert "double_q" not in plain                                        # a plain parse keeps the keys it always had
    check_double_q(plain)
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--double_q", "--n_step", "3",
                                           "--prioritized_replay"]))
    assert args["double_q"] is True and args["n_step"] == 3
    check_double_q(args)
    assert "--double_q" in build_parser().format_help()


@pytest.mark.parametrize("argv", [["--model", "SuccessorMLP", "--double_q"],
                                  ["--model", "SuccessorMLP", "--num_envs", "1", "--double_q"]])
def test_cli_refuses_the_single_env_loop_in_words(argv):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and "--double_q" in e.value.code and "--num_envs" in e.value.code, e.value.code


def test_next_targets_refuses_select_q_without_lin():
    """The single-env form (lin=None) has no double-Q target: refused before anything touches the GPU."""
    from bridges_hip import dqn_ops
    nq = torch.zeros(4)
    seg = torch.tensor([0, 2, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="lin"):
        dqn_ops.next_targets(seg, nq, torch.zeros(2, dtype=torch.bool), GAMMA, select_q=nq.clone())
