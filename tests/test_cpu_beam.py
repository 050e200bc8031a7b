"""CPU-only: the select rule of bridges_beam_select in numpy (tests/beam_ref.py) -- its probe tables tell every defective twin from
the rule --, the bookkeeping of VecDQN.beam_search restated on a scripted toy, the header / abi.py mirror of the three new symbols,
the command line of --eval_beam, and the fork's array table against the buffer tables of abi.py."""
import os
import re

import numpy as np
import pytest

import beam_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")
NEW_SYMBOLS = ("bridges_env_fork_scratch", "bridges_env_fork", "bridges_beam_select")


# ---- the select rule -----------------------------------------------------------------------------------------------------------
def _sorted_statement(case):
    """The rule once more, through Python's sort on a key: candidates by (-S, -q, env, row)."""
    B, E = case["B"], len(case["seg_lo"])
    out = BR.reference(dict(case, live=np.zeros(E, np.uint8)))          # all padded
    for g in range(E // B):
        c = []
        for e in range(g * B, (g + 1) * B):
            if not case["live"][e]:
                continue
            for j in range(int(case["seg_lo"][e]), int(case["seg_hi"][e])):
                v = float(case["q"][j])
                if v != v or v == -np.inf:
                    continue
                S = float(case["ret"][e]) + float(case["disc"][e]) * v
                if S == S:
                    c.append((-S, -v, e, j))
        for i, (mS, mv, e, j) in enumerate(sorted(c)[:B]):
            s = g * B + i
            owner = e if case["rep"] is None else int(case["rep"][e])
            out["src"][s], out["sel_compact"][s] = e, case["idx"][j]
            out["sel_index"][s] = max(int(case["idx"][j]) - int(case["cand_offset"][owner]), 0)
            out["q_sel"][s], out["score"][s], out["live"][s] = case["q"][j], -mS, 1
    return out


def test_reference_agrees_with_a_second_statement_of_the_rule():
    cases = list(BR.probe_tables().values()) + [BR.random_case(G, B, seed=10 * G + B) for G in (1, 5) for B in (1, 2, 8, 16)]
    for case in cases:
        a, b = BR.reference(case), _sorted_statement(case)
        for k in BR.OUTPUTS:                                             # (-0.0 scores: compare values, not bits)
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_probe_tables_hold_what_the_rule_names():
    t = BR.probe_tables()
    ref = {name: BR.reference(case) for name, case in t.items()}
    r = ref["ties_in_S_different_q"]
    assert r["score"][:3].tolist() == [2.0, 2.0, 2.0] and r["q_sel"][:3].tolist() == [2.0, 1.0, 0.0] and r["src"][:3].tolist() == [1, 0, 2]
    r = ref["ties_in_q"]
    assert r["src"].tolist() == [0, 0] and r["sel_compact"].tolist() == [int(t["ties_in_q"]["idx"][3]), int(t["ties_in_q"]["idx"][4])]
    r = ref["nan_and_minus_inf"]
    assert r["live"].tolist() == [1, 1, 1, 1] and r["q_sel"].tolist() == [np.inf, 1.0, 0.5, -2.0] and not np.isnan(r["score"]).any()
    r = ref["empty_and_short"]
    assert r["live"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and r["src"].tolist() == [1, 1, 2, 3, 4, 5, 6, 7]
    assert r["score"][2:].tolist() == [-np.inf] * 6 and r["sel_index"][2:].tolist() == [0] * 6
    r, c = ref["shared_rep_rows"], t["shared_rep_rows"]
    assert r["src"].tolist() == [1, 0, 2, 1]                             # env 1 (ret 0.25) and env 0 on the shared row q = 0.9, ...
    assert r["sel_index"][0] == c["idx"][1] - c["cand_offset"][0]        # ... with the REPRESENTATIVE's offset
    r = ref["dead_beams"]
    assert r["src"].tolist() == [1, 1, 2, 2]
    assert ref["score_needs_f64"]["src"].tolist() == [0, 1]
    r = ref["width_1"]
    assert r["sel_compact"].tolist() == [int(t["width_1"]["idx"][1]), int(t["width_1"]["idx"][5]), 0] and r["live"].tolist() == [1, 1, 0]


@pytest.mark.parametrize("twin", BR.TWINS)
def test_every_defective_twin_is_rejected_by_a_probe(twin):
    t = BR.probe_tables()
    rejected = [name for name, case in t.items() if not BR.same(BR.reference(case), BR.reference(case, twin=twin))]
    assert rejected, f"no probe table tells the twin {twin!r} from the rule"


def test_width_1_with_every_beam_live_is_the_first_maximum():
    case = BR.random_case(12, 1, seed=3)
    case["live"][:] = 1
    ok = ~np.isnan(case["q"]) & (case["q"] != -np.inf)
    case["q"][~ok] = 0.25                                                # (NaN rows: the greedy kernel decides those its own way)
    out = BR.reference(case)
    for e in range(12):
        lo, hi = int(case["seg_lo"][e]), int(case["seg_hi"][e])
        if hi > lo:
            assert out["sel_compact"][e] == case["idx"][lo + int(np.argmax(case["q"][lo:hi]))]
        else:
            assert out["live"][e] == 0


# ---- the bookkeeping of the loop ----------------------------------------------------------------------------------------------
def test_best_finished_ordering():
    better = BR.better_finished
    assert better((False, -5.0, 3, 2), None)
    assert better((True, -5.0, 3, 2), (False, 9.0, 0, 0)) and not better((False, 9.0, 0, 0), (True, -5.0, 3, 2))   # success first
    assert better((True, 1.5, 3, 2), (True, 1.0, 0, 0)) and not better((True, 1.0, 0, 0), (True, 1.5, 3, 2))       # then the return
    assert better((True, 1.0, 1, 3), (True, 1.0, 2, 0)) and not better((True, 1.0, 2, 0), (True, 1.0, 1, 3))       # then the earlier depth
    assert better((True, 1.0, 1, 0), (True, 1.0, 1, 1)) and not better((True, 1.0, 1, 1), (True, 1.0, 1, 1))       # then the lower slot


def _toy():
    """Two actions per state.  q misleads a greedy policy: action 0 looks better at the root but its subtree never succeeds; action
    1 at the root, then 1 again, reaches the target (reward 1 = n_targets) at depth 1.  Every path is done at depth 2 at the latest."""
    def q_of(state):
        return [1.0, 0.9] if state == () else ([0.4, 0.6] if state == (1,) else [0.5, 0.4])

    def step_of(state, a):
        path = state + (a,)
        if path == (1, 1):
            return 0.75, 1.0, True
        return 0.25, (0.0 if len(path) < 3 else -1.0), len(path) == 3
    return q_of, step_of


def test_toy_search_a_wider_beam_finds_what_greedy_misses_and_a_done_beam_dies():
    q_of, step_of = _toy()
    gamma = 0.5
    best1, trace1 = BR.toy_search(1, 3, gamma, 1, q_of, step_of)
    assert trace1 == [[(0,)], [(0, 0)], []]                              # greedy: the first maximum at every depth, dead after done
    assert best1[0][0] is False and best1[1] == (0, 0, 0)
    assert best1[0][1] == 0.25 + 0.5 * 0.25 + 0.25 * 0.25                # ret += disc * lin, disc *= gamma
    best2, trace2 = BR.toy_search(2, 3, gamma, 1, q_of, step_of)
    # depth 0: both root actions; depth 1: S = 0.25 + 0.5 * q keeps (1, 1) (0.55) and (0, 0) (0.5); (1, 1) succeeds and dies
    assert trace2 == [[(0,), (1,)], [(0, 0)], []]
    assert best2[0][0] is True and best2[1] == (1, 1) and best2[0][2] == 1
    assert best2[0][1] == 0.25 + 0.5 * 0.75 and best2[2] == 0.0 + 0.5 * 1.0
    assert all((1, 1) not in live for live in trace2)                    # the finished beam is not expanded again
    # a later, failing episode with a higher return does not displace the success
    assert BR.toy_search(2, 3, gamma, 1, q_of, lambda s, a: (5.0, -1.0, True) if len(s) == 2 else step_of(s, a))[0][0][0] is True


# ---- header / abi.py ------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "bridges_hip.h")).read()


def test_new_symbols_are_declared_and_mirrored():
    import ctypes as C
    from bridges_hip import abi
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/bridges_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        sig = abi.SIGNATURES[name]
        assert len(params) == len(sig), (name, params)
        for p, ct in zip(params, sig):
            if "*" in p:
                assert ct is abi.vp or isinstance(ct, type(C.POINTER(C.c_int64))), (name, p, ct)
            elif p.startswith("int32_t"):
                assert ct is abi.i32, (name, p)
            elif p.startswith("int64_t"):
                assert ct is abi.i64, (name, p)
            else:
                pytest.fail(f"{name}: unexpected parameter {p!r}")
        assert name in abi.EXPORTED_SYMBOLS
    assert abi.BEAM_MAX_WIDTH == 16 and "1 <= B <= 16" in _header()


def _fork_table_of_the_source():
    text = open(os.path.join(PKG, "csrc", "api.hip")).read()
    body = text[text.index("static int fork_table("):text.index("#undef FORK_ROW")]
    return re.findall(r"FORK_ROW\((\w)\.(\w+),", body)


def test_fork_table_names_every_per_env_state_buffer_or_excludes_it():
    from bridges_hip import abi
    rows = _fork_table_of_the_source()
    assert [n for s, n in rows if s == "b"] == list(abi.FORK_ENV_FIELDS)
    assert [n for s, n in rows if s == "t"] == list(abi.FORK_TASK_FIELDS)
    assert [n for s, n in rows if s == "f"] == list(abi.FORK_FAMILY_FIELDS)
    forked = set(abi.FORK_ENV_FIELDS)
    # every per-env buffer of bridges_env_buffers (shape [E, ...]) is forked or excluded with a reason; candidate arrays ([C, ...]),
    # shared tables and scratch are neither
    per_env = [name for name, _dt, shape in abi.ENV_BUFFER_FIELDS + abi.ENV_BUFFER_FIELDS_TAIL if shape.split(",")[0] in ("E", "E1")]
    per_env.append("lp_snap")                                            # [E, lp_snap_stride]: set outside the two field tables
    for name in per_env:
        assert (name in forked) != (name in abi.FORK_EXCLUDED), f"{name}: per-env buffer neither forked nor excluded (or both)"
    assert forked <= set(per_env) and set(abi.FORK_EXCLUDED) <= set(per_env)
    assert all(isinstance(r, str) and r for r in abi.FORK_EXCLUDED.values())
    # the task buffers: every device buffer of bridges_task_buffers is per env, and every one is forked
    task = [name for name, _dt, _shape in abi.TASK_BUFFER_FIELDS + abi.OBSTACLE_BUFFER_FIELDS]
    assert sorted(task) == sorted(abi.FORK_TASK_FIELDS)
    # and the header's struct has no device pointer the tables above do not know
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    struct = text[text.index("typedef struct {", text.index("#define BRIDGES_MAX_OBSTACLES")):text.index("} bridges_task_buffers;")]
    pointers = re.findall(r"\*\s*(\w+)\s*;", struct)
    assert sorted(pointers) == sorted(task + ["gauss_k"])                # gauss_k: one table for all envs
    env_struct = text[text.index("typedef struct {", text.index("} bridges_task;")):text.index("} bridges_env_buffers;")]
    env_pointers = re.findall(r"\*\s*(\w+)\s*;", env_struct)
    known = [n for n, _d, _s in abi.ENV_BUFFER_FIELDS + abi.ENV_BUFFER_FIELDS_TAIL] + ["stats", "lp_snap"]
    assert sorted(env_pointers) == sorted(known)
    assert "task_class" in abi.FORK_FAMILY_FIELDS


# ---- command line -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,word", [(["--model", "SuccessorMLP", "--eval_beam", "4"], "--num_envs"),
                                       (["--model", "SuccessorMLP", "--num_envs", "64", "--eval_beam", "4"], "--eval_envs"),
                                       (["--model", "SuccessorMLP", "--num_envs", "64", "--eval_envs", "0", "--eval_beam", "4"], "--eval_envs"),
                                       (["--model", "SuccessorMLP", "--num_envs", "64", "--eval_envs", "8", "--eval_beam", "0"], "1..16"),
                                       (["--model", "SuccessorMLP", "--num_envs", "64", "--eval_envs", "8", "--eval_beam", "17"], "1..16")])
def test_cli_refuses_in_words(argv, word):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and "--eval_beam" in e.value.code and word in e.value.code, e.value.code


def test_cli_option_is_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_eval_beam
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64"]))
    assert "eval_beam" not in plain                                      # a plain parse keeps the keys it always had
    check_eval_beam(plain)
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--eval_envs", "8", "--eval_beam", "16"]))
    assert args["eval_beam"] == 16
    check_eval_beam(args)
    assert "beam_success_rate" in build_parser().format_help()


def test_beam_search_refuses_a_width_or_env_it_cannot_run():
    from robotoddler.training.vec_dqn import VecDQN, beam_env_like
    agent = VecDQN.__new__(VecDQN)
    agent.env = object()
    for width in (0, 17):
        with pytest.raises(ValueError, match="1..16"):
            agent.beam_search(object(), width)
        with pytest.raises(ValueError, match="1..16"):
            beam_env_like(object(), width)
    with pytest.raises(ValueError, match="VecAssemblyGym"):
        agent.beam_search(object(), 4)
    with pytest.raises(ValueError, match="VecAssemblyGym"):
        beam_env_like(object(), 4)
