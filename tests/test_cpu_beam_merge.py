"""CPU-only: the rule of bridges_beam_merge in numpy (tests/beam_merge_ref.py) against a second statement of it through Python's
sorted / Counter on tuples, what its probe tables hold, the defective twins each rejected by a probe, the header / abi.py mirror of the
new symbol, and the command line of --eval_beam_merge."""
import collections
import os
import re
import struct

import numpy as np
import pytest

import beam_merge_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def _second_statement(case):
    """The rule once more, on Python tuples: a block is (shape as u32, occupancy, four 8-byte strings), an env's key is
    (nb, targets_left, last block or None, the sorted items of a Counter of its blocks)."""
    B, K, E = case["B"], case["K"], len(case["n_blocks"])

    def block(e, i):
        return (int(case["blk_shape"][e, i]) & 0xFFFFFFFF, int(case["blk_occ"][e, i])) + tuple(
            struct.pack("<d", v) for v in case["blk_pose"][e, i])

    def key(e):
        nb = min(max(int(case["n_blocks"][e]), 0), K)
        blocks = [block(e, i) for i in range(nb)]
        last = blocks[-1] if case["key_last"] and nb else None
        return nb, int(case["targets_left"][e]), last, tuple(sorted(collections.Counter(blocks).items()))

    def order(e):                                                # first: the highest return, a NaN after every number, then the env
        r = float(case["ret"][e])
        return (1, 0.0, e) if r != r else (0, -r, e)
    rep = list(range(E))
    for g in range(E // B):
        classes = collections.defaultdict(list)
        for e in range(g * B, (g + 1) * B):
            if case["live"][e]:
                classes[key(e)].append(e)
        for members in classes.values():
            first = sorted(members, key=order)[0]
            for e in members:
                rep[e] = first
    live = [int(bool(case["live"][e]) and rep[e] == e) for e in range(E)]
    n_merged = [sum(1 for e in range(g * B, (g + 1) * B) if case["live"][e] and rep[e] != e) for g in range(E // B)]
    return dict(rep=np.array(rep, np.int32), live=np.array(live, np.uint8), n_merged=np.array(n_merged, np.int32))


def _random_cases():
    return [MR.random_case(G, B, K, seed=100 * G + 10 * B + K + kl, key_last=kl)
            for G in (1, 5) for B in (1, 2, 8, 16) for K in (1, 6, 64) for kl in (0, 1)]


def test_reference_agrees_with_a_second_statement_of_the_rule():
    cases = list(MR.probe_tables().values()) + _random_cases()
    merged = 0
    for case in cases:
        a, b = MR.reference(case), _second_statement(case)
        assert MR.same(a, b), (case["B"], case["K"], a, b)
        merged += int(a["n_merged"].sum())
    assert merged > 100                                          # the random tables are full of classes, not of singletons


def test_probe_tables_hold_what_the_rule_names():
    t = MR.probe_tables()
    ref = {name: MR.reference(case) for name, case in t.items()}
    r = ref["permuted"]
    assert r["rep"].tolist() == [1, 1] and r["live"].tolist() == [0, 1] and r["n_merged"].tolist() == [1]
    for name in ("one_bit_of_pose",):
        assert ref[name]["rep"].tolist() == [0, 1, 2, 0] and ref[name]["n_merged"].tolist() == [1]      # only the exact copy merges
    for name in ("occupancy", "targets_left", "last_block_key_last_1"):
        assert ref[name]["rep"].tolist() == [0, 1] and ref[name]["live"].tolist() == [1, 1] and ref[name]["n_merged"].tolist() == [0], name
    assert ref["last_block_key_last_0"]["rep"].tolist() == [1, 1]
    assert ref["multiplicity"]["rep"].tolist() == [0, 1, 3, 3]
    assert ref["nb_0"]["rep"].tolist() == [1, 1, 2, 3] and ref["nb_0"]["n_merged"].tolist() == [1]
    assert ref["nb_K"]["rep"].tolist() == [1, 1, 2, 2] and ref["nb_K"]["live"].tolist() == [0, 1, 1, 0]
    r = ref["dead_duplicate"]
    assert r["rep"].tolist() == [0, 1, 0, 3] and r["live"].tolist() == [1, 0, 0, 0] and r["n_merged"].tolist() == [1]
    r = ref["other_group"]
    assert r["rep"].tolist() == [0, 1, 2, 3] and r["n_merged"].tolist() == [0, 0]
    r = ref["three_way"]
    assert r["rep"].tolist() == [2, 4, 2, 2, 4, 5, 6, 6] and r["n_merged"].tolist() == [4]
    assert ref["ret_ties"]["rep"].tolist() == [0, 1, 1, 1]
    assert ref["nan_ret"]["rep"].tolist() == [1, 1, 2, 2]


@pytest.mark.parametrize("twin", MR.TWINS)
def test_every_defective_twin_is_rejected_by_a_probe(twin):
    t = MR.probe_tables()
    rejected = [name for name, case in t.items() if not MR.same(MR.reference(case), MR.reference(case, twin=twin))]
    assert rejected, f"no probe table tells the twin {twin!r} from the rule"


def test_outputs_are_consistent_on_random_cases():
    for case in _random_cases():
        out, B, E = MR.reference(case), case["B"], len(case["n_blocks"])
        for e in range(E):
            r = int(out["rep"][e])
            assert r // B == e // B and out["rep"][r] == r                       # a representative of the same group, of itself
            assert bool(case["live"][e]) or r == e
            assert not case["live"][e] or case["live"][r]                        # a live env is never represented by a dead one
        assert out["n_merged"].sum() == int(case["live"].sum()) - int(out["live"].sum())


# ---- header / abi.py ------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_and_mirrored():
    import ctypes as C
    from bridges_hip import abi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bridges_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bridges_beam_merge\s*\(([^;]*)\)\s*;", text)
    assert m, "bridges_beam_merge is not declared in include/bridges_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = abi.SIGNATURES["bridges_beam_merge"]
    assert len(params) == len(sig) == 15
    for p, ct in zip(params, sig):
        assert (ct is abi.vp) if "*" in p else (p.startswith("int32_t") and ct is abi.i32), p
    assert [p.split()[-1].lstrip("*") for p in params] == ["E", "B", "K", "n_blocks", "blk_shape", "blk_pose", "blk_occ", "targets_left",
                                                           "live", "ret", "key_last", "rep", "live_out", "n_merged", "stream"]
    assert "bridges_beam_merge" in abi.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(abi.LIB_PATH), "bridges_beam_merge")
    assert abi.BEAM_MAX_WIDTH == 16 and abi.BEAM_MAX_SLOTS == 64


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_cli_refuses_merging_without_a_beam_in_words():
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(["--model", "SuccessorMLP", "--num_envs", "64", "--eval_envs", "8", "--eval_beam_merge"])
    assert isinstance(e.value.code, str) and "--eval_beam_merge" in e.value.code and "--eval_beam B" in e.value.code, e.value.code


def test_cli_option_is_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_eval_beam
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--eval_envs", "8", "--eval_beam", "8"]))
    assert "eval_beam_merge" not in plain                            # a parse without the flag keeps the keys it always had
    check_eval_beam(plain)
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--eval_envs", "8", "--eval_beam", "8",
                                           "--eval_beam_merge"]))
    assert args["eval_beam_merge"] is True and args["eval_beam"] == 8
    check_eval_beam(args)
    assert "eval_merged_beams" in build_parser().format_help()


def test_beam_search_takes_merge_and_on_depth():
    import inspect
    from robotoddler.training.vec_dqn import VecDQN
    p = inspect.signature(VecDQN.beam_search).parameters
    assert list(p)[:5] == ["self", "beam_env", "width", "merge", "on_depth"]
    assert p["merge"].default is False and p["on_depth"].default is None
