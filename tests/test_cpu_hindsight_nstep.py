"""CPU: the rule of hindsight relabelling under n-step returns (tests/hindsight_nstep_ref.py) -- the probes of the GPU test hold
every case of it, n = 1 is the one-step relabelling with a column of ones, a walk that ends done is what the n-step window of
tests/nstep_ref.py makes of its rows, every defective twin is told apart -- and what VecDQN(hindsight_fold=...) /
--hindsight_fold accept, refuse, allocate and checkpoint without a GPU."""
import functools
import types

import numpy as np
import pytest
import torch

import hindsight_nstep_ref as HN
import hindsight_ref as H
import nstep_ref as N
from robotoddler.training import records as R

SEED, BASE, CONFIGS = H.PROBE_SEED, H.PROBE_BASE, H.PROBE_CONFIGS
NS, GAMMA = (1, 2, 3, 8), 0.95
BIG = (64, 3, 4, 0, "trapezoid")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def case(E, T, G, O, shape):
    """The probe and its relabelled walks, computed once and shared (never written)."""
    p = H.probe(E, T, O, shape, seed=H.probe_seed(E))
    ws = HN.walks(p["buf"], p["flags"], p["length"], p["ended"], p["episode"], p["shapes"], SEED, BASE, G, T)
    for _e, _g, rows in ws:
        rows.setflags(write=False)
    return p, ws


def test_the_probes_hold_every_case():
    union = set()
    for cfg in CONFIGS:
        p, ws = case(*cfg)
        for n in NS:
            seen = HN.census(ws, n, p["K"])
            print(cfg, n, sorted(seen), "walks", len(ws), "open", sum(1 for w in ws if not w[2][-1, R.O_DONE] > 0.5))
            union |= seen
    assert union == set(HN.CASES)
    p, ws = case(*BIG)
    assert HN.census(ws, 3, p["K"]) == set(HN.CASES)
    # an open-ended walk longer than the window: asserted for n = 2 and 3 only -- no probe holds a walk of 9 or more steps that
    # ends open (an episode that long ends truncated or collapsed, both done), so at n = 8 an open end is always a short walk
    for n in (2, 3):
        assert "open_long" in set().union(*(HN.census(case(*cfg)[1], n, 16) for cfg in CONFIGS)), n
    lengths = {len(rows) for cfg in CONFIGS if cfg[0] >= 64 for _e, _g, rows in case(*cfg)[1]}
    assert lengths == set(range(1, 17))


@pytest.mark.parametrize("cfg", CONFIGS)
def test_one_step_is_the_relabelling_with_a_column_of_ones(cfg):
    E, T, G, O, shape = cfg
    p, ws = case(*cfg)
    one = H.relabel(p["buf"], p["flags"], p["length"], p["ended"], p["episode"], p["shapes"], SEED, BASE, G, T)
    got = HN.fold_walks(ws, p["buf"], 1, GAMMA)
    assert np.array_equal(bits(got), bits(np.concatenate([one, np.ones((len(one), 1))], axis=1)))
    for n in NS:                                                  # every walk step starts exactly one row
        assert len(HN.fold_walks(ws, p["buf"], n, GAMMA)) == len(one)


@pytest.mark.parametrize("n", NS)
def test_a_walk_that_ends_done_is_the_window_of_the_nstep_reference(n):
    """Fed step by step through nstep_ref.RefWindow.fold, a walk whose last row -- and no other -- has O_DONE gives the rows of
    fold_walk: every column but the return bit for bit, h included, and the return within the bound that reference states for
    its own sum (it adds the terms with math.fsum, not in the kernel's order: check_fold's comparison); a row of h = 1 and a
    row of one term hold lin itself."""
    checked = 0
    for cfg in CONFIGS:
        for _e, _g, rows in case(*cfg)[1]:
            if not rows[-1, R.O_DONE] > 0.5 or np.any(rows[:-1, R.O_DONE] > 0.5):
                continue
            win = N.RefWindow(1, n, GAMMA)
            got, bound = [], []
            for r in rows:
                out, valid, g_bound = win.fold(r[None, :], np.array([True]))
                got += [out[valid]]
                bound += [g_bound[valid]]
            got, bound = np.concatenate(got), np.concatenate(bound)
            want = HN.fold_walk(rows, n, GAMMA)
            N.check_fold(want, np.ones(len(want), dtype=bool), got, np.ones(len(got), dtype=bool), bound, name=str(cfg))
            h1 = want[:, -1] == 1.0
            assert np.array_equal(bits(want[h1, R.O_LIN]), bits(got[h1, R.O_LIN]))
            checked += len(want)
    assert checked >= 100


@pytest.mark.parametrize("twin", HN.TWINS)
def test_every_twin_is_rejected(twin):
    rejected = []
    for cfg in CONFIGS:
        p, ws = case(*cfg)
        for n in NS:
            ref, bad = HN.fold_walks(ws, p["buf"], n, GAMMA), HN.fold_walks(ws, p["buf"], n, GAMMA, twin=twin)
            if ref.shape != bad.shape or not np.array_equal(bits(ref), bits(bad)):
                rejected.append((cfg, n))
    print(twin, len(rejected), "of", len(CONFIGS) * len(NS))
    assert rejected
    assert (BIG, 3) in rejected


# ------------------------------------------------------------------------------------------------------------------------ VecDQN
def stand_in_env(**kw):
    base = dict(per_env_tasks=True, per_env_obstacles=False, img=64, n_targets=3, n_obstacles=0, device="cpu", K=4, E=2,
                stable_actions_only=False, max_steps=4)
    base.update(kw)
    return types.SimpleNamespace(**base)


def host_agent(monkeypatch, env, **kw):
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "_make_replay_env", lambda self, n: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8])
    return VecDQN(net, net, torch.optim.Adam(net.parameters(), lr=1e-4), env, 16, 4, 0.9, 0.05, "mse_block_features", **kw)


def test_the_option_is_refused_and_accepted_in_words(monkeypatch):
    from robotoddler.training import distributed as D
    with pytest.raises(ValueError, match="hindsight_fold=True"):                                  # both ways out are named
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", n_step=2)
    with pytest.raises(ValueError, match="n_step=1"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", n_step=2)
    with pytest.raises(ValueError, match="hindsight='final'"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight_fold=True, n_step=2)
    with pytest.raises(ValueError, match="hindsight='final'"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight_fold=True)
    a = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", hindsight_fold=True, n_step=3, hindsight_goals=2)
    assert a.hindsight_fold and a._count_names == ("valid", "done", "emitted", "hindsight")
    # the ring holds h-step rows, the buffer one-step records one column narrower, the operator's output the ring's rows
    W1 = R.RECORD_WIDTH + 9
    hb = a.hindsight_buffer
    assert a.ring.width == W1 + 1 and hb.width == W1 and (hb.n_step, hb.gamma) == (3, 0.9)
    assert tuple(hb.rows.shape) == (2, 4, W1) and tuple(hb.out.shape) == (2 * 4 * 2, W1 + 1) and tuple(hb.flags.shape) == (2, 4, 8)
    # n_step = 1: the one-step loop -- the old entry, the ring's width unchanged
    b = host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", hindsight_fold=True)
    hb = b.hindsight_buffer
    assert b.ring.width == W1 and tuple(hb.rows.shape) == (2, 4, W1) and tuple(hb.out.shape) == (2 * 4, W1)
    assert (hb.n_step, hb.gamma, hb.fold) == (1, None, False) and b._count_names == ("valid", "done", "hindsight")
    with pytest.raises(ValueError, match="n_step"):                                               # BRIDGES_NSTEP_MAX stays the limit
        host_agent(monkeypatch, stand_in_env(max_steps=16), per_env_tasks=True, hindsight="final", hindsight_fold=True, n_step=9)
    monkeypatch.setattr(D, "active", lambda: True)
    with pytest.raises(ValueError, match="one rank"):
        host_agent(monkeypatch, stand_in_env(), per_env_tasks=True, hindsight="final", hindsight_fold=True, n_step=2)


def test_buffer_shapes_under_n_step():
    hb = R.HindsightBuffer(3, R.RECORD_WIDTH + 3 + 1, "cpu", goals=2, n_blocks=4, n_step=3, gamma=0.95)
    assert hb.fold and hb.width == R.RECORD_WIDTH + 3 and tuple(hb.rows.shape) == (3, 4, hb.width)
    assert tuple(hb.out.shape) == (3 * 4 * 2, hb.width + 1)
    rec = torch.arange(3 * hb.width, dtype=torch.float64).reshape(3, hb.width)                    # write takes one-step records
    hb.write(rec, torch.zeros((3, 8), dtype=torch.uint8), torch.tensor([True, False, True]), torch.tensor([4, 5, 6], dtype=torch.int32))
    assert hb.length.tolist() == [1, 0, 1] and torch.equal(hb.rows[2, 0], rec[2])
    assert set(hb.state_dict()) == {"rows", "flags", "length", "episode"}
    hb.clear()
    assert int(hb.length.sum()) == 0
    plain = R.HindsightBuffer(3, R.RECORD_WIDTH + 3, "cpu", goals=2, n_blocks=4)
    assert not plain.fold and plain.width == R.RECORD_WIDTH + 3 and tuple(plain.out.shape) == (24, R.RECORD_WIDTH + 3)


def test_checkpoint_entries_both_ways(monkeypatch, tmp_path):
    kw = dict(per_env_tasks=True, hindsight="final")
    plain = host_agent(monkeypatch, stand_in_env(), **kw)
    fold1 = host_agent(monkeypatch, stand_in_env(), hindsight_fold=True, **kw)
    fold3 = host_agent(monkeypatch, stand_in_env(), hindsight_fold=True, n_step=3, **kw)
    p0, p1, p3 = (str(tmp_path / f"{name}.pt") for name in ("plain", "fold1", "fold3"))
    plain.save_extra(p0, lockstep=1)
    fold1.save_extra(p1, lockstep=2)
    fold3.hindsight_buffer.rows.normal_()
    fold3.hindsight_buffer.length[:] = torch.tensor([2, 1], dtype=torch.int32)
    fold3.save_extra(p3, lockstep=3)
    b0, b1, b3 = (torch.load(p, weights_only=True) for p in (p0, p1, p3))
    assert "hindsight_fold" not in b0 and tuple(b0["hindsight"]) == ("final", 1)                   # a run without the option: its file
    assert set(b1) - set(b0) == {"hindsight_fold"} and b1["hindsight_fold"] is True                # with it: one entry more
    assert b3["hindsight_fold"] is True and int(b3["n_step"]) == 3
    for agent, path in ((plain, p1), (fold1, p0)):
        with pytest.raises(ValueError, match="hindsight"):
            agent.load_extra(path)
    with pytest.raises(ValueError, match="n_step"):                                               # the n-step entry of the file
        fold1.load_extra(p3)
    again = host_agent(monkeypatch, stand_in_env(), hindsight_fold=True, n_step=3, **kw)
    assert again.load_extra(p3) == dict(lockstep=3)
    for name in ("rows", "flags", "length", "episode"):
        assert torch.equal(getattr(again.hindsight_buffer, name), getattr(fold3.hindsight_buffer, name))
    assert plain.load_extra(p0) == dict(lockstep=1) and fold1.load_extra(p1) == dict(lockstep=2)
    fold3.reset_window()
    assert int(fold3.hindsight_buffer.length.sum()) == 0


def test_command_line():
    from robotoddler.training import successor_dqn as S
    parse = lambda *argv: vars(S.build_parser().parse_args(list(argv)))
    assert "hindsight_fold" not in parse()                                                        # SUPPRESS: a plain parse is as it was
    ok = parse("--num_envs", "8", "--random_targets", "3", "--hindsight", "final")
    assert S.hindsight_from_args(ok) == dict(hindsight="final", hindsight_goals=1)                 # ... and so is one without the flag
    fold = parse("--num_envs", "8", "--random_targets", "3", "--hindsight", "final", "--hindsight_fold", "--n_step", "3")
    assert fold["hindsight_fold"] is True and fold["n_step"] == 3
    assert S.hindsight_from_args(fold) == dict(hindsight="final", hindsight_goals=1, hindsight_fold=True)
    assert S.hindsight_from_args(dict(ok, hindsight_fold=True)) == dict(hindsight="final", hindsight_goals=1, hindsight_fold=True)
    for words in ("--n_step 1", "--hindsight_fold"):                                               # both ways out are named
        with pytest.raises(SystemExit, match=words):
            S.check_hindsight(dict(ok, n_step=2))
    with pytest.raises(SystemExit, match="--hindsight final"):
        S.check_hindsight(parse("--hindsight_fold"))
    with pytest.raises(SystemExit, match="--random_targets"):
        S.check_hindsight(parse("--num_envs", "8", "--hindsight", "final", "--hindsight_fold", "--n_step", "3"))


def test_entry_point_is_declared_with_its_rule():
    import os
    from bridges_hip import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bridges_hip.h")).read()
    assert "int bridges_hindsight_relabel_nstep(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G," in header
    assert "whether or not r_{L-1} has DONE" in header
    assert "bridges_hindsight_relabel_nstep" in abi.EXPORTED_SYMBOLS
    assert len(abi.SIGNATURES["bridges_hindsight_relabel_nstep"]) == len(abi.SIGNATURES["bridges_hindsight_relabel"]) + 2
