"""CPU: the references of the n-step returns (tests/nstep_ref.py) checked against each other and against their defective twins,
and the host side of VecDQN(n_step=n) -- the refusals of the constructor and the CLI, the ring width, the checkpoint refusal, the
new entry points in the header and its ctypes mirror."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import nstep_ref as N
from mlp_conformance import td_plain, td_probe
from robotoddler.training import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.8


def run_script(E, n, W, seed=0):
    steps = N.scripted_records(E, n, W, seed)
    win = N.RefWindow(E, n, GAMMA)
    return steps, win, [win.fold(rec, valid) for rec, valid in steps]


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_window_emits_every_valid_transition_once_with_the_direct_sum(n):
    """O_TD of a scripted record is a random double: it names the one-step transition an emitted row STARTS at.  Every valid
    transition is emitted exactly once, except the ones still pending at the end; emissions of an env come oldest first with
    h = count - j; G is sum_k gamma^k lin_k over the h transitions from the start on."""
    E, W = 7, R.RECORD_WIDTH + 3
    steps, win, folds = run_script(E, n, W)
    for e in range(E):
        mine = [(rec[e], t) for t, (rec, valid) in enumerate(steps) if valid[e]]         # the env's one-step transitions, in order
        ids = [r[R.O_TD] for r, _ in mine]
        assert len(set(ids)) == len(ids)
        emitted = []
        for t, (out, out_valid, _) in enumerate(folds):
            block = slice(e * n, (e + 1) * n)
            k = int(out_valid[block].sum())
            assert out_valid[block][:k].all()                                          # the emissions lead the env's block
            rows = out[block][:k]
            hs = rows[:, W]
            assert list(hs) == sorted(hs, reverse=True)                                # oldest first: the longest horizon first
            for row in rows:
                start = ids.index(row[R.O_TD])
                h = int(row[W])
                assert mine[start + h - 1][1] == t                                     # the row's last step is this lock-step's
                last = mine[start + h - 1][0]
                direct = math.fsum(GAMMA ** k * mine[start + k][0][R.O_LIN] for k in range(h))
                assert row[R.O_LIN] == direct
                assert row[R.O_STABLE_S] == mine[start][0][R.O_STABLE_S]
                keep = [c for c in range(W) if c not in (R.O_LIN, R.O_STABLE_S, R.O_TD)]
                assert np.array_equal(row[keep], last[keep])
                assert h == n or last[R.O_DONE] > 0.5                                  # a short horizon only at the end of an episode
                emitted.append(start)
        pending = len(win.pending[e])
        assert sorted(emitted) == list(range(len(mine) - pending)) and len(emitted) == len(set(emitted))
        assert pending < n


def test_script_holds_the_cases_it_names():
    for n in (2, 3, 8):
        sc = N.episode_script(n, 0)
        lengths, run, gaps = [], 0, 0
        for valid, done in sc:
            gaps += not valid
            run += valid
            if done:
                lengths.append(run)
                run = 0
        assert lengths[:5] == [1, n, n + 2, 2, 1] and gaps == 2 and len(sc) == N.script_length(n)
        assert sc[1] == (False, False) and sc[2][0] and sc[2 + n][0]                   # a gap, then back-to-back episodes
        assert not N.episode_script(n, 2)[1][0]                                        # env % 3 leading reset-only lock-steps


def test_n_1_is_the_identity_with_h_1():
    E, W = 5, R.RECORD_WIDTH
    steps, _, folds = run_script(E, 1, W)
    for (rec, valid), (out, out_valid, g_bound) in zip(steps, folds):
        assert np.array_equal(out_valid, valid)
        assert np.array_equal(out[valid][:, :W], rec[valid]) and np.all(out[valid][:, W] == 1.0)
        assert np.all(g_bound[~valid] == 0)


def test_a_recursive_float64_fold_passes_the_bound_and_a_wrong_discount_does_not():
    """The kernel's arithmetic in numpy (acc += disc * lin; disc *= gamma) against the direct sum; gamma off by 1e-9 is rejected."""
    E, n, W = 6, 3, R.RECORD_WIDTH
    steps, _, folds = run_script(E, n, W)
    for gamma, ok in ((GAMMA, True), (GAMMA + 1e-9, False)):
        count = np.zeros(E, dtype=int)
        acc, disc, ss, td = (np.zeros((E, n)) for _ in range(4))
        failed = False
        for (rec, valid), (ref_out, ref_valid, g_bound) in zip(steps, folds):
            out, out_valid = np.zeros_like(ref_out), np.zeros_like(ref_valid)
            for e in np.nonzero(valid)[0]:
                c = count[e]
                acc[e, c], disc[e, c], ss[e, c], td[e, c] = 0.0, 1.0, rec[e, R.O_STABLE_S], rec[e, R.O_TD]
                c += 1
                acc[e, :c] += disc[e, :c] * rec[e, R.O_LIN]
                disc[e, :c] *= gamma
                done = rec[e, R.O_DONE] > 0.5
                k = c if done else (1 if c == n else 0)
                for r in range(k):
                    row = rec[e].copy()
                    row[R.O_LIN], row[R.O_STABLE_S], row[R.O_TD] = acc[e, r], ss[e, r], td[e, r]
                    out[e * n + r, :W], out[e * n + r, W] = row, c - r
                    out_valid[e * n + r] = True
                if done:
                    c = 0
                elif k:
                    for a in (acc, disc, ss, td):
                        a[e, :c - 1] = a[e, 1:c].copy()
                    c -= 1
                count[e] = c
            try:
                N.check_fold(out, out_valid, ref_out, ref_valid, g_bound)
            except AssertionError:
                failed = True
        assert failed != ok


def test_raster_sum_plain_passes_and_every_twin_is_rejected():
    bits, cases = N.raster_probe()
    for first, h in cases:
        ref = N.raster_sum_ref(bits, first, h, GAMMA)
        s, d = N.raster_sum_plain(bits, first, h, GAMMA)
        N.check_raster_sum(s, d, ref)
        if (h == 1).all():
            assert np.array_equal(s, N.images(bits)[first].astype(np.float32)) and not ref["sum_bound"].any()
        for twin in N.RASTER_TWINS:
            if twin == "undiscounted" and (h == 1).all():
                continue                                                               # h = 1 has nothing to discount
            with pytest.raises(AssertionError):
                N.check_raster_sum(*N.raster_sum_plain(bits, first, h, GAMMA, twin=twin), ref)


def test_raster_probe_holds_the_cases_it_names():
    bits, cases = N.raster_probe()
    img = N.images(bits)
    assert img[1].sum() == 0 and img[0].sum() == 1 and img[0][5, 0] == 1 and img[2][40, 63] == 1
    assert img[-1][0, 0] == 1 and img[-2][63, 63] == 1 and img[-1].sum() == img[-2].sum() == 1
    assert sorted({int(h[0]) for _, h in cases[:4]}) == [1, 2, 3, 8]
    assert all(int((first + h).max()) == bits.shape[0] for first, h in cases)          # up to the last row of the table
    assert all(int(first.min()) == 0 for first, _ in cases)


@pytest.mark.parametrize("sf_dim", [0, 4, 4096])
def test_td_rows_reference_accepts_plain_float32_and_agrees_with_the_scalar_operator(sf_dim):
    pr = td_probe(sf_dim, "cpu")
    B = len(pr["lo"])
    same = torch.full((B,), GAMMA, dtype=torch.float32)
    ref, rows = N.td_rows_ref(pr, same)
    N.check_td_rows(td_plain(pr, float(same[0])), ref, rows)                           # the scalar operator is the constant case
    disc = N.row_discounts(B, GAMMA)
    assert len(set(disc.tolist())) > 2
    ref, rows = N.td_rows_ref(pr, disc)
    N.check_td_rows(N.td_rows_plain(pr, disc), ref, rows)
    with pytest.raises(AssertionError):
        N.check_td_rows(N.td_rows_plain(pr, disc, twin="scalar_gamma"), ref, rows)


# ---------------------------------------------------------------------------------------------------------------------------
# host side

NEW_SYMBOLS = ("bridges_nstep_fold", "bridges_bits_discounted_sum", "bridges_td_target_rows")


def test_new_entry_points_are_declared_and_mirrored():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        raw = fh.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    n_args = lambda name: re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M).group(1).count(",") + 1
    for name in NEW_SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS and n_args(name) == len(abi.SIGNATURES[name])
    assert len(abi.SIGNATURES["bridges_td_target_rows"]) == len(abi.SIGNATURES["bridges_td_target"])
    assert re.search(r"#define\s+BRIDGES_NSTEP_MAX\s+8\b", raw) and abi.NSTEP_MAX == N.NSTEP_MAX == 8


def stand_in_env(**kw):
    base = dict(per_env_tasks=False, per_env_obstacles=False, img=64, n_targets=1, n_obstacles=0, device="cpu", K=4, E=2,
                stable_actions_only=False, max_steps=4)
    base.update(kw)
    return types.SimpleNamespace(**base)


def host_agent(monkeypatch, env, **kw):
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "_make_replay_env", lambda self, n: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8])
    return VecDQN(net, net, torch.optim.Adam(net.parameters(), lr=1e-4), env, 16, 4, 0.9, 0.05, "mse_q_values", **kw)


def test_ring_width_and_constructor_refusals(monkeypatch):
    assert host_agent(monkeypatch, stand_in_env()).ring.width == R.RECORD_WIDTH                      # n_step = 1: no extra column
    assert host_agent(monkeypatch, stand_in_env(), n_step=1).ring.width == R.RECORD_WIDTH
    a = host_agent(monkeypatch, stand_in_env(), n_step=3)
    assert a.n_step == 3 and a.ring.width == a.ring.data.shape[1] == R.RECORD_WIDTH + 1 and a._counts_host.numel() == 3
    env = stand_in_env(per_env_tasks=True, per_env_obstacles=True, n_targets=2, n_obstacles=1)
    a = host_agent(monkeypatch, env, n_step=2, per_env_tasks=True, per_env_obstacles=True)
    assert a.ring.width == R.RECORD_WIDTH + 9 + 1
    a.reset_window()                                                                               # no window yet: a no-op
    for bad in (0, -1, 9):
        with pytest.raises(ValueError, match="n_step"):
            host_agent(monkeypatch, stand_in_env(), n_step=bad)
    with pytest.raises(ValueError, match="max_steps = 4"):
        host_agent(monkeypatch, stand_in_env(), n_step=5)
    assert host_agent(monkeypatch, stand_in_env(), n_step=4).n_step == 4


def test_load_extra_refuses_another_n_step(tmp_path):
    from robotoddler.training.vec_dqn import VecDQN

    def agent(n_step):
        a = VecDQN.__new__(VecDQN)
        a.n_task_targets, a.n_task_obstacles = 0, 0
        a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
        a.step_images = torch.zeros((3, 4, 4))
        a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        if n_step is not None:
            a.n_step = n_step
        return a
    path = str(tmp_path / "agent.pt")
    agent(3).save_extra(path, lockstep=5)
    assert agent(3).load_extra(path) == dict(lockstep=5)
    for other in (1, 2, 8):
        with pytest.raises(ValueError, match=f"n_step = 3.*n_step = {other}"):
            agent(other).load_extra(path)
    # a file from before the loop had n-step returns has no entry: one-step records
    blob = torch.load(path, weights_only=True)
    del blob["n_step"]
    torch.save(blob, path)
    assert agent(1).load_extra(path) == dict(lockstep=5)
    with pytest.raises(ValueError, match="n_step = 1.*n_step = 3"):
        agent(3).load_extra(path)


@pytest.mark.parametrize("argv,word", [(["--model", "SuccessorMLP", "--n_step", "3"], "--num_envs"),
                                       (["--model", "SuccessorMLP", "--num_envs", "1", "--n_step", "2"], "--num_envs"),
                                       (["--model", "SuccessorMLP", "--num_envs", "64", "--n_step", "0"], "1..8"),
                                       (["--model", "SuccessorMLP", "--num_envs", "64", "--n_step", "9"], "1..8"),
                                       (["--model", "SuccessorMLP", "--num_envs", "64", "--max_steps", "4", "--n_step", "5"], "--max_steps")])
def test_cli_refuses_in_words(argv, word):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and "--n_step" in e.value.code and word in e.value.code, e.value.code


def test_cli_option_is_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_n_step
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64"]))
    assert "n_step" not in plain                                          # a plain parse keeps the keys it always had
    check_n_step(plain)
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--n_step", "3"]))
    assert args["n_step"] == 3
    check_n_step(args)
    check_n_step(vars(build_parser().parse_args(["--n_step", "1"])))      # n = 1 is the one-step loop: the single-env loop runs it
    assert "h-step" in build_parser().format_help() and "mean_lin_reward" in build_parser().format_help()


def test_all_gather_rows_without_a_process_group_is_the_identity():
    from robotoddler.training import distributed as D
    rec, valid = torch.rand((5, 4), dtype=torch.float64), torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool)
    out, v = D.all_gather_rows(rec, valid)
    assert out is rec and v is valid
