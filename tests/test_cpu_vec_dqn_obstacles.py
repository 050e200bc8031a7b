"""CPU: the host side of the vectorised DQN on per-env obstacles -- the three new entry points in the header and its ctypes
mirror, the refusals of VecDQN(per_env_obstacles=...) and of --random_obstacles (decided before anything touches the GPU), the
record width, the (T, O) check of a checkpoint and the first-layer table without its obstacle term."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_three_entry_points():
    """bridges_bits_linear2(n, bits_a, bits_row_a, wt_a, bits_b, bits_row_b, wt_b, d, base, base_row, out, stream) and the _task_rows
    forms with the argument lists of the _rows forms (the obstacle as bits); tests/test_cpu_host.py::
    test_library_exports_every_declared_symbol covers the export of everything in abi.SIGNATURES."""
    from bridges_hip import abi
    vp, i32, i64 = abi.vp, abi.i32, abi.i64
    assert abi.SIGNATURES["bridges_bits_linear2"] == [i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    assert abi.SIGNATURES["bridges_mlp_input_task_rows"] == abi.SIGNATURES["bridges_mlp_input_rows"] \
        == [i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    assert abi.SIGNATURES["bridges_mlp_input_batches_task_rows"] == abi.SIGNATURES["bridges_mlp_input_batches_rows"] \
        == [i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    # the entry points they stand beside keep their signatures
    assert abi.SIGNATURES["bridges_bits_linear"] == [i32, vp, vp, vp, i32, vp, vp, vp, vp]
    assert abi.SIGNATURES["bridges_mlp_input"] == [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("bridges_bits_linear2", "bridges_mlp_input_task_rows", "bridges_mlp_input_batches_task_rows"):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M).group(1)
        assert decl.count(",") + 1 == len(abi.SIGNATURES[name]) and name in abi.EXPORTED_SYMBOLS
        assert ("const uint64_t* obstacle_bits" in decl) == name.endswith("task_rows")
    names = [a.split()[-1].lstrip("*") for a in
             re.search(r"^int\s+bridges_bits_linear2\s*\(([^;]*)\);", text, flags=re.M).group(1).split(",")]
    assert names == ["n_rows", "bits_a", "bits_row_a", "wt_a", "bits_b", "bits_row_b", "wt_b", "d", "base", "base_row", "out", "stream"]


def fake_env(per_env_tasks, per_env_obstacles, img=64):
    return types.SimpleNamespace(per_env_tasks=per_env_tasks, per_env_obstacles=per_env_obstacles, img=img, n_targets=3, n_obstacles=2)


def test_vec_dqn_refusals_name_the_condition_that_failed():
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    mlp = SuccessorMLP(img_size=(64, 64), hidden_dims=[8])
    mk = lambda env, **kw: VecDQN(mlp, mlp, None, env, 64, 8, 0.9, 0.05, "mse_q_values", **kw)
    with pytest.raises(ValueError, match="per-env obstacles") as e:
        mk(fake_env(True, True), per_env_tasks=True)                      # the default: still refused ...
    assert "per_env_obstacles=True" in str(e.value)                       # ... and the message names the option
    with pytest.raises(ValueError, match="one shared obstacle list"):
        mk(fake_env(True, False), per_env_tasks=True, per_env_obstacles=True)
    with pytest.raises(ValueError, match="needs per_env_tasks=True"):
        mk(fake_env(True, True), per_env_obstacles=True)
    with pytest.raises(ValueError, match="needs per_env_tasks=True"):
        mk(fake_env(False, False), per_env_tasks=False, per_env_obstacles=True)


CLI = ["--model", "SuccessorMLP", "--num_envs", "64", "--random_targets", "3", "--random_obstacles", "2"]


@pytest.mark.parametrize("argv,word", [(["--model", "SuccessorMLP", "--num_envs", "64", "--random_obstacles", "2"], "--random_targets"),
                                       (CLI[:-1] + ["0"], "--random_obstacles"),
                                       (CLI[:-1] + ["5"], "--random_obstacles"),
                                       (["--model", "ConvNet", *CLI[2:]], "ConvNet")])
def test_cli_refuses_in_words(argv, word):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and word in e.value.code, e.value.code


def test_cli_option_is_opt_in():
    from bridges_hip import abi
    from robotoddler.training.successor_dqn import build_parser, check_random_targets
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64", "--random_targets", "3"]))
    assert "random_obstacles" not in plain
    check_random_targets(plain)
    for O in range(1, abi.MAX_OBSTACLES + 1):
        args = vars(build_parser().parse_args(CLI[:-1] + [str(O)]))
        assert args["random_obstacles"] == O
        check_random_targets(args)


def test_record_width_and_ring(monkeypatch):
    """RECORD_WIDTH + 3 T + 3 O: VecDQN's arithmetic on a host-only stand-in for the env (the scratch env and the pinned counter
    buffer are the two things its constructor needs a GPU for), and a ReplayRing of that width."""
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training import records as R
    from robotoddler.training.vec_dqn import VecDQN
    assert R.RECORD_WIDTH == 111
    monkeypatch.setattr(VecDQN, "_make_replay_env", lambda self, n: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8])
    for T, O in ((3, 2), (1, 4), (8, 1)):
        env = types.SimpleNamespace(per_env_tasks=True, per_env_obstacles=True, img=64, n_targets=T, n_obstacles=O, device="cpu", K=4, E=2,
                                    stable_actions_only=False)
        agent = VecDQN(net, net, torch.optim.Adam(net.parameters(), lr=1e-4), env, 16, 4, 0.9, 0.05, "mse_q_values",
                       per_env_tasks=True, per_env_obstacles=True)
        assert agent.task_width == 3 * T + 3 * O and (agent.n_task_targets, agent.n_task_obstacles) == (T, O)
        assert agent.ring.width == agent.ring.data.shape[1] == 111 + 3 * T + 3 * O
    ring = R.ReplayRing(8, "cpu", width=111 + 9 + 6)
    g = torch.Generator().manual_seed(0)
    rec = torch.rand((5, 126), generator=g, dtype=torch.float64)
    ring.push(rec)
    assert len(ring) == 5 and torch.equal(ring.data[:5], rec) and tuple(ring.sample(7, g).shape) == (7, 126)


def test_load_extra_refuses_another_task_shape(tmp_path):
    """Width 120 is T = 3, O = 0 and T = 1, O = 2 alike: the file carries (T, O)."""
    from robotoddler.training.vec_dqn import VecDQN

    def agent(T, O):
        a = VecDQN.__new__(VecDQN)
        a.n_task_targets, a.n_task_obstacles = T, O
        a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
        a.step_images = torch.zeros((3, 4, 4))
        a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        return a
    path = str(tmp_path / "agent.pt")
    agent(3, 2).save_extra(path, lockstep=5)
    fresh = agent(3, 2)
    fresh.epsilon = 0.0
    assert fresh.load_extra(path) == dict(lockstep=5) and fresh.epsilon == 0.25 and fresh.env_steps == 99
    for T, O in ((3, 0), (2, 3), (4, 1), (1, 4)):                         # (2, 3), (4, 1), (1, 4): the same width as (3, 2)
        with pytest.raises(ValueError, match=f"3 targets and 2 obstacles.*{T} targets and {O} obstacles"):
            agent(T, O).load_extra(path)
    agent(3, 0).save_extra(path, lockstep=1)
    with pytest.raises(ValueError, match="3 targets and 0 obstacles"):
        agent(1, 2).load_extra(path)
    # a file from before the tails held obstacles has no entry: targets only
    blob = torch.load(path, weights_only=True)
    del blob["task_shape"]
    torch.save(blob, path)
    assert agent(3, 0).load_extra(path) == dict(lockstep=1)
    with pytest.raises(ValueError, match="0 obstacles.*2 obstacles"):
        agent(3, 2).load_extra(path)


def test_first_layer_tables_without_the_obstacle_term():
    """first_layer_stable_tables(maps, None) + W_obst @ o == first_layer_stable_tables(maps, o), float64 on a tiny net; with an
    obstacle the result is the statement it always was."""
    from robotoddler.models.cv import SuccessorMLP
    torch.manual_seed(3)
    S = 4
    px = S * S
    net = SuccessorMLP(img_size=(S, S), hidden_dims=[12, 5]).double()
    lin = net.first_layer()
    W, b = lin.weight.detach(), lin.bias.detach()
    E = 7
    maps = torch.rand((E, px), dtype=torch.float64)
    o = (torch.rand(px, dtype=torch.float64) < 0.4).double()
    bare, full = net.first_layer_stable_tables(maps, None), net.first_layer_stable_tables(maps, o)
    assert tuple(bare.shape) == tuple(full.shape) == (E, 2, 12)
    assert torch.allclose(bare + W[:, 3 * px:4 * px] @ o, full, rtol=1e-13, atol=1e-13)
    want0 = maps @ W[:, 2 * px:3 * px].T + b
    assert torch.allclose(bare[:, 0], want0, rtol=1e-13, atol=1e-13)
    assert torch.allclose(bare[:, 1], want0 + W[:, 4 * px], rtol=1e-13, atol=1e-13)
    assert torch.allclose(full[:, 0], want0 + W[:, 3 * px:4 * px] @ o, rtol=1e-13, atol=1e-13)
    assert torch.equal(net.first_layer_stable_tables(maps.reshape(E, S, S), o.reshape(S, S)), full)
