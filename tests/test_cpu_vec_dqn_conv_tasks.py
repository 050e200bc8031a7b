"""CPU: the host side of the conv Q-networks on per-env tasks -- bridges_conv_input_rows in the header and its ctypes mirror, the
refusals of VecDQN(task_channels=...) and of --task_channels (decided before anything touches the GPU), dqn_ops.stack_channels,
the task words in the key of VecDQN._distinct_rows, the record width."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARG_NAMES = ["n_rows", "block_bits", "block_row", "action_bits", "action_row", "reward", "reward_row", "reward_stride",
             "obstacle_bits", "obstacle_row", "obstacle_stride", "x", "stream"]


def test_abi_declares_the_entry_point():
    from bridges_hip import abi
    vp, i32, i64 = abi.vp, abi.i32, abi.i64
    assert abi.SIGNATURES["bridges_conv_input_rows"] == [i32, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp]
    assert "bridges_conv_input_rows" in abi.EXPORTED_SYMBOLS
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    decl = re.search(r"^int\s+bridges_conv_input_rows\s*\(([^;]*)\);", text, flags=re.M).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ARG_NAMES
    # the entry points it stands beside keep their signatures
    assert abi.SIGNATURES["bridges_bits_to_f32"] == [i32, vp, vp, vp]
    assert abi.SIGNATURES["bridges_bits_linear2"] == [i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]


def test_argument_checks_need_no_device():
    """A refused call returns the error code from the host, before anything could be launched (the pointers are never read)."""
    import ctypes as C
    from bridges_hip import abi
    fn, p, nul = abi.lib().bridges_conv_input_rows, C.c_void_p(4096), None
    call = lambda n=4, bb=p, rw=p, rs=4096, ob=p, os_=64, x=p: fn(n, bb, nul, p, nul, rw, nul, rs, ob, nul, os_, x, nul)
    for bad in (dict(rs=1), dict(rs=4095), dict(rs=128), dict(os_=1), dict(os_=4096), dict(n=-1), dict(bb=nul), dict(rw=nul), dict(ob=nul),
                dict(x=nul), dict(rw=C.c_void_p(4100)), dict(x=C.c_void_p(4104))):
        assert call(**bad) == -1, bad
        assert b"bad argument" in abi.lib().bridges_last_error()
    assert call(n=0) == 0 and call(n=0, rs=0, os_=0) == 0                 # nothing to do: success, nothing launched


def fake_env(per_env_tasks=True, per_env_obstacles=False, img=64):
    return types.SimpleNamespace(per_env_tasks=per_env_tasks, per_env_obstacles=per_env_obstacles, img=img, n_targets=3, n_obstacles=2)


def test_vec_dqn_refusals_name_the_condition_that_failed():
    """Every refusal of task_channels=True is decided from the arguments alone, before VecDQN allocates anything."""
    from robotoddler.models.cv import ConvNet, Policy, SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    conv = ConvNet(img_size=(64, 64))
    mk = lambda pol, env, **kw: VecDQN(pol, pol, None, env, 64, 8, 0.9, 0.05, "mse_q_values", **kw)
    with pytest.raises(ValueError, match="needs per_env_tasks=True"):
        mk(conv, fake_env(), task_channels=True)
    with pytest.raises(ValueError, match="needs per_env_tasks=True"):
        mk(conv, fake_env(False), task_channels=True)
    with pytest.raises(ValueError, match="fixed task"):
        mk(conv, fake_env(False), per_env_tasks=True, task_channels=True)
    with pytest.raises(ValueError, match="SuccessorMLP"):
        mk(SuccessorMLP(img_size=(64, 64), hidden_dims=[8]), fake_env(), per_env_tasks=True, task_channels=True)
    with pytest.raises(ValueError, match=r"target net is a SuccessorMLP"):
        VecDQN(conv, SuccessorMLP(img_size=(64, 64), hidden_dims=[8]), None, fake_env(), 64, 8, 0.9, 0.05, "mse_q_values",
               per_env_tasks=True, task_channels=True)
    with pytest.raises(ValueError, match=r"ConvNet\(in_channels=4, img_size=\(64, 64\)\)"):
        mk(ConvNet(img_size=(32, 32)), fake_env(), per_env_tasks=True, task_channels=True)        # a ConvNet of another size
    with pytest.raises(ValueError, match=r"ConvNet\(in_channels=4, img_size=\(64, 64\)\)"):
        mk(ConvNet(in_channels=2, img_size=(64, 64)), fake_env(), per_env_tasks=True, task_channels=True)
    with pytest.raises(ValueError, match="64x64.*32x32"):
        mk(Policy(), fake_env(img=32), per_env_tasks=True, task_channels=True)
    # per-env obstacles combine with it as they always did
    with pytest.raises(ValueError, match="one shared obstacle list"):
        mk(conv, fake_env(True, False), per_env_tasks=True, per_env_obstacles=True, task_channels=True)
    with pytest.raises(ValueError, match="per_env_obstacles=True"):
        mk(conv, fake_env(True, True), per_env_tasks=True, task_channels=True)
    # without the option the conv nets stay refused, and the message names the option
    for net, name in ((conv, "ConvNet"), (Policy(), "Policy")):
        with pytest.raises(ValueError, match=name) as e:
            mk(net, fake_env(), per_env_tasks=True)
        assert "task_channels=True" in str(e.value)


def test_train_step_refuses_per_transition_maps_for_other_autograd_bodies():
    """task_rows=True with fused=False is legal for the conv nets at 64x64 alone."""
    from robotoddler.models.cv import ConvNet, Policy, SuccessorMLP
    from robotoddler.training import train_step as T
    parts = ("mse_q_values",)
    bits = torch.zeros(64, dtype=torch.int64)
    for net in (None, SuccessorMLP(img_size=(64, 64), hidden_dims=[8]), ConvNet(img_size=(32, 32)), ConvNet(in_channels=2, img_size=(64, 64))):
        with pytest.raises(ValueError, match="per-transition"):
            T.CapturedTrainStep(net, None, 8, parts, (64, 64), False, task=(None, bits), task_rows=True)
    with pytest.raises(ValueError, match="per-transition"):
        T.CapturedTrainStep(Policy(), None, 8, parts, (32, 32), False, task=(None, bits), task_rows=True)
    with pytest.raises(ValueError, match="per-transition"):
        T.CapturedTrainStep(Policy(), None, 8, parts, (64, 64), False, task=(torch.zeros(4096), bits), task_rows=True)
    with pytest.raises(ValueError, match="obstacle_rows=True"):
        T.CapturedTrainStep(Policy(), None, 8, parts, (64, 64), False, task=(None, None), task_rows=True)
    for net in (ConvNet(img_size=(64, 64)), Policy()):
        assert T.CapturedTrainStep(net, None, 8, parts, (64, 64), False, task=(None, bits), task_rows=True).conv_rows
        assert T.CapturedTrainStep(net, None, 8, parts, (64, 64), False, task=(None, None), task_rows=True, obstacle_rows=True).conv_rows
        assert not T.CapturedTrainStep(net, None, 8, parts, (64, 64), False, task=(torch.zeros(4096), torch.zeros(4096))).conv_rows


CLI = ["--num_envs", "64", "--random_targets", "3", "--task_channels"]


@pytest.mark.parametrize("argv,word", [(["--model", "ConvNet", "--num_envs", "64", "--task_channels"], "--random_targets"),
                                       (["--num_envs", "64", "--task_channels"], "--random_targets"),
                                       (["--model", "SuccessorMLP", *CLI], "SuccessorMLP"),
                                       (["--model", "ConvNet", *CLI, "--image_size", "32x32"], "64x64"),
                                       ([*CLI, "--image_size", "32x32"], "64x64"),
                                       (["--model", "ConvNet", "--random_targets", "3", "--task_channels"], "--num_envs"),
                                       (["--model", "ConvNet", "--num_envs", "1", "--random_targets", "3", "--task_channels"], "--num_envs"),
                                       # without the flag every refusal stands and names it
                                       (["--model", "ConvNet", "--num_envs", "64", "--random_targets", "3"], "--task_channels"),
                                       (["--num_envs", "64", "--random_targets", "3", "--random_obstacles", "2"], "--task_channels")])
def test_cli_refuses_in_words(argv, word):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and word in e.value.code, e.value.code


def test_cli_option_is_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_random_targets
    plain = vars(build_parser().parse_args(["--model", "ConvNet", "--num_envs", "64"]))
    assert "task_channels" not in plain                                   # a plain parse keeps the keys it always had
    check_random_targets(plain)
    for argv in (["--model", "ConvNet", *CLI], CLI, ["--model", "UNet", *CLI, "--random_obstacles", "2"],
                 ["--model", "ConvNet", *CLI, "--random_obstacles", "1"]):
        args = vars(build_parser().parse_args(argv))
        assert args["task_channels"] is True and args["random_targets"] == 3
        check_random_targets(args)


def views(x):
    return x[:, 0:1], x[:, 1:2], x[:, 2:3], x[:, 3:4]


def test_stack_channels_returns_the_base_of_consecutive_views():
    from bridges_hip.dqn_ops import stack_channels
    g = torch.Generator().manual_seed(0)
    x = torch.rand((5, 4, 6, 8), generator=g)
    got = stack_channels(*views(x))
    assert got.data_ptr() == x.data_ptr() and tuple(got.shape) == (5, 4, 6, 8) and got.is_contiguous() and torch.equal(got, x)
    big = torch.rand((9, 4, 6, 8), generator=g)
    mid = big[2:7]                                                        # a slice of rows: still one contiguous [n, 4, H, W]
    got = stack_channels(*views(mid))
    assert got.data_ptr() == mid.data_ptr() and tuple(got.shape) == (5, 4, 6, 8) and torch.equal(got, mid)


def test_stack_channels_concatenates_everything_else():
    from bridges_hip.dqn_ops import stack_channels
    g = torch.Generator().manual_seed(1)
    x, y = torch.rand((5, 4, 6, 8), generator=g), torch.rand((5, 4, 6, 8), generator=g)
    b, a, r, o = views(x)
    wide = torch.rand((5, 8, 6, 8), generator=g)
    strided = torch.rand((5, 4, 6, 16), generator=g)[..., ::2]            # a non-contiguous base
    moved = torch.rand((4, 5, 6, 8), generator=g).transpose(0, 1)         # another one
    cases = dict(order=(a, b, r, o), gap=(b, a, o, o), two_tensors=(b, a, y[:, 2:3], o), other_tensor_same_offsets=(b, a, r, y[:, 3:4]),
                 wider_base=views(wide), strided_base=views(strided), transposed_base=views(moved),
                 separate=tuple(t.clone() for t in (b, a, r, o)))
    ptrs = {t.data_ptr() for t in (x, y, wide, strided, moved)}
    for name, args in cases.items():
        got = stack_channels(*args)
        assert torch.equal(got, torch.cat(args, dim=1)), name
        assert tuple(got.shape) == (5, 4, 6, 8) and got.is_contiguous() and got.data_ptr() not in ptrs, name


def test_conv_nets_compute_the_same_from_views_and_from_separate_tensors():
    from robotoddler.models.cv import ConvNet, UNet
    torch.manual_seed(2)
    n, S = 3, 16
    x = torch.rand((n, 4, S, S), dtype=torch.float64)
    binary = torch.rand((n, 6), dtype=torch.float64)
    sep = [t.clone() for t in views(x)]
    with torch.no_grad():
        for net in (ConvNet(img_size=(S, S)).double(), UNet(1).double()):
            a = net(x[:, 0:1], binary, x[:, 1:2], x[:, 2:3], x[:, 3:4])
            b = net(sep[0], binary, sep[1], sep[2], sep[3])
            for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert (u is None and v is None) or torch.equal(u, v)


def stand_in(targets=None, obstacles=None):
    """Four envs in two states; envs 0 and 2 hold the same state and candidate rasters, 1 and 3 another."""
    g = torch.Generator().manual_seed(3)
    state = torch.randint(-2 ** 62, 2 ** 62, (2, 64), generator=g, dtype=torch.int64)[[0, 1, 0, 1]]
    cand = torch.randint(-2 ** 62, 2 ** 62, (2, 3, 64), generator=g, dtype=torch.int64)[[0, 1, 0, 1]].reshape(12, 64)
    env = types.SimpleNamespace(state_bits=state, cand_bits=cand, per_env_tasks=targets is not None,
                                per_env_obstacles=obstacles is not None)
    if targets is not None:
        env.env_targets = targets
    if obstacles is not None:
        env.env_obstacles = obstacles
    return env


def groups_of(env):
    from robotoddler.training.vec_dqn import VecDQN
    agent = VecDQN.__new__(VecDQN)
    agent.device = torch.device("cpu")
    idx, row_env = torch.arange(12), torch.arange(4).repeat_interleave(3)
    out = agent._distinct_rows(env, idx, row_env, torch.ones(4, dtype=torch.bool))
    return None if out is None else (out[0].tolist(), out[1].tolist())


def test_distinct_rows_key_on_the_task_words():
    same = ([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5])     # env 2 shares env 0's rows, env 3 env 1's
    assert groups_of(stand_in()) is not None
    rep, inv = groups_of(stand_in())
    assert sorted(rep) == same[0] and [rep[g] for g in inv] == same[1]      # without per-env tasks: grouped as ever
    t = torch.tensor([[[0.5, 0.0, 1.2]], [[0.5, 0.0, 1.2]], [[0.5, 0.0, 1.2]], [[0.5, 0.0, 1.2]]], dtype=torch.float64)
    o = torch.tensor([[[1.0, 0.0, 0.3]]] * 4, dtype=torch.float64)
    rep, inv = groups_of(stand_in(t))
    assert [rep[g] for g in inv] == same[1]                                # one task over all envs: grouped
    rep, inv = groups_of(stand_in(t, o))
    assert [rep[g] for g in inv] == same[1]
    t2 = t.clone()
    t2[2, 0, 2] = torch.nextafter(t[2, 0, 2], torch.tensor(2.0, dtype=torch.float64))     # one bit of one target of env 2
    rep, inv = groups_of(stand_in(t2))
    assert [rep[g] for g in inv] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 3, 4, 5]    # env 2 keeps rows of its own, env 3 still shares
    o2 = o.clone()
    o2[3, 0, 0] = -1.0
    rep, inv = groups_of(stand_in(t, o2))
    assert [rep[g] for g in inv] == [0, 1, 2, 3, 4, 5, 0, 1, 2, 9, 10, 11]  # equal targets, another obstacle: not grouped
    t3, o3 = t.clone(), o.clone()
    t3[0, 0, 0], o3[1, 0, 2] = -0.0, 0.31
    assert groups_of(stand_in(t3, o3)) is None                             # nothing left to share
    z = t.clone()
    z[:, 0, 1], z2 = 0.0, t.clone()
    z2[:, 0, 1] = 0.0
    z2[2, 0, 1] = -0.0                                                     # the words are bit patterns: -0.0 is another task
    rep, inv = groups_of(stand_in(z2))
    assert [rep[g] for g in inv] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 3, 4, 5]


def test_record_width_and_ring(monkeypatch):
    """RECORD_WIDTH + 3 T + 3 O in the new mode: VecDQN's arithmetic on a host-only stand-in for the env (the scratch env and the
    pinned counter buffer are the two things its constructor needs a GPU for), and no f32 rasters in the scratch env."""
    from robotoddler.models.cv import ConvNet, Policy
    from robotoddler.training import records as R
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setattr(VecDQN, "_make_replay_env", lambda self, n: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    for net in (ConvNet(img_size=(64, 64)), Policy()):
        for T, O in ((3, 0), (3, 2), (1, 4)):
            env = types.SimpleNamespace(per_env_tasks=True, per_env_obstacles=O > 0, img=64, n_targets=T, n_obstacles=O, device="cpu",
                                        K=4, E=2, stable_actions_only=False)
            agent = VecDQN(net, net, torch.optim.Adam(net.parameters(), lr=1e-4), env, 16, 4, 0.9, 0.05, "mse_q_values",
                           per_env_tasks=True, per_env_obstacles=O > 0, task_channels=True)
            assert agent.task_channels and agent.task_width == 3 * T + 3 * O
            assert agent.ring.width == agent.ring.data.shape[1] == R.RECORD_WIDTH + 3 * T + 3 * O == 111 + 3 * T + 3 * O
            assert agent._replay_f32() is False
    ring = R.ReplayRing(8, "cpu", width=111 + 9)
    g = torch.Generator().manual_seed(0)
    rec = torch.rand((5, 120), generator=g, dtype=torch.float64)
    ring.push(rec)
    assert len(ring) == 5 and torch.equal(ring.data[:5], rec) and tuple(ring.sample(7, g).shape) == (7, 120)
