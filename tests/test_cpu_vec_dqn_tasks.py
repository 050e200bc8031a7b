"""CPU: the host side of the vectorised DQN on per-env tasks -- the refusals of VecDQN(per_env_tasks=...) and of the CLI (decided
before anything touches the GPU), the record width of the replay ring, the new entry points in the header and its ctypes mirror."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {
    "bridges_head_sigmoid_dot_rows": "bridges_head_sigmoid_dot",
    "bridges_sigmoid_dot_rows": "bridges_sigmoid_dot",
    "bridges_env_groups_keyed": "bridges_env_groups",
    "bridges_mlp_input_rows": "bridges_mlp_input",
    "bridges_mlp_input_batches_rows": "bridges_mlp_input_batches",
    "bridges_successor_loss_rows": "bridges_successor_loss",
}


def test_new_entry_points_stand_beside_the_old_ones():
    from bridges_hip import abi
    with open(os.path.join(ROOT, "include", "bridges_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    n_args = lambda name: re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M).group(1).count(",") + 1
    for new, old in NEW_SYMBOLS.items():
        assert new in abi.SIGNATURES and old in abi.SIGNATURES and new in abi.EXPORTED_SYMBOLS
        assert n_args(new) == len(abi.SIGNATURES[new]) > n_args(old) == len(abi.SIGNATURES[old])
    # the old entry points keep the signatures INTEGRATION.md documents
    vp, i32, i64 = abi.vp, abi.i32, abi.i64
    assert abi.SIGNATURES["bridges_head_sigmoid_dot"] == [i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, i32, vp]
    assert abi.SIGNATURES["bridges_env_groups"] == [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    assert abi.SIGNATURES["bridges_mlp_input"] == [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    assert len(abi.SIGNATURES["bridges_successor_loss"]) == 20 and len(abi.SIGNATURES["bridges_successor_loss_rows"]) == 21


def fake_env(per_env_tasks, img=64):
    return types.SimpleNamespace(per_env_tasks=per_env_tasks, img=img, n_targets=3)


def test_vec_dqn_refusals_name_the_condition_that_failed(monkeypatch):
    """Every refusal is decided from the arguments alone, before VecDQN allocates anything."""
    from robotoddler.models.cv import ConvNet, Policy, SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    mlp = lambda s=64: SuccessorMLP(img_size=(s, s), hidden_dims=[8])
    mk = lambda pol, env, **kw: VecDQN(pol, pol, None, env, 64, 8, 0.9, 0.05, "mse_q_values", **kw)
    with pytest.raises(ValueError, match="per-env tasks") as e:
        mk(mlp(), fake_env(True))                                        # the default: still refused ...
    assert "per_env_tasks=True" in str(e.value)                          # ... and the message names the option
    with pytest.raises(ValueError, match="per-env tasks"):
        VecDQN(None, None, None, fake_env(True), 64, 8, 0.9, 0.05, "q")
    with pytest.raises(ValueError, match="fixed task"):
        mk(mlp(), fake_env(False), per_env_tasks=True)
    with pytest.raises(ValueError, match="ConvNet"):
        mk(ConvNet(img_size=(64, 64)), fake_env(True), per_env_tasks=True)
    with pytest.raises(ValueError, match="Policy"):
        mk(Policy(), fake_env(True), per_env_tasks=True)
    with pytest.raises(ValueError, match="64x64"):
        mk(mlp(32), fake_env(True, img=32), per_env_tasks=True)
    with pytest.raises(ValueError, match="fused optimiser step"):
        VecDQN(mlp(), mlp(), None, fake_env(True), 64, 8, 0.9, 0.05, "huber", per_env_tasks=True)     # not one of the MSE losses
    monkeypatch.setenv("BRIDGES_FUSED_MLP_STEP", "0")
    with pytest.raises(ValueError, match="BRIDGES_FUSED_MLP_STEP"):
        mk(mlp(), fake_env(True), per_env_tasks=True)
    monkeypatch.setattr(VecDQN, "FACTORED_ACTING", False)
    monkeypatch.delenv("BRIDGES_FUSED_MLP_STEP")
    with pytest.raises(ValueError, match="FACTORED_ACTING"):
        mk(mlp(), fake_env(True), per_env_tasks=True)


CLI = ["--model", "SuccessorMLP", "--num_envs", "64", "--random_targets", "3"]


@pytest.mark.parametrize("argv,word", [(CLI + ["--tower_height", "2"], "--tower_height"),
                                       (CLI + ["--bridge_length", "3"], "--bridge_length"),
                                       (["--model", "SuccessorMLP", "--random_targets", "3"], "--num_envs"),
                                       (["--model", "SuccessorMLP", "--num_envs", "1", "--random_targets", "3"], "--num_envs"),
                                       (["--model", "ConvNet", "--num_envs", "64", "--random_targets", "3"], "ConvNet"),
                                       (["--num_envs", "64", "--random_targets", "3"], "UNet"),
                                       (CLI + ["--image_size", "32x32"], "64x64"),
                                       (CLI + ["--shapes", "hexagon"], "trapezoid"),
                                       (CLI[:-1] + ["0"], "--random_targets"),
                                       (CLI[:-1] + ["9"], "--random_targets")])
def test_cli_refuses_in_words(argv, word):
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and word in e.value.code, e.value.code


def test_cli_option_is_opt_in():
    from robotoddler.training.successor_dqn import build_parser, check_random_targets
    plain = vars(build_parser().parse_args(["--model", "SuccessorMLP", "--num_envs", "64"]))
    assert "random_targets" not in plain                                  # a plain parse keeps the keys it always had
    check_random_targets(plain)
    args = vars(build_parser().parse_args(CLI))
    assert args["random_targets"] == 3
    check_random_targets(args)


def test_replay_ring_width(tmp_path):
    from robotoddler.training import records as R
    assert R.RECORD_WIDTH == 111
    ring = R.ReplayRing(8, "cpu")
    assert ring.width == ring.data.shape[1] == R.RECORD_WIDTH
    wide = R.ReplayRing(8, "cpu", width=R.RECORD_WIDTH + 9)
    assert wide.width == wide.data.shape[1] == 120
    with pytest.raises(ValueError):
        R.ReplayRing(8, "cpu", width=R.RECORD_WIDTH - 1)
    g = torch.Generator().manual_seed(0)
    rec = torch.rand((11, 120), generator=g, dtype=torch.float64)
    wide.push(rec)
    assert len(wide) == 8 and tuple(wide.sample(5, g).shape) == (5, 120)
    path = str(tmp_path / "ring.pt")
    wide.save(path)
    again = R.ReplayRing(8, "cpu", width=120)
    again.load(path)
    order = lambda r: r.data[(r.head - r.size + torch.arange(r.size)) % r.capacity]
    assert torch.equal(order(again), order(wide)) and torch.equal(order(wide), rec[-8:])
    with pytest.raises(ValueError, match="120 columns.*111"):
        ring.load(path)                                                   # a fixed-task ring refuses a per-env-task checkpoint
    narrow = str(tmp_path / "narrow.pt")
    ring.push(rec[:3, :111].contiguous())
    ring.save(narrow)
    with pytest.raises(ValueError, match="111 columns.*120"):
        wide.load(narrow)
    assert len(wide) == 8                                                 # a refused load leaves the ring as it was
    ring.load(narrow)
    assert len(ring) == 3


def test_target_batch_fields_and_class_defaults():
    """The batch _targets returns keeps a plain agent's five values in front and fills the rest only where a mode has them; an
    agent that __init__ has not filled reads every option as switched off."""
    from robotoddler.training.vec_dqn import TargetBatch, VecDQN
    assert TargetBatch._fields[:5] == ("block_f", "binary", "action_f", "q_target", "sf_target")
    assert TargetBatch._fields[5:] == ("reward_maps", "obstacle_bits", "state_bits", "action_bits")
    five = tuple(torch.zeros(1) for _ in range(5))
    batch = TargetBatch(*five)
    assert all(a is b for a, b in zip(batch[:5], five)) and batch[5:] == (None, None, None, None)
    a = VecDQN.__new__(VecDQN)
    assert a.exploration == "epsilon_greedy" and a.n_step == 1 and a.rows_fed == 0 and a.rows_seen == 0
    for name in ("hindsight", "hindsight_buffer", "curriculum", "priority_beta", "_rows_seen_dev", "_hash_mult", "_task_mult"):
        assert getattr(a, name) is None and name not in vars(a), name
