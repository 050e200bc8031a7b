"""CPU-only: the stable_actions_only option is declared at every layer -- the C ABI, the env, the vectorised DQN, the
single-env rollout, the command line and the tools -- defaults to off, and leaves every other default as it was."""
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# build_parser()'s defaults before the option existed
DEFAULTS = dict(num_episodes=1000, max_steps=10, seed=None, num_training_steps=20, learning_rate=0.01, loss_function='mse_q_values',
                tau=0.01, batch_size=32, gamma=0.8, model='UNet', device='cuda', image_size=(64, 64), load_checkpoint=None,
                save_checkpoint=None, checkpoint_every=1000, evaluate_every=100, aim=False, aim_repo='aim-data/', bridge_length=1,
                tower_height=None, verbose=False, log_images=False, replay_buffer_capacity=2000, wandb=False, num_envs=1,
                prioritized_replay=False, shapes='trapezoid')


def test_flag_parses_defaults_off_and_keeps_the_other_defaults():
    from robotoddler.training.successor_dqn import build_parser
    a = vars(build_parser().parse_args([]))
    assert a.pop("stable_actions_only") is False
    assert {k: tuple(v) if isinstance(v, list) else v for k, v in a.items()} == \
        {k: tuple(v) if isinstance(v, list) else v for k, v in DEFAULTS.items()}
    on = vars(build_parser().parse_args(["--stable_actions_only", "--num_envs", "256"]))
    assert on["stable_actions_only"] is True and on["num_envs"] == 256


def test_keyword_defaults_off_at_every_layer():
    from bridges_hip.vec_env import VecAssemblyGym
    from robotoddler.training.successor_dqn import rollout_episode
    from robotoddler.training.vec_dqn import VecDQN
    for fn in (VecAssemblyGym.__init__, VecDQN.__init__, rollout_episode):
        assert inspect.signature(fn).parameters["stable_actions_only"].default is False, fn


def test_entry_points_declared_in_the_header_and_the_bindings():
    from bridges_hip import abi
    text = open(os.path.join(ROOT, "include", "bridges_hip.h")).read()
    for name in ("bridges_env_restrict_to_stable", "bridges_env_rebuild_contacts"):
        assert f"int {name}(bridges_env* env, void* stream);" in text
        assert name in abi.SIGNATURES and name in abi.EXPORTED_SYMBOLS


def test_filters_of_an_empty_action_list():
    import torch
    from robotoddler.utils.actions import filter_stable_actions
    kept, feats = filter_stable_actions(None, [], torch.zeros((0, 1, 64, 64)))
    assert kept == [] and feats.shape[0] == 0


def test_tools_take_the_flag():
    for tool in ("train_throughput.py", "learning_curve.py"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "--stable_actions_only" in out.stdout
