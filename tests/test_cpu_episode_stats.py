"""CPU-only: the command-line surface of the vectorised loop's episode statistics and greedy evaluation -- the two new flags and
their defaults, the log keys of a lock-step, an evaluation through the logging sinks, the evaluation thresholds."""
import pytest


class _FakeAim:
    def __init__(self):
        self.calls = []

    def track(self, value, name=None, step=None, context=None):
        self.calls.append((name, value, step, context))


class _FakeWandb:
    def __init__(self):
        self.calls = []

    def log(self, payload):
        self.calls.append(dict(payload))


def test_eval_flags_parse_and_default_to_no_evaluation():
    from robotoddler.training.successor_dqn import EVAL_DEFAULTS, build_parser
    plain = vars(build_parser().parse_args([]))
    assert "eval_envs" not in plain and "eval_epsilon" not in plain      # a plain parse keeps the keys it always had
    assert EVAL_DEFAULTS == dict(eval_envs=0, eval_epsilon=0.0)
    on = vars(build_parser().parse_args(["--num_envs", "256", "--eval_envs", "64", "--eval_epsilon", "0.05"]))
    assert on["eval_envs"] == 64 and on["eval_epsilon"] == 0.05
    assert isinstance(on["eval_envs"], int) and isinstance(on["eval_epsilon"], float)


def test_lockstep_log_values_keep_their_keys_and_append_the_episode_statistics():
    from robotoddler.training.vec_dqn import EPISODE_KEYS, lockstep_log_values
    info = dict(lockstep=3, episodes=41, env_steps=900, lockstep_env_steps=300, avg_loss=0.5, mean_reward=-0.5,
                mean_lin_reward=0.125, epsilon=0.4, steps_per_s=1e5, episodes_finished=4, episode_reward=0.25,
                episode_lin_reward=0.0625, episode_num_steps=3.5, episode_stable=0.75, success_rate=0.25)
    vals = lockstep_log_values(info)
    assert list(vals) == ["reward", "lin_reward", "avg_loss", "num_steps", "epsilon", "env_steps", "steps_per_s",
                          "episodes_finished", "episode_reward", "episode_lin_reward", "episode_num_steps", "episode_stable",
                          "success_rate"]
    assert list(EPISODE_KEYS) == list(vals)[7:]
    # the old meanings: transition means of the lock-step, its env-step count
    assert vals["reward"] == -0.5 and vals["lin_reward"] == 0.125 and vals["num_steps"] == 300
    assert vals["episodes_finished"] == 4 and vals["episode_reward"] == 0.25 and vals["success_rate"] == 0.25
    # a lock-step in which no episode ended, and an info without the keys: None
    old = {k: v for k, v in info.items() if k not in EPISODE_KEYS}
    assert all(lockstep_log_values(old)[k] is None for k in EPISODE_KEYS)


def test_an_evaluation_goes_through_the_sinks_in_the_evaluation_context():
    from robotoddler.training.successor_dqn import track_run_sinks
    ev = dict(reward=0.75, lin_reward=0.3125, avg_loss=None, num_steps=2.5, stable=1.0, collision=0.0, success_rate=0.75,
              episodes=16)
    aim_run, wb = _FakeAim(), _FakeWandb()
    track_run_sinks(ev, 600, 'evaluation', aim_run=aim_run, wandb_run=wb)
    names = [c[0] for c in aim_run.calls]
    assert names == ["reward", "lin_reward", "num_steps", "stable", "collision", "success_rate", "episodes"]   # avg_loss None
    assert all(c[2] == 600 and c[3] == {"context": "evaluation"} for c in aim_run.calls)
    p = wb.calls[0]
    assert p["episode"] == 600 and p["avg_loss"] is None and p["eval_reward"] == ev["lin_reward"] == p["lin_reward"]
    assert p["success_rate"] == 0.75 and p["episode_00600_combined_image"] is None


def test_evaluation_thresholds_follow_the_checkpoint_arithmetic():
    from robotoddler.training.vec_dqn import next_multiple
    every = 300
    nxt, evaluated = next_multiple(0, every), []
    assert nxt == 300
    for done in (120, 250, 310, 590, 640, 899, 1200, 1210, 1499, 1500):      # episodes_done after successive lock-steps
        if done >= nxt:
            evaluated.append(done)
            nxt = next_multiple(done, every)
    # one evaluation per crossed multiple; a lock-step that crosses two (900 and 1200 at 1200) evaluates once
    assert evaluated == [310, 640, 1200, 1500]
    assert nxt == 1800
    # resume from a checkpoint taken at 610 finished episodes: the next evaluation is at 900, as the next checkpoint would be
    assert next_multiple(610, every) == 900 and next_multiple(600, every) == 900 and next_multiple(599, every) == 600
    import inspect
    from robotoddler.training import vec_dqn
    src = inspect.getsource(vec_dqn.run_vectorised)
    assert "next_eval = next_multiple(agent.episodes_done, args['evaluate_every'])" in src
    assert "track_run_sinks(ev, agent.episodes_done, 'evaluation'" in src


def test_the_vectorised_agent_keeps_episode_statistics_off_by_default():
    import inspect
    from robotoddler.training.vec_dqn import VecDQN
    assert inspect.signature(VecDQN.__init__).parameters["episode_stats"].default is False
    assert inspect.signature(VecDQN.evaluate).parameters["epsilon"].default == 0.0


def test_entry_point_declared_in_the_header_and_the_bindings():
    import os
    from bridges_hip import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bridges_hip.h")).read()
    assert "int bridges_episode_stats(int32_t E, int32_t K, const double* rec, const uint8_t* valid, const float* gpow," in text
    assert "bridges_episode_stats" in abi.SIGNATURES and "bridges_episode_stats" in abi.EXPORTED_SYMBOLS
    assert len(abi.SIGNATURES["bridges_episode_stats"]) == 11
