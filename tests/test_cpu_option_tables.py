"""CPU: the two places that list VecDQN's options once -- agent_options_from_args (parsed options -> VecDQN's keyword arguments,
shared by run_vectorised and the tools) and VecDQN._recorded_options (what a checkpoint records about them).  The literals are
what the call sites and save_extra produced before the lists were folded."""
import pytest
import torch

from robotoddler.training.curriculum import Curriculum

PLAIN = dict(curriculum=None, n_step=1, double_q=False, prioritized=False, priority_alpha=1.0, priority_refresh=False)
BOLTZMANN = dict(exploration="boltzmann", temp_start=1.0, temp_end=0.1, temp_decay=0.999)
LINES = {
    "": {},
    "--random_bridge_length 1:3 --curriculum --curriculum_every 5 --curriculum_beta 0.5":
        dict(curriculum=Curriculum(beta=0.5, floor=0.1, every=5, min_episodes=16)),
    "--n_step 3": dict(n_step=3),
    "--double_q": dict(double_q=True),
    "--target_temperature 0.5": dict(target_temperature=0.5),
    "--exploration boltzmann --temp_relative --target_temperature 0.5 --target_temp_relative --spread_floor 0.01":
        dict(BOLTZMANN, target_temperature=0.5, temp_relative=True, target_temp_relative=True, spread_floor=0.01),
    "--target_temperature 0.5 --munchausen_alpha 0.9 --munchausen_clip -0.5":
        dict(target_temperature=0.5, munchausen_alpha=0.9, munchausen_clip=-0.5),
    "--prioritized_replay --priority_alpha 0.6 --priority_refresh --priority_beta 0.4 --priority_beta_anneal 100":
        dict(prioritized=True, priority_alpha=0.6, priority_refresh=True, priority_beta=0.4, priority_beta_anneal=100),
    "--exploration boltzmann --temp_start 2.0 --temp_end 0.2 --temp_decay 0.99":
        dict(exploration="boltzmann", temp_start=2.0, temp_end=0.2, temp_decay=0.99),
    "--random_targets 2 --model SuccessorMLP --hindsight final --hindsight_goals 2": dict(hindsight="final", hindsight_goals=2),
    "--search_every 4 --search_tasks 8 --search_width 4 --search_merge --search_particles --search_temperature 0.5 "
    "--search_resample_temperature 2.0":
        dict(search_every=4, search_tasks=8, search_width=4, search_merge=True, search_sampler="particles", search_temperature=0.5,
             search_resample_temperature=2.0),
    # every group that runs beside the others (Munchausen targets refuse --double_q and --n_step 3; a curriculum refuses hindsight)
    "--random_targets 2 --model SuccessorMLP --n_step 3 --double_q --target_temperature 0.5 --target_temp_relative --temp_relative "
    "--prioritized_replay --priority_alpha 0.6 --priority_beta 0.4 --exploration boltzmann --temp_start 2.0 --hindsight final "
    "--hindsight_fold --search_every 4 --search_width 4":
        dict(BOLTZMANN, temp_start=2.0, n_step=3, double_q=True, target_temperature=0.5, target_temp_relative=True, temp_relative=True,
             prioritized=True, priority_alpha=0.6, priority_beta=0.4, priority_beta_anneal=0, hindsight="final", hindsight_goals=1,
             hindsight_fold=True, search_every=4, search_width=4, search_merge=False),
}


@pytest.mark.parametrize("line", LINES)
def test_keywords_of_an_argument_line(line):
    from robotoddler.training.successor_dqn import agent_options_from_args, build_parser
    args = vars(build_parser().parse_args(["--num_envs", "64"] + line.split()))
    assert agent_options_from_args(args) == dict(PLAIN, **LINES[line])


def test_num_envs_override_and_a_tools_parser():
    """A tool's parser has --envs and its own --prioritized_replay: the override reaches the groups that read num_envs."""
    import argparse
    from robotoddler.training.successor_dqn import add_training_arguments, agent_options_from_args
    ap = argparse.ArgumentParser()
    add_training_arguments(ap, prioritized_flag=True)
    a = vars(ap.parse_args("--prioritized_replay --priority_alpha 0.5 --search_every 2 --search_tasks 4".split()))
    want = dict(PLAIN, prioritized=True, priority_alpha=0.5, search_every=2, search_tasks=4, search_width=8, search_merge=False)
    assert agent_options_from_args(a, num_envs=64) == want and "num_envs" not in a
    with pytest.raises(SystemExit, match="--search_tasks must be 1..--num_envs"):
        agent_options_from_args(a, num_envs=2)


def test_two_faults_are_refused_in_the_words_of_the_group_main_checks_first():
    """--munchausen_alpha without --target_temperature and --priority_alpha without --prioritized_replay: main() checks the
    Munchausen group before the prioritised-replay group, and so does the keyword function."""
    from robotoddler.training.successor_dqn import agent_options_from_args, build_parser, main
    argv = ["--num_envs", "64", "--model", "SuccessorMLP", "--priority_alpha", "0.5", "--munchausen_alpha", "0.9"]
    with pytest.raises(SystemExit) as by_main:
        main(argv)
    with pytest.raises(SystemExit) as by_keywords:
        agent_options_from_args(vars(build_parser().parse_args(argv)))
    assert by_keywords.value.code == by_main.value.code and "--munchausen_alpha" in by_main.value.code
    assert "--target_temperature" in by_main.value.code and "--priority_alpha" not in by_main.value.code


def stand_in(full):
    from robotoddler.training.vec_dqn import VecDQN
    a = VecDQN.__new__(VecDQN)
    a.n_task_targets, a.n_task_obstacles = 2, 1
    a.epsilon, a.episodes_done, a.env_steps, a.rank, a.seed = 0.25, 7, 99, 0, 0
    a.step_images = torch.zeros((3, 4, 4))
    a.sample_gen, a.explore_gen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
    if full:
        a.n_step = 3
        a.target_temperature, a.target_temp_relative, a.spread_floor, a.munchausen = 0.5, True, 0.01, (0.9, -0.5)
        a.exploration, a.temperature, a.temp_start, a.temp_relative = "boltzmann", 0.7, 1.0, True
        a.search_every, a.search_calls = 4, 2
        a.search_sampler, a.search_temperature, a.search_resample_temperature = "particles", 0.5, 2.0
        a.search_gen = torch.Generator().manual_seed(3)
        a._search_generator = lambda: a.search_gen
        a.priority_beta, a.priority_beta_calls = 0.4, 11

        class Buffer:
            def state_dict(self):
                return dict(rows=torch.arange(3))

            def load_state_dict(self, state):
                self.loaded = state
        a.hindsight, a.hindsight_goals, a.hindsight_fold, a.hindsight_buffer = "final", 2, True, Buffer()
    return a


BLOB = {
    False: dict(counters=dict(lockstep=5), env_steps=99, episodes_done=7, epsilon=0.25, n_step=1, task_shape=(2, 1)),
    True: dict(counters=dict(lockstep=5), env_steps=99, episodes_done=7, epsilon=0.25, n_step=3, task_shape=(2, 1),
               hindsight=("final", 2), hindsight_fold=True, munchausen=(0.9, -0.5), priority_beta_calls=11, search_phase=2,
               search_sampler=("particles", 0.5, 2.0), target_temp_relative=0.01, target_temperature=0.5, temp_relative=0.01,
               temperature=0.7),
}
TENSORS = {False: {"explore_gen", "sample_gen", "step_images"},
           True: {"explore_gen", "sample_gen", "step_images", "search_gen", "hindsight_buffer"}}


@pytest.mark.parametrize("full", [False, True])
def test_checkpoint_blob_of_a_stand_in(tmp_path, full):
    path = str(tmp_path / "agent.pt")
    stand_in(full).save_extra(path, lockstep=5)
    blob = torch.load(path, weights_only=True)
    assert set(blob) == set(BLOB[full]) | TENSORS[full]
    for key, want in BLOB[full].items():
        assert blob[key] == want and type(blob[key]) is type(want), key
    again = stand_in(full)
    again.temperature, again.search_calls, again.priority_beta_calls = 0.1, 0, 0
    assert again.load_extra(path) == dict(lockstep=5)
    if full:
        assert (again.temperature, again.search_calls, again.priority_beta_calls) == (0.7, 2, 11)
        assert torch.equal(again.hindsight_buffer.loaded["rows"], torch.arange(3))
    # the other kind refuses the file, with the first entry of the table that differs
    with pytest.raises(ValueError, match="n_step = 3.*n_step = 1" if full else "n_step = 1.*n_step = 3"):
        stand_in(not full).load_extra(path)
