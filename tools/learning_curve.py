"""Does the vectorised loop learn?  With --random_bridge_length LO:HI / --random_tower_height LO:HI on a task family, success
printed per span / height as well.  Trains a Q-network (--model SuccessorMLP | ConvNet | UNet) on tower_height=2 for a fixed
number of lock-steps and prints per block of lock-steps the statistics of the training episodes that ended in it (EpisodeStats:
log_episode's discounted reward / lin_reward, length, final stability, and success_rate = the fraction that reached the target,
all under the running epsilon-greedy exploration) and the mean loss; with --eval_envs N also the greedy evaluation of the policy
at the end of the block (VecDQN.evaluate: one episode in each of N envs, --eval_epsilon 0 = the reference's greedy policy).
With --eval_envs the line also holds eval_q_first, the mean over the evaluation envs of the policy net's q of the row chosen in
the FIRST step of the episode: the net's own forecast of eval_lin_reward, the discounted lin_reward the same episodes then
realise -- their difference is the over-estimation that --double_q is meant to reduce.
With --eval_beam B beside --eval_envs the line also holds beam_success_rate / beam_reward / beam_lin_reward: the same tasks under a
beam search of width B with the policy net's q as the heuristic (VecDQN.beam_search).  With --eval_beam_merge beside it the same
search runs once more with merge=True (beams that hold the same structure are closed after every depth): merge_success_rate /
merge_reward / merge_lin_reward, eval_merged_beams, and per depth merged_by_depth / live_by_depth (closed / looked at).
With --eval_particles B --eval_particle_temperature T beside --eval_envs (alone or beside --eval_beam: the searches touch no
training state and draw from a stream of their own, so one run holds them all on the same tasks) the line also holds
particle_success_rate / particle_reward / particle_lin_reward / particle_ess / particle_p_sel: the same tasks under
VecDQN.particle_search; with --eval_particle_control a further leg control_*: the same B rollouts without resampling and without the
elite (resample temperature inf), the plain best-of-B control.
    python tools/learning_curve.py --locksteps 1500 --envs 1024 [--model ConvNet --loss mse_q_values]
                                   [--eval_envs 64 [--eval_beam 8 [--eval_beam_merge]]
                                    [--eval_particles 8 --eval_particle_temperature T [--eval_particle_control]]]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")]
import numpy as np
import torch
from robotoddler.training.successor_dqn import (add_eval_beam_argument, add_eval_particle_arguments, add_training_arguments,
                                                agent_options_from_args, build_parser, check_curriculum, eval_particles_from_args,
                                                make_nets)
from robotoddler.training.vec_dqn import VecDQN, beam_env_like
from bridges_hip import ops
from bridges_hip.shapes import load_urdf
from bridges_hip.vec_env import RandomBridges, RandomObstacles, RandomTargets, VecAssemblyGym

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--locksteps", type=int, default=1500)
ap.add_argument("--tower", type=int, default=2)
ap.add_argument("--max_steps", type=int, default=10)
ap.add_argument("--train_steps", type=int, default=10)
ap.add_argument("--loss", default="mse_q_values+mse_block_features")
ap.add_argument("--lr", type=float, default=1e-4)
ap.add_argument("--block", type=int, default=100)
ap.add_argument("--model", default="SuccessorMLP")
ap.add_argument("--stable_actions_only", action="store_true", help="every action set restricted to the stable placements")
ap.add_argument("--eval_envs", type=int, default=0, help="> 0: greedy evaluation over this many envs at the end of every block")
ap.add_argument("--eval_epsilon", type=float, default=0.0, help="exploration rate of the evaluation episodes")
ap.add_argument("--random_targets", type=int, default=0, metavar="T",
                help="> 0: per-env random tasks instead of the tower (tower_setup(num_targets=T) per env and episode, no obstacles; "
                     "SuccessorMLP, or ConvNet / UNet with --task_channels); --eval_envs then evaluates on a fixed held-out set of N tasks")
ap.add_argument("--random_obstacles", type=int, default=0, metavar="O",
                help="> 0, with --random_targets: O obstacles per env and episode beside the targets, x ~ U[-3, 3), z ~ U[0.3, 2.5); "
                     "the evaluation env draws its own")
ap.add_argument("--task_channels", action="store_true",
                help="with --random_targets and --model ConvNet | UNet: the conv Q-network on the per-env tasks (VecDQN(task_channels=True))")
ap.add_argument("--random_bridge_length", default=None, metavar="LO:HI",
                help="a task family instead: horizontal_bridge_setup(num_obstacles=n) per env and episode, n drawn from LO..HI "
                     "(RandomBridges; SuccessorMLP, or ConvNet / UNet with --task_channels)")
ap.add_argument("--random_tower_height", default=None, metavar="LO:HI",
                help="a task family instead: bridge_setup(num_stories=n) per env and episode, n drawn from LO..HI")
add_training_arguments(ap, prioritized_flag=True)    # the training options of the vectorised loop, as successor_dqn.py takes them
add_eval_beam_argument(ap)               # --eval_beam B: beam search of width B on the evaluation tasks (VecDQN.beam_search)
add_eval_particle_arguments(ap)          # --eval_particles B --eval_particle_temperature T [...]: VecDQN.particle_search on the evaluation tasks
ap.add_argument("--eval_particle_control", action="store_true",
                help="with --eval_particles: one more leg, the same rollouts without resampling and without the elite (best-of-B)")
a = ap.parse_args()
# (here the particle search may stand beside --eval_beam: the legs of one comparison)
eval_particles = eval_particles_from_args({k: v for k, v in dict(vars(a), num_envs=a.envs).items() if k != "eval_beam"})
if a.eval_particle_control and eval_particles is None:
    ap.error("--eval_particle_control is a leg of --eval_particles B: it needs --eval_particles B")
eval_beam = vars(a).get("eval_beam")
if eval_beam is not None and not (1 <= eval_beam <= 16 and a.eval_envs > 0):
    ap.error("--eval_beam B needs 1 <= B <= 16 and --eval_envs M, M > 0")
eval_beam_merge = bool(vars(a).get("eval_beam_merge"))
if eval_beam_merge and eval_beam is None:
    ap.error("--eval_beam_merge merges the beams of the search --eval_beam B runs: it needs --eval_beam B")
if a.random_bridge_length and a.random_tower_height:
    ap.error("--random_bridge_length and --random_tower_height name two task families: give one")
family = None
if a.random_bridge_length or a.random_tower_height:
    if a.random_targets or a.random_obstacles:
        ap.error("a task family draws targets and obstacles from one integer: not with --random_targets / --random_obstacles")
    lo, hi = (a.random_bridge_length or a.random_tower_height).split(":")
    family = ("span" if a.random_bridge_length else "tower", int(lo), int(hi))
check_curriculum(vars(a), family[1:] if family else None)
if a.random_obstacles and not a.random_targets:
    ap.error("--random_obstacles rides on --random_targets")
if a.task_channels and not (a.random_targets or family):
    ap.error("--task_channels rides on --random_targets")
dev = torch.device("cuda:0")
args = vars(build_parser().parse_args(["--model", a.model, "--loss_function", a.loss]))
H = 0.8
torch.manual_seed(0)
pol, tgt = make_nets(args, dev)
obstacles, targets = (lambda: [(0.5, 0., i * H + H / 2) for i in range(a.tower)]), (lambda: [(0.5, 0, a.tower * H + H / 2)])
if a.random_targets:
    obstacles, targets = (lambda: []), (lambda: RandomTargets(a.random_targets))
if a.random_obstacles:
    obstacles = lambda: RandomObstacles([((-3.0, 3.0), (0.3, 2.5))] * a.random_obstacles)
train_targets = targets
if family:                                                      # the weights are the training env's: evaluation stays uniform
    obstacles, targets = (lambda: []), (lambda: RandomBridges(family[0], sizes=family[1:]))
    train_targets = lambda: RandomBridges(family[0], sizes=family[1:], weights=vars(a).get("family_weights"))
env = VecAssemblyGym(a.envs, [load_urdf("shapes/trapezoid.urdf")], obstacles(), train_targets(), max_steps=a.max_steps, seed=0, device=dev,
                     f32_rasters=VecDQN.acting_needs_f32_rasters(pol) and not a.task_channels, stable_actions_only=a.stable_actions_only)
agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=a.lr, fused=True), env, 200000, 32, 0.95, 0.01, a.loss,
               eps_decay=0.997, stable_actions_only=a.stable_actions_only, episode_stats=True, per_env_tasks=bool(a.random_targets or family),
               per_env_obstacles=bool(a.random_obstacles or family), task_channels=a.task_channels,
               **agent_options_from_args(vars(a), num_envs=a.envs))
eval_env = None
if a.eval_envs > 0:
    eval_env = VecAssemblyGym(a.eval_envs, [load_urdf("shapes/trapezoid.urdf")], obstacles(), targets(), max_steps=a.max_steps, seed=1, device=dev,
                              f32_rasters=VecDQN.acting_needs_f32_rasters(pol) and not a.task_channels,
                              stable_actions_only=a.stable_actions_only)
beam_env = beam_env_like(eval_env, eval_beam) if eval_beam else None
particle_env = None
if eval_particles is not None:
    particle_env = beam_env if eval_beam == eval_particles["width"] else beam_env_like(eval_env, eval_particles["width"])
r4 = lambda v: None if v is None else round(v, 4)


def evaluate_with_first_q(agent, eval_env, epsilon):
    """agent.evaluate plus the mean q of the rows chosen in the episodes' first step (read after the evaluation's own wait)."""
    act_on, first = agent._act_on, []

    def recording(*args, **kw):
        out = act_on(*args, **kw)
        if not first:
            first.append(out[2].mean())
        return out
    agent._act_on = recording
    try:
        ev = agent.evaluate(eval_env, epsilon)
    finally:
        del agent._act_on
    return ev, float(first[0])


t0 = time.time()
deferred, searches = [], []
for it in range(1, a.locksteps + 1):
    deferred.append(agent.lockstep(a.train_steps, defer_losses=True)[0])
    if agent.last_search is not None:                           # search in training: the lock-steps of the block that searched
        searches.append(agent.last_search)
    if it % a.block == 0:
        ep = agent.episode_stats.take().get()                   # the episodes that ended in the block: one read per block
        losses = [l for d in deferred for l in d.get()]
        line = dict(lockstep=it, seconds=round(time.time() - t0, 1), epsilon=round(agent.epsilon, 3), episodes=ep["episodes"],
                    success_rate=r4(ep["success_rate"]), episode_reward=r4(ep["reward"]), episode_lin_reward=r4(ep["lin_reward"]),
                    episode_num_steps=r4(ep["num_steps"]), episode_stable=r4(ep["stable"]),
                    mean_loss=round(float(np.mean(losses)), 5) if losses else None)
        if agent.exploration == "boltzmann":                    # the block's last lock-step: its share of draws off the arg-max
            line.update(temperature=round(agent.temperature, 4), explored_fraction=r4(agent.explored_fraction))
        if agent.target_temperature is not None:                # soft targets: means over the block's lock-steps of the two log keys
            soft = [d.soft for d in deferred if d.soft is not None]
            line.update(target_entropy=r4(float(np.mean([s["target_entropy"] for s in soft])) if soft else None),
                        soft_value_gap=r4(float(np.mean([s["soft_value_gap"] for s in soft])) if soft else None))
            if agent.target_temp_relative:                      # ... and of the mean effective temperature of the backups
                line.update(target_temperature_effective=r4(float(np.mean([s["target_temperature_effective"] for s in soft])) if soft else None))
            if agent.munchausen is not None:                    # ... and of the three Munchausen keys (missed: the block's sum)
                line.update(munchausen_bonus=r4(float(np.mean([s["munchausen_bonus"] for s in soft])) if soft else None),
                            munchausen_clipped=r4(float(np.mean([s["munchausen_clipped"] for s in soft])) if soft else None),
                            munchausen_missed=float(np.sum([s["munchausen_missed"] for s in soft])) if soft else None)
        if agent.temp_relative:                                 # the block's last lock-step: the mean temperature its envs drew at
            line.update(temperature_effective=r4(agent.temperature_effective))
        if agent.hindsight is not None:                         # the block's last lock-step: the relabelled rows it pushed
            line.update(hindsight_rows=agent.hindsight_rows)
        if agent.search_every:                                  # means over the block's searches, and the rows they pushed
            line.update(searches=len(searches), search_rows=sum(s["search_rows"] for s in searches),
                        search_success_rate=r4(float(np.mean([s["search_success_rate"] for s in searches])) if searches else None),
                        search_lin_reward=r4(float(np.mean([s["search_lin_reward"] for s in searches])) if searches else None))
            searches = []
        if family:                                              # success per span / height n = LO..HI, and the episodes behind it
            line.update(success_by_class={n: r4(c["success_rate"]) for n, c in enumerate(ep["by_class"]) if n >= family[1]},
                        episodes_by_class={n: c["episodes"] for n, c in enumerate(ep["by_class"]) if n >= family[1]})
            if env.family_weights is not None:                  # the weights the next block draws under (one read per block)
                line.update(weights_by_class={family[1] + k: w for k, w in enumerate(env.family_weights.tolist())})
        if eval_env is not None:
            ev, q_first = evaluate_with_first_q(agent, eval_env, a.eval_epsilon)
            line.update(eval_success_rate=r4(ev["success_rate"]), eval_reward=r4(ev["reward"]), eval_num_steps=r4(ev["num_steps"]),
                        eval_lin_reward=r4(ev["lin_reward"]), eval_q_first=r4(q_first))
            if beam_env is not None:                            # the same tasks under a beam of width B
                bs = agent.beam_search(beam_env, eval_beam)
                line.update(beam_width=eval_beam, beam_success_rate=r4(bs["success_rate"]), beam_reward=r4(bs["reward"]),
                            beam_lin_reward=r4(bs["lin_reward"]), beam_num_steps=r4(bs["num_steps"]))
                if eval_beam_merge:                             # ... and under the same beam with merging, beside it
                    bm = agent.beam_search(beam_env, eval_beam, merge=True)
                    line.update(merge_success_rate=r4(bm["success_rate"]), merge_reward=r4(bm["reward"]),
                                merge_lin_reward=r4(bm["lin_reward"]), merge_num_steps=r4(bm["num_steps"]),
                                eval_merged_beams=sum(bm["merged_beams"]), merged_by_depth=bm["merged_by_depth"],
                                live_by_depth=bm["live_by_depth"])
            if particle_env is not None:                        # the same tasks under B sampled, resampled rollouts
                legs = [("particle", eval_particles)]
                if a.eval_particle_control:                     # ... and under B independent rollouts, the best kept
                    legs.append(("control", dict(eval_particles, resample_temperature=float("inf"), elite=False)))
                for name, kw in legs:
                    ps = agent.particle_search(particle_env, **kw)
                    line.update({f"{name}_success_rate": r4(ps["success_rate"]), f"{name}_reward": r4(ps["reward"]),
                                 f"{name}_lin_reward": r4(ps["lin_reward"]), f"{name}_num_steps": r4(ps["num_steps"]),
                                 f"{name}_ess": [r4(v) for v in ps["ess_by_depth"]], f"{name}_p_sel": [r4(v) for v in ps["p_sel_mean_by_depth"]]})
                # what the temperature stands against: the mean over the tasks of the spread (population standard deviation) of
                # q among the candidates of the empty state, from the relative-temperature operator at multiple 1
                particle_env.reset()                            # (explicit task arrays: a reset redraws nothing)
                stable = agent._stable_flags(particle_env)
                idx, row_env, seg, rep = agent._rows(particle_env, stable)
                spread = ops.boltzmann_select(seg, agent._policy_q(particle_env, idx, row_env, stable),
                                              torch.zeros(particle_env.E, device=dev), 1.0, False, idx,
                                              particle_env.cand_offset[:particle_env.E], rep=rep, relative=True, spread_floor=1e-30)[5]
                line.update(particles=eval_particles["width"], particle_temperature=eval_particles["temperature"],
                            eval_q_spread_first=r4(float(spread.mean())))
            if family:
                line.update(eval_success_by_class={n: r4(s) for n, s in enumerate(ev["success_by_class"]) if n >= family[1]})
        print(json.dumps(line), flush=True)
        deferred = []
