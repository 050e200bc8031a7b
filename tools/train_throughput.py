"""Training-in-the-loop throughput of the vectorised successor-DQN (reported separately from the simulator bench)."""
import argparse, json, os, sys, time
if "--miopen_search" not in sys.argv:
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")]
import torch
from robotoddler.training.successor_dqn import (add_training_arguments, agent_options_from_args, build_parser, check_curriculum,
                                                make_nets)
from robotoddler.training.vec_dqn import VecDQN
from bridges_hip.shapes import load_urdf
from bridges_hip.vec_env import RandomBridges, RandomObstacles, RandomTargets, VecAssemblyGym

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--tower", type=int, default=4)
ap.add_argument("--max_steps", type=int, default=15)
ap.add_argument("--model", default="SuccessorMLP")
ap.add_argument("--loss", default="mse_block_features")
ap.add_argument("--locksteps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--train_steps", type=int, default=25)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--no_fused_adam", action="store_true")
ap.add_argument("--no_dedup", action="store_true",
                help="A/B: every env its own candidate rows and every row fed, also when envs are in the same state / rows have identical inputs")
ap.add_argument("--miopen_search", action="store_true", help="let MIOpen benchmark its algorithms (one shape per run)")
ap.add_argument("--channels_last", action="store_true")
ap.add_argument("--shapes", default="trapezoid", choices=["trapezoid", "hexagon", "both"])
ap.add_argument("--bridge_length", type=int, default=0, help="> 0: horizontal_bridge_setup(num_obstacles=N) instead of the tower")
ap.add_argument("--stable_actions_only", action="store_true", help="every action set restricted to the stable placements")
ap.add_argument("--episode_stats", action="store_true",
                help="per-episode statistics on (one bridges_episode_stats launch per lock-step, read one lock-step late)")
ap.add_argument("--random_targets", type=int, default=0, metavar="T",
                help="> 0: per-env random tasks (tower_setup(num_targets=T) per env and episode, no obstacles; VecDQN(per_env_tasks=True))")
ap.add_argument("--fixed_targets", type=int, default=0, metavar="T",
                help="> 0: the fixed-task counterpart of --random_targets T: T targets shared by every env (T = 3: fixed3 of "
                     "tools/random_task_throughput.py), no obstacles")
ap.add_argument("--random_obstacles", type=int, default=0, metavar="O",
                help="> 0, with --random_targets: O obstacles per env and episode beside the targets, x ~ U[-3, 3), z ~ U[0.3, 2.5) "
                     "(VecDQN(per_env_obstacles=True))")
ap.add_argument("--task_channels", action="store_true",
                help="with --random_targets and --model ConvNet | UNet: the conv Q-network on the per-env tasks, its rows written by "
                     "k_conv_input (VecDQN(task_channels=True)); the like-for-like baseline is --fixed_targets T --no_dedup")
ap.add_argument("--fixed_obstacles", type=int, default=0, metavar="O",
                help="> 0, with --fixed_targets: the like-for-like baseline of --random_obstacles O: O fixed obstacles on the floor, "
                     "shared by all envs (combine with --no_dedup)")
ap.add_argument("--random_bridge_length", default=None, metavar="LO:HI",
                help="a task family instead: horizontal_bridge_setup(num_obstacles=n) per env and episode, n drawn from LO..HI "
                     "(RandomBridges; SuccessorMLP, or ConvNet / UNet with --task_channels)")
ap.add_argument("--random_tower_height", default=None, metavar="LO:HI",
                help="a task family instead: bridge_setup(num_stories=n) per env and episode, n drawn from LO..HI")
add_training_arguments(ap, prioritized_flag=True)    # the training options of the vectorised loop, as successor_dqn.py takes them
a = ap.parse_args()
if a.random_bridge_length and a.random_tower_height:
    ap.error("--random_bridge_length and --random_tower_height name two task families: give one")
family = None
if a.random_bridge_length or a.random_tower_height:
    if a.random_targets or a.random_obstacles:
        ap.error("a task family draws targets and obstacles from one integer: not with --random_targets / --random_obstacles")
    lo, hi = (a.random_bridge_length or a.random_tower_height).split(":")
    family = ("span" if a.random_bridge_length else "tower", int(lo), int(hi))
check_curriculum(vars(a), family[1:] if family else None)
if a.random_targets and a.fixed_targets:
    ap.error("--random_targets and --fixed_targets are two legs of one comparison: give one")
if a.random_obstacles and not a.random_targets:
    ap.error("--random_obstacles rides on --random_targets")
if a.task_channels and not (a.random_targets or family):
    ap.error("--task_channels rides on --random_targets")
if a.fixed_obstacles and not a.fixed_targets:
    ap.error("--fixed_obstacles is the baseline of --random_obstacles: give it with --fixed_targets")
dev = torch.device("cuda:0")
if a.miopen_search:
    torch.backends.cudnn.benchmark = True
args = vars(build_parser().parse_args(["--model", a.model, "--loss_function", a.loss, "--learning_rate", "1e-4"]))
H = 0.8
torch.manual_seed(0)
pol, tgt = make_nets(args, dev)
if a.channels_last:
    pol, tgt = pol.to(memory_format=torch.channels_last), tgt.to(memory_format=torch.channels_last)
names = dict(trapezoid=["trapezoid"], hexagon=["hexagon"], both=["trapezoid", "hexagon"])[a.shapes]
if family:
    obstacles, targets = [], RandomBridges(family[0], sizes=family[1:], weights=vars(a).get("family_weights"))
elif a.random_targets:
    targets = RandomTargets(a.random_targets)
    obstacles = RandomObstacles([((-3.0, 3.0), (0.3, 2.5))] * a.random_obstacles) if a.random_obstacles else []
elif a.fixed_targets:
    import numpy as np
    # the three shared targets tools/random_task_throughput.py calls fixed3; beyond three: one draw of tower_setup's
    # distribution (x ~ U[-4, 4], z ~ U[0, 4], y = 0)
    rng = np.random.default_rng(0)
    fixed3 = [(0.5, 0.0, 1.2), (-1.5, 0.0, 2.6), (2.5, 0.0, 0.4)]
    # --fixed_obstacles O: cube06 obstacles resting on the floor (z = half their 0.6 side), spread over the sampler's x range
    obstacles = [(-2.4 + 4.8 * i / max(a.fixed_obstacles - 1, 1), 0.0, 0.3) for i in range(a.fixed_obstacles)]
    targets = (fixed3 + [(float(rng.uniform(-4, 4)), 0.0, float(rng.uniform(0, 4))) for _ in range(a.fixed_targets - 3)])[:a.fixed_targets]
elif a.bridge_length:
    sq, nn = 0.6, a.bridge_length
    obstacles, targets = [(i * sq, 0.0, sq / 2) for i in range(1, nn + 1)], [(nn * sq + 2.5 * sq, 0.0, sq / 2)]
else:
    obstacles, targets = [(0.5, 0., i * H + H / 2) for i in range(a.tower)], [(0.5, 0, a.tower * H + H / 2)]
env = VecAssemblyGym(a.envs, [load_urdf(f"shapes/{n}.urdf") for n in names], obstacles, targets, max_steps=a.max_steps, seed=0,
                     device=dev, f32_rasters=VecDQN.acting_needs_f32_rasters(pol) and not a.task_channels, candidate_snapshots=a.stable_actions_only,
                     stable_actions_only=a.stable_actions_only)
opt = torch.optim.Adam(pol.parameters(), lr=1e-4, fused=not a.no_fused_adam)
agent = VecDQN(pol, tgt, opt, env, 200000, a.batch, 0.95, 0.01, a.loss, stable_actions_only=a.stable_actions_only,
               episode_stats=a.episode_stats, per_env_tasks=bool(a.random_targets or family),
               per_env_obstacles=bool(a.random_obstacles or family), task_channels=a.task_channels,
               **agent_options_from_args(vars(a), num_envs=a.envs))
VecDQN.TRACK_ROWS = True
if a.no_dedup:
    VecDQN.DEDUP_ROWS = VecDQN.DEDUP_STATES = False
for i in range(a.warmup):
    agent.lockstep(a.train_steps)
    print("warm-up lock-step", i, "done", flush=True)
# 1) the loop as run_vectorised runs it: nothing between lock-steps waits for the optimiser steps (deferred loss readback)
agent._rows_seen_dev, agent.rows_fed = None, 0
torch.cuda.synchronize(); s0 = agent.env_steps; t0 = time.perf_counter()
pending, per_step, tp = None, [], t0
hindsight_rows = 0
searched, search_rows, search_success = [], 0, []
for _ in range(a.locksteps):
    deferred, _rec = agent.lockstep(a.train_steps, defer_losses=True)
    hindsight_rows += agent.hindsight_rows
    searched.append(agent.last_search is not None)
    if agent.last_search is not None:
        search_rows += agent.last_search["search_rows"]
        search_success.append(agent.last_search["search_success_rate"])
    stats = agent.episode_stats.take() if agent.episode_stats is not None else None
    if pending is not None:
        pending[0].get()
        if pending[1] is not None:
            pending[1].get()
    pending = (deferred, stats)
    tn = time.perf_counter(); per_step.append(tn - tp); tp = tn
losses = pending[0].get()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
steps_done = agent.env_steps - s0
rows_seen, rows_fed = getattr(agent, "rows_seen", 0), getattr(agent, "rows_fed", 0)
# search in training: the host time of the lock-steps that searched beside that of the others (medians)
_med = lambda v: sorted(v)[len(v) // 2] * 1e3 if v else None
ms_searching = _med([t for t, s in zip(per_step, searched) if s])
ms_not_searching = _med([t for t, s in zip(per_step, searched) if not s])
per_step.sort()
median = per_step[len(per_step) // 2]
# 2) the same lock-steps with a device synchronisation between the phases, for the per-phase times only
t_targets = [0.0]
_orig_targets = agent._targets
def _timed_targets(rec):
    torch.cuda.synchronize(); ta = time.perf_counter()
    out = _orig_targets(rec)
    torch.cuda.synchronize(); t_targets[0] += time.perf_counter() - ta
    return out
agent._targets = _timed_targets
t_act = t_train = 0.0
n_phase = max(2, a.locksteps // 2)
for _ in range(n_phase):
    torch.cuda.synchronize(); t1 = time.perf_counter()
    rec, valid = agent.act()
    agent.env_steps += int(valid.sum().item())
    if agent.n_step > 1:                                         # the h-step rows the fold emits, as lockstep pushes them
        out, out_valid = agent._fold(agent.with_task(rec), valid)
        agent.ring.push(out[out_valid])
    else:
        agent.ring.push(agent.with_task(rec)[valid])
    torch.cuda.synchronize(); t2 = time.perf_counter()
    agent.train_steps(a.train_steps)
    agent.update_target()
    torch.cuda.synchronize(); t3 = time.perf_counter()
    t_act += t2 - t1; t_train += t3 - t2
print(json.dumps(dict(config=vars(a), family_weights=env.family_weights.tolist() if getattr(env, "family_weights", None) is not None else None,
                      env_steps_per_s=steps_done / dt,
                      env_steps_per_s_at_median_lockstep=steps_done / a.locksteps / median, ms_median_lockstep=median * 1e3,
                      ms_per_lockstep=dt / a.locksteps * 1e3,
                      # host time between consecutive lock-steps, sorted: min, 10 / 25 / 75 / 90 % points, max (the host runs ahead
                      # of the GPU and waits one lock-step late, so single lock-steps can read far below and above the mean)
                      ms_lockstep_points=[round(per_step[min(len(per_step) - 1, int(f * len(per_step)))] * 1e3, 2)
                                          for f in (0.0, 0.1, 0.25, 0.75, 0.9, 1.0)],
                      rows_per_lockstep=rows_seen / a.locksteps, rows_fed_per_lockstep=rows_fed / a.locksteps,
                      ms_lockstep_per_1000_fed_rows=(dt * 1e3 / (rows_fed / 1000.0)) if rows_fed else None, rows_fed_fraction=(rows_fed / rows_seen) if rows_seen else None,
                      ms_act=t_act / n_phase * 1e3, ms_targets=t_targets[0] / n_phase * 1e3, ms_train=t_train / n_phase * 1e3,
                      ms_per_train_step=(t_train - t_targets[0]) / n_phase / a.train_steps * 1e3, last_loss=losses[-1] if losses else None,
                      hindsight_rows_per_lockstep=(hindsight_rows / a.locksteps) if agent.hindsight is not None else None,
                      searches=sum(searched), ms_median_lockstep_searching=ms_searching, ms_median_lockstep_not_searching=ms_not_searching,
                      search_rows_per_search=(search_rows / sum(searched)) if sum(searched) else None,
                      search_success_rates=search_success if agent.search_every else None,
                      note="env_steps_per_s: pipelined loop (VecDQN.lockstep, deferred loss readback); ms_act / ms_targets / "
                           "ms_train: separate pass with a device synchronisation between the phases (they overlap in the loop)")))
