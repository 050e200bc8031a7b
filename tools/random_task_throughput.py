#!/usr/bin/env python3
"""What per-env tasks cost the lock-step simulator: the headline workload's shape (4096 envs as two groups with the raster gate,
trapezoid, max_steps 15, uniform-random policy, f32 rasters) on three tasks --
  bridge   the benchmark's bridge_setup(4): one target, four obstacles, shared by all envs (k_step / k_raster);
  fixed3   three fixed targets, no obstacle, shared by all envs (the same kernels);
  random3  RandomTargets(): three targets per env, redrawn on the device every episode (the per-env instantiations + k_task_features).
fixed3 against random3 isolates the feature (same shapes, same max_steps).  Candidates per state differ between tasks, so read
the time per lock-step together with the candidates per lock-step, not env-steps/s alone.  Prints one JSON line.
--random_obstacles O adds (or, with --tasks, makes available) two more tasks on fixed3's targets --
  obst_fixed   O fixed obstacles on the floor, shared by all envs (k_step / k_raster, the shared obstacle raster);
  obst_random  RandomObstacles: O obstacles per env, x ~ U[-3, 3), z ~ U[0.3, 2.5), redrawn on the device every episode (per-env
               k_step, k_task_features for the obstacle raster alone, k_raster reading env_obstacle_bits per work item).

--family span:LO:HI | tower:LO:HI adds (or, with --tasks, makes available) one more task --
  family       RandomBridges: one target and up to HI obstacles per env, both named by ONE integer n in LO..HI redrawn on the
               device every episode (the per-env kernels, one k_task_features launch per lock-step that draws n).  Its like-for-like
               counterpart is --random_targets 1 --random_obstacles HI.

  python tools/random_task_throughput.py [--envs 4096] [--groups 2] [--steps 100] [--warmup 20] [--tasks bridge,fixed3,random3]
                                         [--random_obstacles O] [--random_targets T] [--family span:1:4]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")]
import torch
from bridges_hip.shapes import load_urdf
from bridges_hip.vec_env import RandomBridges, RandomObstacles, RandomTargets, VecAssemblyGymGroups

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--groups", type=int, default=2)
ap.add_argument("--steps", type=int, default=100, help="timed lock-steps (at least 100, as the side modes of bench.py)")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--max_steps", type=int, default=15)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--tasks", default=None, help="default: bridge,fixed3,random3 (+ obst_fixed,obst_random with --random_obstacles)")
ap.add_argument("--random_obstacles", type=int, default=0, metavar="O", help="obstacles per env of the obst_* tasks (1..4)")
ap.add_argument("--random_targets", type=int, default=0, metavar="T",
                help="> 0: task `uniform` = RandomTargets(T) beside RandomObstacles of --random_obstacles O: the independent samplers")
ap.add_argument("--family", default=None, metavar="KIND:LO:HI", help="task `family` = RandomBridges(KIND, sizes=(LO, HI)), KIND span | tower")
ap.add_argument("--family_weights", default=None, metavar="W,W,...",
                help="with --family: HI - LO + 1 integer weights of the classes LO..HI (the weighted draw: a threshold table read by "
                     "the task kernel); equal weights draw the classes of the uniform draw")
ap.add_argument("--curriculum", action="store_true",
                help="refused here: the curriculum follows a policy's success per class, and this tool steps a uniform-random "
                     "policy without records (tools/train_throughput.py and tools/learning_curve.py run it)")
a = ap.parse_args()
if a.curriculum:
    ap.error("--curriculum needs the training loop: use tools/train_throughput.py or tools/learning_curve.py")
if a.family_weights and not a.family:
    ap.error("--family_weights weighs the classes of --family KIND:LO:HI")
if a.tasks is None:
    a.tasks = ("family" + (",uniform" if a.random_targets else "") if a.family else
               "bridge,fixed3,random3" + (",obst_fixed,obst_random" if a.random_obstacles else ""))
if a.steps < 100:
    sys.exit("--steps must be at least 100")

H = 0.8                                                       # bridge_setup(H=.8, num_stories=4), gym_env.py:36-46
TASKS = dict(bridge=([(0.5, 0.0, i * H + H / 2) for i in range(4)], [(0.5, 0.0, 4 * H + H / 2)]),
             fixed3=([], [(0.5, 0.0, 1.2), (-1.5, 0.0, 2.6), (2.5, 0.0, 0.4)]),
             random3=([], RandomTargets()))
if a.random_obstacles:
    O = a.random_obstacles
    TASKS["obst_fixed"] = ([(-3.0 + 6.0 * (o + 0.5) / O, 0.0, 0.3) for o in range(O)], TASKS["fixed3"][1])
    TASKS["obst_random"] = (RandomObstacles([((-3.0, 3.0), (0.3, 2.5))] * O), TASKS["fixed3"][1])
if a.random_targets:
    TASKS["uniform"] = (RandomObstacles([((-3.0, 3.0), (0.3, 2.5))] * a.random_obstacles) if a.random_obstacles else [],
                        RandomTargets(a.random_targets))
if a.family:
    kind, lo, hi = a.family.split(":")
    weights = [int(w) for w in a.family_weights.split(",")] if a.family_weights else None
    TASKS["family"] = ([], RandomBridges(kind, sizes=(int(lo), int(hi)), weights=weights))
geoms = [load_urdf("shapes/trapezoid.urdf")]
out = dict(tool="random_task_throughput", envs=a.envs, groups=a.groups, steps=a.steps, warmup=a.warmup, max_steps=a.max_steps,
           device=torch.cuda.get_device_name(0), family_weights=a.family_weights, tasks={})
for name in a.tasks.split(","):
    obstacles, targets = TASKS[name]
    env = VecAssemblyGymGroups(a.envs, geoms, obstacles, targets, groups=a.groups, max_steps=a.max_steps, seed=a.seed,
                               f32_rasters=True, candidate_snapshots=False)
    for _ in range(a.warmup):
        env.lockstep_random()
    env.sync()
    torch.cuda.synchronize()
    s0 = env.read_stats()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        env.lockstep_random()
    env.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s1 = env.read_stats()
    d = {k: s1[k] - s0[k] for k in s1}
    assert d["lp_errors"] == 0 and d["if_overflow"] == 0 and d["cand_overflow"] == 0, d
    states = a.steps * a.envs                                  # candidate sets produced: one per env and lock-step
    r = dict(env_steps_per_s=d["env_steps"] / dt, us_per_lockstep=1e6 * dt / a.steps, env_steps=d["env_steps"],
             reset_only=d["reset_only"], candidates_per_state=d["sum_cand"] / states,
             candidates_per_lockstep=d["sum_cand"] / a.steps, valid_per_state=d["sum_valid"] / states,
             blocks_per_state=d["sum_blocks"] / states)
    if name in ("random3", "obst_random", "uniform", "family"):
        ep = torch.cat([e.task_episode for e in env.envs]).double()
        r["episodes_per_env"] = float(ep.mean())               # since the reset: warm-up included
        r["tasks_drawn_per_lockstep"] = float(ep.sum()) / (a.steps + a.warmup)
    if name == "family":
        cls = torch.cat([e.task_class for e in env.envs])
        r["envs_by_class"] = torch.bincount(cls, minlength=int(hi) + 1).tolist()      # the tasks held at the end of the run
    out["tasks"][name] = r
    del env
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
