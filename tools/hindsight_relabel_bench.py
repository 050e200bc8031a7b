"""The hindsight relabelling launches on their own (bridges_hindsight_relabel through records.HindsightBuffer): a rollout env on
random targets under the synthetic random policy, the loop's buffer written every lock-step, and around the operator HIP events
-- alternating, in one process, between the call the loop makes (the envs whose episode ended in the lock-step) and the same
call with nothing ended (three launches that leave at once: the floor a lock-step without finished episodes pays).  The buffer
write (two indexed copies) is timed beside them.  Warm-up first; prints one JSON line with the medians and the spread.
    python tools/hindsight_relabel_bench.py [--envs 4096] [--random_targets 3] [--hindsight_goals 1] [--max_steps 15] [--reps 40]
The work of a call grows with the episodes that ended: ended_per_call and rows_per_call are printed beside the times.
--n_step n: in front of those calls, on the same buffers (the operator only reads them), the folding entry
(bridges_hindsight_relabel_nstep, gamma 0.95) and the one-step entry, alternating likewise: nstep_fold and one_step in the line.
--strategy per_step: on the same buffers again, the per-step entry (bridges_hindsight_per_step; with --n_step n its folding
sibling) on the envs that ended and with nothing ended, alternating with the "final" calls: per_step and per_step_nothing_ended in
the line, with the rows it emits per call and the cost per emitted row beside "final"'s cost per (episode, slot)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")]
import numpy as np
import torch
from bridges_hip.shapes import load_urdf
from bridges_hip.vec_env import RandomTargets, VecAssemblyGym
from bridges_hip import dqn_ops
from robotoddler.training import records as R

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--random_targets", type=int, default=3, metavar="T")
ap.add_argument("--hindsight_goals", type=int, default=1, metavar="G")
ap.add_argument("--max_steps", type=int, default=15)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--n_step", type=int, default=0, metavar="n", help="also time the folding entry at this n against the one-step entry")
ap.add_argument("--strategy", choices=("final", "per_step"), default="final",
                help="per_step: also time the per-step entry, alternating with the 'final' entry on the same buffers")
ap.add_argument("--warmup", type=int, default=20, help="lock-steps before the timed ones (episodes of every length are then in flight)")
a = ap.parse_args()
assert a.reps >= 20
dev = torch.device("cuda:0")
E, T = a.envs, a.random_targets
env = VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [], RandomTargets(T), max_steps=a.max_steps, seed=0, device=dev,
                     f32_rasters=False)
env.reset()
hb = R.HindsightBuffer(E, R.RECORD_WIDTH + 3 * T, dev, goals=a.hindsight_goals, n_blocks=env.K)
nothing = torch.zeros(E, dtype=torch.bool, device=dev)
if a.n_step:
    out_n = torch.empty((hb.out.shape[0], hb.out.shape[1] + 1), dtype=torch.float64, device=dev)
    count_n = torch.zeros(1, dtype=torch.int32, device=dev)
if a.strategy == "per_step":
    out_s = torch.empty((hb.out.shape[0], hb.out.shape[1] + bool(a.n_step)), dtype=torch.float64, device=dev)
    count_s = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch_s = torch.empty(dqn_ops.hindsight_relabel_scratch(E, hb.goals, "per_step"), dtype=torch.uint8, device=dev)


def per_step(ended):
    """The per-step entry on the buffer as it stands (nothing is emptied)."""
    kw = dict(n_step=a.n_step, gamma=0.95) if a.n_step else {}
    return dqn_ops.hindsight_relabel(env, hb.rows, hb.flags, hb.length, ended, hb.episode, hb.goals, out=out_s, count=count_s,
                                     scratch=scratch_s, strategy="per_step", **kw)


def entry(ended, fold):
    """One of the two entries on the buffer as it stands (nothing is emptied)."""
    kw = dict(out=out_n, count=count_n, n_step=a.n_step, gamma=0.95) if fold else dict(out=hb.out, count=hb.count)
    return dqn_ops.hindsight_relabel(env, hb.rows, hb.flags, hb.length, ended, hb.episode, hb.goals, scratch=hb._scratch, **kw)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3, out                      # us


times = dict(relabel=[], nothing_ended=[], buffer_write=[], **(dict(nstep_fold=[], one_step=[]) if a.n_step else {}),
             **(dict(per_step=[], per_step_nothing_ended=[]) if a.strategy == "per_step" else {}))
ended_n, rows_n, rows_s = [], [], []
for it in range(a.warmup + a.reps):
    env.select_random()
    rec = R.pack_state(env, env.cand_offset[:E].long() + env.buf["sel_index"].long())
    tail, episode = env.env_targets.reshape(E, -1).clone(), env.task_episode.clone()
    env.step()
    valid = R.pack_result(env, rec)
    ended = valid & (rec[:, R.O_DONE] > 0.5)
    full = torch.cat([rec, tail], dim=1)
    torch.cuda.synchronize()
    t_write, _ = timed(lambda: hb.write(full, env.step_flags, valid, episode))
    order = ("nothing_ended", "relabel") if it % 2 else ("relabel", "nothing_ended")
    got = {}
    for name in (("nstep_fold", "one_step") if it % 2 else ("one_step", "nstep_fold")) if a.n_step else ():
        got[name], _ = timed(lambda: entry(ended, name == "nstep_fold"))
    for name in (("per_step_nothing_ended", "per_step") if it % 2 else ("per_step", "per_step_nothing_ended")) if a.strategy == "per_step" else ():
        got[name], out = timed(lambda: per_step(ended if name == "per_step" else nothing))
        if name == "per_step":
            rows_step = int(out[1].item())
    for name in order:                                               # (the call with nothing ended leaves the buffer as it is)
        got[name], out = timed(lambda: hb.relabel(env, ended if name == "relabel" else nothing))
        if name == "relabel":
            rows = int(out[1].item())
    if it >= a.warmup:
        times["buffer_write"].append(t_write)
        for name, t in got.items():
            times[name].append(t)
        ended_n.append(int(ended.sum().item()))
        rows_n.append(rows)
        if a.strategy == "per_step":
            rows_s.append(rows_step)
summary = {}
for name, t in times.items():
    t = np.array(t)
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    summary[name] = dict(median_us=float(med), min_us=float(t.min()), max_us=float(t.max()), iqr_us=float(q3 - q1), calls=len(t))
if a.strategy == "per_step":
    work = summary["per_step"]["median_us"] - summary["per_step_nothing_ended"]["median_us"]
    final = summary["relabel"]["median_us"] - summary["nothing_ended"]["median_us"]
    summary.update(rows_per_call_per_step=float(np.mean(rows_s)), us_per_row_per_step=work / max(np.mean(rows_s), 1e-9),
                   us_per_episode_slot_final=final / max(np.mean(ended_n) * hb.goals, 1e-9))
if a.n_step:
    summary["nstep_minus_one_step_us"] = summary["nstep_fold"]["median_us"] - summary["one_step"]["median_us"]
print(json.dumps(dict(config=vars(a), **summary, ended_per_call=float(np.mean(ended_n)), rows_per_call=float(np.mean(rows_n)),
                      us_per_ended_episode=(summary["relabel"]["median_us"] - summary["nothing_ended"]["median_us"]) / max(np.mean(ended_n), 1e-9),
                      note="HIP events around single calls (host launch gaps included), the two calls alternating in one process; "
                           "relabel: the three launches on the envs whose episode ended; nothing_ended: the same launches, all leaving at once")),
      flush=True)
