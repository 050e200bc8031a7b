"""Reference of hindsight relabelling under n-step returns (VecDQN(hindsight="final", hindsight_fold=True, n_step=n),
bridges_hindsight_relabel_nstep, the rule in include/bridges_hip.h): the relabelled walk of tests/hindsight_ref.py per (env, slot),
then one h-step row per start of the walk -- numpy float64, the return in the order the header states.  Test infrastructure, not a
test module: nothing here needs a GPU.  tests/test_cpu_hindsight_nstep.py checks the statement against the window reference of
tests/nstep_ref.py and against the deliberately defective twins below; tests/test_gpu_hindsight_nstep.py compares the kernel with
it bit for bit."""
import numpy as np

import hindsight_ref as H
from robotoddler.training import records as R

TWINS = ("done_only_flush", "td_of_last", "stable_s_of_last", "disc_after", "h_uncapped", "lin_of_original", "order_by_last")
CASES = ("short", "exact", "long", "open_end", "done_end", "open_long", "full")


def fold_walk(rows, n, gamma, twin=None, original_lin=None):
    """rows [L, W]: the one-step rows r_0 .. r_{L-1} of one relabelled walk -> [L, W + 1], one row per start t, ascending:
    h = min(n, L - t), last = t + h - 1; r_last with O_LIN = acc (acc = 0, disc = 1; k < h: acc += disc * lin(r_{t+k});
    disc *= gamma -- float64, product and sum rounded separately), O_STABLE_S and O_TD of r_t, and h in column W.  The end of the
    walk flushes every pending start whether or not r_{L-1} has O_DONE.
    ``twin``: one of TWINS --
      done_only_flush   the pending starts of a walk whose last row is not done are dropped (bridges_nstep_fold's flush);
      td_of_last / stable_s_of_last   the column of r_last instead of the start's;
      disc_after        disc *= gamma before the product;
      h_uncapped        column W = n in the tail of the walk;
      lin_of_original   the return folded from ``original_lin`` [L] (the rollout's O_LIN) instead of the relabelled one;
      order_by_last     the rows in the order of the step that stores them, the starts of the final flush newest first."""
    rows = np.asarray(rows, dtype=np.float64)
    L, W = rows.shape
    n, gamma = int(n), np.float64(gamma)
    lin = np.asarray(original_lin, dtype=np.float64) if twin == "lin_of_original" else rows[:, R.O_LIN]
    out, keys = [], []
    for t in range(L):
        h = min(n, L - t)
        last = t + h - 1
        if twin == "done_only_flush" and h < n and not rows[L - 1, R.O_DONE] > 0.5:
            continue
        acc, disc = np.float64(0.0), np.float64(1.0)
        for k in range(h):
            if twin == "disc_after":
                disc = disc * gamma
                acc = acc + disc * lin[t + k]
            else:
                acc = acc + disc * lin[t + k]
                disc = disc * gamma
        row = np.empty(W + 1)
        row[:W] = rows[last]
        row[R.O_LIN] = acc
        row[R.O_STABLE_S] = rows[last if twin == "stable_s_of_last" else t, R.O_STABLE_S]
        row[R.O_TD] = rows[last if twin == "td_of_last" else t, R.O_TD]
        row[W] = float(n if twin == "h_uncapped" else h)
        out.append(row)
        keys.append((last, -t))
    if twin == "order_by_last":
        out = [out[i] for i in sorted(range(len(out)), key=lambda i: keys[i])]
    return np.stack(out) if out else np.zeros((0, W + 1))


def walks(buf, flags, length, ended, episode, shapes, seed, env_id_base, n_goals, n_targets, task_cls=H.DeviceTask):
    """The relabelled walks of the operator's inputs -> [(env, slot, rows [L, W]), ...] in output order: hindsight_ref.relabel's
    rows, cut by its trace."""
    trace = []
    flat = H.relabel(buf, flags, length, ended, episode, shapes, seed, env_id_base, n_goals, n_targets, task_cls=task_cls, trace=trace)
    out, at = [], 0
    for e, g, _targets, _picks, lefts in trace:
        out.append((e, g, flat[at:at + len(lefts)]))
        at += len(lefts)
    assert at == len(flat)
    return out


def fold_walks(ws, buf, n, gamma, twin=None):
    """The operator's output from walks(): every walk folded, concatenated -> [count, W + 1]."""
    W = np.asarray(buf).shape[2]
    parts = [np.zeros((0, W + 1))]
    for e, _g, rows in ws:
        parts.append(fold_walk(rows, n, gamma, twin=twin, original_lin=np.asarray(buf)[e, :len(rows), R.O_LIN]))
    return np.concatenate(parts, axis=0)


def relabel_nstep(buf, flags, length, ended, episode, shapes, seed, env_id_base, n_goals, n_targets, n, gamma, task_cls=H.DeviceTask,
                  twin=None):
    """The operator: the arguments of hindsight_ref.relabel, then n and gamma -> rows [count, W + 1], env ascending, then slot,
    then start."""
    ws = walks(buf, flags, length, ended, episode, shapes, seed, env_id_base, n_goals, n_targets, task_cls=task_cls)
    return fold_walks(ws, buf, n, gamma, twin=twin)


def census(ws, n, K):
    """Which CASES the walks hold for a window of n (K: the block slots of the buffer)."""
    seen = set()
    for _e, _g, rows in ws:
        L, done = len(rows), rows[-1, R.O_DONE] > 0.5
        seen |= {"short"} if L < n else set()
        seen |= {"exact"} if L == n else set()
        seen |= {"long"} if L > n else set()
        seen |= {"open_end"} if not done and L >= 2 else set()
        seen |= {"done_end"} if done else set()
        seen |= {"open_long"} if not done and L >= 2 and L > n else set()
        seen |= {"full"} if L == K else set()
    return seen
