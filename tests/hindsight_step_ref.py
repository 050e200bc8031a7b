"""Reference of hindsight relabelling with per-step goals (VecDQN(hindsight="per_step"), bridges_hindsight_per_step and
bridges_hindsight_per_step_nstep, the rule in include/bridges_hip.h): hindsight experience replay's "future" strategy -- every
transition of a finished episode gets goals that the episode achieves from that transition onward.  Test infrastructure, not a
test module: nothing here needs a GPU.  The draw hash, the geometry of a record, the reached-test, the tasks and the probes are
tests/hindsight_ref.py's; tests/test_cpu_hindsight_step.py checks the statement against the oracle env and against the
deliberately defective twins below, tests/test_gpu_hindsight_step.py compares the kernels with it bit for bit.

One work item is (env, slot g, step t < m'); it emits at most one row.
  draw     h2 as hindsight_ref.hind_draw's; h3 = splitmix64(h2 ^ ((t + 1) << 8)); r_i = splitmix64(h3 ^ i); u_i = r_i >> 32
  future   f = t + ((u_0 * (m' - t)) >> 32)
  goals    n = f + 1, idx = 0 .. n - 1, swap(idx[0], idx[f]); i = 1 .. min(T, n) - 1: swap(idx[i], idx[i + ((u_i * (n - i)) >> 32)]);
           target q = box centre of block idx[q mod n]
  exists   the reached-test of steps 0 .. t - 1 under these targets leaves a target open
  row      record t (fold: record last) under these targets, as hindsight_ref.relabel_episode writes a row
"""
import numpy as np

import hindsight_ref as H
from hindsight_ref import (F_NO_ACTIONS, F_STABLE_FROZEN, F_STABLE_UNFROZEN, F_TRUNCATED, HIND_SALT, DeviceTask, OracleTask,  # noqa: F401
                           PROBE_BASE, PROBE_CONFIGS, PROBE_SEED, block_of, box_centre, cached_device_task, eligible, lin_rule, probe,
                           probe_seed, reach)
from oracle.env import M64, splitmix64
from robotoddler.training import records as R

TWINS = ("future_from_zero", "no_step_key", "future_not_forced", "fresh_mask", "row_after_end", "row_of_collapse",
         "window_past_end", "start_of_last", "open_end_dropped")
FOLD_TWINS = TWINS[6:]
CASES = ("no_eligible", "collapse_no_row", "over_before_t", "future_is_t", "future_is_last", "repeated_targets", "done_at_t",
         "nothing_reached_at_t", "quirk", "truncated_last")


def step_draw(seed, env_id, episode, slot, t, i, twin=None):
    """Uniform u64 for (seed, global env id, task_episode, slot, step t, draw index i): the "hind_rng" stream with one more key."""
    h0 = splitmix64(((((seed & 0xFFFFFFFF) << 32) | (env_id & 0xFFFFFFFF)) ^ HIND_SALT) & M64)
    h1 = splitmix64(h0 ^ (episode & 0xFFFFFFFF))
    h2 = splitmix64(h1 ^ (slot & M64))
    h3 = h2 if twin == "no_step_key" else splitmix64(h2 ^ (((t + 1) << 8) & M64))
    return splitmix64(h3 ^ (i & M64))


def choose_step_blocks(seed, env_id, episode, slot, t, n_eligible, n_targets, twin=None):
    """-> (f, the block of every target): integers only."""
    mp, T = int(n_eligible), int(n_targets)
    assert 0 <= t < mp
    u0 = step_draw(seed, env_id, episode, slot, t, 0, twin) >> 32
    f = ((u0 * mp) >> 32) if twin == "future_from_zero" else t + ((u0 * (mp - t)) >> 32)
    n = f + 1
    idx = list(range(n))
    first = 1
    if twin == "future_not_forced":
        first = 0
    else:
        idx[0], idx[f] = idx[f], idx[0]
    for i in range(first, min(T, n)):
        u = step_draw(seed, env_id, episode, slot, t, i, twin) >> 32
        j = i + ((u * (n - i)) >> 32)
        idx[i], idx[j] = idx[j], idx[i]
    return f, [idx[q % n] for q in range(T)]


def step_goals(rows, shapes, seed, env_id, episode, slot, t, n_targets, twin=None):
    """-> (targets [(x, 0, z)] * T, f, picks) of step t < m'."""
    f, picks = choose_step_blocks(seed, env_id, episode, slot, t, eligible(rows), n_targets, twin)
    return [box_centre(block_of(rows[b], shapes)) for b in picks], f, picks


def _relabelled(row, flag, block, left, targets, task, T):
    """Record ``row`` as the env would have written it under ``targets`` with ``left`` open after its step
    (hindsight_ref.relabel_episode's expressions)."""
    st_frozen, st_free = bool(flag[F_STABLE_FROZEN]), bool(flag[F_STABLE_UNFROZEN])
    truncated, no_actions = bool(flag[F_TRUNCATED]), bool(flag[F_NO_ACTIONS])
    n_reached, all_reached = T - bin(left).count("1"), left == 0
    row = np.array(row, dtype=np.float64)
    row[R.O_REWARD] = -1.0 if not st_frozen else float(n_reached if all_reached else -1 + n_reached)
    row[R.O_LIN] = float(lin_rule(task.base(block), st_free, st_frozen))
    row[R.O_DONE] = 1.0 if (not st_frozen or all_reached or truncated or no_actions) else 0.0
    row[R.RECORD_WIDTH:R.RECORD_WIDTH + 3 * T] = np.asarray(targets, dtype=np.float64).reshape(-1)
    return row


def relabel_step(rows, flags, shapes, seed, env_id, episode, slot, t, n_targets, n_step=None, gamma=None, task_cls=DeviceTask,
                 twin=None, trace=None):
    """The row of work item (slot, t) of one finished episode (rows [m, W], flags [m, 8]), or None.  ``n_step`` None: the
    one-step row [W]; else the h-step row [W + 1].  ``trace``: a dict that receives targets, f, picks, left_before, left_after
    (of step t), h, last."""
    rows = np.asarray(rows, dtype=np.float64)
    m, T = len(rows), int(n_targets)
    mp = eligible(rows)
    if t >= mp and not (twin == "row_of_collapse" and t < m and mp > 0):
        return None
    tt = min(t, mp - 1)                                            # (the twin's collapsed step draws as step m' - 1 would)
    targets, f, picks = step_goals(rows, shapes, seed, env_id, episode, slot, tt, T, twin)
    left = (1 << T) - 1
    if twin != "fresh_mask":
        for s in range(t):
            left = reach(left, targets, block_of(rows[s], shapes))
    if left == 0:
        if twin != "row_after_end":
            return None
    task = cached_device_task(targets) if task_cls is DeviceTask else task_cls(targets)
    before = left
    if n_step is None:
        block = block_of(rows[t], shapes)
        left = reach(left, targets, block)
        if trace is not None:
            trace.update(targets=targets, f=f, picks=picks, left_before=before, left_after=left, h=1, last=t)
        return _relabelled(rows[t], flags[t], block, left, targets, task, T)
    # the walk under goals(t): from t to the first step that leaves no target open, else to m - 1 (a collapsed last step included)
    n, gamma = int(n_step), np.float64(gamma)
    lefts, end = [], m - 1
    for s in range(t, m):
        left = reach(left, targets, block_of(rows[s], shapes))
        lefts.append(left)
        if left == 0 and twin != "window_past_end":
            end = s
            break
    h = min(n, end - t + 1)
    if twin == "open_end_dropped" and h < n and not _relabelled(rows[end], flags[end], block_of(rows[end], shapes), lefts[end - t],
                                                                targets, task, T)[R.O_DONE] > 0.5:
        return None
    last = t + h - 1
    acc, disc = np.float64(0.0), np.float64(1.0)
    for k in range(h):
        r_k = _relabelled(rows[t + k], flags[t + k], block_of(rows[t + k], shapes), lefts[k], targets, task, T)
        acc = acc + disc * r_k[R.O_LIN]
        disc = disc * gamma
    out = np.empty(rows.shape[1] + 1)
    out[:-1] = r_k
    out[R.O_LIN] = acc
    src = last if twin == "start_of_last" else t
    out[R.O_STABLE_S], out[R.O_TD] = rows[src, R.O_STABLE_S], rows[src, R.O_TD]
    out[-1] = float(h)
    if trace is not None:
        trace.update(targets=targets, f=f, picks=picks, left_before=before, left_after=lefts[0], h=h, last=last)
    return out


def relabel(buf, flags, length, ended, episode, shapes, seed, env_id_base, n_goals, n_targets, n_step=None, gamma=None,
            task_cls=DeviceTask, twin=None, trace=None):
    """The operator: buf [E, K, W], flags [E, K, 8], length [E], ended [E], episode [E] -> rows [count, W] (n_step None) or
    [count, W + 1], env ascending, then slot, then step.  ``trace``: a list that receives (env, slot, t, dict) of every row."""
    buf = np.asarray(buf, dtype=np.float64)
    wout = buf.shape[2] + (0 if n_step is None else 1)
    out = []
    for e in range(buf.shape[0]):
        m = int(length[e])
        if not ended[e] or m <= 0:
            continue
        for g in range(int(n_goals)):
            for t in range(m):
                tr = {}
                row = relabel_step(buf[e, :m], np.asarray(flags)[e, :m], shapes, seed, env_id_base + e, int(episode[e]), g, t,
                                   n_targets, n_step=n_step, gamma=gamma, task_cls=task_cls, twin=twin, trace=tr)
                if row is None:
                    continue
                out.append(row)
                if trace is not None:
                    trace.append((e, g, t, tr))
    return np.stack(out) if out else np.zeros((0, wout))


def census(p, seed, env_id_base, G):
    """Which CASES the probe p holds under (seed, env_id_base, G slots), by the restatement itself (no tasks are built)."""
    seen = set()
    T = p["T"]
    for e in range(len(p["length"])):
        m = int(p["length"][e])
        if not p["ended"][e] or m <= 0:
            continue
        rows, fl = p["buf"][e, :m], p["flags"][e, :m]
        mp = eligible(rows)
        seen |= {"no_eligible"} if mp == 0 else set()
        seen |= {"collapse_no_row"} if 0 < mp < m else set()
        for g in range(G):
            for t in range(mp):
                targets, f, _ = step_goals(rows, p["shapes"], seed, env_id_base + e, int(p["episode"][e]), g, t, T)
                left = (1 << T) - 1
                for s in range(t):
                    left = reach(left, targets, block_of(rows[s], p["shapes"]))
                if left == 0:
                    seen.add("over_before_t")
                    continue
                block = block_of(rows[t], p["shapes"])
                after = reach(left, targets, block)
                inside = sum(1 << k for k in range(T) if (left >> k) & 1 and block.aabb_contains(targets[k]))
                seen |= {"quirk"} if after & inside else set()
                seen |= {"future_is_t"} if f == t else set()
                seen |= {"future_is_last"} if f == mp - 1 and f > t else set()
                seen |= {"repeated_targets"} if f + 1 < T else set()
                seen |= {"done_at_t"} if after == 0 else set()
                seen |= {"nothing_reached_at_t"} if after == left else set()
                seen |= {"truncated_last"} if t == m - 1 and fl[t][F_TRUNCATED] else set()
    return seen
