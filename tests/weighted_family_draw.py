"""Python restatement of the weighted task-family draw and of the curriculum update (include/bridges_hip.h,
bridges_env_set_family_thresholds / bridges_family_thresholds / bridges_family_curriculum), beside tests/family_draw.py, whose
word and uniform draw it builds on.  Test infrastructure: the tests compare the device's classes, weights, tables and state with
these numbers exactly.  Integers are Python ints (exact); the curriculum's float64 steps are Python floats, one operation per
expression, so every operation is rounded to binary64 on its own."""
from family_draw import family_word

MAX_CLASSES = 8
MAX_WEIGHT = 1 << 20
FAIL_SCALE = 65536.0


def thresholds(weights):
    """thr[k] = ceil((w[0] + .. + w[k]) * 2^32 / sum(w)), k = 0..C-2.  As the device builds it: a weight above 2^20 counts as
    2^20, and a zero sum gives the table of equal weights."""
    ws = [min(int(w), MAX_WEIGHT) for w in weights]
    assert 1 <= len(ws) <= MAX_CLASSES and all(w >= 0 for w in ws)
    total = sum(ws)
    if total == 0:
        ws, total = [1] * len(ws), len(ws)
    out, cum = [], 0
    for w in ws[:-1]:
        cum += w
        out.append(((cum << 32) + total - 1) // total)
    return out


def class_of(u, lo, thr):
    """n = lo + #{k : u >= thr[k]} for u = the high 32 bits of the family's word."""
    return lo + sum(1 for t in thr if u >= t)


def weighted_family_draw(seed, env_id, episode, lo, hi, thr=None):
    """n in [lo, hi] of (seed, global env id, episode): by the table thr [hi - lo], or -- thr None -- the uniform draw."""
    u = family_word(seed, env_id, episode) >> 32
    if thr is None:
        return lo + ((u * (hi - lo + 1)) >> 32)
    assert len(thr) == hi - lo
    return class_of(u, lo, thr)


def curriculum_update(sums, state, lo, hi, beta, w_min, min_episodes):
    """One bridges_family_curriculum: sums [n_classes][8] and state [n_classes][2] (lists of lists of floats) are updated in
    place; -> (w [C], thr [C-1])."""
    w = []
    for n in range(lo, hi + 1):
        ema, seen = state[n][0], state[n][1] != 0.0
        e = sums[n][0]
        if e >= float(min_episodes):
            rate = sums[n][5] / e
            if seen:
                d = rate - ema
                d = beta * d
                ema = ema + d
            else:
                ema = rate
            seen = True
            state[n][0], state[n][1] = ema, 1.0
            sums[n][:] = [0.0] * 8
        fail = 1.0
        if seen:
            fail = 1.0 - ema
            fail = fail if fail > 0.0 else 0.0
            fail = fail if fail < 1.0 else 1.0
        x = fail * FAIL_SCALE
        x = x + 0.5
        w.append(w_min + int(x))
    return w, thresholds(w)
