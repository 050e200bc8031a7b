"""CPU: the references of tests/vec_dqn_oracle.py -- the ring order, the n-step fold and reference_targets on a hand-made three-env
trace whose numbers are written out here, the acceptance rule, the undecided rule, and the evidence that each of the eight
defective twins of the reference is rejected.  The oracle track itself runs one oracle-only rollout and its own record rows."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vec_dqn_oracle as V
from robotoddler.training import records as R

GAMMA = 0.5
P = [np.array(m, dtype=bool).reshape(2, 2) for m in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))]      # one pixel each
MAP_A = np.array([[1, 2], [4, 8]], dtype=np.float32)
MAP_B = np.array([[8, 4], [2, 1]], dtype=np.float32)
NONE = np.zeros((2, 2), dtype=bool)


class HandNet(torch.nn.Module):
    """q = scale (sum(action * reward) + binary_0 / 2 + sum(block) / 4), psi_0 = scale (block + 2 action): sums of a few dyadic
    numbers, exact in float32 and float64 alike."""

    def __init__(self, scale):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(float(scale)))

    def forward(self, block, binary, action, reward, obstacle):
        q = self.scale * ((action * reward).sum(dim=(1, 2, 3)) + binary[:, 0] / 2 + block.sum(dim=(1, 2, 3)) / 4)
        psi = self.scale * (block + 2 * action)
        return q, torch.cat([psi, -psi], dim=1), None


def step(env, t, state, action, lin, stable_s, stable_frozen, done=False, no_actions=False, nxt=None, reward_map=MAP_A):
    tr = dict(env=env, t=t, state=state, action_raster=action, lin=np.float32(lin), stable_s=stable_s, stable_frozen=stable_frozen,
              done=done, no_actions=no_actions, reward_map=reward_map, obstacle_raster=NONE)
    if nxt is not None:
        tr["next_state"], tr["next_rasters"] = nxt[0], np.stack(nxt[1])
    return tr


def hand_trace():
    """Three envs, three lock-steps (steps in ring order: lock-step major, env minor):
      env 0 runs one episode: 0 (t 0), 3 (t 1), 5 (t 2), all bootstrapping; stable(s') of step 0 is False;
      env 1: 1 (t 0) leads to a state without a valid candidate (no_actions, not done), t 1 is reset-only, 6 (t 2) bootstraps;
      env 2: 2 (t 0, map A, bootstraps), 4 (t 1, done; the state it would have led to is kept for the twin that bootstraps anyway),
             then a new episode on map B: 7 (t 2)."""
    s = [None] * 8
    s[0] = step(0, 0, NONE, P[0], 1.0, True, False, nxt=(P[0], [P[1], P[2]]))
    s[1] = step(1, 0, NONE, P[3], 0.5, True, True, no_actions=True)
    s[2] = step(2, 0, NONE, P[1], 2.0, True, True, nxt=(P[1], [P[0], P[2]]))
    s[3] = step(0, 1, P[0], P[1], 2.0, False, True, nxt=(P[0] | P[1], [P[2], P[3]]))
    s[4] = step(2, 1, P[1], P[0], 1.0, True, False, done=True, nxt=(P[0] | P[1], [P[2]]))
    s[5] = step(0, 2, P[0] | P[1], P[3], 8.0, True, True, nxt=(P[0] | P[1] | P[3], [P[2]]))
    s[6] = step(1, 2, NONE, P[2], 4.0, True, True, nxt=(P[2], [P[0], P[1], P[3]]))
    s[7] = step(2, 2, NONE, P[0], 8.0, True, True, nxt=(P[0], [P[1], P[2]]), reward_map=MAP_B)
    grid = [[0, 1, 2], [3, None, 4], [5, 6, 7]]
    return SimpleNamespace(E=3, steps=s, grid=grid)


def nets(dtype):
    return HandNet(2.0).to(dtype), HandNet(-1.0).to(dtype)          # (target, policy): the policy net's maximum is the target net's minimum


def evaluate(n_step, double_q, dtype=torch.float64, **kw):
    track = hand_trace()
    rows = V.ring_rows(track, n_step)
    tgt, pol = nets(dtype)
    return rows, V.reference_targets(track, rows, tgt, pol, GAMMA, n_step, double_q, True, **kw)


def test_ring_order_and_windows():
    track = hand_trace()
    assert [r["window"] for r in V.ring_rows(track, 1)] == [[i] for i in range(8)]
    # t 0: env 1's episode ends; t 1: env 0's window is full, env 2's episode ends with two pending starts; t 2: env 0's again
    assert [r["window"] for r in V.ring_rows(track, 2)] == [[1], [0, 3], [2, 4], [4], [3, 5]]
    assert [r["h"] for r in V.ring_rows(track, 2)] == [1, 2, 2, 1, 2]
    assert [r["window"] for r in V.ring_rows(track, 3)] == [[1], [2, 4], [4], [0, 3, 5]]


def test_fold_return():
    G, bound = V.fold_return([np.float32(1.0), np.float32(2.0), np.float32(8.0)], 0.5)
    assert G == 1.0 + 1.0 + 2.0 and bound == 6 * 2.0 ** -53 * 4.0
    G, bound = V.fold_return([np.float32(0.1)], 0.95)
    assert G == float(np.float32(0.1)) and bound == 2 * 2.0 ** -53 * G
    lins = [np.float32(v) for v in (0.3, -0.7, 0.11)]
    G, _ = V.fold_return(lins, 0.95)
    assert abs(G - (float(lins[0]) + 0.95 * float(lins[1]) + 0.95 ** 2 * float(lins[2]))) <= 4 * 2.0 ** -53


def test_reference_targets_on_the_hand_made_trace():
    """n_step = 2, rows [1], [0, 3], [2, 4], [4], [3, 5]; gamma = 1/2, the target net's scale 2.
    [1]: no valid candidate follows: q = 0.5, sf = P3.
    [0, 3]: G = 1 + 2/2 = 2; s' = P0|P1 (2 pixels), stable; q' = 2 (4 + 1/2 + 2/4) = 10 for P2 and 2 (8 + 1) = 18 for P3:
            q = 2 + 18/4 = 6.5, psi'_0 = 2 (s' + 2 P3) = (2, 2, 0, 4), sf = (1, 1/2, 0, 0) + psi'_0 / 4 = (1.5, 1, 0, 1).
    [2, 4]: done: q = G = 2 + 1/2, sf = P1 + P0 / 2.     [4]: q = 1, sf = P0.
    [3, 5]: G = 2 + 8/2 = 6; s' has 3 pixels, one candidate P2: q' = 2 (4 + 1/2 + 3/4) = 10.5, q = 6 + 10.5/4 = 8.625,
            psi'_0 = 2 (s' + 2 P2) = (2, 2, 4, 2), sf = (0, 1, 0, 1/2) + psi'_0 / 4 = (0.5, 1.5, 1, 1)."""
    rows, ref = evaluate(2, False)
    assert ref["q"].tolist() == [0.5, 6.5, 2.5, 1.0, 8.625]
    assert ref["sf"].tolist() == [[0, 0, 0, 1], [1.5, 1, 0, 1], [0.5, 1, 0, 0], [1, 0, 0, 0], [0.5, 1.5, 1, 1]]
    assert ref["boot"].tolist() == [False, True, False, False, True]
    assert ref["best"] == [None, 1, None, None, 0] and ref["second"] == [None, 0, None, None, None]
    assert ref["gap"].tolist() == [math.inf, 8.0, math.inf, math.inf, math.inf]
    assert ref["binary"][:, 0].tolist() == [1, 1, 1, 1, 0] and not ref["binary"][:, 1:].any()        # stable(s) of the START
    assert [b.reshape(-1).tolist() for b in ref["block"]] == [[0] * 4, [0] * 4, [0] * 4, [0, 1, 0, 0], [1, 0, 0, 0]]
    assert [a.reshape(-1).tolist() for a in ref["action"]] == [[0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]]
    assert ref["sf_second"][1].tolist() == [1.5, 1, 1, 0]                      # (1, 1/2, 0, 0) + 2 (s' + 2 P2) / 4
    # double Q-learning: the policy net (scale -1) selects P2 in [0, 3]; value and psi' stay the target net's: q = 2 + 10/4
    _, dq = evaluate(2, True)
    assert dq["q"].tolist() == [0.5, 4.5, 2.5, 1.0, 8.625] and dq["best"][1] == 0 and dq["sf"][1].tolist() == [1.5, 1, 1, 0]
    assert dq["q_second"][1] == 6.5
    # n_step = 1: step 2 on map A: q' = 2 (1 + 1/2 + 1/4) = 3.5 for P0 and 2 (4 + 3/4) = 9.5 for P2: q = 2 + 9.5/2;
    # step 7 on map B: s' = P0, q' = 2 (4 + 3/4) = 9.5 for P1, 2 (2 + 3/4) = 5.5 for P2: q = 8 + 9.5/2; step 4 is done: q = 1
    _, one = evaluate(1, False)
    assert one["q"][2] == 6.75 and one["q"][7] == 12.75 and one["q"][4] == 1.0 and one["q"][1] == 0.5
    assert torch.equal(one["map"][7], torch.as_tensor(MAP_B).double()) and torch.equal(one["map"][2], torch.as_tensor(MAP_A).double())
    # the float32 evaluation of these dyadic numbers is the same numbers, and it is accepted with nothing but the floor
    rows, ref = evaluate(2, False)
    _, lib = evaluate(2, False, dtype=torch.float32, pick=list(zip(ref["best"], ref["second"])))
    assert torch.equal(lib["q"], ref["q"]) and torch.equal(lib["sf"], ref["sf"])
    und = V.undecided(ref, lib)
    assert not und.any()
    ok, worst, failed = V.conforms(dict(q=lib["q"], sf=lib["sf"], block=lib["block"], action=lib["action"], binary=lib["binary"]), ref, lib, und)
    assert ok and worst == 0.0 and failed == []


# the configuration at which each defect shows on the hand-made trace, and where
TWIN_AT = dict(done_without_no_actions=(2, False, "row [1]: a maximum over no candidate"),
               bootstrap_kept_when_done=(2, False, "row [4]: q = 1 + 9/2"),
               gamma_h_minus_1=(2, False, "rows [0, 3] and [3, 5]"),
               binary_of_next_state=(2, False, "row [0, 3]: stable(s') of step 0 is False"),
               double_q_policy_value=(2, True, "row [0, 3]: the policy net's -5"),
               action_of_last_step=(2, False, "row [0, 3]: P1 for P0"),
               current_task_map=(1, False, "step 2 under map B"),
               candidate_dropped=(2, False, "row [0, 3]: P3, the maximum, is the last candidate"))


@pytest.mark.parametrize("twin", V.TWINS)
def test_each_defective_twin_is_rejected(twin):
    n_step, double_q, _where = TWIN_AT[twin]
    rows, ref = evaluate(n_step, double_q)
    pick = list(zip(ref["best"], ref["second"]))
    _, lib = evaluate(n_step, double_q, dtype=torch.float32, pick=pick)
    und = V.undecided(ref, lib)
    _, bad = evaluate(n_step, double_q, dtype=torch.float32, twin=twin)
    ok, worst, failed = V.conforms({k: bad[k] for k in ("q", "sf", "block", "action", "binary")}, ref, lib, und, double_q=double_q)
    assert not ok and failed, twin
    # and the twin is the only difference: without it the same evaluation passes
    _, good = evaluate(n_step, double_q, dtype=torch.float32)
    assert V.conforms({k: good[k] for k in ("q", "sf", "block", "action", "binary")}, ref, lib, und, double_q=double_q)[0]


def test_twin_table_is_complete():
    assert set(TWIN_AT) == set(V.TWINS) and len(V.TWINS) == 8


def test_accept_rule():
    ref = torch.tensor([1.0, -2.0, 4.0], dtype=torch.float64)
    lib = ref + torch.tensor([1e-6, 0.0, -2e-6], dtype=torch.float64)
    floor = 32 * V.U32 * 4.0
    ok, share = V.accept(ref + 0.999 * (4 * 2e-6 + floor), ref, lib)
    assert ok and abs(share - 0.999) < 1e-6
    assert not V.accept(ref + 1.001 * (4 * 2e-6 + floor), ref, lib)[0]
    assert V.accept(ref, ref, ref) == (True, 0.0)
    assert not V.accept(torch.tensor([1.0, math.nan, 4.0]), ref, lib)[0]
    inf = torch.tensor([1.0, -math.inf], dtype=torch.float64)
    assert V.accept(inf, inf, inf)[0] and not V.accept(torch.tensor([1.0, 5.0]), inf, inf)[0]


def test_undecided_rows_may_follow_either_row_and_the_cap_counts_them():
    """Two bootstrapping rows with a runner-up: the first 1e-7 ahead under a measured |q32 - q64| of 1e-6 (undecided), the second 1.0
    ahead (decided).  The undecided row's sf may be the runner-up's, the decided row's may not; the plain q is checked either way."""
    q64 = [torch.tensor([1.0, 1.0 - 1e-7], dtype=torch.float64), torch.tensor([2.0, 1.0], dtype=torch.float64)]
    q32 = [q + 1e-6 * torch.tensor([1.0, -1.0], dtype=torch.float64) for q in q64]
    sf, sf2 = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64), torch.tensor([[5.0, 6.0], [7.0, 8.0]], dtype=torch.float64)
    ref = dict(q=torch.tensor([1.0, 2.0], dtype=torch.float64), q_second=torch.tensor([1.0, 2.0], dtype=torch.float64), sf=sf, sf_second=sf2,
               gap=torch.tensor([1e-7, 1.0], dtype=torch.float64), boot=torch.tensor([True, True]), best=[0, 0], second=[1, 1], qsel=q64,
               block=torch.zeros(2, 1, 1, dtype=torch.float64), action=torch.zeros(2, 1, 1, dtype=torch.float64), binary=torch.zeros(2, 6, dtype=torch.float64))
    lib = dict(ref, qsel=q32)
    und = V.undecided(ref, lib)
    assert und.tolist() == [True, False]
    base = dict(q=ref["q"], block=ref["block"], action=ref["action"], binary=ref["binary"])
    assert V.conforms(dict(base, sf=torch.stack([sf2[0], sf[1]])), ref, lib, und)[0]
    assert not V.conforms(dict(base, sf=torch.stack([sf[0], sf2[1]])), ref, lib, und)[0]
    assert not V.conforms(dict(base, sf=sf, q=ref["q"] + torch.tensor([1e-3, 0.0], dtype=torch.float64)), ref, lib, und)[0]
    with pytest.raises(AssertionError, match="undecided"):
        V.check_cap(ref, und)                                                  # 1 of 2 is above 10 %
    many = dict(ref, boot=torch.ones(40, dtype=torch.bool))
    assert V.check_cap(many, torch.zeros(40, dtype=torch.bool)) == (40, 0)
    with pytest.raises(AssertionError, match="decided"):
        V.check_cap(dict(ref, boot=torch.ones(29, dtype=torch.bool)), torch.zeros(29, dtype=torch.bool))


def record_row(tr):
    row = np.zeros(R.RECORD_WIDTH)
    row[R.O_ATB], row[R.O_ATF], row[R.O_ASHAPE], row[R.O_AFACE] = tr["action"][:4]
    row[R.O_APOSE:R.O_APOSE + 4] = tr["action_pose"]
    return row


def test_oracle_track_follows_recorded_actions_and_keeps_the_oracle_s_numbers():
    """An oracle-only rollout of case a (6 envs, 10 lock-steps, max_steps 4), replayed through advance() from record rows built of
    its own actions: the same transitions; one valid candidate matches each row, a row with another pose matches none; stable(s)
    is 1 on a fresh env and the previous frozen verdict otherwise; a bootstrapping transition holds s' and its valid candidates."""
    cfg = V.CASES["a"]
    free = V.OracleTrack(V.gym_factory(cfg["task"]), cfg["E"])
    rng = np.random.default_rng(1)
    for _ in range(cfg["locksteps"]):
        free.advance_random(rng)
    led = V.OracleTrack(V.gym_factory(cfg["task"]), cfg["E"])
    for row in free.grid:
        rec = np.stack([record_row(free.steps[i]) if i is not None else np.zeros(R.RECORD_WIDTH) for i in row])
        valid = np.array([i is not None for i in row])
        if valid.any():
            e = int(np.flatnonzero(valid)[0])
            wrong = rec[e].copy()
            wrong[R.O_APOSE] += 1e-9
            with pytest.raises(AssertionError, match="matches 0"):
                led.match(led.oracles[e], wrong)
        assert led.advance(rec, valid) == row
    assert len(led.steps) == len(free.steps) >= 40
    prev = {}
    for a, b in zip(led.steps, free.steps):
        assert a["action"] == b["action"] and a["lin"] == b["lin"] and a["done"] == b["done"] and np.array_equal(a["state"], b["state"])
        assert a["stable_s"] == (True if a["nb"] == 0 else prev[a["env"]]["stable_frozen"])
        assert a["nb"] == len(a["shapes"]) == len(a["poses"]) and a["cand_rasters"][a["pick"]] is not None
        assert np.array_equal(a["cand_rasters"][a["pick"]], a["action_raster"])
        if a["done"] or a["no_actions"]:
            assert "next_state" not in a
        else:
            assert np.array_equal(a["next_state"], a["state"] | a["action_raster"]) and len(a["next_rasters"]) > 0
        prev[a["env"]] = a
    assert any(s["done"] for s in led.steps) and max(s["nb"] for s in led.steps) == V.MAX_STEPS - 1
    with pytest.raises(AssertionError, match="valid_step"):
        led.advance(np.zeros((cfg["E"], R.RECORD_WIDTH)), np.array([o.needs_reset for o in led.oracles]))


def test_the_reference_alone_stays_inside_the_undecided_cap():
    """The CPU proxy of case c's first seed (the other cases: python tests/vec_dqn_oracle.py, docs/MEASUREMENT_LOG.md)."""
    boot, und = V.proxy_counts("c", V.CASES["c"]["seeds"][0])
    assert boot >= 8 and und <= V.UNDECIDED_CAP * boot
