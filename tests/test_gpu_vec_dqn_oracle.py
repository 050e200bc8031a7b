"""GPU: the vectorised DQN's transitions and targets against the numpy oracle (tests/vec_dqn_oracle.py) -- the junction of the env,
record, fold, replay and target kernels, which every other test of VecDQN compares with the project's own device path.

A rollout: E envs that start in the same state (shared rows are in play; E = 6 is no multiple of the four envs per workgroup of
k_valid_fill, k_env_hash and k_nstep_fold), max_steps = 4 (episodes end, reset, and n-step tails of every h occur), 10 lock-steps
of agent.act() + ring push without an optimiser step, the target net mul_(1.05) of the policy net, then _targets over the whole ring
5 rows at a time in a scratch env of 8 envs (the padding envs repeat record 0).  The oracle track follows the actions the device
took; everything expected comes from it and from the float64 twins' module forward, the allowance from the float32 library
forward (vec_dqn_oracle.accept).  A case pools the rollouts of its seeds (vec_dqn_oracle.CASES says why) and prints one R line;
docs/MEASUREMENT_LOG.md holds a run."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vec_dqn_oracle as V
from gpu_helpers import all_predicates_off, library_twin
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCRATCH_ENVS, ROWS_PER_CALL, GREEDY_LOCKSTEPS = 8, 5, 3


def make_env(cfg, seed):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomObstacles, RandomTargets, VecAssemblyGym
    names, setup = V.case_setup(cfg["task"])
    geoms = [load_urdf(f"shapes/{n}.urdf") for n in names]
    kw = dict(max_steps=V.MAX_STEPS, seed=seed, f32_rasters=cfg["net"] == "conv",
              stable_actions_only=cfg["agent"].get("stable_actions_only", False))
    if cfg["task"] == "random":
        return VecAssemblyGym(cfg["E"], geoms, RandomObstacles([V.OBSTACLE_RANGE]), RandomTargets(2), **kw)
    return VecAssemblyGym(cfg["E"], geoms, setup["obstacles"], setup["targets"], **kw)


def pack_bits(raster):
    """bool [64, 64] -> int64 [64]: pixel (y, x) = bit x of word y, the order of k_bits_to_f32."""
    return np.bitwise_or.reduce(raster.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :], axis=1).view(np.int64)


def rollout(name, seed, prioritized=False, locksteps=None):
    from robotoddler.training.vec_dqn import VecDQN
    cfg = V.CASES[name]
    E, per_env = cfg["E"], cfg["task"] == "random"
    env = make_env(cfg, seed)
    pol, tgt = V.make_nets(cfg["net"], seed, DEV)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 4096, SCRATCH_ENVS, V.GAMMA, 0.01, cfg["loss"],
                   seed=seed, prioritized=prioritized, **cfg["agent"])
    assert agent.replay_env.E == SCRATCH_ENVS > ROWS_PER_CALL

    def task_of(e):
        return [tuple(t) for t in env.env_targets[e].cpu().tolist()], [tuple(o) for o in env.env_obstacles[e].cpu().tolist()]
    track = V.OracleTrack(V.gym_factory(cfg["task"]), E, stable_actions_only=agent.stable_actions_only, task_of=task_of if per_env else None)
    log = SimpleNamespace(recs=[], valids=[], maps=[], td=[], q_sel=[])
    L = locksteps or cfg["locksteps"]
    for t in range(L):
        if t >= L - GREEDY_LOCKSTEPS:
            agent.epsilon = 0.0
        log.maps.append((env.reward_maps_img if per_env else env.reward_features.expand(E, -1, -1)).cpu().numpy().copy())
        rec, valid = agent.act()
        log.q_sel.append(agent._q_sel.cpu())
        if prioritized:
            td = agent.td_errors(rec)
            rec[:, R.O_TD] = td.to(rec.dtype)                                  # as VecDQN.lockstep does
            log.td.append(td.cpu())
        full = agent.with_task(rec)
        if agent.n_step > 1:
            out, out_valid = agent._fold(full, valid)
            agent.ring.push(out[out_valid])
        else:
            agent.ring.push(full[valid])
        log.recs.append(full.cpu().numpy())
        log.valids.append(valid.cpu().numpy().astype(bool))
        track.advance(log.recs[-1], log.valids[-1])                       # asserts valid and finds the ONE candidate the row names
    torch.cuda.synchronize()
    return SimpleNamespace(cfg=cfg, env=env, agent=agent, pol=pol, tgt=tgt, track=track, log=log, per_env=per_env)


def check_records(ro):
    """Every env and lock-step: the record row against the oracle's transition.  -> the worst |O_LIN - lin| / |lin|."""
    track, log, worst = ro.track, ro.log, 0.0
    for t, row in enumerate(track.grid):
        for e, i in enumerate(row):
            if i is None:
                continue
            tr, r, at = track.steps[i], log.recs[t][e], (t, e)
            nb = tr["nb"]
            assert r[R.O_NB] == nb and r[R.O_SHAPE:R.O_SHAPE + nb].tolist() == tr["shapes"], at
            assert [tuple(p) for p in r[R.O_POSE:R.O_POSE + 4 * nb].reshape(nb, 4).tolist()] == tr["poses"], at       # float64, exact
            assert (r[R.O_ATB], r[R.O_ATF], r[R.O_ASHAPE], r[R.O_AFACE]) == tuple(tr["action"][:4]), at
            assert tuple(r[R.O_APOSE:R.O_APOSE + 4].tolist()) == tr["action_pose"], at
            assert r[R.O_REWARD] == tr["reward"], at
            # the linear reward sums the env's own float32 reward map, which the map check below holds within 1e-5 of the oracle's:
            # compared the way tests/test_gpu_env_parity.py compares it, and a float32 value in the record
            assert r[R.O_LIN] == np.float32(r[R.O_LIN]), at
            np.testing.assert_allclose(r[R.O_LIN], tr["lin"], rtol=1e-5, atol=1e-7, err_msg=str(at))
            worst = max(worst, abs(r[R.O_LIN] - float(tr["lin"])) / max(abs(float(tr["lin"])), 1e-30))
            assert r[R.O_DONE] == float(tr["done"] or tr["no_actions"]), at
            assert r[R.O_STABLE_N] == float(tr["stable_frozen"]) and r[R.O_STABLE_S] == float(tr["stable_s"]), at
            np.testing.assert_allclose(log.maps[t][e], tr["reward_map"], rtol=1e-5, atol=1e-7, err_msg=str(at))
            if ro.per_env:                                                 # the tail: the task the transition was taken under
                tail = [v for p in list(tr["targets"]) + list(tr["obstacles"]) for v in p]
                assert r[R.RECORD_WIDTH:].tolist() == tail, at
    return worst


def check_ring(ro, rows):
    """The ring against the oracle's windows: row i is the record of its window's last step with the start's stable flag, h in the
    last column and O_LIN within tests/nstep_ref.py's bound of the float64 fold of the one-step records' linear rewards."""
    track, log, agent = ro.track, ro.log, ro.agent
    ring = agent.ring.data[:agent.ring.size].cpu().numpy()
    assert ring.shape[0] == len(rows) and agent.ring.size < agent.ring.capacity
    W = R.RECORD_WIDTH + agent.task_width
    copied = np.ones(W, dtype=bool)
    copied[[R.O_LIN, R.O_STABLE_S, R.O_TD]] = False
    one_step = lambda tr: log.recs[tr["t"]][tr["env"]]
    for i, row in enumerate(rows):
        win = [track.steps[j] for j in row["window"]]
        assert np.array_equal(ring[i, :W][copied].view(np.int64), one_step(win[-1])[:W][copied].view(np.int64)), i
        assert ring[i, R.O_STABLE_S] == float(win[0]["stable_s"]), i
        if agent.n_step > 1:
            assert ring[i, -1] == row["h"], i
        G, bound = V.fold_return([one_step(tr)[R.O_LIN] for tr in win], V.GAMMA)
        assert abs(ring[i, R.O_LIN] - G) <= bound, (i, row["h"], ring[i, R.O_LIN], G, bound)
    if agent.n_step > 1:
        assert {row["h"] for row in rows} == set(range(1, agent.n_step + 1))      # full windows and the tails of episodes


def device_targets(ro, rows):
    """_targets over the whole ring, ROWS_PER_CALL rows a call -> dict(block, binary, action, q, sf, maps, obstacle_bits)."""
    agent = ro.agent
    ring = agent.ring.data[:agent.ring.size].clone()
    calls = []
    for o in range(0, ring.shape[0], ROWS_PER_CALL):
        calls.append([v.clone() if torch.is_tensor(v) else v for v in agent._targets(ring[o:o + ROWS_PER_CALL])])
    torch.cuda.synchronize()
    cat = lambda k: torch.cat([c[k] for c in calls]).cpu() if calls[0][k] is not None else None
    got = dict(block=cat(0)[:, 0], binary=cat(1), action=cat(2)[:, 0], q=cat(3), sf=cat(4))
    if ro.per_env:
        got["maps"], got["obstacle_bits"] = cat(5), cat(6)
    assert got["q"].dtype == torch.float32 and got["q"].shape[0] == len(rows)
    return got


def check_acting(ro, twin_p):
    """Every lock-step: the q the device reports for the row it took (explored or greedy) against the policy twin's q of that
    candidate, through accept.  The greedy lock-steps: the pick is the twin's first maximum over the oracle's valid candidates, or
    the runner-up where the two lie within FACTOR x the measured |q32 - q64| of the rows.
    -> (greedy picks checked, undecided among them, share of the allowance the reported q used)."""
    track, n, n_und, got, ref, lib = ro.track, 0, 0, [], [], []
    for t, row in enumerate(track.grid):
        for e, i in enumerate(row):
            if i is None:
                continue
            tr = track.steps[i]
            q64 = V.state_q(tr, twin_p, ro.log.maps[t][e]).double().cpu()
            with all_predicates_off():
                q32 = V.state_q(tr, ro.pol, ro.log.maps[t][e]).double().cpu()
            got.append(ro.log.q_sel[t][e])
            ref.append(q64[tr["pick"]])
            lib.append(q32[tr["pick"]])
            if t < len(track.grid) - GREEDY_LOCKSTEPS:
                continue
            best, second, gap = V.first_maximum(q64, tr["cand_rasters"])
            und = second is not None and gap < V.FACTOR * float((q32 - q64).abs().max())
            assert tr["pick"] == best or (und and tr["pick"] == second), (t, e, tr["pick"], best, second, gap)
            n, n_und = n + 1, n_und + int(und)
    ok, share = V.accept(torch.stack(got), torch.stack(ref), torch.stack(lib))
    assert ok, ("q of the chosen rows", share)
    return n, n_und, share


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_transitions_and_targets_follow_the_oracle(name):
    cfg = V.CASES[name]
    n_step, double_q = cfg["agent"].get("n_step", 1), cfg["agent"].get("double_q", False)
    use_sf = "mse_block_features" in cfg["loss"]
    worst, worst_lin, boots, unds, acted, acted_und, differ = 0.0, 0.0, [], [], 0, 0, 0
    for seed in cfg["seeds"]:
        ro = rollout(name, seed)
        track = ro.track
        assert any(tr["done"] for tr in track.steps)
        worst_lin = max(worst_lin, check_records(ro))
        rows = V.ring_rows(track, n_step)
        check_ring(ro, rows)
        got = device_targets(ro, rows)
        maps = [ro.log.maps[track.steps[row["window"][0]]["t"]][track.steps[row["window"][0]]["env"]] for row in rows]
        twin_t, twin_p = library_twin(ro.tgt), library_twin(ro.pol)
        args = (V.GAMMA, n_step, double_q, use_sf)
        ref = V.reference_targets(track, rows, twin_t, twin_p, *args, maps=maps)
        with all_predicates_off():
            lib = V.reference_targets(track, rows, ro.tgt, ro.pol, *args, maps=maps, pick=list(zip(ref["best"], ref["second"])))
        und = V.undecided(ref, lib)
        if double_q:                                                       # how many rows tell the selecting net from the valuing one
            plain = V.reference_targets(track, rows, twin_t, twin_p, V.GAMMA, n_step, False, False, maps=maps)
            differ += sum(a != b for a, b in zip(ref["best"], plain["best"]))
        ok, share, failed = V.conforms(got, ref, lib, und, double_q=double_q)
        print(f"  seed {seed}: rows {len(rows)} bootstrapping {int(ref['boot'].sum())} undecided {int(und.sum())} share {share:.3f} "
              f"|O_LIN - lin| / |lin| <= {worst_lin:.2e}")
        assert ok, (name, seed, failed, share)
        if ro.per_env:
            for i, row in enumerate(rows):
                first = track.steps[row["window"][0]]
                assert np.array_equal(got["maps"][i].numpy().reshape(64, 64), maps[i]), i          # the transition's map, not a later one
                assert np.array_equal(got["obstacle_bits"][i].numpy(), pack_bits(first["obstacle_raster"])), i
        n, n_und, q_share = check_acting(ro, twin_p)
        worst, acted, acted_und = max(worst, share, q_share), acted + n, acted_und + n_und
        boots.append(ref["boot"])
        unds.append(und)
    decided, undecided = V.check_cap(dict(boot=torch.cat(boots)), torch.cat(unds), name=f"case {name}")
    print(f"R vec_dqn_oracle case {name}: worst share of the allowance {worst:.3f} decided {decided} undecided {undecided} "
          f"(greedy picks {acted}, undecided {acted_und})" + (f" rows the two nets select differently {differ}" if double_q else ""))
    assert acted >= GREEDY_LOCKSTEPS * cfg["E"] // 2 and acted_und <= V.UNDECIDED_CAP * acted, (acted, acted_und)


def test_priorities_follow_the_oracle():
    """Case a with prioritized=True: agent.td_errors(rec) of every lock-step against the policy twin on the oracle's rows."""
    ro = rollout("a", V.CASES["a"]["seeds"][0], prioritized=True, locksteps=6)
    track = ro.track
    got = torch.cat([td[torch.as_tensor(valid)] for td, valid in zip(ro.log.td, ro.log.valids)])
    maps = [ro.log.maps[tr["t"]][tr["env"]] for tr in track.steps]
    ref = V.reference_td_errors(track, library_twin(ro.pol), maps)
    with all_predicates_off():
        lib = V.reference_td_errors(track, ro.pol, maps)
    assert got.shape == ref.shape and got.numel() >= 24
    ok, share = V.accept(got, ref, lib)
    print(f"R vec_dqn_oracle priorities: worst share of the allowance {share:.3f} transitions {got.numel()}")
    assert ok, share
    assert torch.equal(ro.agent.ring.data[:ro.agent.ring.size, R.O_TD].float().cpu(), got)
