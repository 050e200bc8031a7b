"""GPU: bridges_env_fork / VecAssemblyGym.fork.  Two identical envs P and Q (same seed, E = 24, max_steps 6) are advanced the same
three random lock-steps; P is forked with a pattern src and must then hold, in env e, the bits Q holds in env src[e]: every state
array, the refreshed candidate sets, and -- stepped with the same actions for three lock-steps, so that a wrongly copied contact
list or tableau would show in a later verdict -- the same results."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
E, H = 24, 0.8
CONFIGS = ("tower", "hexagon_random_tasks", "stable_actions_only", "no_snapshots")
PATTERNS = ("identity", "reversal", "broadcast_0", "swap", "chain", "out_of_range")


def _make(config, seed=11):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomObstacles, RandomTargets, VecAssemblyGym
    kw = dict(max_steps=6, seed=seed, f32_rasters=False)
    if config == "hexagon_random_tasks":
        return VecAssemblyGym(E, [load_urdf("shapes/hexagon.urdf")], RandomObstacles([((-3.0, 3.0), (0.3, 2.5))]), RandomTargets(3), **kw)
    if config == "stable_actions_only":
        kw["stable_actions_only"] = True
    if config == "no_snapshots":
        kw["candidate_snapshots"] = False
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)],
                          [(0.5, 0, 2 * H + H / 2)], **kw)


def _pair(config):
    P, Q = _make(config), _make(config)
    for env in (P, Q):
        for _ in range(3):
            env.select_random()
            env.step()
    return P, Q


def _pattern(name):
    e = np.arange(E)
    src = dict(identity=e, reversal=E - 1 - e, broadcast_0=0 * e, swap=e ^ 1, chain=(e + 1) % E,
               out_of_range=np.where(e % 3 == 0, e[::-1], np.array([-1, E, 2 ** 31 - 1, -2 ** 31, E + 5, -E])[e % 6]))[name]
    eff = np.where((src >= 0) & (src < E), src, e)
    return torch.tensor(src, dtype=torch.int32, device="cuda"), torch.tensor(eff, dtype=torch.long, device="cuda")


def _state_arrays(env):
    """name -> the [E, ...] tensor of every array the fork's table lists (abi.FORK_*), where the env has it."""
    from bridges_hip import abi
    out = {n: (env.lp_snap if n == "lp_snap" else env.buf[n]) for n in abi.FORK_ENV_FIELDS}
    if env.per_env_tasks:
        out.update({n: env.task_buf[n] for n, _d, _s in abi.TASK_BUFFER_FIELDS})
    if env.per_env_obstacles:
        out.update({n: env.obstacle_buf[n] for n, _d, _s in abi.OBSTACLE_BUFFER_FIELDS})
    if env.task_class is not None:
        out["task_class"] = env.task_class
    return {n: t for n, t in out.items() if t is not None}


def _bits(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)


def _assert_rows(P, Q, eff, names=None, rows=None, what=""):
    p, q = _state_arrays(P), _state_arrays(Q)
    assert set(p) == set(q)
    rows = torch.arange(E, device="cuda") if rows is None else rows
    for n in names or p:
        assert torch.equal(_bits(p[n])[rows], _bits(q[n])[eff[rows]]), f"{what}: {n}"


CAND = ("cand_desc", "cand_pose", "cand_bits", "cand_mask", "cand_lin")


def _assert_candidates(P, Q, eff, rows=None, what=""):
    names = CAND + (("cand_stable",) if P.stable_actions_only else ())
    po, pn, qo, qn = (t.cpu().numpy() for t in (P.cand_offset, P.n_cand, Q.cand_offset, Q.n_cand))
    pv, qv = P.n_valid.cpu().numpy(), Q.n_valid.cpu().numpy()
    pb, qb = {n: _bits(P.buf[n]).cpu().numpy() for n in names}, {n: _bits(Q.buf[n]).cpu().numpy() for n in names}
    eff = eff.cpu().numpy()
    for e in (range(E) if rows is None else rows.cpu().tolist()):
        s = eff[e]
        assert pn[e] == qn[s] and pv[e] == qv[s], f"{what}: counts of env {e}"
        for n in names:
            assert np.array_equal(pb[n][po[e]:po[e] + pn[e]], qb[n][qo[s]:qo[s] + qn[s]]), f"{what}: {n} of env {e}"


def _pick(Q, rng):
    """A random valid candidate per env of Q, chosen on the host (select_random would advance Q's draw counters only)."""
    off, n, mask = Q.cand_offset.cpu().numpy(), Q.n_cand.cpu().numpy(), Q.cand_mask.cpu().numpy()
    a = np.zeros(E, dtype=np.int32)
    for e in range(E):
        valid = np.flatnonzero(mask[off[e]:off[e] + n[e]])
        if len(valid):
            a[e] = valid[rng.integers(len(valid))]
    return torch.tensor(a, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("config", CONFIGS)
def test_fork_copies_state_candidates_and_what_the_steps_after_it_say(config, pattern):
    P, Q = _pair(config)
    _assert_rows(P, Q, torch.arange(E, device="cuda"), what="twins before the fork")
    assert int(Q.n_blocks.max()) > 0 and int(Q.n_if.max()) > 0                  # the states are worth copying
    src, eff = _pattern(pattern)
    P.fork(src)
    torch.cuda.synchronize()
    _assert_rows(P, Q, eff, what="after the fork")
    _assert_candidates(P, Q, eff, what="after the fork")
    if config == "hexagon_random_tasks":
        assert not torch.equal(Q.env_targets[0], Q.env_targets[1])             # (every env owns a task: the task rows were compared)
    # the same actions on both sides, three lock-steps.  A clone that starts a new episode under a task SAMPLER draws the task of
    # its own env id, not its source's: those envs leave the comparison (fixed tasks: nobody leaves)
    rng = np.random.default_rng(5)
    results = ("step_flags", "reward", "lin_reward", "n_reached", "targets_left")
    same = torch.ones(E, dtype=torch.bool, device="cuda")
    for k in range(3):
        a = _pick(Q, rng)
        P.step(a[eff])
        Q.step(a)
        torch.cuda.synchronize()
        rows = torch.nonzero(same).flatten()
        if config == "hexagon_random_tasks":
            # no_actions of a step that ends the episode speaks of the fresh state under the NEXT task, which the clone draws as itself
            for env in (P, Q):
                env.step_flags[:, 6] &= ~env.step_flags[:, 5]
        _assert_rows(P, Q, eff, names=results, rows=rows, what=f"step {k}")
        if config == "hexagon_random_tasks":
            same &= ~(P.step_flags[:, 5].bool() | ~P.step_flags[:, 0].bool())     # done, or a reset-only lock-step
            rows = torch.nonzero(same).flatten()
        _assert_rows(P, Q, eff, rows=rows, what=f"state after step {k}")
        _assert_candidates(P, Q, eff, rows=rows, what=f"candidates after step {k}")
        assert k > 0 or rows.numel() > 0                                        # the later steps compare something


@pytest.mark.parametrize("config", ["tower", "hexagon_random_tasks"])
def test_identity_fork_leaves_the_rollout_bit_identical_to_an_unforked_twin(config):
    P, Q = _pair(config)
    ident = torch.arange(E, device="cuda")
    P.fork(ident.to(torch.int32))
    for _ in range(4):
        for env in (P, Q):
            env.select_random()
            env.step()
    torch.cuda.synchronize()
    _assert_rows(P, Q, ident, what="rollout after an identity fork")
    _assert_candidates(P, Q, ident, what="rollout after an identity fork")
    assert torch.equal(P.sel_index, Q.sel_index)


def test_scratch_is_sized_once_and_states_its_bytes():
    from bridges_hip import abi
    P = _make("tower")
    n = C.c_int64(0)
    abi.check(P.L.bridges_env_fork_scratch(P._env, C.byref(n)), "bridges_env_fork_scratch")
    arrays = _state_arrays(P)
    assert n.value == sum(-(-t.numel() * t.element_size() // 16) * 16 for t in arrays.values())
    assert n.value >= E * 8 * (abi.ENV_LP_WS_DOUBLES + abi.ENV_LP_SNAP_DOUBLES)
    P.fork(torch.arange(E, dtype=torch.int32))
    scratch = P._fork_scratch
    P.fork(torch.arange(E, dtype=torch.int32).flip(0))
    assert P._fork_scratch is scratch and scratch.numel() == n.value


def test_refusals_launch_nothing():
    from bridges_hip import abi
    P = _pair("tower")[0]
    L = P.L
    n = C.c_int64(0)
    assert L.bridges_env_fork_scratch(None, C.byref(n)) == -1 and L.bridges_env_fork_scratch(P._env, None) == -1
    abi.check(L.bridges_env_fork_scratch(P._env, C.byref(n)), "bridges_env_fork_scratch")
    scratch = torch.full((n.value + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    src = torch.arange(E + 1, dtype=torch.int32, device="cuda").flip(0)
    torch.cuda.synchronize()
    before = {k: t.clone() for k, t in _state_arrays(P).items()}
    stream = abi.current_stream()
    sp, cp = src.data_ptr(), scratch.data_ptr()
    assert L.bridges_env_fork(None, sp, cp, n.value, stream) == -1
    assert L.bridges_env_fork(P._env, None, cp, n.value, stream) == -1
    assert L.bridges_env_fork(P._env, sp, None, n.value, stream) == -1
    assert L.bridges_env_fork(P._env, sp + 2, cp, n.value, stream) == -1 and b"aligned" in L.bridges_last_error()
    assert L.bridges_env_fork(P._env, sp, cp + 8, n.value, stream) == -1
    assert L.bridges_env_fork(P._env, sp, cp, n.value - 1, stream) == -1 and b"scratch_bytes" in L.bridges_last_error()
    torch.cuda.synchronize()
    assert bool((scratch == 0x5A).all())
    for k, t in _state_arrays(P).items():
        assert torch.equal(_bits(t), _bits(before[k])), k
    assert L.bridges_env_fork(P._env, sp, cp, n.value, stream) == 0             # and the call they guard goes through
    torch.cuda.synchronize()
    assert bool((scratch[n.value:] == 0x5A).all())                              # nothing beyond the sized bytes is written


def test_fork_is_not_offered_on_env_groups():
    from bridges_hip.vec_env import VecAssemblyGymGroups
    assert not hasattr(VecAssemblyGymGroups, "fork")
