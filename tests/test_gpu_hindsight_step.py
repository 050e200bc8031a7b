"""GPU: bridges_hindsight_per_step and bridges_hindsight_per_step_nstep against tests/hindsight_step_ref.py bit for bit on
sentinel-filled outputs, on the scripted probe episodes of tests/hindsight_ref.py (tests/test_cpu_hindsight_step.py checks on the
CPU that they hold every case of the rule): the count, the rows beyond it, the inputs, a second call; every argument the entries
refuse; and, independent of the restatement, a VecAssemblyGym that is given the targets of an emitted row and replays the
recorded placements: its reward, its linear reward and its flags at step t are the row's, bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hindsight_step_ref as S
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, BASE, CONFIGS = S.PROBE_SEED, S.PROBE_BASE, S.PROBE_CONFIGS
FOLD_CONFIGS = ((5, 3, 4, 2, "hexagon"), (64, 3, 4, 0, "trapezoid"), (130, 1, 1, 2, "hexagon"))
NS, GAMMA = (1, 2, 3, 8), 0.95
SENTINEL = -7.25
ROWS = dict(zip(CONFIGS, (1, 76, 843, 754, 384, 449)))          # one-step rows of the rule on the probes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def task_env(T, shape):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomTargets, VecAssemblyGym
    return VecAssemblyGym(2, [load_urdf(f"shapes/{shape}.urdf")], [], RandomTargets(T), max_steps=6, seed=SEED, env_id_base=BASE,
                          device=DEV)


@functools.lru_cache(maxsize=None)
def case(E, T, G, O, shape):
    """The probe and the device copies of its inputs."""
    p = S.probe(E, T, O, shape, seed=S.probe_seed(E))
    dev = {k: torch.from_numpy(p[k]).to(DEV) for k in ("buf", "flags", "length", "ended", "episode")}
    return p, dev


@functools.lru_cache(maxsize=None)
def reference(E, T, G, O, shape, n=None):
    """The reference rows (computed once, shared by the tests, never written); n None: the one-step rows."""
    p, _dev = case(E, T, G, O, shape)
    ref = S.relabel(p["buf"], p["flags"], p["length"], p["ended"], p["episode"], p["shapes"], SEED, BASE, G, T, n_step=n,
                    gamma=None if n is None else GAMMA)
    ref.setflags(write=False)
    return ref


def run(env, dev, G, n=None, ended=None):
    from bridges_hip import dqn_ops
    E, K, W = dev["buf"].shape
    out = torch.full((E * K * G, W + (n is not None)), SENTINEL, dtype=torch.float64, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    dqn_ops.hindsight_relabel(env, dev["buf"], dev["flags"], dev["length"], dev["ended"] if ended is None else ended, dev["episode"],
                              G, out=out, count=count, strategy="per_step", **({} if n is None else dict(n_step=n, gamma=GAMMA)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(count.item())


def check(E, T, G, O, shape, n):
    p, dev = case(E, T, G, O, shape)
    ref = reference(E, T, G, O, shape, n)
    env = task_env(T, shape)
    before = {k: v.clone() for k, v in dev.items()}
    out, count = run(env, dev, G, n)
    print(f"E={E} T={T} G={G} O={O} {shape} n={n}: {count} rows, reference {len(ref)}")
    assert len(ref) == ROWS[(E, T, G, O, shape)]                 # (the window does not change the count)
    assert count == len(ref)
    assert np.array_equal(bits(out[:count]), bits(ref))
    assert np.all(out[count:] == SENTINEL)                       # rows beyond the count are not written
    for k, v in dev.items():                                     # the buffers are only read (envs in mid-episode included)
        assert torch.equal(v, before[k]), k
    again, count2 = run(env, dev, G, n)                          # the same bits on every call
    assert count2 == count and np.array_equal(bits(again), bits(out))


@pytest.mark.parametrize("E,T,G,O,shape", CONFIGS)
def test_one_step_rows_are_the_reference_bit_for_bit(E, T, G, O, shape):
    check(E, T, G, O, shape, None)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("E,T,G,O,shape", FOLD_CONFIGS)
def test_h_step_rows_are_the_reference_bit_for_bit(E, T, G, O, shape, n):
    check(E, T, G, O, shape, n)


def test_nothing_ended_nothing_written():
    _p, dev = case(64, 3, 4, 0, "trapezoid")
    for n in (None, 3):
        out, count = run(task_env(3, "trapezoid"), dev, 4, n, ended=torch.zeros(64, dtype=torch.bool, device=DEV))
        assert count == 0 and np.all(out == SENTINEL)


@pytest.mark.parametrize("fold", (False, True))
def test_argument_errors_launch_nothing(fold):
    from bridges_hip import abi, dqn_ops
    from bridges_hip.ops import _ptr, _stream
    L = abi.lib()
    cfg = (5, 3, 4, 2, "hexagon")
    _p, dev = case(*cfg)
    env = task_env(3, "hexagon")
    E, K, W = dev["buf"].shape
    need = C.c_int64(0)
    assert L.bridges_hindsight_per_step_scratch(E, 4, C.byref(need)) == 0 and need.value == 2 * 4 * E * 4   # a count and a mask
    assert dqn_ops.hindsight_relabel_scratch(E, 4, "per_step") == need.value
    assert L.bridges_hindsight_per_step_scratch(E, 0, C.byref(need)) == -1 and L.bridges_hindsight_per_step_scratch(E, 5, C.byref(need)) == -1
    out = torch.full((E * K * 4 + 1, W + fold), SENTINEL, dtype=torch.float64, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(2 * 4 * E * 4, dtype=torch.uint8, device=DEV)
    ended = dev["ended"].view(torch.uint8)
    good = dict(E=E, K=K, W=W, T=3, G=4, buf=_ptr(dev["buf"]), flags=_ptr(dev["flags"]), len=_ptr(dev["length"]), ended=_ptr(ended),
                episode=_ptr(dev["episode"]), seed=SEED, base=BASE, shapes=env.table.ptr, n_shapes=len(env.table_geoms),
                target_shape=len(env.table_geoms) - 1, gx=_ptr(env.grid_x_dev), gy=_ptr(env.grid_y_dev), img=64,
                gauss=C.c_void_p(env._gauss_k.data_ptr()), **(dict(n_step=3, gamma=GAMMA) if fold else {}), out=_ptr(out),
                count=_ptr(count), scratch=_ptr(scratch), scratch_bytes=scratch.numel())
    entry = L.bridges_hindsight_per_step_nstep if fold else L.bridges_hindsight_per_step

    def call(**kw):
        a = dict(good, **kw)
        return entry(*a.values(), _stream())
    null = C.c_void_p(0)
    bad = [dict(G=0), dict(G=5), dict(E=-1), dict(K=0), dict(K=17), dict(T=0), dict(T=9), dict(W=R.RECORD_WIDTH + 8), dict(img=65),
           dict(n_shapes=0), dict(target_shape=2), dict(scratch_bytes=2 * 4 * E * 4 - 1),
           dict(scratch_bytes=4 * E * 4),                        # what the "final" entries need is not enough
           dict(out=C.c_void_p(out.data_ptr() + 4))]
    if fold:
        bad += [dict(n_step=0), dict(n_step=9), dict(gamma=float("nan")), dict(gamma=float("inf"))]
    bad += [{k: null} for k in ("buf", "flags", "len", "ended", "episode", "shapes", "gx", "gy", "gauss", "out", "count", "scratch")]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "hindsight" in L.bridges_last_error().decode(), kw
    assert call(E=0) == 0                                         # succeeds and launches nothing
    torch.cuda.synchronize()
    assert int(count.item()) == -1 and bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="strategy"):            # the wrapper refuses in words before the call
        dqn_ops.hindsight_relabel(env, dev["buf"], dev["flags"], dev["length"], dev["ended"], dev["episode"], 4, strategy="future")
    assert call() == 0                                            # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    ref = reference(*cfg, 3 if fold else None)
    assert int(count.item()) == len(ref)
    assert np.array_equal(bits(out[:len(ref)].cpu().numpy()), bits(ref)) and bool((out[len(ref):] == SENTINEL).all())


@pytest.mark.parametrize("shape", ("trapezoid", "hexagon"))
def test_an_env_on_a_rows_targets_records_the_row_at_its_step(shape):
    """Independent of the restatement: roll out the first episode of every env under random targets, relabel it per step, then
    give a second env, per env, the targets in the tail of one emitted row -- the row of slot 0 with the largest t -- and replay
    the recorded placements with step(sel_index).  At step t its reward, lin_reward (the rasteriser's cand_lin through k_step's
    rule) and step flags are what the row holds, bitwise."""
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomTargets, VecAssemblyGym
    E, T, MAXS = 48, 3, 6
    geoms = [load_urdf(f"shapes/{shape}.urdf")]
    env = VecAssemblyGym(E, geoms, [], RandomTargets(T), max_steps=MAXS, seed=SEED, env_id_base=BASE, device=DEV)
    env.reset()
    hb = R.HindsightBuffer(E, R.RECORD_WIDTH + 3 * T, DEV, goals=1, n_blocks=env.K, strategy="per_step")
    sels, row_of, first_over = [], {}, torch.zeros(E, dtype=torch.bool, device=DEV)
    for _ in range(MAXS + 1):
        env.select_random()
        sel = env.buf["sel_index"].clone()
        rec = R.pack_state(env, env.cand_offset[:E].long() + sel.long())
        tail, episode = env.env_targets.reshape(E, -1).clone(), env.task_episode.clone()
        env.step()
        valid = R.pack_result(env, rec)
        ended = valid & (rec[:, R.O_DONE] > 0.5)
        rec[:, R.O_TD] = torch.arange(E, dtype=torch.float64, device=DEV)      # a copied column: names the env of every row
        hb.write(torch.cat([rec, tail], dim=1), env.step_flags, valid, episode)
        out, count = hb.relabel(env, ended & ~first_over)
        hb.length.masked_fill_(ended, 0)
        torch.cuda.synchronize()
        got = out[:int(count.item())].cpu().numpy()
        for e in torch.nonzero(ended & ~first_over).flatten().tolist():
            mine = got[got[:, R.O_TD] == e]
            assert np.all(np.diff(mine[:, R.O_NB]) > 0)          # slot 0 alone: t ascending
            if len(mine):
                row_of[e] = mine[-1].copy()                      # the largest t
        sels.append(sel)
        first_over |= ended
    assert len(row_of) >= E // 2
    targets = env.env_targets.cpu().numpy().copy()
    for e, row in row_of.items():
        targets[e] = row[R.RECORD_WIDTH:].reshape(T, 3)
    twin = VecAssemblyGym(E, geoms, [], targets, max_steps=MAXS, seed=SEED, env_id_base=BASE, device=DEV)
    twin.reset()
    checked = early = 0
    over = np.zeros(E, dtype=bool)                               # the twin's episode ended before the row's step
    for t in range(MAXS):
        # an env whose compared step is over plays on with a valid action of its own
        twin.select_random()
        replayed = torch.tensor([e in row_of and t <= int(row_of[e][R.O_NB]) for e in range(E)], device=DEV)
        twin.step(torch.where(replayed, sels[t], twin.buf["sel_index"]))
        torch.cuda.synchronize()
        reward, lin, fl = twin.reward.cpu().numpy(), twin.lin_reward.cpu().numpy(), twin.step_flags.cpu().numpy()
        for e, row in row_of.items():
            if t > int(row[R.O_NB]):
                continue
            assert not over[e] and fl[e, 0] == 1, (e, t)         # the transition exists under the row's targets
            if t < int(row[R.O_NB]):
                over[e] = bool(fl[e, 5] | fl[e, 6])
                continue
            assert np.float32(row[R.O_REWARD]).tobytes() == reward[e].tobytes(), (e, t, row[R.O_REWARD], reward[e])
            assert np.float32(row[R.O_LIN]).tobytes() == lin[e].tobytes() and float(np.float32(row[R.O_LIN])) == row[R.O_LIN], (e, t)
            assert bool(row[R.O_DONE]) == bool(fl[e, 5] | fl[e, 6]), (e, t)
            assert bool(row[R.O_STABLE_N]) == bool(fl[e, 1]), (e, t)
            if fl[e, 3] and fl[e, 1]:
                early += 1                                        # terminated while stable: every hindsight target reached
            checked += 1
    print(f"{shape}: step t of {checked} rows compared, {early} ended on their hindsight targets")
    assert checked >= E and early >= 1                           # one row per env: every first episode had one
