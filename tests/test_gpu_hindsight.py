"""GPU: bridges_hindsight_relabel against tests/hindsight_ref.py bit for bit on sentinel-filled outputs -- scripted probe episodes
that hold every case of the rule (tests/test_cpu_hindsight.py checks on the CPU that they do) -- and, independent of the
restatement, against a VecAssemblyGym that is given the hindsight targets and replays the recorded placements: its reward, its
linear reward and its step flags are the relabelled rows', bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hindsight_ref as H
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, BASE, CONFIGS = H.PROBE_SEED, H.PROBE_BASE, H.PROBE_CONFIGS
SENTINEL = -7.25

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
    """The probe, its reference rows (computed once, shared by the tests, never written) and the device copies of the inputs."""
    p = H.probe(E, T, O, shape, seed=H.probe_seed(E))
    ref = H.relabel(p["buf"], p["flags"], p["length"], p["ended"], p["episode"], p["shapes"], SEED, BASE, G, T)
    ref.setflags(write=False)
    dev = {k: torch.from_numpy(p[k]).to(DEV) for k in ("buf", "flags", "length", "ended", "episode")}
    return p, ref, dev


def run(env, dev, G, ended=None):
    from bridges_hip import dqn_ops
    E, K, W = dev["buf"].shape
    out = torch.full((E * K * G, W), SENTINEL, dtype=torch.float64, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    dqn_ops.hindsight_relabel(env, dev["buf"], dev["flags"], dev["length"], dev["ended"] if ended is None else ended, dev["episode"],
                              G, out=out, count=count)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("E,T,G,O,shape", CONFIGS)
def test_rows_are_the_reference_bit_for_bit(E, T, G, O, shape):
    p, ref, dev = case(E, T, G, O, shape)
    env = task_env(T, shape)
    before = {k: v.clone() for k, v in dev.items()}
    out, count = run(env, dev, G)
    print(f"E={E} T={T} G={G} O={O} {shape}: {count} rows, reference {len(ref)}; cases {sorted(H.census(p, SEED, BASE, G))}")
    assert count == len(ref)
    assert np.array_equal(bits(out[:count]), bits(ref))
    assert np.all(out[count:] == SENTINEL)                       # rows beyond the count are not written
    for k, v in dev.items():                                     # the buffers are only read (envs in mid-episode included)
        assert torch.equal(v, before[k]), k
    again, count2 = run(env, dev, G)                             # the same bits on every call
    assert count2 == count and np.array_equal(bits(again), bits(out))


def test_the_probes_hold_every_case():
    union = set()
    for E, T, G, O, shape in CONFIGS:
        union |= H.census(case(E, T, G, O, shape)[0], SEED, BASE, G)
    assert union == set(H.CASES)
    assert H.census(case(64, 3, 4, 0, "trapezoid")[0], SEED, BASE, 4) == set(H.CASES)


def test_nothing_ended_nothing_written():
    p, _ref, dev = case(64, 3, 4, 0, "trapezoid")
    out, count = run(task_env(3, "trapezoid"), dev, 4, ended=torch.zeros(64, dtype=torch.bool, device=DEV))
    assert count == 0 and np.all(out == SENTINEL)


def test_argument_errors_launch_nothing():
    from bridges_hip import abi
    from bridges_hip.ops import _ptr, _stream
    L = abi.lib()
    p, _ref, dev = case(5, 3, 4, 2, "hexagon")
    env = task_env(3, "hexagon")
    E, K, W = dev["buf"].shape
    out = torch.full((E * K * 4, W), SENTINEL, dtype=torch.float64, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(4 * E * 4, dtype=torch.uint8, device=DEV)
    ended = dev["ended"].view(torch.uint8)
    good = dict(E=E, K=K, W=W, T=3, G=4, buf=_ptr(dev["buf"]), flags=_ptr(dev["flags"]), len=_ptr(dev["length"]), ended=_ptr(ended),
                episode=_ptr(dev["episode"]), seed=SEED, base=BASE, shapes=env.table.ptr, n_shapes=len(env.table_geoms),
                target_shape=len(env.table_geoms) - 1, gx=_ptr(env.grid_x_dev), gy=_ptr(env.grid_y_dev), img=64,
                gauss=C.c_void_p(env._gauss_k.data_ptr()), out=_ptr(out), count=_ptr(count), scratch=_ptr(scratch),
                scratch_bytes=scratch.numel())

    def call(**kw):
        a = dict(good, **kw)
        return L.bridges_hindsight_relabel(*a.values(), _stream())
    null = C.c_void_p(0)
    bad = [dict(G=0), dict(G=5), dict(E=-1), dict(K=0), dict(K=17), dict(T=0), dict(T=9), dict(W=R.RECORD_WIDTH + 8), dict(img=65),
           dict(n_shapes=0), dict(target_shape=2), dict(scratch_bytes=4 * E * 4 - 1),
           dict(out=C.c_void_p(out.data_ptr() + 4))]
    bad += [{k: null} for k in ("buf", "flags", "len", "ended", "episode", "shapes", "gx", "gy", "gauss", "out", "count", "scratch")]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "hindsight" in L.bridges_last_error().decode(), kw
    assert call(E=0) == 0                                         # succeeds and launches nothing
    torch.cuda.synchronize()
    assert int(count.item()) == -1 and bool((out == SENTINEL).all())
    need = C.c_int64(0)
    assert L.bridges_hindsight_relabel_scratch(E, 0, C.byref(need)) == -1 and L.bridges_hindsight_relabel_scratch(E, 5, C.byref(need)) == -1
    assert call() == 0                                            # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert int(count.item()) == len(_ref)


@pytest.mark.parametrize("shape", ("trapezoid", "hexagon"))
def test_an_env_on_the_hindsight_targets_records_the_relabelled_rows(shape):
    """Independent of the restatement: roll out the first episode of every env under random targets, relabel it, then give a
    second env the hindsight targets as its per-env targets and replay the recorded placements with step(sel_index).  Its reward,
    lin_reward (the rasteriser's cand_lin through k_step's rule) and step flags are what the relabelled rows hold, bitwise."""
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import RandomTargets, VecAssemblyGym
    E, T, MAXS = 48, 3, 6
    geoms = [load_urdf(f"shapes/{shape}.urdf")]
    env = VecAssemblyGym(E, geoms, [], RandomTargets(T), max_steps=MAXS, seed=SEED, env_id_base=BASE, device=DEV)
    env.reset()
    hb = R.HindsightBuffer(E, R.RECORD_WIDTH + 3 * T, DEV, goals=1, n_blocks=env.K)
    sels, rows_of, first_over = [], {}, torch.zeros(E, dtype=torch.bool, device=DEV)
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
            rows_of[e] = got[got[:, R.O_TD] == e].copy()
        assert sum(len(rows_of[e]) for e in torch.nonzero(ended & ~first_over).flatten().tolist()) == len(got)
        sels.append(sel)
        first_over |= ended
    assert len(rows_of) >= E // 2 and sum(len(r) for r in rows_of.values()) >= E
    targets = env.env_targets.cpu().numpy().copy()
    for e, rows in rows_of.items():
        if len(rows):
            targets[e] = rows[0][R.RECORD_WIDTH:].reshape(T, 3)
    twin = VecAssemblyGym(E, geoms, [], targets, max_steps=MAXS, seed=SEED, env_id_base=BASE, device=DEV)
    twin.reset()
    checked = early = 0
    for t in range(MAXS):
        # an env whose compared steps are over plays on with a valid action of its own
        twin.select_random()
        replayed = torch.tensor([e in rows_of and t < len(rows_of[e]) for e in range(E)], device=DEV)
        twin.step(torch.where(replayed, sels[t], twin.buf["sel_index"]))
        torch.cuda.synchronize()
        reward, lin, fl = twin.reward.cpu().numpy(), twin.lin_reward.cpu().numpy(), twin.step_flags.cpu().numpy()
        for e, rows in rows_of.items():
            if t >= len(rows):
                continue
            row = rows[t]
            assert int(row[R.O_NB]) == t and fl[e, 0] == 1, (e, t)
            assert np.float32(row[R.O_REWARD]).tobytes() == reward[e].tobytes(), (e, t, row[R.O_REWARD], reward[e])
            assert np.float32(row[R.O_LIN]).tobytes() == lin[e].tobytes() and float(np.float32(row[R.O_LIN])) == row[R.O_LIN], (e, t)
            assert bool(row[R.O_DONE]) == bool(fl[e, 5] | fl[e, 6]), (e, t)
            assert bool(row[R.O_STABLE_N]) == bool(fl[e, 1]), (e, t)
            if t == len(rows) - 1 and fl[e, 3] and fl[e, 1]:
                early += 1                                        # terminated while stable: every hindsight target reached
            checked += 1
    print(f"{shape}: {checked} steps of {len(rows_of)} episodes compared, {early} ended on the hindsight targets")
    assert checked >= E and early >= 1
