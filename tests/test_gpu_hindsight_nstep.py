"""GPU: bridges_hindsight_relabel_nstep against tests/hindsight_nstep_ref.py bit for bit on sentinel-filled outputs, on the scripted
probe episodes of tests/hindsight_ref.py (tests/test_cpu_hindsight_nstep.py checks on the CPU that they hold every case of the
rule): the count, the rows beyond it, the inputs, a second call; n = 1 against the one-step entry's own output; and every argument
the entry refuses."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hindsight_nstep_ref as HN
import hindsight_ref as H
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, BASE, CONFIGS = H.PROBE_SEED, H.PROBE_BASE, H.PROBE_CONFIGS
NS, GAMMA = (1, 2, 3, 8), 0.95
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
    """The probe, its relabelled walks (computed once, shared by the tests, never written) and the device copies of the inputs."""
    p = H.probe(E, T, O, shape, seed=H.probe_seed(E))
    ws = HN.walks(p["buf"], p["flags"], p["length"], p["ended"], p["episode"], p["shapes"], SEED, BASE, G, T)
    for _e, _g, rows in ws:
        rows.setflags(write=False)
    dev = {k: torch.from_numpy(p[k]).to(DEV) for k in ("buf", "flags", "length", "ended", "episode")}
    return p, ws, dev


def run(env, dev, G, n, ended=None, gamma=GAMMA):
    from bridges_hip import dqn_ops
    E, K, W = dev["buf"].shape
    out = torch.full((E * K * G, W + 1), SENTINEL, dtype=torch.float64, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    dqn_ops.hindsight_relabel(env, dev["buf"], dev["flags"], dev["length"], dev["ended"] if ended is None else ended, dev["episode"],
                              G, out=out, count=count, n_step=n, gamma=gamma)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("E,T,G,O,shape", CONFIGS)
def test_rows_are_the_reference_bit_for_bit(E, T, G, O, shape, n):
    p, ws, dev = case(E, T, G, O, shape)
    ref = HN.fold_walks(ws, p["buf"], n, GAMMA)
    env = task_env(T, shape)
    before = {k: v.clone() for k, v in dev.items()}
    out, count = run(env, dev, G, n)
    print(f"E={E} T={T} G={G} O={O} {shape} n={n}: {count} rows, reference {len(ref)}; cases {sorted(HN.census(ws, n, p['K']))}")
    assert count == len(ref)
    assert np.array_equal(bits(out[:count]), bits(ref))
    assert np.all(out[count:] == SENTINEL)                       # rows beyond the count are not written
    for k, v in dev.items():                                     # the buffers are only read (envs in mid-episode included)
        assert torch.equal(v, before[k]), k
    again, count2 = run(env, dev, G, n)                          # the same bits on every call
    assert count2 == count and np.array_equal(bits(again), bits(out))


@pytest.mark.parametrize("E,T,G,O,shape", CONFIGS)
def test_one_step_is_the_one_step_entry_with_a_column_of_ones(E, T, G, O, shape):
    from bridges_hip import dqn_ops
    _p, _ws, dev = case(E, T, G, O, shape)
    env = task_env(T, shape)
    K, W = dev["buf"].shape[1:]
    one = torch.full((E * K * G, W), SENTINEL, dtype=torch.float64, device=DEV)
    count1 = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    dqn_ops.hindsight_relabel(env, dev["buf"], dev["flags"], dev["length"], dev["ended"], dev["episode"], G, out=one, count=count1)
    out, count = run(env, dev, G, 1)
    one = one.cpu().numpy()
    assert count == int(count1.item()) and count > 0
    assert np.array_equal(bits(out[:count, :W]), bits(one[:count])) and np.all(out[:count, W] == 1.0)
    assert np.all(out[count:] == SENTINEL) and np.all(one[count:] == SENTINEL)
    for n in NS[1:]:                                             # the count does not depend on the window
        assert run(env, dev, G, n)[1] == count


def test_nothing_ended_nothing_written():
    _p, _ws, dev = case(64, 3, 4, 0, "trapezoid")
    out, count = run(task_env(3, "trapezoid"), dev, 4, 3, ended=torch.zeros(64, dtype=torch.bool, device=DEV))
    assert count == 0 and np.all(out == SENTINEL)


def test_argument_errors_launch_nothing():
    from bridges_hip import abi, dqn_ops
    from bridges_hip.ops import _ptr, _stream
    L = abi.lib()
    p, ws, dev = case(5, 3, 4, 2, "hexagon")
    env = task_env(3, "hexagon")
    E, K, W = dev["buf"].shape
    out = torch.full((E * K * 4 + 1, W + 1), SENTINEL, dtype=torch.float64, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(4 * E * 4, dtype=torch.uint8, device=DEV)
    ended = dev["ended"].view(torch.uint8)
    good = dict(E=E, K=K, W=W, T=3, G=4, buf=_ptr(dev["buf"]), flags=_ptr(dev["flags"]), len=_ptr(dev["length"]), ended=_ptr(ended),
                episode=_ptr(dev["episode"]), seed=SEED, base=BASE, shapes=env.table.ptr, n_shapes=len(env.table_geoms),
                target_shape=len(env.table_geoms) - 1, gx=_ptr(env.grid_x_dev), gy=_ptr(env.grid_y_dev), img=64,
                gauss=C.c_void_p(env._gauss_k.data_ptr()), n_step=3, gamma=GAMMA, out=_ptr(out), count=_ptr(count),
                scratch=_ptr(scratch), scratch_bytes=scratch.numel())

    def call(**kw):
        a = dict(good, **kw)
        return L.bridges_hindsight_relabel_nstep(*a.values(), _stream())
    null = C.c_void_p(0)
    bad = [dict(G=0), dict(G=5), dict(E=-1), dict(K=0), dict(K=17), dict(T=0), dict(T=9), dict(W=R.RECORD_WIDTH + 8), dict(img=65),
           dict(n_shapes=0), dict(target_shape=2), dict(scratch_bytes=4 * E * 4 - 1),
           dict(out=C.c_void_p(out.data_ptr() + 4)),
           dict(n_step=0), dict(n_step=9), dict(gamma=float("nan")), dict(gamma=float("inf"))]
    bad += [{k: null} for k in ("buf", "flags", "len", "ended", "episode", "shapes", "gx", "gy", "gauss", "out", "count", "scratch")]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "hindsight" in L.bridges_last_error().decode(), kw
    assert call(E=0) == 0                                         # succeeds and launches nothing
    torch.cuda.synchronize()
    assert int(count.item()) == -1 and bool((out == SENTINEL).all())
    # the wrapper refuses in words before the call
    for kw in (dict(n_step=0, gamma=GAMMA), dict(n_step=9, gamma=GAMMA), dict(n_step=3, gamma=None), dict(n_step=3, gamma=float("nan")),
               dict(n_step=1, gamma=float("inf"))):
        with pytest.raises(ValueError, match="hindsight_relabel"):
            dqn_ops.hindsight_relabel(env, dev["buf"], dev["flags"], dev["length"], dev["ended"], dev["episode"], 4, **kw)
    assert call() == 0                                            # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    ref = HN.fold_walks(ws, p["buf"], 3, GAMMA)
    assert int(count.item()) == len(ref)
    assert np.array_equal(bits(out[:len(ref)].cpu().numpy()), bits(ref)) and bool((out[len(ref):] == SENTINEL).all())
