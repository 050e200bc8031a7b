"""GPU: the Munchausen operators.  bridges_soft_value / bridges_soft_value_rel against the rule and the bound of
tests/munchausen_ref.py (checked without a GPU, with its defective twins, by tests/test_cpu_munchausen.py) -- the relative form at
the device's own temp_out bits --, equal bits on a second call, every output inside sentinels, the refusals; bridges_action_row
on a hand-made table and on a small env; load_records(prev=True) against records.unpack_states + load_states."""
import ctypes as C

import numpy as np
import pytest
import torch

import munchausen_ref as M
import relative_temperature_ref as RT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0
PAD = 8
F32 = M.f32
OUT_DTYPES = dict(value=torch.float32, tlogp=torch.float32, bonus=torch.float32, miss=torch.uint8, temp_out=torch.float64)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def padded(n, dtype):
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def guards_intact(buf, n):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_value(case, relative=False, floor=RT.FLOOR, taken=True):
    """bridges_soft_value (relative: _rel) on a case, outputs inside sentinels; asserts the sentinels, that the inputs were only
    read and that what the call does not write stays unwritten -> dict of numpy outputs."""
    from bridges_hip import abi
    L = abi.require_gpu()
    n = len(case["seg_lo"])
    lo, hi, q = dev(case["seg_lo"]), dev(case["seg_hi"]), dev(case["q"])
    row = dev(case["taken_row"]) if taken else None
    keep = [(t, t.clone()) for t in (lo, hi, q, row) if t is not None]
    bufs = {k: padded(n, dt) for k, dt in OUT_DTYPES.items()}
    o = {k: v[1] for k, v in bufs.items()}
    head = (n, _ptr(lo), _ptr(hi), _ptr(q), float(case["T"]))
    tail = (_ptr(row), float(case["alpha"]), float(case["clip_lo"]), _ptr(o["value"]), _ptr(o["tlogp"]), _ptr(o["bonus"]), _ptr(o["miss"]))
    if relative:
        abi.check(L.bridges_soft_value_rel(*head, float(floor), *tail, _ptr(o["temp_out"]), abi.current_stream()), "bridges_soft_value_rel")
    else:
        abi.check(L.bridges_soft_value(*head, *tail, abi.current_stream()), "bridges_soft_value")
    torch.cuda.synchronize()
    written = {"value"} | ({"tlogp", "bonus", "miss"} if taken else set()) | ({"temp_out"} if relative else set())
    for k, (buf, _) in bufs.items():
        assert guards_intact(buf, n), k
        if k not in written:
            assert bool((buf == SENTINEL).all()), k
    for t, was in keep:
        assert same_bits(t.cpu().numpy(), was.cpu().numpy())
    return {k: o[k].cpu().numpy() for k in written}


def conforms(case, what, relative=False, floor=RT.FLOOR):
    got, again = run_value(case, relative, floor), run_value(case, relative, floor)
    for key in got:
        assert same_bits(got[key], again[key]), key                                         # a second call: the same bits
    temps = None
    if relative:
        want, bound = RT.temperatures(case["seg_lo"], case["seg_hi"], case["q"], case["T"], floor)
        err = np.abs(got["temp_out"] - want)
        print(what, "largest |temp_out - T_e| / bound", float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        assert (err <= bound).all(), (what, np.flatnonzero(~(err <= bound))[:8])
        temps = got["temp_out"]                                                             # the device's own bits as T
    ref = M.reference(case, temps=temps)
    figures = {}
    bad = M.violations(got, ref, figures)
    print(what, "segments", len(case["seg_lo"]), "largest |error| / bound:", {k: round(v, 4) for k, v in figures.items()})
    assert not bad, (what, bad[:5])
    only = run_value(case, relative, floor, taken=False)                                    # taken_row NULL: the value alone, the same bits
    assert same_bits(only["value"], got["value"])
    return got, ref


# ------------------------------------------------------------------------------------------------------------ 1: the log-sum-exp value
@pytest.mark.parametrize("T", M.TEMPERATURES)
def test_every_segment_length_shared_and_overlapping_ranges(T):
    case = M.random_probe(T)
    lengths = set((case["seg_hi"].astype(int) - case["seg_lo"]).tolist())
    assert set(M.SEG_LENGTHS) <= lengths
    got, ref = conforms(case, f"random T={T}")
    assert 0 < int(ref["miss"].sum()) < len(ref["miss"])


@pytest.mark.parametrize("n", M.N_SEGMENTS)
def test_a_partly_filled_last_workgroup(n):
    conforms(M.random_probe(1.0, n=n, seed=73100 + n), f"n={n}")
    conforms(M.random_probe(0.1, n=n, seed=73200 + n), f"rel n={n}", relative=True)


def test_nan_and_infinite_rows():
    for k, case in enumerate(M.nonfinite_probe()):
        got, ref = conforms(case, f"nonfinite {k}")
        assert same_bits(got["miss"], ref["miss"])
    got, ref = conforms(M.nonfinite_probe()[4], "m = +inf")                                 # the +inf rows: V = +inf, L = -T ln 2
    assert got["value"][0] == np.inf and got["miss"][0] == 0 and abs(got["tlogp"][0] + 0.5 * np.log(2.0)) < 1e-6
    got, _ = conforms(M.nonfinite_probe()[5], "m = +inf, a finite row")
    assert got["tlogp"][0] == -np.inf and got["bonus"][0] == np.float32(0.9) * np.float32(-1.0) and got["miss"][0] == 0


def test_tied_rows():
    case = M.tied_probe()
    got, _ = conforms(case, "tied")
    n = (case["seg_hi"] - case["seg_lo"]).astype(np.float64)
    T = F32(case["T"])
    assert np.allclose(got["value"], case["q"][case["seg_lo"]] + T * np.log(n), rtol=3e-7, atol=0)
    assert np.allclose(got["tlogp"], -T * np.log(n), rtol=3e-7, atol=0)


def test_single_rows_are_exact():
    case = M.single_probe()
    for relative in (False, True):
        got, _ = conforms(case, "single", relative=relative)
        assert same_bits(got["value"], case["q"])                                          # V == q
        assert same_bits(got["bonus"], np.zeros(len(case["q"]), np.float32))                # +0.0
        assert same_bits(got["tlogp"], np.zeros(len(case["q"]), np.float32)) and not got["miss"].any()


def test_a_large_offset_at_a_small_temperature_and_exponents_past_709():
    got, ref = conforms(M.offset_probe(), "offset")
    live = ~ref["nothing"]
    assert np.isfinite(got["value"][live]).all() and (got["value"][live] >= 1e4 - 10).all()
    conforms(M.offset_probe(seed=73501), "offset rel", relative=True)
    case = dict(seg_lo=np.asarray([0], np.int32), seg_hi=np.asarray([3], np.int32), q=np.asarray([800.0, 799.0, 0.0], np.float32), T=1.0,
                taken_row=np.asarray([2], np.int32), alpha=1.0, clip_lo=-1000.0)
    got, _ = conforms(case, "q / T = 800")
    assert np.isfinite(got["value"][0]) and abs(got["tlogp"][0] + 800.0) < 1.0 and got["bonus"][0] == got["tlogp"][0]


@pytest.mark.parametrize("kw", [dict(alpha=0.0), dict(clip_lo=0.0)])
def test_alpha_or_clip_zero_write_positive_zero_everywhere(kw):
    for case in [M.random_probe(0.1, **kw), M.random_probe(1e-3, **kw)] + M.nonfinite_probe(**kw):
        got, _ = conforms(case, str(kw))
        assert same_bits(got["bonus"], np.zeros(len(case["seg_lo"]), np.float32))


def test_a_taken_row_that_is_no_eligible_row_of_its_segment_misses():
    q = np.asarray([0.5, 1.0, np.nan, -np.inf, 2.0, 3.0, 0.25], dtype=np.float32)
    lo, hi = np.full(7, 1, np.int32), np.full(7, 5, np.int32)
    taken = np.asarray([0, 5, M.NONE_ROW, 2, 3, -1, 4], dtype=np.int32)                    # before, behind, the sentinel, NaN, -inf, < 0; one hit
    case = dict(seg_lo=lo, seg_hi=hi, q=q, T=1.0, taken_row=taken, alpha=0.9, clip_lo=-1.0)
    got, _ = conforms(case, "misses")
    assert got["miss"].tolist() == [1, 1, 1, 1, 1, 1, 0]
    assert not got["tlogp"][:6].any() and same_bits(got["bonus"][:6], np.zeros(6, np.float32)) and got["tlogp"][6] < 0


@pytest.mark.parametrize("multiple", (0.1, 1.0))
def test_the_relative_form_at_the_devices_own_temperature(multiple):
    case = M.random_probe(multiple, seed=73300)
    got, ref = conforms(case, f"rel {multiple}", relative=True)
    fixed = np.asarray([np.isfinite(case["q"][a:b]).sum() < 2 if b > a else True for a, b in zip(case["seg_lo"], case["seg_hi"])])
    assert (got["temp_out"][fixed] == F32(multiple) * F32(RT.FLOOR)).all() and (got["temp_out"] > 0).all()
    tied = M.tied_probe()
    got, _ = conforms(tied, "rel tied", relative=True, floor=0.25)                           # the floor binds
    assert (got["temp_out"] == F32(tied["T"]) * 0.25).all()
    for k, c in enumerate(M.nonfinite_probe()):
        conforms(c, f"rel nonfinite {k}", relative=True)


def test_operator_wrapper_returns_what_the_entry_point_writes():
    from bridges_hip import dqn_ops
    case = M.random_probe(1.0, n=9)
    seg = (dev(case["seg_lo"]), dev(case["seg_hi"]))
    raw = run_value(case)
    out = dqn_ops.soft_value(seg, dev(case["q"]), 1.0, taken_row=dev(case["taken_row"]), alpha=case["alpha"], clip_lo=case["clip_lo"])
    assert len(out) == 4
    for key, t in zip(("value", "tlogp", "bonus", "miss"), out):
        assert same_bits(t.cpu().numpy(), raw[key]), key
    alone = dqn_ops.soft_value(seg, dev(case["q"]), 1.0)
    assert alone[1] is None and alone[2] is None and alone[3] is None and same_bits(alone[0].cpu().numpy(), raw["value"])
    raw = run_value(case, relative=True, floor=0.5)
    out = dqn_ops.soft_value(seg, dev(case["q"]), 1.0, taken_row=dev(case["taken_row"]), alpha=case["alpha"], clip_lo=case["clip_lo"],
                             relative=True, spread_floor=0.5)
    assert len(out) == 5 and same_bits(out[4].cpu().numpy(), raw["temp_out"]) and same_bits(out[2].cpu().numpy(), raw["bonus"])
    offsets = torch.tensor([0, 3, 3, 70], dtype=torch.int32, device=DEV)                     # the prefix-sum form
    q = dev(case["q"])
    a = dqn_ops.soft_value(offsets, q, 0.5)[0]
    b = dqn_ops.soft_value((offsets[:-1].clone(), offsets[1:].clone()), q, 0.5)[0]
    assert torch.equal(a, b) and float(a[1]) == -np.inf


def test_refusals_launch_nothing():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = M.random_probe(1.0, n=6)
    n = 6
    t = dict(lo=dev(case["seg_lo"]), hi=dev(case["seg_hi"]), q=dev(case["q"]), row=dev(case["taken_row"]))
    outs = dict(value=torch.full((n,), SENTINEL, device=DEV), tlogp=torch.full((n,), SENTINEL, device=DEV),
                bonus=torch.full((n,), SENTINEL, device=DEV), miss=torch.full((n,), 7, dtype=torch.uint8, device=DEV),
                temp=torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV))
    base = dict(n=n, T=1.0, F=1e-3, alpha=0.9, clip=-1.0, **{k: _ptr(v) for k, v in t.items()}, **{k: _ptr(v) for k, v in outs.items()})

    def call(rel, **kw):
        a = dict(base, **kw)
        head = (a["n"], a["lo"], a["hi"], a["q"], a["T"])
        tail = (a["row"], a["alpha"], a["clip"], a["value"], a["tlogp"], a["bonus"], a["miss"])
        if rel:
            return L.bridges_soft_value_rel(*head, a["F"], *tail, a["temp"], abi.current_stream())
        return L.bridges_soft_value(*head, *tail, abi.current_stream())
    null, inf, nan = C.c_void_p(0), float("inf"), float("nan")
    bad = [dict(n=-1), dict(T=0.0), dict(T=-1.0), dict(T=inf), dict(T=nan), dict(lo=null), dict(hi=null), dict(q=null), dict(value=null),
           dict(q=C.c_void_p(t["q"].data_ptr() + 2)), dict(value=C.c_void_p(outs["value"].data_ptr() + 1)),
           dict(row=C.c_void_p(t["row"].data_ptr() + 2)),                                                       # bridges_soft_expect's
           dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan), dict(alpha=inf), dict(clip=0.5), dict(clip=-inf), dict(clip=nan), dict(clip=inf),
           dict(tlogp=null), dict(bonus=null), dict(miss=null)]
    for rel, name in ((False, "bridges_soft_value"), (True, "bridges_soft_value_rel")):
        for kw in bad + ([dict(F=0.0), dict(F=-1.0), dict(F=inf), dict(F=nan), dict(temp=null),
                          dict(temp=C.c_void_p(outs["temp"].data_ptr() + 4))] if rel else []):
            assert call(rel, **kw) == -1, (name, kw)
            assert name in L.bridges_last_error().decode(), (name, kw)
        torch.cuda.synchronize()
        assert all(bool((v == 7).all()) for v in outs.values())                             # a refusal launches nothing
        assert call(rel, n=0) == 0
        torch.cuda.synchronize()
        assert all(bool((v == 7).all()) for v in outs.values())
    assert call(False, row=null, tlogp=null, bonus=null, miss=null) == 0                     # no taken row: the three may be NULL
    torch.cuda.synchronize()
    assert bool((outs["value"] != SENTINEL).all()) and all(bool((outs[k] == 7).all()) for k in ("tlogp", "bonus", "miss", "temp"))
    assert call(True) == 0
    torch.cuda.synchronize()
    assert float(outs["temp"][n]) == SENTINEL and bool((outs["temp"][:n] > 0).all()) and bool((outs["miss"] <= 1).all())


# ------------------------------------------------------------------------------------------------------------ 2: the taken row
def run_action_row(t, stride_pad=0):
    from bridges_hip import abi
    L = abi.require_gpu()
    n = len(t["seg_lo"])
    rec = t["rec"]
    if stride_pad:                                           # rows that stand further apart than they are wide
        wide = np.full((n, rec.shape[1] + stride_pad), np.nan)
        wide[:, :rec.shape[1]] = rec
        rec = wide
    d = {k: dev(v) for k, v in dict(t, rec=rec).items()}
    keep = {k: v.clone() for k, v in d.items()}
    buf, row = padded(n, torch.int32)
    abi.check(L.bridges_action_row(n, _ptr(d["seg_lo"]), _ptr(d["seg_hi"]), _ptr(d["idx"]), _ptr(d["cand_desc"]), _ptr(d["cand_pose"]),
                                   _ptr(d["rec"]), rec.shape[1], _ptr(row), abi.current_stream()), "bridges_action_row")
    torch.cuda.synchronize()
    assert guards_intact(buf, n)
    for k in d:
        assert same_bits(d[k].cpu().numpy(), keep[k].cpu().numpy()), k
    return row.cpu().numpy()


def test_action_row_on_the_hand_made_table():
    t = M.action_row_table()
    want = M.action_row(**t)
    got = run_action_row(t)
    assert same_bits(got, want), (got, want)
    assert same_bits(run_action_row(t), got) and same_bits(run_action_row(t, stride_pad=5), got)
    for twin in M.ROW_TWINS:                                 # the descriptor alone, and a float compare of the pose, say otherwise
        assert not np.array_equal(M.action_row(**t, twin=twin), got), twin
    assert got[5] == M.NONE_ROW and got[6] == M.NONE_ROW and got[8] == M.NONE_ROW           # empty; the sign of a zero; no such pose


def test_action_row_over_more_rows_than_a_wave_and_a_partly_filled_workgroup():
    rng = np.random.default_rng(11)
    C_, n = 700, 6
    desc = np.tile(np.asarray([[0, 1, 0, 2]], np.int32), (C_, 1))                           # one descriptor: the pose alone decides
    pose = rng.standard_normal((C_, 4))
    idx = rng.permutation(C_).astype(np.int64)
    lo = np.asarray([0, 0, 100, 630, 64, 0], np.int32)
    hi = np.asarray([700, 64, 229, 700, 65, 700], np.int32)
    at = [699, 63, 228, 630, 64, None]                                                      # the last lane of the last chunk, ...
    rec = np.zeros((n, M.RECORD_WIDTH))
    for i, j in enumerate(at):
        rec[i, [M.O_ATB, M.O_ATF, M.O_ASHAPE, M.O_AFACE]] = desc[0]
        rec[i, M.O_APOSE:M.O_APOSE + 4] = pose[idx[j]] if j is not None else 0.0
    t = dict(seg_lo=lo, seg_hi=hi, idx=idx, cand_desc=desc, cand_pose=pose, rec=rec)
    got = run_action_row(t)
    assert got.tolist() == [699, 63, 228, 630, 64, M.NONE_ROW] and same_bits(got, M.action_row(**t))


def test_action_row_refusals_launch_nothing():
    from bridges_hip import abi
    L = abi.require_gpu()
    t = M.action_row_table()
    n = len(t["seg_lo"])
    d = {k: dev(v) for k, v in t.items()}
    row = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    base = dict(n=n, stride=t["rec"].shape[1], row=_ptr(row), **{k: _ptr(v) for k, v in d.items()})

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_action_row(a["n"], a["seg_lo"], a["seg_hi"], a["idx"], a["cand_desc"], a["cand_pose"], a["rec"], a["stride"], a["row"],
                                    abi.current_stream())
    null = C.c_void_p(0)
    bad = [dict(n=-1), dict(stride=M.RECORD_WIDTH - 1), dict(stride=0), dict(stride=-5)] + [{k: null} for k in list(d) + ["row"]]
    bad += [dict(idx=C.c_void_p(d["idx"].data_ptr() + 4)), dict(cand_pose=C.c_void_p(d["cand_pose"].data_ptr() + 4)),
            dict(rec=C.c_void_p(d["rec"].data_ptr() + 4)), dict(cand_desc=C.c_void_p(d["cand_desc"].data_ptr() + 4)),
            dict(row=C.c_void_p(row.data_ptr() + 2)), dict(seg_lo=C.c_void_p(d["seg_lo"].data_ptr() + 1))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "bridges_action_row" in L.bridges_last_error().decode(), kw
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((row == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert same_bits(row.cpu().numpy(), M.action_row(**t))


def two_shape_env(E, seed):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    H = 0.8
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf"), load_urdf("shapes/hexagon.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)],
                          [(0.5, 0, 2 * H + H / 2)], max_steps=8, seed=seed)


def test_prev_unpack_and_action_row_on_a_small_env():
    """Eight envs of two shapes: load_records(prev=True) leaves the scratch env in the very state unpack_states(rec)[0] + load_states
    do, bit for bit, and bridges_action_row finds every record's action among the rebuilt candidates of s -- the candidate the
    rollout env placed."""
    from bridges_hip import dqn_ops
    from robotoddler.training import records as R
    E = 8
    env, renv_a, renv_b = two_shape_env(E, 7), two_shape_env(E, 1), two_shape_env(E, 2)
    steps = 0
    for it in range(7):
        env.select_random()
        sel = env.cand_offset[:E].long() + env.sel_index.long()
        sel_index = env.sel_index.clone()
        state_bits = env.state_bits.clone()
        rec = R.pack_state(env, sel)
        env.step()
        valid = R.pack_result(env, rec)
        for n_rec in (E, 5):
            part = rec[:n_rec].contiguous()
            full = torch.cat([part, part[:1].expand(E - n_rec, -1)]).contiguous() if n_rec < E else part
            renv_a.load_states(*R.unpack_states(full, renv_a.K)[0])
            bits_s, lin, stable_s, done, stable_n = renv_b.load_records(part, prev=True)
            assert torch.equal(bits_s, renv_b.state_bits)                                   # both ranges cover s
            assert torch.equal(lin, full[:, R.O_LIN].float()) and torch.equal(stable_s, full[:, R.O_STABLE_S].float())
            assert torch.equal(done.bool(), full[:, R.O_DONE] > 0.5) and torch.equal(stable_n.bool(), full[:, R.O_STABLE_N] > 0.5)
            for name in ("n_blocks", "blk_shape", "blk_pose", "blk_occ", "n_cand", "n_valid", "state_bits"):
                assert torch.equal(renv_a.buf[name], renv_b.buf[name]), name
            tot = int(renv_a.cand_offset[E])
            assert tot == int(renv_b.cand_offset[E])
            assert torch.equal(renv_a.buf["cand_mask"][:tot], renv_b.buf["cand_mask"][:tot])
        v = valid.bool()
        assert torch.equal(renv_b.state_bits[:5][v[:5]], state_bits[:5][v[:5]])              # s, as the rollout env held it
        renv_b.load_records(rec, prev=True)
        idx, _ = renv_b.valid_rows()
        seg = renv_b.valid_segments()
        row = dqn_ops.action_row(renv_b, seg, idx, rec)
        torch.cuda.synchronize()
        want = M.action_row(seg[0].cpu().numpy(), seg[1].cpu().numpy(), idx.cpu().numpy(), renv_b.buf["cand_desc"].cpu().numpy(),
                            renv_b.buf["cand_pose"].cpu().numpy(), rec.cpu().numpy())
        assert same_bits(row.cpu().numpy(), want)
        found = row[v].long()
        assert bool((found != M.NONE_ROW).all())
        assert torch.equal((idx[found] - renv_b.cand_offset[:E][v].long()).to(torch.int32), sel_index[v])   # the candidate placed
        assert bool(((found >= seg[0][v]) & (found < seg[1][v])).all())
        steps += int(v.sum())
    assert steps > 3 * E
