"""GPU: the relative-temperature operators (bridges_boltzmann_select_rel / bridges_soft_expect_rel).  temp_out against the exact
spread and the derived bound of tests/relative_temperature_ref.py (checked without a GPU, with its defective twins and the draw
condition, by tests/test_cpu_relative_temperature.py); every other output against the scalar operators' references at the
device's own temp_out bits; bit-exact agreement with the scalar kernels where the spread is exactly 1; exact scale invariance;
the greedy branch; the refusals.  Every output lies inside sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

import boltzmann_ref as B
import relative_temperature_ref as RT
import soft_target_ref as S
from test_gpu_boltzmann import check as check_select

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0
PAD = 8
SELECT_KEYS = ("sel_compact", "sel_index", "q_sel", "explore_w", "p_sel")
EXPECT_KEYS = ("value", "entropy", "argmax_row", "feat_mean")
F32 = lambda x: float(np.float32(x))


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


def run_select(case, floor=RT.FLOOR, greedy=False, relative=True):
    """bridges_boltzmann_select_rel (relative=False: the scalar entry point at case['T']) on a case, outputs inside sentinels;
    asserts the sentinels and that the inputs were only read -> dict of numpy outputs (temp_out too when relative)."""
    from bridges_hip import abi
    L = abi.require_gpu()
    E, n = len(case["u"]), len(case["q"])
    ins = {k: dev(case[k]) for k in ("seg_lo", "seg_hi", "q", "u", "idx", "cand_offset")}
    ins["rep"] = dev(case.get("rep"))
    keep = {k: v.clone() for k, v in ins.items() if v is not None}
    dtypes = dict(sel_compact=torch.int64, sel_index=torch.int32, q_sel=torch.float32, explore_w=torch.float32, p_sel=torch.float32,
                  temp_out=torch.float64)
    bufs = {k: padded(E, dt) for k, dt in dtypes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    head = (E, n, _ptr(ins["seg_lo"]), _ptr(ins["seg_hi"]), _ptr(ins["q"]), _ptr(ins["u"]), float(case["T"]))
    tail = (int(greedy), _ptr(ins["idx"]), _ptr(ins["cand_offset"]), _ptr(ins["rep"]), _ptr(o["sel_compact"]), _ptr(o["sel_index"]),
            _ptr(o["q_sel"]), _ptr(o["explore_w"]), _ptr(o["p_sel"]))
    if relative:
        abi.check(L.bridges_boltzmann_select_rel(*head, float(floor), *tail, _ptr(o["temp_out"]), abi.current_stream()),
                  "bridges_boltzmann_select_rel")
    else:
        abi.check(L.bridges_boltzmann_select(*head, *tail, abi.current_stream()), "bridges_boltzmann_select")
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert guards_intact(buf, E), k
        if not relative and k == "temp_out":
            assert bool((buf == SENTINEL).all())
    for k, v in keep.items():
        assert same_bits(ins[k].cpu().numpy(), v.cpu().numpy()), k                       # inputs are only read
    return {k: v.cpu().numpy() for k, v in o.items() if relative or k != "temp_out"}


def run_expect(case, floor=RT.FLOOR, relative=True):
    from bridges_hip import abi
    L = abi.require_gpu()
    n = len(case["seg_lo"])
    lo, hi, sel = dev(case["seg_lo"]), dev(case["seg_hi"]), dev(case["select_q"])
    nq = sel if case["next_q"] is case["select_q"] else dev(case["next_q"])
    dim = 0 if case["feat"] is None else case["feat"].shape[1]
    feat = dev(case["feat"]) if dim else None
    frow = dev(case.get("feat_row"))
    keep = [(t, t.clone()) for t in (lo, hi, sel, nq, feat, frow) if t is not None]
    bufs = dict(value=padded(n, torch.float32), entropy=padded(n, torch.float32), argmax_row=padded(n, torch.int32),
                feat_mean=padded(n * dim, torch.float32), temp_out=padded(n, torch.float64))
    o = {k: v[1] for k, v in bufs.items()}
    head = (n, _ptr(lo), _ptr(hi), _ptr(sel), _ptr(nq), float(case["T"]))
    tail = (_ptr(feat), feat.stride(0) if dim else 0, _ptr(frow), dim, _ptr(o["value"]), _ptr(o["feat_mean"]) if dim else C.c_void_p(0),
            _ptr(o["entropy"]), _ptr(o["argmax_row"]))
    if relative:
        abi.check(L.bridges_soft_expect_rel(*head, float(floor), *tail, _ptr(o["temp_out"]), abi.current_stream()), "bridges_soft_expect_rel")
    else:
        abi.check(L.bridges_soft_expect(*head, *tail, abi.current_stream()), "bridges_soft_expect")
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert guards_intact(buf, n * dim if k == "feat_mean" else n), k
    for t, was in keep:
        assert same_bits(t.cpu().numpy(), was.cpu().numpy())                             # inputs are only read
    out = {k: v.cpu().numpy() for k, v in o.items() if relative or k != "temp_out"}
    out["feat_mean"] = out["feat_mean"].reshape(n, dim)
    return out


def check_temp_out(got, want, bound, what, exact_value=None):
    """|temp_out - T_e| <= bound on every segment (bound 0: equality, the cases where the rule fixes the bits)."""
    err = np.abs(got - want)
    held = bound > 0
    print(what, "segments", len(want), "largest |temp_out - T_e| / bound",
          float(np.max(err[held] / bound[held], initial=0.0)), "exact segments", int((~held).sum()))
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], bound[bad[:8]])
    if exact_value is not None:
        assert (got[~held] == exact_value).all(), what


def no_finite_pair(q, lo, hi):
    return np.asarray([np.isfinite(q[a:b]).sum() < 2 if b > a else True for a, b in zip(lo, hi)])


# ------------------------------------------------------------------------------------------------------------ 1: temp_out and the draw
SELECT_CASES = RT.select_cases() + RT.select_exact_cases()


@pytest.mark.parametrize("k", range(len(SELECT_CASES)))
def test_select_temp_out_within_its_bound_and_the_draw_at_the_devices_own_temperature(k):
    case = SELECT_CASES[k]
    got, again = run_select(case), run_select(case)
    for key in got:
        assert same_bits(got[key], again[key]), key                                        # a second call: the same bits
    want, bound = RT.select_temperatures(case)
    check_temp_out(got["temp_out"], want, bound, f"select {k}")
    fixed = no_finite_pair(case["q"], case["seg_lo"], case["seg_hi"])                       # empty, no or one finite row
    assert (got["temp_out"][fixed] == F32(case["T"]) * F32(RT.FLOOR)).all()
    ref = RT.select_reference(case, got["temp_out"])                                        # the device's own bits as T
    check_select({key: got[key] for key in SELECT_KEYS}, ref, f"select {k}")


def test_select_where_the_floor_binds_writes_the_product_exactly():
    case = RT.select_tied_probe(0.3)
    for floor in (1e-3, 0.25, 7.0):
        got = run_select(case, floor=floor)
        assert (got["temp_out"] == F32(0.3) * F32(floor)).all()
    case = RT.select_offset_probe()                                                         # spreads of 0.003 .. 0.87 under a floor of 2
    got = run_select(case, floor=2.0)
    assert (got["temp_out"] == 2.0).all()
    check_select({key: got[key] for key in SELECT_KEYS}, B.reference(dict(case, T=2.0)), "floor 2")


# ------------------------------------------------------------------------------------------------------------ 2: the expectation
EXPECT_CASES = RT.expect_cases()


@pytest.mark.parametrize("k", range(len(EXPECT_CASES)))
def test_expect_temp_out_within_its_bound_and_the_outputs_at_the_devices_own_temperature(k):
    case = EXPECT_CASES[k]
    got, again = run_expect(case), run_expect(case)
    for key in got:
        assert same_bits(got[key], again[key]), key
    want, bound = RT.expect_temperatures(case)
    check_temp_out(got["temp_out"], want, bound, f"expect {k}")
    fixed = no_finite_pair(case["select_q"], case["seg_lo"], case["seg_hi"])
    assert (got["temp_out"][fixed] == F32(case["T"]) * F32(RT.FLOOR)).all()
    ref = RT.expect_reference(case, got["temp_out"])
    figures = {}
    bad = S.violations(got, ref, figures)
    print(f"expect {k}", "largest |error| / bound:", {key: round(v, 4) for key, v in figures.items()})
    assert not bad, bad[:5]


def test_expect_spread_is_select_qs_not_next_qs():
    case = S.random_probe(1.0, 0, double=True)
    got = run_expect(case)
    other, _ = RT.expect_temperatures(case, twin="spread_of_next_q")
    want, bound = RT.expect_temperatures(case)
    assert (np.abs(got["temp_out"] - want) <= bound).all() and (np.abs(got["temp_out"] - other) > bound)[bound > 0].any()


# ------------------------------------------------------------------------------------------------------------ 3: exact cross-checks
def unit_segments(rng):
    """Segments of RT.UNIT_LENGTHS, two of each, rows a - 1 / a + 1 in equal number: s = 1 exactly in any order of the sums."""
    lengths = np.repeat(RT.UNIT_LENGTHS, 2)
    lo = 3 + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    hi = lo + lengths
    q = np.zeros(int(hi[-1]) + 2, dtype=np.float32)
    for k, (a, b) in enumerate(zip(lo, hi)):
        q[a:b] = RT.unit_spread_rows(b - a, float([-3, 0, 2, 5][k % 4]), rng)
    return lo.astype(np.int32), hi.astype(np.int32), q


@pytest.mark.parametrize("T,floor", [(1.0, 1e-3), (0.1, 1.0), (0.37, 0.5)])
def test_select_equals_the_scalar_kernel_bit_for_bit_where_the_spread_is_one(T, floor):
    rng = np.random.default_rng(31)
    lo, hi, q = unit_segments(rng)
    E = 4 * len(lo)                                                                         # four draws per segment through (lo, hi) and rep
    idx = np.arange(len(q), dtype=np.int64) * 3 + 1
    case = dict(seg_lo=np.tile(lo, 4), seg_hi=np.tile(hi, 4), q=q, u=rng.random(E, dtype=np.float32), T=T, idx=idx,
                cand_offset=np.zeros(E, np.int32), rep=np.tile(np.arange(len(lo), dtype=np.int32), 4))
    rel, scalar = run_select(case, floor=floor), run_select(case, relative=False)
    assert (rel["temp_out"] == F32(T)).all()                                                # T * 1, exactly
    for key in SELECT_KEYS:
        assert same_bits(rel[key], scalar[key]), key
    assert len(set(rel["sel_compact"].tolist())) > len(lo)                                  # (the draws do spread over the rows)


@pytest.mark.parametrize("T,floor,dim", [(1.0, 1e-3, 5), (0.1, 1.0, 1027), (0.37, 0.5, 0)])
def test_expect_equals_the_scalar_kernel_bit_for_bit_where_the_spread_is_one(T, floor, dim):
    rng = np.random.default_rng(32)
    lo, hi, q = unit_segments(rng)
    R = len(q)
    case = dict(seg_lo=lo, seg_hi=hi, select_q=q, next_q=(3.0 * rng.standard_normal(R)).astype(np.float32), T=T,
                feat=rng.standard_normal((R, dim)).astype(np.float32) if dim else None, feat_row=None)
    rel, scalar = run_expect(case, floor=floor), run_expect(case, relative=False)
    assert (rel["temp_out"] == F32(T)).all()
    for key in EXPECT_KEYS:
        assert same_bits(rel[key], scalar[key]), key
    assert (rel["entropy"] > 0).all()


@pytest.mark.parametrize("T", RT.MULTIPLES)
def test_select_scale_invariance_is_exact(T):
    for case in (B.random_probe(T), RT.select_offset_probe(T)):
        scaled = dict(case, q=(case["q"] * np.float32(4.0)).astype(np.float32))
        assert np.array_equal(scaled["q"].astype(np.float64), 4.0 * case["q"].astype(np.float64))
        a, b = run_select(case, floor=RT.FLOOR), run_select(scaled, floor=F32(RT.FLOOR) * 4.0)
        assert same_bits(b["temp_out"], 4.0 * a["temp_out"])
        assert same_bits(b["q_sel"], np.float32(4.0) * a["q_sel"])
        for key in ("sel_compact", "sel_index", "explore_w", "p_sel"):
            assert same_bits(a[key], b[key]), key


@pytest.mark.parametrize("T,dim", [(1e-6, 5), (0.1, 1027), (1.0, 0), (1e30, 5)])
def test_expect_scale_invariance_is_exact(T, dim):
    for case in (S.random_probe(T, dim, mapped=dim == 1027, feat_rows=19), RT.expect_offset_probe(dim if dim != 1027 else 5, T)):
        scaled = dict(case, select_q=case["select_q"] * np.float32(4.0), next_q=case["next_q"] * np.float32(4.0))
        a, b = run_expect(case, floor=RT.FLOOR), run_expect(scaled, floor=F32(RT.FLOOR) * 4.0)
        assert same_bits(b["temp_out"], 4.0 * a["temp_out"])
        assert same_bits(b["value"], np.float32(4.0) * a["value"])
        for key in ("entropy", "argmax_row", "feat_mean"):
            assert same_bits(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------------------ 4: greedy
@pytest.mark.parametrize("T", (0.1, 1e30))
def test_greedy_is_the_scalar_operators_greedy_branch_and_writes_zero(T):
    for case in (B.random_probe(T), B.shared_probe(E=256), B.nonfinite_probe()[0], RT.select_tied_probe(T)):
        rel, scalar = run_select(case, greedy=True), run_select(case, greedy=True, relative=False)
        for key in SELECT_KEYS:
            assert same_bits(rel[key], scalar[key]), key
        assert same_bits(rel["temp_out"], np.zeros(len(case["u"])))                         # +0.0


# ------------------------------------------------------------------------------------------------------------ 5: the operator layer
def test_operator_wrappers_return_temp_out_as_a_further_result():
    from bridges_hip import dqn_ops, ops
    case = B.random_probe(1.0)
    seg = (dev(case["seg_lo"]), dev(case["seg_hi"]))
    out = ops.boltzmann_select(seg, dev(case["q"]), dev(case["u"]), 1.0, False, dev(case["idx"]), dev(case["cand_offset"]), relative=True)
    raw = run_select(case)
    assert len(out) == 6 and same_bits(out[5].cpu().numpy(), raw["temp_out"])
    for key, t in zip(SELECT_KEYS, out):
        assert same_bits(t.cpu().numpy(), raw[key]), key
    case = S.random_probe(1.0, 5)
    out = dqn_ops.soft_expect((dev(case["seg_lo"]), dev(case["seg_hi"])), dev(case["select_q"]), dev(case["next_q"]), 1.0,
                              feat=dev(case["feat"]), relative=True, spread_floor=0.5)
    raw = run_expect(case, floor=0.5)
    assert len(out) == 5 and same_bits(out[4].cpu().numpy(), raw["temp_out"])
    for key, t in zip(("value", "feat_mean", "entropy", "argmax_row"), out):
        assert same_bits(t.cpu().numpy(), raw[key]), key


# ------------------------------------------------------------------------------------------------------------ 6: refusals
def test_select_refusals_launch_nothing():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = B.random_probe(1.0)
    E, n = len(case["u"]), len(case["q"])
    t = {k: dev(case[k]) for k in ("seg_lo", "seg_hi", "q", "u", "idx", "cand_offset")}
    outs = dict(sel_compact=torch.full((E,), 7, dtype=torch.int64, device=DEV), sel_index=torch.full((E,), 7, dtype=torch.int32, device=DEV),
                **{k: torch.full((E,), 7.0, device=DEV) for k in ("q_sel", "explore_w", "p_sel")},
                temp_out=torch.full((E + 1,), 7.0, dtype=torch.float64, device=DEV))
    base = dict(E=E, n=n, T=1.0, F=1e-3, **{k: _ptr(v) for k, v in t.items()}, **{k: _ptr(v) for k, v in outs.items()})

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_boltzmann_select_rel(a["E"], a["n"], a["seg_lo"], a["seg_hi"], a["q"], a["u"], a["T"], a["F"], 0, a["idx"],
                                              a["cand_offset"], None, a["sel_compact"], a["sel_index"], a["q_sel"], a["explore_w"],
                                              a["p_sel"], a["temp_out"], abi.current_stream())
    null = C.c_void_p(0)
    bad = [dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(n=0), dict(n=-3), dict(E=-1)]     # the sibling's
    bad += [{k: null} for k in list(t) + list(outs)]
    bad += [dict(F=0.0), dict(F=-1e-3), dict(F=float("nan")), dict(F=float("inf")), dict(F=-float("inf")),
            dict(temp_out=C.c_void_p(outs["temp_out"].data_ptr() + 4))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "bridges_boltzmann_select_rel" in L.bridges_last_error().decode(), kw
    assert "spread floor" in (call(F=0.0), L.bridges_last_error().decode())[1]
    assert "temp_out" in (call(temp_out=null), L.bridges_last_error().decode())[1]
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())                                 # a refusal launches nothing
    assert call(E=0) == 0 and call(E=0, T=0.0, n=0) == 0                                    # nothing to do is answered first, as the sibling does
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())
    assert call() == 0
    torch.cuda.synchronize()
    assert float(outs["temp_out"][E]) == 7.0 and bool((outs["temp_out"][:E] > 0).all())


def test_expect_refusals_launch_nothing():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = S.random_probe(1.0, 8, n_trans=6)
    n, dim = 6, 8
    t = dict(lo=dev(case["seg_lo"]), hi=dev(case["seg_hi"]), sel=dev(case["select_q"]), nq=dev(case["next_q"]), feat=dev(case["feat"]),
             frow=torch.arange(len(case["select_q"]), dtype=torch.int64, device=DEV))
    outs = dict(value=torch.full((n,), SENTINEL, device=DEV), mean=torch.full((n, dim), SENTINEL, device=DEV),
                ent=torch.full((n,), SENTINEL, device=DEV), arg=torch.full((n,), 7, dtype=torch.int32, device=DEV),
                temp=torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV))
    base = dict(n=n, T=1.0, F=1e-3, stride=dim, dim=dim, **{k: _ptr(v) for k, v in t.items()}, **{k: _ptr(v) for k, v in outs.items()})

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_soft_expect_rel(a["n"], a["lo"], a["hi"], a["sel"], a["nq"], a["T"], a["F"], a["feat"], a["stride"], a["frow"],
                                         a["dim"], a["value"], a["mean"], a["ent"], a["arg"], a["temp"], abi.current_stream())
    null = C.c_void_p(0)
    bad = [dict(n=-1), dict(dim=-1), dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan")), dict(lo=null), dict(hi=null),
           dict(sel=null), dict(nq=null), dict(value=null), dict(arg=null), dict(feat=null), dict(mean=null), dict(stride=-8),
           dict(sel=C.c_void_p(t["sel"].data_ptr() + 2)), dict(value=C.c_void_p(outs["value"].data_ptr() + 1)),
           dict(feat=C.c_void_p(t["feat"].data_ptr() + 2)), dict(frow=C.c_void_p(t["frow"].data_ptr() + 4))]               # the sibling's
    bad += [dict(F=0.0), dict(F=-1.0), dict(F=float("inf")), dict(F=float("nan")), dict(temp=null),
            dict(temp=C.c_void_p(outs["temp"].data_ptr() + 4))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "bridges_soft_expect_rel" in L.bridges_last_error().decode(), kw
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())                                 # a refusal launches nothing
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())
    assert call(ent=null) == 0 and call(frow=null) == 0 and call(dim=0, feat=null, frow=null, mean=null) == 0
    torch.cuda.synchronize()
    assert float(outs["temp"][n]) == SENTINEL and bool((outs["temp"][:n] > 0).all())
