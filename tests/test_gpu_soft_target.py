"""GPU: the expected-value target operator (bridges_soft_expect) against the float64 rule and the bound of
tests/soft_target_ref.py (checked without a GPU, with its defective twins, by tests/test_cpu_soft_target.py), its refusals, and
its agreement with the max-operator target kernel where the two must agree."""
import ctypes as C

import numpy as np
import pytest
import torch

import soft_target_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0
PAD = 8                                                       # sentinel words in front of and behind every output


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def padded(n, dtype):
    """An output of n words inside a sentinel-filled buffer -> (buffer, the output's view)."""
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def guards_intact(buf, n):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())


def run(case, feat_dev=None, pair=False):
    """The entry point on a case, outputs inside sentinels -> dict of numpy outputs (asserting the sentinels around them).
    ``feat_dev``: the device tensor to pass for feat (a strided or offset view holding case['feat']).  ``pair``: segments as
    separate lo / hi arrays, else the prefix-sum form where the case allows it."""
    from bridges_hip import abi
    L = abi.require_gpu()
    B = len(case["seg_lo"])
    lo = torch.from_numpy(case["seg_lo"]).to(DEV)
    hi = torch.from_numpy(case["seg_hi"]).to(DEV)
    sel = torch.from_numpy(case["select_q"]).to(DEV)
    nq = sel if case["next_q"] is case["select_q"] else torch.from_numpy(case["next_q"]).to(DEV)
    dim = 0 if case["feat"] is None else case["feat"].shape[1]
    feat = feat_dev if feat_dev is not None else (torch.from_numpy(case["feat"]).to(DEV) if dim else None)
    frow = torch.from_numpy(case["feat_row"]).to(DEV) if case.get("feat_row") is not None else None
    vb, value = padded(B, torch.float32)
    eb, entropy = padded(B, torch.float32)
    ab, arg = padded(B, torch.int32)
    fb, mean = padded(B * dim, torch.float32)
    abi.check(L.bridges_soft_expect(B, _ptr(lo), _ptr(hi), _ptr(sel), _ptr(nq), float(case["T"]), _ptr(feat), feat.stride(0) if dim else 0,
                                    _ptr(frow), dim, _ptr(value), _ptr(mean) if dim else C.c_void_p(0), _ptr(entropy), _ptr(arg),
                                    abi.current_stream()), "bridges_soft_expect")
    torch.cuda.synchronize()
    assert guards_intact(vb, B) and guards_intact(eb, B) and guards_intact(ab, B) and guards_intact(fb, B * dim)
    return dict(value=value.cpu().numpy(), entropy=entropy.cpu().numpy(), argmax_row=arg.cpu().numpy(),
                feat_mean=mean.cpu().numpy().reshape(B, dim))


def conform(case, got, what):
    ref = S.reference(case)
    figures = {}
    bad = S.violations(got, ref, figures)
    print(what, "largest |error| / bound:", {k: round(v, 4) for k, v in figures.items()})
    assert not bad, (what, bad[:5])


# ------------------------------------------------------------------------------------------------------------ 1: the probe tables
@pytest.mark.parametrize("T", S.TEMPERATURES)
def test_kernel_on_the_random_probe_at_every_temperature(T):
    """Every segment length (0 .. 1025: beyond one LDS chunk), shared and overlapping ranges, planted ties, one and two value
    vectors, every output element against its bound; two calls give equal bits."""
    for double in (True, False):
        case = S.random_probe(T, 5, double=double)
        got = run(case)
        conform(case, got, ("random", T, double))
        again = run(case)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), k


def test_kernel_on_the_nonfinite_tables():
    for k, case in enumerate(S.nonfinite_probe()):
        conform(case, run(case), ("nonfinite", k))


DIMS = (0, 1, 3, 4, 5, 255, 256, 260, 1024, 1028, 4096)


@pytest.mark.parametrize("dim", DIMS)
def test_kernel_at_every_dim(dim):
    """dim below, at and beyond a lane's four columns and a workgroup's 1024, with n_trans 5 and 33; rows through a feat_row with
    duplicates where dim is large (and without one where it is small)."""
    for n_trans in (5, 33):
        mapped = dim >= 1024 or n_trans == 33
        case = S.random_probe(0.5, dim, n_trans=n_trans, mapped=mapped and dim > 0, feat_rows=23)
        conform(case, run(case), ("dim", dim, n_trans))


@pytest.mark.parametrize("n_trans,dim", [(1, 5), (1, 260), (257, 0), (257, 5), (257, 260), (257, 1028)])
def test_kernel_at_one_and_at_many_transitions(n_trans, dim):
    case = S.random_probe(1.0, dim, n_trans=n_trans, mapped=dim > 0, feat_rows=31)
    conform(case, run(case), ("n_trans", n_trans, dim))


@pytest.mark.parametrize("dim", [4, 5, 260, 1028])
def test_kernel_on_a_strided_feat_and_on_one_offset_by_a_float(dim):
    case = S.random_probe(0.5, dim, n_trans=9, mapped=True, feat_rows=17)
    F = case["feat"].shape[0]
    wide = torch.full((F, 2 * dim + 3), float("nan"), device=DEV)                 # rows 2 dim + 3 floats apart: an odd stride
    wide[:, :dim] = torch.from_numpy(case["feat"]).to(DEV)
    conform(case, run(case, feat_dev=wide[:, :dim]), ("strided", dim))
    even = torch.full((F, 2 * dim + (-2 * dim) % 4 + 4), float("nan"), device=DEV)  # a stride that is a multiple of 4: the 16-byte path
    even[:, :dim] = torch.from_numpy(case["feat"]).to(DEV)
    conform(case, run(case, feat_dev=even[:, :dim]), ("strided16", dim))
    flat = torch.full((F * dim + 1,), float("nan"), device=DEV)                   # the base one float off 16 bytes
    off = flat[1:].view(F, dim)
    off.copy_(torch.from_numpy(case["feat"]).to(DEV))
    assert off.data_ptr() % 16 == 4
    conform(case, run(case, feat_dev=off), ("offset", dim))


def test_operator_wrapper_and_the_prefix_sum_form():
    from bridges_hip import dqn_ops
    rng = np.random.default_rng(3)
    lengths = np.asarray([3, 0, 65, 1, 300], dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    R = int(seg[-1])
    case = dict(seg_lo=seg[:-1].copy(), seg_hi=seg[1:].copy(), select_q=rng.standard_normal(R).astype(np.float32),
                next_q=rng.standard_normal(R).astype(np.float32), T=0.3, feat=rng.standard_normal((R, 12)).astype(np.float32), feat_row=None)
    dev = {k: torch.from_numpy(case[k]).to(DEV) for k in ("select_q", "next_q", "feat")}
    value, mean, entropy, arg = dqn_ops.soft_expect(torch.from_numpy(seg).to(DEV), dev["select_q"], dev["next_q"], 0.3, feat=dev["feat"])
    pair = dqn_ops.soft_expect((torch.from_numpy(seg[:-1].copy()).to(DEV), torch.from_numpy(seg[1:].copy()).to(DEV)), dev["select_q"],
                               dev["next_q"], 0.3, feat=dev["feat"])
    torch.cuda.synchronize()
    got = dict(value=value.cpu().numpy(), feat_mean=mean.cpu().numpy(), entropy=entropy.cpu().numpy(), argmax_row=arg.cpu().numpy())
    conform(case, got, "wrapper")
    for a, b in zip((value, mean, entropy, arg), pair):
        assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all()
    v0, m0, e0, _ = dqn_ops.soft_expect(torch.from_numpy(seg).to(DEV), dev["select_q"], dev["next_q"], 0.3, want_entropy=False)
    assert m0 is None and e0 is None and torch.equal(v0, value)


# ------------------------------------------------------------------------------------------------------------ 2: refusals
def test_refusals_launch_nothing():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = S.random_probe(1.0, 8, n_trans=6)
    B, dim = 6, 8
    t = dict(lo=torch.from_numpy(case["seg_lo"]).to(DEV), hi=torch.from_numpy(case["seg_hi"]).to(DEV),
             sel=torch.from_numpy(case["select_q"]).to(DEV), nq=torch.from_numpy(case["next_q"]).to(DEV),
             feat=torch.from_numpy(case["feat"]).to(DEV), frow=torch.arange(len(case["select_q"]), dtype=torch.int64, device=DEV))
    outs = dict(value=torch.full((B,), SENTINEL, device=DEV), mean=torch.full((B, dim), SENTINEL, device=DEV),
                ent=torch.full((B,), SENTINEL, device=DEV), arg=torch.full((B,), 7, dtype=torch.int32, device=DEV))
    base = dict(n=B, T=1.0, stride=dim, dim=dim, **{k: _ptr(v) for k, v in t.items()}, **{k: _ptr(v) for k, v in outs.items()})

    def call(**kw):
        a = dict(base, **kw)
        return L.bridges_soft_expect(a["n"], a["lo"], a["hi"], a["sel"], a["nq"], a["T"], a["feat"], a["stride"], a["frow"], a["dim"],
                                     a["value"], a["mean"], a["ent"], a["arg"], abi.current_stream())
    null = C.c_void_p(0)
    bad = [dict(n=-1), dict(dim=-1), dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan")), dict(lo=null), dict(hi=null),
           dict(sel=null), dict(nq=null), dict(value=null), dict(arg=null), dict(feat=null), dict(mean=null), dict(stride=-8),
           dict(sel=C.c_void_p(t["sel"].data_ptr() + 2)), dict(value=C.c_void_p(outs["value"].data_ptr() + 1)),
           dict(feat=C.c_void_p(t["feat"].data_ptr() + 2)), dict(frow=C.c_void_p(t["frow"].data_ptr() + 4))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "bridges_soft_expect" in L.bridges_last_error().decode(), kw
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())                       # a refusal launches nothing
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())                       # nothing to do launches nothing either
    assert call(ent=null) == 0 and call(frow=null) == 0                           # the two optional arrays
    assert call(dim=0, feat=null, frow=null, mean=null) == 0                      # dim = 0 needs none of the three
    torch.cuda.synchronize()
    assert bool((outs["arg"].cpu() == torch.from_numpy(S.reference(case)["argmax_row"]).int()).all())


# ------------------------------------------------------------------------------------------------------------ 3: select_q is next_q
def finite_table(dim, seed=11):
    """Finite q with unique maxima (a permutation of multiples of 1/4) over segments of every probe length but 0."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray([n for n in S.SEG_LENGTHS if n] + [5, 17])
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    R = int(seg[-1])
    q = (0.25 * rng.permutation(R)).astype(np.float32) - 100.0
    return seg, q, rng.standard_normal((R, dim)).astype(np.float32)


@pytest.mark.parametrize("dim", [0, 6, 64])
def test_with_one_value_vector_the_rows_are_td_targets_and_a_small_temperature_gives_its_targets(dim):
    """argmax_row equals bridges_td_target's; at T = 1e-6 with unique maxima (gaps of 0.25: every other weight underflows to 0)
    stage one plus stage two -- next_targets(temperature=...) -- reproduces the max-operator kernel's q_target and sf_target.
    The expectation then IS the arg-max row's float32 value, so the reference's bound (half a float32 ulp at a float32 number,
    the float64 term 0 because one weight is 1 and the rest 0) asks for equality, and equality is asserted."""
    from bridges_hip import dqn_ops
    seg, q, feat = finite_table(dim)
    B = len(seg) - 1
    rng = np.random.default_rng(2)
    segd, qd = torch.from_numpy(seg).to(DEV), torch.from_numpy(q).to(DEV)
    featd = torch.from_numpy(feat).to(DEV) if dim else None
    lin = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(DEV)
    done = torch.from_numpy(rng.random(B) < 0.3).to(DEV)
    act = torch.from_numpy(rng.standard_normal((B, dim)).astype(np.float32)).to(DEV) if dim else None
    disc = torch.from_numpy((0.8 ** rng.integers(1, 4, size=B)).astype(np.float32)).to(DEV)
    for d in (None, disc):
        want_q, want_sf, want_rows = dqn_ops.td_target(segd, qd, lin, done, 0.8, next_sf=featd, action_raster=act, discount=d, select_q=qd)
        _, _, _, rows = dqn_ops.soft_expect(segd, qd, qd, 1.0)
        assert torch.equal(rows, want_rows)
        got_q, got_sf = dqn_ops.next_targets(segd, qd, done, 0.8, action_raster=act, lin=lin, discount=d, temperature=1e-6, next_feat=featd)
        torch.cuda.synchronize()
        assert torch.equal(got_q, want_q)
        assert (got_sf is None and want_sf is None) or torch.equal(got_sf, want_sf)
    # an empty segment that is not done is marked as the max-operator kernel marks it
    seg2 = torch.tensor([0, 0, 3], dtype=torch.int32, device=DEV)
    q2, _ = dqn_ops.next_targets(seg2, qd[:3].contiguous(), torch.zeros(2, dtype=torch.bool, device=DEV), 0.8, lin=lin[:2].contiguous(), temperature=0.5)
    assert float(q2[0]) == -float("inf") and np.isfinite(float(q2[1]))
