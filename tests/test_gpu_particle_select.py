"""GPU: bridges_particle_select against the numpy statement of its rule (tests/particle_ref.py) on sentinel-filled outputs: every
decided slot of the probe tables in all outputs (integers and live exactly, q_sel and score as bits, p_sel and ess within the
bounds derived there), the exact probes bit for bit without a margin, B in {1, 2, 3, 16} x G in {1, 5, 130} over the segment
lengths and temperatures of boltzmann_ref, the same bits on a second call, the rule's exact properties and limits, the non-finite
table, and the refusals, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_ref as BR
import boltzmann_ref as BZ
import particle_ref as P

pytestmark = pytest.mark.gpu
INF = float("inf")
INPUTS = ("seg_lo", "seg_hi", "q", "idx", "cand_offset", "rep", "live", "ret", "disc", "u_act", "u_res")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev(case):
    d = torch.device("cuda")
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(d) if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def _run(case, check_inputs=True):
    """One call on sentinel-filled outputs -> the outputs as numpy arrays (key "live" as ops returns it)."""
    from bridges_hip import ops
    c = _dev(case)
    E, G = len(case["seg_lo"]), len(case["u_res"])
    out = {k: torch.from_numpy(v).cuda() for k, v in P.sentinels(E, G).items()}
    got = ops.particle_select((c["seg_lo"], c["seg_hi"]), c["q"], case["B"], c["live"], c["ret"], c["disc"], c["idx"], c["cand_offset"],
                              c["u_act"], c["u_res"], case["T"], case["Tr"], elite=case["elite"], rep=c["rep"], out=out)
    torch.cuda.synchronize()
    assert got is out
    if check_inputs:                                                      # nothing but the outputs is written
        for k in INPUTS:
            if case.get(k) is not None:
                assert c[k].cpu().numpy().tobytes() == np.ascontiguousarray(case[k]).tobytes(), k
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(case, got, ref, name=""):
    """Every decided slot (every slot of an exact case) in all outputs; the undecided ones still hold a legal answer."""
    E, B = len(case["seg_lo"]), case["B"]
    d = np.ones(E, bool) if case.get("exact") else ref["decided"]
    for k in ("src", "sel_compact", "sel_index", "live"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k][d], ref[k][d]), (name, k, got[k], ref[k])
    for k in ("q_sel", "score"):
        assert got[k].dtype == ref[k].dtype and got[k][d].tobytes() == ref[k][d].tobytes(), (name, k, got[k], ref[k])
    assert got["p_sel"].dtype == np.float32 and got["ess"].dtype == np.float64
    want_p = ref["p_sel"].astype(np.float32).astype(np.float64)
    err = np.abs(got["p_sel"].astype(np.float64) - want_p)
    assert (err[d] <= P.p_sel_bound(ref["p_sel"], ref["n_rows"])[d]).all(), (name, "p_sel", got["p_sel"], ref["p_sel"])
    if case.get("exact"):
        assert got["p_sel"].tobytes() == ref["p_sel"].astype(np.float32).tobytes() and got["ess"].tobytes() == ref["ess"].tobytes(), name
    assert (np.abs(got["ess"] - ref["ess"]) <= P.ess_bound(ref["ess"], B)).all(), (name, "ess", got["ess"], ref["ess"])
    # an undecided slot: nothing of it is compared with the reference, but it is a slot of its group all the same
    und = np.flatnonzero(~d)
    assert (got["live"][und] == 1).all() and (got["src"][und] // B == und // B).all()


@pytest.mark.parametrize("name", sorted(P.all_probes()))
def test_probe_tables(name):
    case = P.all_probes()[name]
    _compare(case, _run(case), P.reference(case), name)


@pytest.mark.parametrize("B", [1, 2, 3, 16])
@pytest.mark.parametrize("G", [1, 5, 130])
def test_shapes_and_the_same_bits_on_a_second_call(G, B):
    decided = slots = 0
    for i, T in enumerate(BZ.TEMPERATURES):
        Tr = P.RESAMPLE_TEMPERATURES[(i + B) % 3]
        case = P.random_probe(G, B, T, Tr, elite=bool((i + G) % 2), seed=31 * G + 7 * B + i)
        got, ref = _run(case), P.reference(case)
        _compare(case, got, ref, (G, B, T, Tr))
        again = _run(case, check_inputs=False)
        assert all(again[k].tobytes() == got[k].tobytes() for k in P.OUTPUTS), (G, B, T)
        decided, slots = decided + int(ref["decided"].sum()), slots + G * B
        if G * B >= 10:
            assert 0 < got["live"].sum()
    assert decided * 100 >= slots * 99                                       # (the comparison is not an empty one)
    if G == 130:
        lens = set((case["seg_hi"] - case["seg_lo"]).tolist())
        assert lens == set(BZ.SEG_LENGTHS)


def test_width_1_with_the_elite_is_beam_select_bit_for_bit():
    from bridges_hip import ops
    case = P.random_probe(130, 1, 0.5, 1.0, True, seed=71)
    got = _run(case)
    c = _dev(case)
    want = ops.beam_select((c["seg_lo"], c["seg_hi"]), c["q"], 1, c["live"], c["ret"], c["disc"], c["idx"], c["cand_offset"], rep=c["rep"])
    torch.cuda.synchronize()
    for k in BR.OUTPUTS:
        assert got[k].tobytes() == want[k].cpu().numpy().tobytes(), k
    assert 0 < got["live"].sum() < 130 and np.array_equal(got["p_sel"], got["live"].astype(np.float32))


def test_without_resampling_src_is_the_identity():
    for B in (1, 2, 3, 16):
        case = P.random_probe(5, B, 1.0, INF, False, seed=50 + B, all_parents=True)
        case["u_res"][:3] = [0.0, 1.0 - 2.0 ** -24, 2.0 ** -149]
        got = _run(case)
        assert got["live"].all() and np.array_equal(got["src"], np.arange(5 * B)), B
        assert np.array_equal(got["ess"], np.full(5, float(B)))


def test_cold_resampling_takes_the_best_parent_everywhere():
    for B in (2, 3, 16):
        case = P.random_probe(5, B, 1.0, 1e-6, False, seed=60 + B)
        case["ret"] = case["ret"] + 1e-3 * np.arange(len(case["ret"]))          # no two parents tie in S
        got, ref = _run(case), P.reference(case)
        for g in range(5):
            vals = [P.env_value(case, e) for e in range(g * B, (g + 1) * B)]
            S = [v[1] if v[0] else -INF for v in vals]
            if max(S) == -INF:
                assert not got["live"][g * B:(g + 1) * B].any()
                continue
            assert (got["src"][g * B:(g + 1) * B] == g * B + int(np.argmax(S))).all(), (B, g)
            assert got["ess"][g] == 1.0


def test_cold_action_draw_takes_a_maximum_of_the_parent():
    case = P.random_probe(5, 16, 1e-6, 1.0, False, seed=88)
    got = _run(case)
    seen_tie = False
    for s in np.flatnonzero(got["live"]):
        lo, hi = P._rows(case, int(got["src"][s]))
        seg = case["q"][lo:hi]
        m = seg[~np.isnan(seg)].max()
        assert got["q_sel"][s] == m, s                                       # the first maximum or an exact tie of it
        rows = lo + np.flatnonzero(seg == m)
        assert got["sel_compact"][s] in case["idx"][rows]
        seen_tie |= len(rows) > 1 and got["sel_compact"][s] != case["idx"][rows[0]]
    assert seen_tie                                                          # (ties are planted: some draw falls on a later one)


def test_argument_errors_launch_nothing():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = P.random_probe(3, 4, 1.0, 1.0, True, seed=1)
    c = _dev(case)
    E, G, n = 12, 3, len(case["q"])
    out = {k: torch.from_numpy(v).cuda() for k, v in P.sentinels(E, G).items()}
    q8 = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    stream = abi.current_stream()

    def call(E=E, B=4, n=n, T=1.0, Tr=1.0, **swap):
        a = dict(seg_lo=c["seg_lo"], seg_hi=c["seg_hi"], q=c["q"], idx=c["idx"], cand_offset=c["cand_offset"], rep=c["rep"],
                 live=c["live"], ret=c["ret"], disc=c["disc"], u_act=c["u_act"], u_res=c["u_res"], src=out["src"],
                 sel_compact=out["sel_compact"], sel_index=out["sel_index"], q_sel=out["q_sel"], score=out["score"],
                 live_out=out["live"], p_sel=out["p_sel"], ess=out["ess"])
        a.update(swap)
        p = {k: (v if isinstance(v, C.c_void_p) else _ptr(v)) for k, v in a.items()}
        return L.bridges_particle_select(E, B, n, p["seg_lo"], p["seg_hi"], p["q"], p["idx"], p["cand_offset"], p["rep"], p["live"],
                                         p["ret"], p["disc"], p["u_act"], p["u_res"], T, Tr, 1, p["src"], p["sel_compact"],
                                         p["sel_index"], p["q_sel"], p["score"], p["live_out"], p["p_sel"], p["ess"], stream)
    assert call(B=0) == -1 and call(B=17) == -1 and b"bridges_particle_select" in L.bridges_last_error()
    assert call(E=11) == -1 and call(E=-4) == -1 and call(n=0) == -1
    for T in (0.0, -1.0, INF, float("nan")):
        assert call(T=T) == -1 and b"bridges_particle_select" in L.bridges_last_error(), T
    for Tr in (0.0, -1.0, -INF, float("nan")):
        assert call(Tr=Tr) == -1 and b"bridges_particle_select" in L.bridges_last_error(), Tr
    for name in ("seg_lo", "seg_hi", "q", "idx", "cand_offset", "live", "ret", "disc", "u_act", "u_res", "src", "sel_compact", "sel_index",
                 "q_sel", "score", "live_out", "p_sel", "ess"):
        assert call(**{name: None}) == -1 and b"bridges_particle_select" in L.bridges_last_error(), name
    assert call(q=C.c_void_p(q8.data_ptr() + 2)) == -1 and b"misaligned" in L.bridges_last_error()
    assert call(ret=C.c_void_p(c["ret"].data_ptr() + 4)) == -1 and call(ess=C.c_void_p(out["ess"].data_ptr() + 4)) == -1
    assert call(u_act=C.c_void_p(c["u_act"].data_ptr() + 2)) == -1
    assert call(E=0) == 0                                                    # nothing to do, nothing launched
    torch.cuda.synchronize()
    want = P.sentinels(E, G)
    for k in P.OUTPUTS:
        assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert call(Tr=INF) == 0 and call(rep=None) == 0 and call() == 0        # the same call unbroken then runs
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _compare(case, got, P.reference(case), "after the refusals")
