"""GPU: bridges_beam_select against the numpy statement of its rule (tests/beam_ref.py), bit for bit on sentinel-filled outputs:
the probe tables, seeded tables at G in {1, 5, 33} x B in {1, 2, 8, 16}, the same bits on a second call, B = 1 against
bridges_eps_greedy_select(greedy = 1), and the refusals, which leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_ref as BR

pytestmark = pytest.mark.gpu


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev(case):
    d = torch.device("cuda")
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(d) if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def _run(case, out=None):
    """One call on sentinel-filled outputs (or on ``out``) -> the outputs as numpy arrays."""
    from bridges_hip import ops
    c = _dev(case)
    E = len(case["seg_lo"])
    if out is None:
        out = {k: torch.from_numpy(v).cuda() for k, v in BR.sentinels(E).items()}
    ops.beam_select((c["seg_lo"], c["seg_hi"]), c["q"], case["B"], c["live"], c["ret"], c["disc"], c["idx"], c["cand_offset"],
                    rep=c["rep"], out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(BR.probe_tables()))
def test_probe_tables_bit_for_bit(name):
    case = BR.probe_tables()[name]
    got, want = _run(case), BR.reference(case)
    for k in BR.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (name, k, got[k], want[k])


@pytest.mark.parametrize("B", [1, 2, 8, 16])
@pytest.mark.parametrize("G", [1, 5, 33])
def test_seeded_tables_bit_for_bit_and_the_same_on_a_second_call(G, B):
    case = BR.random_case(G, B, seed=100 * G + B)
    got, want = _run(case), BR.reference(case)
    for k in BR.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert BR.same(_run(case), got)
    assert got["live"].sum() > 0                                          # (the table is not empty)


def test_width_1_with_every_beam_live_is_the_greedy_selection():
    from bridges_hip import ops
    case = BR.random_case(33, 1, seed=7)
    case["live"][:] = 1
    bad = np.isnan(case["q"]) | (case["q"] == -np.inf)
    case["q"][bad] = 0.25                                                # finite q: what a Q pass gives
    case["seg_hi"] = np.maximum(case["seg_hi"], case["seg_lo"] + 1).clip(max=len(case["q"])).astype(np.int32)
    case["seg_lo"] = np.minimum(case["seg_lo"], case["seg_hi"] - 1).astype(np.int32)      # every env has rows
    got = _run(case)
    c = _dev(case)
    E = len(case["seg_lo"])
    zeros = torch.zeros(len(case["q"]), dtype=torch.float32, device="cuda")
    _sc, sel_index, q_sel, _w = ops.eps_greedy_select((c["seg_lo"], c["seg_hi"]), c["q"], zeros, torch.zeros(E, device="cuda"), 0.0, True,
                                                      c["idx"], c["cand_offset"], rep=c["rep"])
    assert got["live"].all() and np.array_equal(got["src"], np.arange(E))
    assert np.array_equal(got["sel_index"], sel_index.cpu().numpy())
    assert got["q_sel"].tobytes() == q_sel.cpu().numpy().tobytes()
    assert np.array_equal(got["sel_compact"], _sc.cpu().numpy())


def test_refusals_leave_the_outputs_untouched():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = BR.random_case(3, 4, seed=1)
    c = _dev(case)
    E, n = 12, len(case["q"])
    out = {k: torch.from_numpy(v).cuda() for k, v in BR.sentinels(E).items()}
    q8 = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    stream = abi.current_stream()

    def call(E=E, B=4, n=n, **swap):
        a = dict(seg_lo=c["seg_lo"], seg_hi=c["seg_hi"], q=c["q"], idx=c["idx"], cand_offset=c["cand_offset"], rep=c["rep"],
                 live=c["live"], ret=c["ret"], disc=c["disc"], src=out["src"], sel_compact=out["sel_compact"],
                 sel_index=out["sel_index"], q_sel=out["q_sel"], score=out["score"], live_out=out["live"])
        a.update(swap)
        p = {k: (v if isinstance(v, C.c_void_p) else _ptr(v)) for k, v in a.items()}
        return L.bridges_beam_select(E, B, n, p["seg_lo"], p["seg_hi"], p["q"], p["idx"], p["cand_offset"], p["rep"], p["live"], p["ret"],
                                     p["disc"], p["src"], p["sel_compact"], p["sel_index"], p["q_sel"], p["score"], p["live_out"], stream)
    assert call(B=0) == -1 and call(B=17) == -1 and b"1..16" in L.bridges_last_error()
    assert call(E=11) == -1 and call(E=-4) == -1                         # E % B != 0, a negative count
    assert call(n=0) == -1
    for name in ("seg_lo", "seg_hi", "q", "idx", "cand_offset", "live", "ret", "disc", "src", "sel_compact", "sel_index", "q_sel", "score",
                 "live_out"):
        assert call(**{name: None}) == -1, name
    assert call(q=C.c_void_p(q8.data_ptr() + 2)) == -1 and b"misaligned" in L.bridges_last_error()
    assert call(ret=C.c_void_p(c["ret"].data_ptr() + 4)) == -1
    assert call(E=0) == 0                                                # nothing to do, nothing launched
    torch.cuda.synchronize()
    want = BR.sentinels(E)
    for k in BR.OUTPUTS:
        assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert call(rep=None) == 0                                           # rep may be NULL
    torch.cuda.synchronize()
    assert out["live"].max().item() <= 1
