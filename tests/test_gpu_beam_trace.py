"""GPU: bridges_beam_trace against the numpy statement of its rule (tests/beam_trace_ref.py) on sentinel-filled outputs, bit for bit
-- the h-step return included, whose summation order the rule fixes, and additionally within the bound of the n-step window --: the
probe tables, seeded tables at G in {1, 5, 33} x B in {1, 2, 8, 16} x D in {1, 6, 16} under (n_step, n_tail) in {(1, 0), (3, 9),
(8, 9), (1, 9)} (W_out odd and even, E up to 528), rows beyond offset[G] untouched, the same bits on a second call, the refusals,
which leave the outputs untouched, and E == 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_trace_ref as TR
from robotoddler.training import records as R

pytestmark = pytest.mark.gpu
INPUTS = ("rec", "valid", "parent", "end_env", "end_depth", "tail")


def _dev(case):
    return {k: (None if case[k] is None else torch.from_numpy(np.ascontiguousarray(case[k])).cuda()) for k in INPUTS}


def _outputs(case):
    return {k: torch.from_numpy(v).cuda() for k, v in TR.sentinels(case).items()}


def _run(case):
    """One call on sentinel-filled outputs -> the outputs as numpy arrays."""
    from bridges_hip import ops
    c, out = _dev(case), _outputs(case)
    got = ops.beam_trace(c["rec"], c["valid"], c["parent"], c["end_env"], c["end_depth"], case["B"], case["gamma"], n_step=case["n_step"],
                         tail=c["tail"], priority=case["priority"], out=out["rows"], offset=out["offset"], status=out["status"])
    assert got["rows"] is out["rows"] and got["offset"] is out["offset"] and got["status"] is out["status"]
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_exact(got, want, what):
    for k in ("status", "offset"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    g, w = got["rows"].view(np.uint64), want["rows"].view(np.uint64)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert not len(bad), (what, "rows differ first at (row, column)", bad[0].tolist(), hex(g[tuple(bad[0])]), hex(w[tuple(bad[0])]))
    n = int(want["offset"][-1])
    assert np.all(g[n:] == TR.ROW_SENTINEL), (what, "a row beyond offset[G] was written")
    ok = np.isfinite(want["g_bound"][:n])                                    # and within the window's bound of the direct sum
    err = np.abs(got["rows"][:n, R.O_LIN][ok] - want["g_exact"][:n][ok])     # (h = 1: the record's own value, error 0)
    assert np.all(err <= want["g_bound"][:n][ok]), (what, "a return outside its bound")


@pytest.mark.parametrize("name", sorted(TR.probe_tables()))
def test_probe_tables_exactly(name):
    case = TR.probe_tables()[name]
    _assert_exact(_run(case), TR.reference(case), name)


@pytest.mark.parametrize("D", [1, 6, 16])
@pytest.mark.parametrize("B", [1, 2, 8, 16])
@pytest.mark.parametrize("G", [1, 5, 33])
def test_seeded_tables_exactly_and_the_same_on_a_second_call(G, B, D):
    emitted = broken = 0
    for n_step, n_tail in ((1, 0), (3, 9), (8, 9), (1, 9)):
        case = TR.random_case(G, B, D, n_step, n_tail, seed=1000 * G + 100 * B + 10 * D + n_step + n_tail)
        got, want = _run(case), TR.reference(case)
        _assert_exact(got, want, (G, B, D, n_step, n_tail))
        assert TR.same(_run(case), got)
        emitted += int(want["offset"][-1])
        broken += int(want["status"].sum())
    assert emitted > 0 and (G < 33 or broken > 0)                            # (the tables hold rows to write and chains to refuse)


def test_widths_and_sizes_cover_what_they_should():
    widths = {TR.W + nt + (n > 1) for n, nt in ((1, 0), (3, 9), (8, 9), (1, 9))}
    assert {w % 2 for w in widths} == {0, 1} and 33 * 16 == 528 > 256       # E beyond a workgroup, G beyond a wave


def test_refusals_leave_the_outputs_untouched():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = TR.random_case(3, 4, 6, 3, 5, seed=1)
    c, out = _dev(case), _outputs(case)
    E = 12
    stream = abi.current_stream()

    def call(E=E, B=4, D=6, n_step=3, n_tail=5, gamma=0.95, **swap):
        a = dict(c, out=out["rows"], offset=out["offset"], status=out["status"])
        a.update(swap)
        p = {k: (v if isinstance(v, C.c_void_p) else C.c_void_p(v.data_ptr() if v is not None else 0)) for k, v in a.items()}
        return L.bridges_beam_trace(E, B, D, n_step, n_tail, p["rec"], p["valid"], p["parent"], p["end_env"], p["end_depth"], p["tail"],
                                    gamma, 0.0, p["out"], p["offset"], p["status"], stream)
    assert call(B=0) == -1 and call(B=17) == -1 and b"1..16" in L.bridges_last_error()
    assert call(E=11) == -1 and call(E=-4) == -1                             # E % B != 0, a negative count
    assert call(D=0) == -1 and call(D=17) == -1 and b"BRIDGES_REC_K" in L.bridges_last_error()
    assert call(n_step=0) == -1 and call(n_step=9) == -1 and b"BRIDGES_NSTEP_MAX" in L.bridges_last_error()
    assert call(n_tail=-1) == -1
    assert call(gamma=float("nan")) == -1 and call(gamma=float("inf")) == -1 and b"finite" in L.bridges_last_error()
    for name in INPUTS + ("out", "offset", "status"):
        assert call(**{name: None}) == -1, name
    assert call(rec=C.c_void_p(c["rec"].data_ptr() + 4)) == -1 and b"misaligned" in L.bridges_last_error()
    assert call(parent=C.c_void_p(c["parent"].data_ptr() + 2)) == -1
    assert call(offset=C.c_void_p(out["offset"].data_ptr() + 1)) == -1
    assert call(E=0) == 0                                                    # nothing to do, nothing launched
    torch.cuda.synchronize()
    want = TR.sentinels(case)
    for k in TR.OUTPUTS:
        assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert call() == 0                                                       # and the call they guard goes through
    torch.cuda.synchronize()
    _assert_exact({k: v.cpu().numpy() for k, v in out.items()}, TR.reference(dict(case, priority=0.0)), "after the refusals")


def test_no_tail_takes_a_null_pointer_and_no_envs_give_no_rows():
    from bridges_hip import ops
    case = TR.make_case(2, 2, 3, 1, 0, seed=5, ends=[2, 1])
    assert case["tail"] is None
    _assert_exact(_run(case), TR.reference(case), "n_tail = 0")
    empty = ops.beam_trace(torch.zeros((3, 0, TR.W), dtype=torch.float64, device="cuda"), torch.zeros((3, 0), dtype=torch.uint8, device="cuda"),
                           torch.zeros((3, 0), dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                           torch.zeros(0, dtype=torch.int32, device="cuda"), 4, 0.9)
    assert tuple(empty["rows"].shape) == (0, TR.W) and empty["offset"].tolist() == [0] and empty["status"].numel() == 0
