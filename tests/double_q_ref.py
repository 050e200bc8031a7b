"""Double Q-learning targets (bridges_td_target_select, VecDQN(double_q=True)): the probe, the float64 reference with its bound, a
plain float32 statement and deliberately defective twins.  Test infrastructure, not a test module: nothing here needs a GPU --
every function takes the device -- so tests/test_cpu_double_q.py checks on the CPU that the reference accepts the plain statement
and rejects every twin, and tests/test_gpu_double_q.py applies the same rule to the kernel.

The operator: per transition i with rows [lo, hi) of select_q / next_q / next_sf,
    row = the FIRST maximum of select_q over the segment,
    q   = lin + d_i * (done ? 0 : next_q[row]),      sf = action raster + d_i * (done ? 0 : next_sf[row]),
d_i the scalar gamma AS A FLOAT32 (the entry point takes it as one) or discount[i]; an empty segment: row NO_ROW,
q = lin + d_i * (done ? 0 : -inf), sf = the action raster."""
import math

import numpy as np
import torch

from gpu_helpers import U32
from mlp_conformance import NO_ROW, TD_PEAK, conform, dense, td_plain, td_probe       # noqa: F401  (td_plain: re-exported)

SELECT_SF_DIMS = (0, 4, 6, 64, 4096)
TWINS = ("selects_by_next_q", "value_from_select_q", "last_maximum")
SAME_SEGMENT = 2                                  # the segment (256 rows) on which select_q == next_q


def select_probe(sf_dim, device, seed=0, strided=True):
    """td_probe (segments of 1, 255, 256, 257, 513, 700 rows back to back, three -inf rows, an empty done segment, two shared
    (lo, hi) ranges) plus ``select_q`` [R], quantised to quarters like next_q so that ties are plentiful, with maxima of its own:
      700 rows   TD_PEAK at lo + 7 and lo + 7 + 256: the same thread, a later stride (next_q's: lo + 5, lo + 5 + 256)
      257 rows   TD_PEAK at lo + 100 and lo + 256: different waves, the LATER row in wave 0 (next_q's: lo + 200, lo + 256)
      513 rows   TD_PEAK at lo + 63 and lo + 64: the last lane of wave 0 and the first of wave 1 (next_q's: lo + 44, lo + 300)
      255 rows   TD_PEAK at lo + 130 (next_q plants none there)
      256 rows   select_q == next_q (SAME_SEGMENT)
      3 rows     next_q is -inf; select_q is finite (0.25, 1, 1): the row is well defined, the value taken is -inf
    sf_dim = 6 (no multiple of 4: rows that are not 16-byte aligned) is built here on td_probe(0): next_sf the [:, 0] view of a
    [R, 2, 6] tensor (``strided``) or contiguous, the action raster [B, 6]."""
    pr = td_probe(0 if sf_dim == 6 else sf_dim, device, seed, strided)
    g = torch.Generator().manual_seed(7000003 * seed + 31 * sf_dim + 5)
    lo, hi = pr["lo"], pr["hi"]
    R, B = pr["next_q"].numel(), len(lo)
    sel = torch.round(torch.randn(R, generator=g) * 4) / 4
    l255, l257, l513, l700 = lo[1], lo[3], lo[4], lo[5]
    sel[[l700 + 7, l700 + 7 + 256, l257 + 100, l257 + 256, l513 + 63, l513 + 64, l255 + 130]] = TD_PEAK
    sel[lo[SAME_SEGMENT]:hi[SAME_SEGMENT]] = pr["next_q"][lo[SAME_SEGMENT]:hi[SAME_SEGMENT]].cpu()
    sel[lo[6]:hi[6]] = torch.tensor([0.25, 1.0, 1.0])
    pr["select_q"] = sel.to(device)
    if sf_dim == 6:
        full = dense(g, R, 2, 6).to(device)
        pr["next_sf"] = full[:, 0] if strided else full[:, 0].contiguous()
        pr["act"] = (torch.rand(B, 6, generator=g) > 0.5).float().to(device)
        pr["sf_dim"] = 6
    return pr


def discounts(gamma_or_discount, B):
    """float64 [B]: the float32 scalar, or the per-row discounts, as the operator reads them."""
    if torch.is_tensor(gamma_or_discount):
        return gamma_or_discount.detach().float().double().cpu().reshape(B)
    return torch.full((B,), float(np.float32(gamma_or_discount)), dtype=torch.float64)


def first_max(values, lo, hi, last=False):
    if hi <= lo:
        return NO_ROW
    seg = values[lo:hi]
    return lo + (hi - lo - 1 - int(seg.flip(0).argmax()) if last else int(seg.argmax()))      # torch.argmax: the first maximum


def td_select_ref(pr, gamma_or_discount):
    """float64 -> {q, sf: (reference, bound)}, rows.  Bound: td_ref's 2 u (|a| + |d s|) -- the product and the sum, rounded
    separately or fused -- zero where done (the target is the float32 input itself) and where the target is infinite (met
    exactly)."""
    B, D = len(pr["lo"]), pr["sf_dim"]
    sel, nq = pr["select_q"].double().cpu(), pr["next_q"].double().cpu()
    lin, disc = pr["lin"].double().cpu(), discounts(gamma_or_discount, B)
    q, e_q, rows = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), []
    sf = e_sf = None
    if D:
        act = pr["act"].double().cpu().reshape(B, -1)
        sf, e_sf = act.clone(), torch.zeros(B, D, dtype=torch.float64)
    for i, (lo, hi) in enumerate(zip(pr["lo"], pr["hi"])):
        row = first_max(sel, lo, hi)
        rows.append(row)
        if pr["done"][i]:
            q[i] = lin[i]
            continue
        nxt = nq[row] if hi > lo else torch.tensor(-math.inf, dtype=torch.float64)
        q[i] = lin[i] + disc[i] * nxt
        e_q[i] = 2 * U32 * (abs(float(lin[i])) + abs(float(disc[i] * nxt)))
        if D and hi > lo:
            s = pr["next_sf"][row].double().cpu().reshape(-1)
            sf[i] = act[i] + disc[i] * s
            e_sf[i] = 2 * U32 * (act[i].abs() + (disc[i] * s).abs())
    e_q = torch.nan_to_num(e_q, nan=0.0, posinf=0.0)                          # an infinite target is met exactly
    dev = pr["next_q"].device
    return dict(q=(q.to(dev), e_q.to(dev)), sf=(sf.to(dev), e_sf.to(dev)) if D else None), rows


def td_select_plain(pr, gamma_or_discount, twin=None):
    """The operator in plain float32 torch -> (q [B], sf [B, D] or None, rows).  Twins: 'selects_by_next_q' ignores select_q (the
    plain target), 'value_from_select_q' takes the value from the vector it selected by (the policy net's), 'last_maximum' takes
    the last row of a tie."""
    assert twin is None or twin in TWINS, twin
    nq, B = pr["next_q"], len(pr["lo"])
    d = discounts(gamma_or_discount, B).float().to(nq.device)
    by = nq if twin == "selects_by_next_q" else pr["select_q"]
    val = pr["select_q"] if twin == "value_from_select_q" else nq
    q, sf, rows = [], [], []
    for i, (lo, hi) in enumerate(zip(pr["lo"], pr["hi"])):
        rows.append(first_max(by, lo, hi, last=twin == "last_maximum"))
        live = not pr["done"][i] and hi > lo
        nxt = val[rows[-1]] if live else torch.zeros((), device=nq.device)
        if hi == lo and not pr["done"][i]:
            nxt = torch.full((), -math.inf, device=nq.device)
        q.append(pr["lin"][i] + d[i] * nxt)
        if pr["sf_dim"]:
            a = pr["act"][i].reshape(-1)
            sf.append(a + d[i] * pr["next_sf"][rows[-1]].reshape(-1) if live else a.clone())
    return torch.stack(q), (torch.stack(sf) if pr["sf_dim"] else None), rows


def select_conform(name, got, lib, ref, ref_rows, shape=None):
    """got / lib = (q, sf, rows): the rows exact, q and sf through conform (mlp_conformance.td_conform's rule)."""
    assert [int(r) for r in got[2]] == [int(r) for r in ref_rows], f"{name} {shape}: rows {[int(r) for r in got[2]]} != {ref_rows}"
    conform(name + ".q", got[0], lib[0], *ref["q"], shape)
    if ref["sf"] is not None:
        B = got[0].numel()
        conform(name + ".sf", got[1].reshape(B, -1), lib[1].reshape(B, -1), *ref["sf"], shape)


def segment_first_max(values, lo, hi):
    """Rows of the first maximum of ``values`` over [lo[i], hi[i]) for tensors lo, hi (host loop; NO_ROW for an empty one)."""
    v = values.detach().cpu()
    return [first_max(v, int(l), int(h)) for l, h in zip(lo.cpu().tolist(), hi.cpu().tolist())]
