"""Conformance of the kernels behind VecDQN's factored acting forward (csrc/dqn_kernels.hip: k_bits_linear, k_bits_linear2,
k_sigmoid_dot, k_bits_dot, k_bits_accumulate; csrc/mlp_kernels.hip: k_head_sigmoid_dot, k_head_sum; csrc/ops_kernels.hip:
k_bits_to_f32, k_bits_or): shape tables, probe data, references with their bounds, the library's float32 statements and
deliberately defective twins.  Test infrastructure, not a test module: nothing here needs a GPU -- every function takes the device
-- so tests/test_cpu_acting_conformance_refs.py checks on the CPU that the references accept a clean float32 evaluation and reject
every twin, and tests/test_gpu_acting_conformance.py applies the same rule (mlp_conformance.conform) to the kernels.

Bounds are first-order forward-error bounds in u = 2**-24 (gpu_helpers.dot_bound for sums); the derivation stands next to each."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from gpu_helpers import U32, dot_bound
from mlp_conformance import FACTOR, ROW_FACTOR, ceil_div, conform, conform_pooled, dense  # noqa: F401  (one rule, re-exported)

CPU = torch.device("cpu")
IMG, PX, WAVE = 64, 4096, 64
MAX_WAVES = 4 * 2048           # grid_for_waves (csrc/api.hip): at most 2048 workgroups of four waves, one row per wave and round
TINY = 2.0 ** -126             # the smallest normal float32: what a flush to zero may cost
FEW_ROWS = 5                   # a row of a table with at most this many output elements gives either q as the largest of a few draws:
                               # its elements are held to their bounds, the two q are compared over such rows pooled (conform_pooled)


def launch_waves(n_rows):
    """Waves of a one-wave-per-row launch sized by grid_for_waves: rows >= this many are served in a later grid-stride round."""
    return 4 * min(max(ceil_div(n_rows, 4), 1), 2048)


def same_bits(a, b):
    """torch.equal on the bit patterns: -0.0 differs from +0.0 (torch.equal alone takes them as equal)."""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# Rasters.  bit x of word y = pixel p = 64 y + x (pack_bits / unpack_bits of tests/test_gpu_vec_dqn_obstacles.py); bit 63 is the
# sign bit of the int64.

RASTER_NAMES = ("empty", "full", "px_0_0", "px_0_63", "px_63_0", "px_63_63", "row_17", "col_63") + tuple(f"block_{i}" for i in range(8))
N_RASTERS = len(RASTER_NAMES)
BLOCKS = ((0, 0, 5, 7), (59, 57, 5, 7), (0, 57, 5, 7), (59, 0, 5, 7), (30, 29, 7, 5), (13, 40, 5, 7), (44, 7, 6, 6), (21, 57, 5, 7))   # y, x, h, w


def pack_bits(mask):
    """bool [n, 64, 64] -> int64 [n, 64]."""
    return (mask.long() << torch.arange(64, device=mask.device)).sum(dim=-1)


def unpack_bits(bits):
    """int64 [n, 64] -> bool [n, 4096]: the shift-and-mask expansion."""
    return (((bits.unsqueeze(-1) >> torch.arange(64, device=bits.device)) & 1) != 0).reshape(bits.shape[0], -1)


@functools.lru_cache(maxsize=None)
def raster_masks():
    """bool [16, 64, 64] on the CPU, in the order of RASTER_NAMES: empty, full, the four corner pixels (bits 0 and 63 of words 0
    and 63), one full row (every bit of word 17), one full column (bit 63 of every word: each word is INT64_MIN) and eight
    block-like rasters of 35 or 36 pixels, four of them in the corners of the image."""
    m = torch.zeros((N_RASTERS, IMG, IMG), dtype=torch.bool)
    m[1] = True
    for i, (y, x) in enumerate(((0, 0), (0, 63), (63, 0), (63, 63))):
        m[2 + i, y, x] = True
    m[6, 17, :] = True
    m[7, :, 63] = True
    for i, (y, x, h, w) in enumerate(BLOCKS):
        m[8 + i, y:y + h, x:x + w] = True
    return m


def raster_probe(device):
    """-> (bits int64 [16, 64], dense bool [16, 4096]) on ``device``."""
    m = raster_masks()
    return pack_bits(m).to(device), m.reshape(N_RASTERS, PX).to(device)


def raster_expand(bits):
    """The CPU statement of bridges_bits_to_f32: int64 [n, 64] -> float32 [n, 64, 64], numpy shifts on the unsigned words."""
    words = bits.cpu().numpy().astype(np.int64).view(np.uint64)
    out = np.zeros(words.shape + (IMG,), dtype=np.float32)
    for x in range(IMG):
        out[..., x] = ((words >> np.uint64(x)) & np.uint64(1)).astype(np.float32)
    return torch.from_numpy(out)


BITS_TO_F32_N = (1, 4, 5)      # one wave of a workgroup, a full workgroup, a second workgroup with one live wave
BITS_OR_RANGES = ((0, 0), (3, 4), (0, 16), (2, 9), (5, 12), (16, 16), (8, 16))     # empty, one raster, all, two that overlap, empty at the end


def bits_or_ref(bits, ranges):
    words = bits.cpu().numpy().astype(np.int64)
    return torch.from_numpy(np.stack([np.bitwise_or.reduce(words[lo:hi], axis=0) if hi > lo else np.zeros(IMG, np.int64) for lo, hi in ranges]))


# ---------------------------------------------------------------------------------------------------------------------------
# k_bits_linear / k_bits_linear2: out[r] = base[base_row[r]] + the rows of wt at the set pixels, ASCENDING p, operand a before b.
# One wave per output row, lane l holds columns c0 + 4 l .. + 3 of column group c0 = 0, 256, 512, ...

BL_D = (4, 252, 256, 260, 516, 772)    # one lane; 63 lanes; exactly one group; a second / third / fourth group whose only lane is 0
BL_N = (1, 5, 8193)                    # 8193: row 8192 is served in the second grid-stride round
BL_BIG_D = (4, 260)                    # the d at which 8193 rows run
BL_NB = 3                              # rows of the base table
BL_BASE_FORMS = ("none", "row0", "rows")       # no base; base without base_row (EVERY row gets base row 0); base with base_row
BL_CASES = [(n, d, s) for d in BL_D for n, shifts in ((1, (1, 8)), (5, (0, 5, 10))) for s in shifts] + [(8193, d, 0) for d in BL_BIG_D]


def bl_rows(n, shift):
    """(raster of operand a, raster of operand b, base row) of every output row, int64 [n] each.  Up to 16 rows take consecutive
    rasters from ``shift``; the long case strides through the pool so that row 8192 holds the FULL raster.  Operand b and the base
    row follow from the row, so the distinct (a, b, base) triples stay few whatever n (16 x 3)."""
    i = torch.arange(n)
    a = (shift + i) % N_RASTERS if n <= N_RASTERS else (7 * i + 1) % N_RASTERS
    return a, (3 * a + 2) % N_RASTERS, (2 * i + 2) % BL_NB          # base rows 2, 1, 0, 2, ...: repeats, and the last row first


@functools.lru_cache(maxsize=None)
def bl_weights(d):
    """(wt_a, wt_b [4096, d], base [3, d]) on the CPU; base holds -0.0 in rows 0 and 2 (first and last column)."""
    g = torch.Generator().manual_seed(7919 * d + 1)
    wt_a, wt_b, base = dense(g, PX, d), dense(g, PX, d), dense(g, BL_NB, d)
    base[0, 0] = base[0, d - 1] = base[2, 0] = -0.0
    return wt_a, wt_b, base


def bl_probe(n, d, shift, device):
    wt_a, wt_b, base = bl_weights(d)
    bits, _ = raster_probe(device)
    a, b, br = bl_rows(n, shift)
    return dict(bits=bits, wt_a=wt_a.to(device), wt_b=wt_b.to(device), base=base.to(device), row_a=a.to(device), row_b=b.to(device),
                base_row=br.to(device))


def bl_sequence(sel, wt, acc, descending=False):
    """The documented float sequence in float32: for p ascending, acc = where(pixel p set, acc + wt[p], acc).  ``where``, not
    ``+ 0.0``: a -0.0 start under an empty raster survives, and a weight row that is not selected -- inf, NaN -- never enters."""
    order = torch.nonzero(sel.any(0)).flatten().tolist()
    for p in (reversed(order) if descending else order):
        acc = torch.where(sel[:, p:p + 1], acc + wt[p], acc)
    return acc


POOL_VARIANTS = {
    None: lambda m: m,
    "bit63_dropped": lambda m: m & (torch.arange(IMG) < 63),                  # the sign bit of every word lost
    "transposed": lambda m: m.transpose(1, 2),                                # pixel index 64 x + y
}


def bl_table_of(wts, variant=None, descending=False):
    """The sequence for every (base option, raster a) pair: ([64, d] after operand a, [64, d] after operand b = (3 a + 2) % 16
    as well), float32 on the CPU; index = 16 * o + a with o = 0 for no base (+0.0) and 1 + j for base row j."""
    wt_a, wt_b, base = wts
    sel = POOL_VARIANTS[variant](raster_masks()).reshape(N_RASTERS, PX)
    start = torch.cat([torch.zeros(1, base.shape[1]), base]).repeat_interleave(N_RASTERS, dim=0)
    a = torch.arange(N_RASTERS).repeat(BL_NB + 1)
    one = bl_sequence(sel[a], wt_a, start, descending)
    return one, bl_sequence(sel[(3 * a + 2) % N_RASTERS], wt_b, one, descending)


@functools.lru_cache(maxsize=None)
def bl_table(d, variant=None, descending=False):
    """bl_table_of on the weights of the table's d, computed once."""
    return bl_table_of(bl_weights(d), variant, descending)


def bl_second_statement(d, two):
    """The same order stated independently: per (base option, raster) a numpy float32 row to which the weight rows of the LISTED
    set pixels are added one by one, ascending."""
    wt_a, wt_b, base = (t.numpy() for t in bl_weights(d))
    sel = raster_masks().reshape(N_RASTERS, PX).numpy()
    out = np.empty(((BL_NB + 1) * N_RASTERS, d), dtype=np.float32)
    for o in range(BL_NB + 1):
        for a in range(N_RASTERS):
            acc = np.zeros(d, dtype=np.float32) if o == 0 else base[o - 1].copy()
            for p in np.flatnonzero(sel[a]):
                acc = acc + wt_a[p]
            if two:
                for p in np.flatnonzero(sel[(3 * a + 2) % N_RASTERS]):
                    acc = acc + wt_b[p]
            out[N_RASTERS * o + a] = acc
    return torch.from_numpy(out)


def bl_option(n, shift, base_form):
    """Index into bl_table of every output row."""
    a, _, br = bl_rows(n, shift)
    o = {"none": torch.zeros_like(br), "row0": torch.ones_like(br), "rows": 1 + br}[base_form]
    return N_RASTERS * o + a


def bl_expected(n, d, shift, two, base_form):
    return bl_table(d)[int(two)][bl_option(n, shift, base_form)]


def bl_ref(n, d, shift, two, base_form):
    """-> (float64 sum, bound): the order-free net.  K = set pixels + 1 terms per output row (the base is the one more)."""
    wt_a, wt_b, base = (t.double() for t in bl_weights(d))
    sel = raster_masks().reshape(N_RASTERS, PX).double()
    a = torch.arange(N_RASTERS)
    b = (3 * a + 2) % N_RASTERS
    ref, mag, K = sel @ wt_a, sel @ wt_a.abs(), sel.sum(1)
    if two:
        ref, mag, K = ref + sel[b] @ wt_b, mag + sel[b] @ wt_b.abs(), K + sel[b].sum(1)
    start = torch.cat([torch.zeros(1, d, dtype=torch.float64), base])
    ref = (start[:, None, :] + ref[None]).reshape(-1, d)
    mag = (start.abs()[:, None, :] + mag[None]).reshape(-1, d)
    bound = torch.stack([dot_bound(int(K[i % N_RASTERS]) + 1, mag[i]) for i in range(mag.shape[0])])
    idx = bl_option(n, shift, base_form)
    return ref[idx], bound[idx]


def bl_lib(n, d, shift, two, base_form, device=CPU):
    """The plain torch float32 statement: the expanded rasters times the weights."""
    wt_a, wt_b, base = (t.to(device) for t in bl_weights(d))
    sel = raster_masks().reshape(N_RASTERS, PX).float().to(device)
    a, b, br = (t.to(device) for t in bl_rows(n, shift))
    y = sel[a] @ wt_a
    if base_form != "none":
        y = (base[br] if base_form == "rows" else base[:1]) + y
    return y + sel[b] @ wt_b if two else y


def bl_check(name, got, n, d, shift, two, base_form, lib=None):
    """``got`` [n, d] float32 on the CPU: bit for bit the documented sequence, inside the order-free bound (the q of a SEQUENTIAL sum
    is a property of the documented order, so the comparison with the library's q is left out), rows of a later grid round named."""
    want = bl_expected(n, d, shift, two, base_form)
    shape = (n, d, shift, base_form)
    assert got.shape == want.shape, (name, shape, tuple(got.shape))
    diff = (got.view(torch.int32) != want.view(torch.int32)).any(1)
    assert not bool(diff.any()), f"{name} {shape}: rows {torch.nonzero(diff).flatten()[:8].tolist()} differ from the documented sequence"
    first_late = launch_waves(n)
    if n > first_late:
        assert bool((want[first_late:] != 0).any(1).all()) and same_bits(got[first_late:], want[first_late:]), (name, shape, "rows of the second round")
    ref, bound = bl_ref(n, d, shift, two, base_form)
    lib = bl_lib(n, d, shift, two, base_form) if lib is None else lib
    return conform(name, got, lib, ref, bound, shape, tight=False)


def _bl_twin_table(variant=None, descending=False):
    return lambda n, d, shift, two, base_form: bl_table(d, variant, descending)[int(two)][bl_option(n, shift, base_form)]


def _bl_twin_last_group(n, d, shift, two, base_form):
    out = bl_expected(n, d, shift, two, base_form).clone()
    out[:, 256 * ((d - 1) // 256):] = 0.0
    return out


def _bl_twin_late_rows(n, d, shift, two, base_form):
    out = bl_expected(n, d, shift, two, base_form).clone()
    out[MAX_WAVES:] = 0.0
    return out


def _bl_selected(n, shift, two):
    a, b, _ = bl_rows(n, shift)
    return torch.cat([a, b]) if two else a


def _bl_any(pred):
    """applies(case, two, base_form): some selected raster satisfies pred(mask [64, 64])."""
    return lambda n, d, shift, two, base_form: any(bool(pred(raster_masks()[int(i)])) for i in set(_bl_selected(n, shift, two).tolist()))


BL_TWINS = {           # name -> (evaluation, applies(n, d, shift, two, base_form))
    "bit63_dropped": (_bl_twin_table("bit63_dropped"), _bl_any(lambda m: m[:, 63].any())),
    "pixel_index_transposed": (_bl_twin_table("transposed"), _bl_any(lambda m: (m != m.T).any())),
    # seen by the BITWISE check alone -- the sum of the same terms in another order stays inside the order-free bound; three or more
    # terms (with the start value) are needed for the order to show
    "descending_pixels": (_bl_twin_table(None, True), _bl_any(lambda m: m.sum() >= 30)),
    "last_column_group_left_out": (_bl_twin_last_group, lambda n, d, shift, two, base_form: True),
    "base_row_ignored": (lambda n, d, shift, two, base_form: bl_expected(n, d, shift, two, "row0"),
                         lambda n, d, shift, two, base_form: base_form == "rows"),
    "late_rows_unwritten": (_bl_twin_late_rows, lambda n, d, shift, two, base_form: n > MAX_WAVES),
}

BL_POISON = (64 * 20 + 20, 64 * 61 + 60)       # pixels of the weight rows that hold NaN / inf: inside full and block_1 (59.., 57..) only


def bl_poison_probe(d, device):
    """The probe with NaN in weight row 1300 and inf in weight row 3964 of BOTH operands, over all 16 rasters in order (b = (3 a + 2)
    % 16, base rows as bl_rows) -> (probe, expected [16, d] float32 on the CPU by the sequence, clean bool [16] per operand count:
    clean[two][r] = no poisoned pixel is selected for row r)."""
    wt_a, wt_b, base = (t.clone() for t in bl_weights(d))
    for wt in (wt_a, wt_b):
        wt[BL_POISON[0]] = math.nan
        wt[BL_POISON[1]] = math.inf
    one, both = bl_table_of((wt_a, wt_b, base))
    idx = bl_option(N_RASTERS, 0, "rows")
    a, b, br = bl_rows(N_RASTERS, 0)
    sel = raster_masks().reshape(N_RASTERS, PX)[:, list(BL_POISON)].any(1)
    bits, _ = raster_probe(device)
    pr = dict(bits=bits, wt_a=wt_a.to(device), wt_b=wt_b.to(device), base=base.to(device), row_a=a.to(device), row_b=b.to(device),
              base_row=br.to(device))
    return pr, (one[idx], both[idx]), (~sel[a], ~sel[a] & ~sel[b])


# ---------------------------------------------------------------------------------------------------------------------------
# The sigmoid as both head kernels write it: rcp(1 + exp(-x)), exp(y) = exp2(y * log2 e) on the hardware's v_exp_f32 / v_rcp_f32.

def sigmoid_allowance(x, s=None):
    """Absolute error allowed to a float32 sigmoid(x) evaluated as rcp(1 + exp2(-x * log2 e)), first order in u; x float64.
      t = -x * log2 e   the rounded product moves exp(-x) by |x| u relative (d exp(-x) / exp(-x) = |x| * relative error of t)
      e = exp2(t)       1 ulp (the kernel's comment and the ISA on v_exp_f32): at most 2 u relative
      d = 1 + e         half an ulp: u
      s = rcp(d)        1 ulp (v_rcp_f32): at most 2 u
    A relative error r of e moves s = 1 / (1 + e) by (1 - s) r relative (e / (1 + e) = 1 - s); those of d and s reach it in full:
      |ds| <= s (1 - s) (|x| + 2) u + 3 u s,
    plus 2**-126: a result (or an exp) flushed to zero is no error, so sigma of a logit below -88, where the kernel's exp overflows
    and the result is exactly 0, is none.  An infinite logit is met exactly (exp gives 0 or inf, rcp gives 1 or 0)."""
    s = torch.sigmoid(x) if s is None else s
    e = s * (1.0 - s) * (x.abs() + 2.0) * U32 + 3.0 * U32 * s
    return torch.where(torch.isinf(x), torch.zeros_like(s), e) + TINY


# ---------------------------------------------------------------------------------------------------------------------------
# k_sigmoid_dot<false|true>: out[r] = sum_j w[j] sigmoid(x[r, j]); one wave per row, lane l starts at column 4 l; an unrolled body
# of four float4 (`j + 768 < k`, step 1024) and a float4 tail (step 256).

SD_K = (4, 252, 256, 260, 772, 1024, 1028, 4096, 4100)
SD_N = (1, 5, 777, 8193)
SD_BIG_K = 260
SD_SHAPES = [(n, k) for k in SD_K for n in SD_N if n <= MAX_WAVES or k == SD_BIG_K]
SD_MAPS = 9
SD_EDGES = (0.0, -0.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, math.inf, -math.inf)


def sd_lane_plan(k):
    """Per lane (body trips, tail trips, first tail column or None) of k_sigmoid_dot's two loops."""
    plan = []
    for lane in range(WAVE):
        j, body, tail = 4 * lane, 0, 0
        while j + 12 * WAVE < k:
            j, body = j + 16 * WAVE, body + 1
        first = j if j < k else None
        while j < k:
            j, tail = j + 4 * WAVE, tail + 1
        plan.append((body, tail, first))
    return plan


def sd_body_columns(k):
    """bool [k]: the columns the unrolled body serves."""
    m = torch.zeros(k, dtype=torch.bool)
    for lane, (body, _, _) in enumerate(sd_lane_plan(k)):
        for t in range(body):
            for q in range(4):
                c = 4 * lane + 16 * WAVE * t + 4 * WAVE * q
                m[c:c + 4] = True
    return m


def sd_tail_first(k):
    firsts = [f for _, _, f in sd_lane_plan(k) if f is not None]
    return min(firsts) if firsts else None


def sd_probe(n, k, device, strided=False, seed=0):
    """x [n, k] (a view of a [n, k + 64] buffer when ``strided``), w [k], maps [9, k], w_row int32 [n] (maps 0 and 8 among them).
    Logits 3 randn; row r carries three of SD_EDGES at column 0, the first column of the tail loop and column k - 1."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * n + k)
    full = 3.0 * torch.randn(n, k + 64 if strided else k, generator=g)
    edges = torch.tensor(SD_EDGES)
    r = torch.arange(n)
    cols = [0, k - 1] + ([sd_tail_first(k)] if sd_tail_first(k) is not None else [])
    for i, c in enumerate(cols):
        full[:, c] = edges[(r + 3 * i) % len(SD_EDGES)]
    maps = dense(g, SD_MAPS, k)
    w_row = ((5 * r + 8) % SD_MAPS).to(torch.int32)              # row 0: map 8; row 2: map 0
    full = full.to(device)
    return dict(x=full[:, :k], w=maps[3].clone().to(device), maps=maps.to(device), w_row=w_row.to(device))


def sd_ref(x, w):
    """-> (float64 sum_j w_j sigmoid(x_j), bound); w [k] or, per row, [n, k].
    (a) the summation, the products' roundings with it: dot_bound(k, sum |w_j| s_j) -- any order, so the f32 lane sums, their f64
        total and its one rounding are covered;
    (b) every term's sigmoid: |w_j| * sigmoid_allowance(x_j)."""
    xd, wd = x.double(), w.double()
    s = torch.sigmoid(xd)
    terms = wd.abs() * s
    return (wd * s).sum(1), dot_bound(x.shape[1], terms.sum(1)) + (wd.abs() * sigmoid_allowance(xd, s)).expand_as(s).sum(1)


def sd_lib(x, w):
    return (torch.sigmoid(x) * w).sum(1)


def sd_exact_probe(k, device):
    """Rows that pin the infinities: all -inf (exactly 0.0), and all -inf but one +inf at column 0, the first tail column and k - 1
    (exactly w_j: every other term is w * 0 = 0) -> (x [4, k], w [k], expected [4])."""
    g = torch.Generator().manual_seed(k)
    w = dense(g, k)
    cols = [0, sd_tail_first(k) if sd_tail_first(k) is not None else 0, k - 1]
    x = torch.full((4, k), -math.inf)
    want = torch.zeros(4)
    for i, c in enumerate(cols):
        x[1 + i, c] = math.inf
        want[1 + i] = w[c]
    return x.to(device), w.to(device), want.to(device)


def twin_sd_tail_dropped(x, w):
    """The k % 1024 part behind the unrolled trips never summed."""
    kk = x.shape[1] - x.shape[1] % 1024
    return sd_lib(x[:, :kk], w[..., :kk])


def twin_sd_body_dropped(x, w):
    """The lanes that reach the unrolled body lose its columns."""
    keep = ~sd_body_columns(x.shape[1]).to(x.device)
    return sd_lib(x[:, keep], w[..., keep])


def twin_sd_late_rows(x, w):
    """Rows >= 8192 -- those of a second grid-stride round -- left unwritten."""
    out = sd_lib(x, w).clone()
    out[MAX_WAVES:] = 0.0
    return out


SD_TWINS = {
    "late_rows_unwritten": (twin_sd_late_rows, lambda n, k: n > MAX_WAVES),
    "tail_dropped": (twin_sd_tail_dropped, lambda n, k: k % 1024 != 0),
    "unrolled_body_dropped": (twin_sd_body_dropped, lambda n, k: bool(sd_body_columns(k).any())),
}


# ---------------------------------------------------------------------------------------------------------------------------
# k_head_sigmoid_dot<false|true> + k_head_sum: out[r] = sum_j w[j] sigmoid(h[r] . Wd[j] + bd[j]); 128 rows per workgroup, a 32-row
# slab per wave, 32-column tiles double-buffered in LDS (tile t in buffer t & 1), column ranges of `per` tiles per blockIdx.y.

HD_K = 256
HD_N_ROWS = (1, 31, 32, 33, 127, 128, 129, 257)
HD_N_COLS = (1, 31, 32, 33, 64, 100, 224, 4096)
HD_BIG_ROWS = (33, 129)                # the rows at which N = 4096 runs
HD_SHAPES = [(n, N) for N in HD_N_COLS for n in HD_N_ROWS if N < 4096 or n in HD_BIG_ROWS]
HD_MAPS = 11
HD_BIG_MAP = 1                         # the map of 1e30 everywhere: the last row's, and the one behind map 0 in memory
HD_BIG = 1e30


# The last rows of the per-row-map form at N = 4096 (hd_probe: the map of 1e30 in every column), pooled over n and splits: measured
# 1.067e-03 against 1.824e-04 (5.9 x; docs/MEASUREMENT_LOG.md, "Conformance of the acting-path kernels").  4096 POSITIVE terms, no
# cancellation.  The worst are the two launches with splits = 128 (9.478e-04 at n = 33, 1.067e-03 at n = 129): every range is one
# tile and k_head_sum adds the 128 partial sums one after the other -- its documented fixed order -- so the roundings random-walk
# over 127 additions (0.29 sqrt(128 / 3) u = 1.9 u expected, 3.9 u and 4.4 u of the sum measured, the bound allows 4096 u) where
# the library's tree lands within 0.75 u.  The wrapper's own choice never exceeds 32 ranges; with one range the same rows measure
# 7.3e-05 and 4.3e-05.
ROW_FACTOR[("head.rows.big_map", 4096)] = 8.0


def hd_plan(N, splits):
    """(tiles, per, used) as head_sigmoid_dot of csrc/api.hip chooses: ``used`` ranges hold a tile, range i starts at tile i * per."""
    tiles = ceil_div(N, 32)
    per = ceil_div(tiles, splits)
    return tiles, per, ceil_div(tiles, per)


def hd_splits(N):
    """The ``splits`` arguments a shape runs with (None: the wrapper's own choice)."""
    if N == 224:
        return (1, 2, 3, 7, 9)          # 3: per = 3, the second range starts at the odd tile 3; 9: used = 7 < splits
    return tuple(dict.fromkeys((None, 1, ceil_div(N, 32))))


def hd_probe(n, N, device, strided=False, seed=0):
    """h [n, 256] (a view of a [n, 320] buffer when ``strided``; rows distinct, row i scaled by 1 + i / n), Wd [N, 256], bd [N], w [N],
    maps [11, N] and w_row int32 [n].  w_row alternates between map 0 and map 10 inside every slab; the LAST row names map 1, which
    holds 1e30 in every column: the map a row beyond n would take (my_row is clamped to n - 1), its column N - 1 the weight a column
    beyond N would take (wc is clamped to N - 1), and -- lying behind map 0 in memory -- what an unclamped column index of a map-0
    row would read."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * n + N)
    full = torch.zeros(n, 320 if strided else HD_K)
    full[:, :HD_K] = torch.relu(torch.randn(n, HD_K, generator=g)) * (1.0 + torch.arange(n)[:, None] / n)
    Wd, bd = dense(g, N, HD_K) * 0.05, dense(g, N) * 0.1
    maps = dense(g, HD_MAPS, N)
    maps[HD_BIG_MAP] = HD_BIG
    w_row = torch.where(torch.arange(n) % 2 == 0, 0, HD_MAPS - 1).to(torch.int32)
    w_row[n - 1] = HD_BIG_MAP
    full = full.to(device)
    return dict(h=full[:, :HD_K], Wd=Wd.to(device), bd=bd.to(device), w=maps[3].clone().to(device), maps=maps.to(device), w_row=w_row.to(device))


def hd_ref(h, Wd, bd, w):
    """-> (float64 reference, bound); w [N] or per row [n, N].  With x_j = h . Wd_j + bd_j in float64:
      the logit     D_j = dot_bound(257, |h| . |Wd_j| + |bd_j|): 256 products and the bias, any order (the MFMA chain's included)
      its passage   through the sigmoid with a rigorous slope: max s (1 - s) over [x - D, x + D] = s'(max(|x| - D, 0)), 1 / 4 at most
      the sigmoid   sigmoid_allowance at the far end of that interval (|x| + D, the larger s)
      the sum       dot_bound(N, sum |w_j| s_j): N products in any order -- any split of the columns is admitted."""
    hd, Wdd, bdd, wd = h.double(), Wd.double(), bd.double(), w.double()
    x = hd @ Wdd.T + bdd
    D = dot_bound(HD_K + 1, hd.abs() @ Wdd.abs().T + bdd.abs())
    s = torch.sigmoid(x)
    near = torch.sigmoid((x.abs() - D).clamp_min(0.0))
    slope = near * (1.0 - near)
    far = torch.sigmoid(x + D)
    e_s = slope * D + sigmoid_allowance(x.abs() + D, far)
    return (wd * s).sum(1), dot_bound(Wd.shape[0], (wd.abs() * s).sum(1)) + (wd.abs() * e_s).sum(1)


def hd_lib(h, Wd, bd, w):
    return (torch.sigmoid(F.linear(h, Wd, bd)) * w).sum(1)


def twin_hd_slab_map(pr, N, splits):
    """Rows form: the map of a slab's first row weighs the whole slab."""
    r = torch.arange(pr["w_row"].numel(), device=pr["w_row"].device)
    return hd_lib(pr["h"], pr["Wd"], pr["bd"], pr["maps"][pr["w_row"][32 * (r // 32)].long()])


def twin_hd_dead_columns(pr, N, splits):
    """Rows form: a column beyond N is weighed with the clamped weight w[map][N - 1] (its logit is h . Wd[N - 1], no bias)."""
    w = pr["maps"][pr["w_row"].long()]
    dead = 32 * ceil_div(N, 32) - N
    return hd_lib(pr["h"], pr["Wd"], pr["bd"], w) + dead * w[:, N - 1] * torch.sigmoid(pr["h"] @ pr["Wd"][N - 1])


def twin_hd_last_split(pr, N, splits):
    """k_head_sum adds one range too few (shared map)."""
    _, per, used = hd_plan(N, splits)
    nn = (used - 1) * per * 32
    return hd_lib(pr["h"], pr["Wd"][:nn], pr["bd"][:nn], pr["w"][:nn])


def twin_hd_rows_permuted(pr, N, splits):
    """Neighbouring rows of a slab written to each other's place (shared map)."""
    out = hd_lib(pr["h"], pr["Wd"], pr["bd"], pr["w"])
    n = out.numel()
    r = torch.arange(n, device=out.device)
    return out[torch.where((r ^ 1) < n, r ^ 1, r)]


HD_TWINS = {           # name -> (evaluation, rows form?, applies(n, N, splits))
    "slab_first_row_map": (twin_hd_slab_map, True, lambda n, N, s: n >= 2),
    "dead_column_weighted": (twin_hd_dead_columns, True, lambda n, N, s: N % 32 != 0),
    "last_split_left_out": (twin_hd_last_split, False, lambda n, N, s: s is not None and hd_plan(N, s)[2] > 1),
    "rows_permuted_in_slab": (twin_hd_rows_permuted, False, lambda n, N, s: n >= 2),
}


# ---------------------------------------------------------------------------------------------------------------------------
# k_bits_dot: out[r] = sum over the set pixels of bits[bits_row[r]] of img[slot[r]], accumulated in f64 and rounded ONCE.

BD_N = (1, 5, 500)
BD_SLOTS = 4


def bd_probe(n, device, seed=0):
    """Non-integer count images img [4, 64, 64] (randn), rows over the 16 probe rasters (row 0 the empty one, row 1 the full one
    where n allows; n = 1: the full one), slots with repeats."""
    g = torch.Generator().manual_seed(1000003 * seed + n)
    img = torch.randn(BD_SLOTS, IMG, IMG, generator=g)
    r = torch.arange(n)
    rows = r % N_RASTERS if n > 1 else torch.ones(1, dtype=torch.int64)
    slot = (r * 3 + r // 7) % BD_SLOTS
    bits, sel = raster_probe(device)
    return dict(bits=bits, sel=sel, img=img.to(device), rows=rows.to(device), slot=slot.to(device))


def bd_ref(pr):
    """-> (float64 sum, bound = u |ref| + 4096 * 2**-53 * sum |terms|): at most 4096 terms added in f64, then one rounding to f32."""
    terms = pr["img"].double().reshape(-1, PX)[pr["slot"]] * pr["sel"][pr["rows"]].double()
    ref = terms.sum(1)
    return ref, U32 * ref.abs() + PX * 2.0 ** -53 * terms.abs().sum(1)


def bd_lib(pr):
    return (pr["img"].reshape(-1, PX)[pr["slot"]] * pr["sel"][pr["rows"]].float()).sum(1)


def twin_bd_float32(pr):
    """Accumulated in float32, pixel after pixel."""
    img = pr["img"].reshape(-1, PX)[pr["slot"]]
    sel = pr["sel"][pr["rows"]]
    acc = torch.zeros(sel.shape[0], device=img.device)
    for p in torch.nonzero(sel.any(0)).flatten().tolist():
        acc = torch.where(sel[:, p], acc + img[:, p], acc)
    return acc


BD_TWINS = {"accumulated_in_float32": (twin_bd_float32, lambda n: True)}        # every n of BD_N holds the full raster


def bd_count_probe(device):
    """Integer counts that reach 2**24: slot 0 holds 4096 everywhere (the full raster sums to 2**24 exactly), slot 1 integers
    below 4096 -> (probe, exact int64 sums)."""
    g = torch.Generator().manual_seed(24)
    img = torch.stack([torch.full((IMG, IMG), 4096.0), torch.randint(0, 4096, (IMG, IMG), generator=g).float()])
    rows = torch.arange(2 * N_RASTERS) % N_RASTERS
    slot = torch.arange(2 * N_RASTERS) // N_RASTERS
    bits, sel = raster_probe(device)
    want = (img.long().reshape(2, PX)[slot] * sel.cpu()[rows].long()).sum(1)
    assert int(want.max()) == 2 ** 24
    return dict(bits=bits, sel=sel, img=img.to(device), rows=rows.to(device), slot=slot.to(device)), want


# ---------------------------------------------------------------------------------------------------------------------------
# k_bits_accumulate: img[slot[r]] += weight[r] * raster(bits[bits_row[r]]) with float atomics; rows of weight 0 are skipped.

ACC_PATTERN = (-2147483648, 0x7fc12345, 0x3fc00000, -4194303, 0x00000001, 0x7f800000)   # -0.0, a NaN payload, 1.5, a negative NaN (0xffc00001), a subnormal, inf


def acc_pattern_image(slots, device):
    """float32 [slots, 64, 64] whose int32 view cycles through ACC_PATTERN (period 6 against rows of 64: every row differs)."""
    p = torch.tensor(ACC_PATTERN, dtype=torch.int32)
    return p[torch.arange(slots * PX) % len(ACC_PATTERN)].view(torch.float32).reshape(slots, IMG, IMG).clone().to(device)


def acc_contention_probe(device, n=500):
    """(a) n rows of the full raster onto ONE slot of three, weights in {1, 2} -> (bits_row, slot, weight, exact total)."""
    r = torch.arange(n)
    weight = 1.0 + (r % 3 == 0).float()
    return (torch.ones(n, dtype=torch.int64).to(device), torch.ones(n, dtype=torch.int64).to(device), weight.to(device), float(weight.sum()))


def acc_disjoint_probe(device):
    """(b) rows whose (slot, pixel) sets are disjoint, arbitrary weights: slot 0 takes the four corner pixels and row 17, slot 1
    column 63 and block_0, slot 2 the full raster, slot 3 nothing (the empty raster) -> (bits_row, slot, weight)."""
    g = torch.Generator().manual_seed(11)
    rows = torch.tensor([2, 3, 4, 5, 6, 7, 8, 1, 0])
    slot = torch.tensor([0, 0, 0, 0, 0, 1, 1, 2, 3])
    return rows.to(device), slot.to(device), dense(g, rows.numel()).to(device)


def acc_single_add(img, sel, rows, slot, weight):
    """The single float32 add of (b): every touched pixel img + w, every other one as it was."""
    out = img.clone().reshape(-1, PX)
    for r in range(rows.numel()):
        s = int(slot[r])
        out[s] = torch.where(sel[int(rows[r])], out[s] + weight[r], out[s])
    return out.reshape(img.shape)
