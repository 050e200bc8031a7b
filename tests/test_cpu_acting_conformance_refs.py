"""CPU: the references, bounds and twins of tests/acting_conformance.py checked without a GPU.

* At every row of every table torch's own float32 CPU evaluation passes ``conform`` against the reference (with itself as the
  yardstick); for the bitwise checks the sequential reference equals an independent second statement of the order.
* Every defective twin -- a float32 evaluation wrong in one way a kernel could be -- is rejected at every row where its defect
  applies, and applies to at least one row: the evidence that tests/test_gpu_acting_conformance.py would notice such a kernel.
* The tables reach the branches they are there for, recomputed from the shapes with the formulas of csrc/api.hip."""
import math

import pytest
import torch

import acting_conformance as A

CPU = A.CPU


def rejected(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------
# rasters

def test_raster_probe_holds_every_named_raster():
    bits, sel = A.raster_probe(CPU)
    m = A.raster_masks()
    count = dict(zip(A.RASTER_NAMES, m.reshape(A.N_RASTERS, -1).sum(1).tolist()))
    assert count["empty"] == 0 and count["full"] == 4096 and count["row_17"] == count["col_63"] == 64
    assert all(count[k] == 1 for k in A.RASTER_NAMES[2:6]) and all(35 <= count[f"block_{i}"] <= 36 for i in range(8))
    assert m[2, 0, 0] and m[3, 0, 63] and m[4, 63, 0] and m[5, 63, 63]
    # the packing convention: bit x of word y is pixel 64 y + x; bit 63 is the sign bit
    assert int(bits[2, 0]) == 1 and int(bits[3, 0]) == -2 ** 63 and int(bits[4, 63]) == 1 and int(bits[5, 63]) == -2 ** 63
    assert bool((bits[1] == -1).all()) and int(bits[6, 17]) == -1 and bool((bits[7] == -2 ** 63).all()) and not bool(bits[0].any())
    assert torch.equal(A.unpack_bits(bits), sel) and torch.equal(A.raster_expand(bits), m.float())
    ored = A.bits_or_ref(bits, A.BITS_OR_RANGES)
    assert not bool(ored[0].any()) and not bool(ored[5].any()) and torch.equal(ored[1], bits[3]) and bool((ored[2] == -1).all())
    assert {hi - lo for lo, hi in A.BITS_OR_RANGES} >= {0, 1} and A.BITS_OR_RANGES[3][1] > A.BITS_OR_RANGES[4][0]      # overlapping


# ---------------------------------------------------------------------------------------------------------------------------
# bits_linear / bits_linear2

def bl_forms():
    return [(two, form) for two in (False, True) for form in A.BL_BASE_FORMS]


@pytest.mark.parametrize("d", A.BL_D)
def test_bits_linear_sequence_has_two_statements_and_the_library_is_inside_the_bound(d):
    one, both = A.bl_table(d)
    assert A.same_bits(one, A.bl_second_statement(d, False)) and A.same_bits(both, A.bl_second_statement(d, True))
    # the -0.0 of the base survives an empty raster, and +0.0 stands where there is neither base nor pixel
    assert math.copysign(1.0, float(one[A.N_RASTERS * 1 + 0, 0])) == -1.0 and math.copysign(1.0, float(one[0, 0])) == 1.0
    for n, dd, shift in [c for c in A.BL_CASES if c[1] == d]:
        for two, form in bl_forms():
            want = A.bl_expected(n, d, shift, two, form)
            A.bl_check("bits_linear2" if two else "bits_linear", want, n, d, shift, two, form)
            lib = A.bl_lib(n, d, shift, two, form)
            A.conform("bits_linear.library", lib, lib, *A.bl_ref(n, d, shift, two, form), (n, d, shift, form))


@pytest.mark.parametrize("twin", sorted(A.BL_TWINS))
def test_defective_bits_linear_twins_are_rejected(twin):
    fn, applies = A.BL_TWINS[twin]
    hit = [(c, two, form) for c in A.BL_CASES for two, form in bl_forms() if applies(*c, two, form)]
    assert hit, twin
    for (n, d, shift), two, form in hit:
        assert rejected(A.bl_check, twin, fn(n, d, shift, two, form), n, d, shift, two, form), (twin, n, d, shift, two, form)
    if twin == "descending_pixels":                 # the order-free net alone does NOT see this one: the bitwise check is what does
        n, d, shift = 5, 260, 10
        got = fn(n, d, shift, True, "rows")
        A.conform(twin, got, A.bl_lib(n, d, shift, True, "rows"), *A.bl_ref(n, d, shift, True, "rows"), tight=False)


def test_bits_linear_poison_probe_keeps_clean_rows_finite():
    for d in (4, 260):
        _, (one, both), (clean1, clean2) = A.bl_poison_probe(d, CPU)
        for out, clean in ((one, clean1), (both, clean2)):
            assert bool(clean.any()) and not bool(clean.all())
            assert bool(torch.isfinite(out[clean]).all()) and not bool(torch.isfinite(out[~clean]).all(1).any())
        assert A.same_bits(one[clean1], A.bl_table(d)[0][A.bl_option(A.N_RASTERS, 0, "rows")][clean1])


def test_bits_linear_table_reaches_its_branches():
    assert {d for _, d, _ in A.BL_CASES} == set(A.BL_D) == {4, 252, 256, 260, 516, 772} and {n for n, _, _ in A.BL_CASES} == set(A.BL_N)
    big = [(n, d) for n, d, _ in A.BL_CASES if n > 16]
    assert big == [(8193, 4), (8193, 260)]
    for n, d in big:                                 # the launch is capped: row 8192 waits for the second round, and holds the full raster
        assert A.launch_waves(n) == A.MAX_WAVES == 8192 < n and int(A.bl_rows(n, 0)[0][8192]) == A.RASTER_NAMES.index("full")
    assert A.launch_waves(777) == 780 and A.launch_waves(1) == 4
    for d, lanes_of_last_group in ((4, 1), (252, 63), (256, 64), (260, 1), (516, 1), (772, 1)):
        assert len(range(256 * ((d - 1) // 256), d, 4)) == lanes_of_last_group
    # every raster is met as operand a and as operand b, every base row with repeats, below the long case already
    small = [c for c in A.BL_CASES if c[0] <= 16 and c[1] == 260]
    a = torch.cat([A.bl_rows(n, s)[0] for n, _, s in small])
    assert set(a.tolist()) >= set(range(15)) and set(A.bl_rows(8193, 0)[1].tolist()) == set(range(16))
    br = A.bl_rows(5, 0)[2].tolist()
    assert br[0] == A.BL_NB - 1 and len(set(br)) < len(br) and set(br) == set(range(A.BL_NB))


# ---------------------------------------------------------------------------------------------------------------------------
# sigmoid_dot

def sd_conform_all(shape, fn):
    n, k = shape
    for strided in (False, True):
        pr = A.sd_probe(n, k, CPU, strided)
        A.conform("sigmoid_dot", fn(pr["x"], pr["w"]), A.sd_lib(pr["x"], pr["w"]), *A.sd_ref(pr["x"], pr["w"]), shape)
        wr = pr["maps"][pr["w_row"].long()]
        A.conform("sigmoid_dot.rows", fn(pr["x"], wr), A.sd_lib(pr["x"], wr), *A.sd_ref(pr["x"], wr), shape)


@pytest.mark.parametrize("k", A.SD_K)
def test_float32_sigmoid_dot_passes(k):
    for shape in [s for s in A.SD_SHAPES if s[1] == k]:
        sd_conform_all(shape, A.sd_lib)
    x, w, want = A.sd_exact_probe(k, CPU)
    assert torch.equal(A.sd_lib(x, w), want)         # +inf contributes exactly w_j, -inf exactly 0


@pytest.mark.parametrize("twin", sorted(A.SD_TWINS))
def test_defective_sigmoid_dot_twins_are_rejected(twin):
    fn, applies = A.SD_TWINS[twin]
    hit = [s for s in A.SD_SHAPES if applies(*s)]
    assert hit, twin
    for shape in hit:
        assert rejected(sd_conform_all, shape, fn), (twin, shape)


def test_sigmoid_dot_table_reaches_its_branches():
    assert {k for _, k in A.SD_SHAPES} == set(A.SD_K) and {n for n, _ in A.SD_SHAPES} == set(A.SD_N)
    assert [(n, k) for n, k in A.SD_SHAPES if n > A.MAX_WAVES] == [(8193, 260)] and A.launch_waves(8193) == 8192
    plans = {k: A.sd_lane_plan(k) for k in A.SD_K}
    # 772: lane 0 is in the unrolled body while lanes 1..63 are in the tail; 1028, 4100: a tail of lane 0 alone behind the body
    assert plans[772][0][:2] == (1, 0) and all(p[:2] == (0, 3) for p in plans[772][1:])
    assert any({b > 0 for b, t, _ in p} == {True, False} for p in plans.values())
    for k in (1028, 4100):
        assert plans[k][0][1] == 1 and all(p[1] == 0 for p in plans[k][1:]) and all(p[0] == k // 1024 for p in plans[k])
    assert all(p[:2] == (1, 0) for p in plans[1024]) and all(p[:2] == (4, 0) for p in plans[4096])
    assert [p[1] for p in plans[4]] == [1] + [0] * 63 and [p[1] for p in plans[252]] == [1] * 63 + [0]
    assert [p[1] for p in plans[260]] == [2] + [1] * 63
    assert A.sd_tail_first(772) == 4 and A.sd_tail_first(1028) == 1024 and A.sd_tail_first(4096) is None
    # every column is served exactly once
    for k, p in plans.items():
        assert sum(16 * b + 4 * t for b, t, _ in p) == k
    pr = A.sd_probe(777, 260, CPU)
    assert {0, A.SD_MAPS - 1} <= set(pr["w_row"].tolist()) and int(pr["w_row"][0]) == A.SD_MAPS - 1
    edge_cols = pr["x"][:, [0, 259, 256]]
    assert all(bool((edge_cols == e).any()) for e in A.SD_EDGES) and bool((edge_cols == 0).any())


def test_sigmoid_allowance_covers_the_documented_cases():
    x = torch.tensor([0.0, -0.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, math.inf, -math.inf, 3.0], dtype=torch.float64)
    e = A.sigmoid_allowance(x)
    s = torch.sigmoid(x)
    assert bool((e[8:10] == A.TINY).all())                                          # an infinite logit: exact but for the floor
    assert bool((s[[5, 7]] < A.TINY).all()) and bool((s[[5, 7]] <= e[[5, 7]]).all())   # below -88: returning exactly 0 is inside
    assert float(s[3]) > A.TINY                                                     # -87 is still a normal float32 result
    assert abs(float(e[10]) / A.U32 - (float(s[10] * (1 - s[10])) * 5.0 + 3.0 * float(s[10]))) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# head_sigmoid_dot

def hd_conform(shape, rows_form, fn, strided=False):
    n, N, splits = shape
    pr = A.hd_probe(n, N, CPU, strided)
    w = pr["maps"][pr["w_row"].long()] if rows_form else pr["w"]
    got = fn(pr, N, splits)
    A.conform("head.rows" if rows_form else "head", got, A.hd_lib(pr["h"], pr["Wd"], pr["bd"], w), *A.hd_ref(pr["h"], pr["Wd"], pr["bd"], w), shape)


def hd_clean(rows_form):
    return lambda pr, N, splits: A.hd_lib(pr["h"], pr["Wd"], pr["bd"], pr["maps"][pr["w_row"].long()] if rows_form else pr["w"])


@pytest.mark.parametrize("N", A.HD_N_COLS)
def test_float32_head_passes(N):
    for n, _ in [s for s in A.HD_SHAPES if s[1] == N]:
        for rows_form in (False, True):
            for strided in (False, True):
                hd_conform((n, N, None), rows_form, hd_clean(rows_form), strided)


@pytest.mark.parametrize("twin", sorted(A.HD_TWINS))
def test_defective_head_twins_are_rejected(twin):
    fn, rows_form, applies = A.HD_TWINS[twin]
    hit = [(n, N, s) for n, N in A.HD_SHAPES for s in A.hd_splits(N) if applies(n, N, s)]
    assert hit, twin
    for shape in hit:
        assert rejected(hd_conform, shape, rows_form, fn), (twin, shape)


def test_head_table_reaches_its_branches():
    assert {n for n, _ in A.HD_SHAPES} == set(A.HD_N_ROWS) and {N for _, N in A.HD_SHAPES} == set(A.HD_N_COLS)
    assert sorted(n for n, N in A.HD_SHAPES if N == 4096) == [33, 129]
    assert A.hd_splits(224) == (1, 2, 3, 7, 9) and A.hd_plan(224, 1)[0] == 7
    tiles, per, used = A.hd_plan(224, 3)
    assert (per, used) == (3, 3) and [i * per for i in range(used)][1] % 2 == 1          # an odd t_beg: the first tile lands in buffer 1
    tiles, per, used = A.hd_plan(224, 9)
    assert used == 7 < 9                                                                 # k_head_sum runs over `used`, not `splits`
    assert A.hd_plan(224, 2)[1:] == (4, 2) and A.hd_plan(224, 7)[1:] == (1, 7)
    assert any(N % 32 and n % 32 for n, N in A.HD_SHAPES) and A.hd_splits(4096) == (None, 1, 128) and A.hd_splits(1) == (None, 1)
    for n, N in A.HD_SHAPES:                                                             # every range of every row holds a tile
        for s in A.hd_splits(N):
            if s is not None:
                tiles, per, used = A.hd_plan(N, s)
                assert (used - 1) * per < tiles <= used * per and used <= s
    pr = A.hd_probe(129, 100, CPU)
    wr = pr["w_row"].tolist()
    assert wr[:4] == [0, 10, 0, 10] and wr[-1] == A.HD_BIG_MAP and wr.count(A.HD_BIG_MAP) == 1
    assert bool((pr["maps"][A.HD_BIG_MAP] == A.HD_BIG).all())
    assert len({tuple(r.tolist()) for r in pr["h"]}) == 129 and A.hd_probe(129, 100, CPU, True)["h"].stride(0) == 320


# ---------------------------------------------------------------------------------------------------------------------------
# bits_dot, bits_accumulate

@pytest.mark.parametrize("n", A.BD_N)
def test_float32_bits_dot_passes_and_a_float32_accumulation_is_rejected(n):
    pr = A.bd_probe(n, CPU)
    ref, bound = A.bd_ref(pr)
    once = ref.float()                                # f64 accumulation rounded once: what the kernel promises
    A.conform("bits_dot", once, once, ref, bound, n)
    twin, applies = A.BD_TWINS["accumulated_in_float32"]
    assert applies(n) and bool((pr["rows"] == A.RASTER_NAMES.index("full")).any())
    assert rejected(A.conform, "bits_dot", twin(pr), once, ref, bound, n)
    if n > 1:
        assert float(ref[0]) == 0.0 and float(bound[0]) == 0.0                           # the empty raster: exactly 0.0
    assert len(set(pr["slot"].tolist())) < max(n, 2)


def test_bits_dot_count_probe_is_exact_in_either_precision():
    pr, want = A.bd_count_probe(CPU)
    assert torch.equal(A.bd_lib(pr).long(), want) and torch.equal(A.twin_bd_float32(pr).long(), want)


def test_bits_accumulate_probes():
    _, sel = A.raster_probe(CPU)
    rows, slot, weight, total = A.acc_contention_probe(CPU)
    assert rows.numel() == 500 and set(weight.tolist()) == {1.0, 2.0} and total == 667.0 and len(set(slot.tolist())) == 1
    rows, slot, weight = A.acc_disjoint_probe(CPU)
    for s in set(slot.tolist()):                      # disjoint inside every slot
        assert int(sel[rows[slot == s]].long().sum(0).max()) <= 1
    img = A.acc_pattern_image(4, CPU)
    iv = img.view(torch.int32)
    assert set(iv.flatten().tolist()) == set(A.ACC_PATTERN) and bool(torch.isnan(img).any()) and int(iv[0, 0, 0]) == -2 ** 31
    start = torch.randn(4, 64, 64, generator=torch.Generator().manual_seed(3))
    out = A.acc_single_add(start, sel, rows, slot, weight)
    ref = start.clone()
    ref.index_add_(0, slot, sel[rows].float().reshape(-1, 64, 64) * weight[:, None, None])
    touched = torch.zeros(4, 4096, dtype=torch.bool).index_put_((slot,), sel[rows], accumulate=True).reshape(4, 64, 64)
    assert torch.equal(out[touched], ref[touched]) and A.same_bits(out[~touched], start[~touched]) and bool(touched[3].sum() == 0)
