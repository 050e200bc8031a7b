"""GPU: conformance of the kernels behind VecDQN's factored acting forward -- k_bits_linear / k_bits_linear2, k_sigmoid_dot<false|true>,
k_head_sigmoid_dot<false|true> + k_head_sum, k_bits_dot / k_bits_accumulate and the raster helpers k_bits_to_f32 / k_bits_or --
through bridges_hip.ops (the C ABI where a wrapper narrows the entry point).

Tables, probe data, references, bounds and twins come from tests/acting_conformance.py (checked without a GPU by
tests/test_cpu_acting_conformance_refs.py, which also shows that a kernel wrong in one of fourteen ways would be rejected); the
acceptance rule is tests/mlp_conformance.py's ``conform``:

* every element inside the first-order float32 bound around the float64 result, and q_kernel <= FACTOR * q_library, the library
  being the plain torch float32 expression on the same device (``Q ...`` lines are printed; docs/MEASUREMENT_LOG.md records a run);
* where a kernel documents its float sequence (k_bits_linear, k_bits_linear2) or an exact result, the bits of that result;
* every row table holds a launch of more than 8192 rows where the launch is capped, so the grid-stride round runs;
* refusals return -1 and leave a sentinel-filled output alone."""
import ctypes as C
import math

import pytest
import torch

import acting_conformance as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -77.25
E_ARG = -1                                          # BRIDGES_E_ARG


def lib():
    from bridges_hip import abi
    return abi.require_gpu()


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else C.c_void_p(0)


def stream():
    from bridges_hip import abi
    return abi.current_stream()


def poison(*shape):
    """Fill a block of the size the next result takes with NaN and hand it back to the allocator: a row the kernel leaves unwritten
    then shows NaN, not what an earlier call left there."""
    torch.full(shape, math.nan, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# bits_linear / bits_linear2

def run_bits_linear(pr, two, form, identity=False):
    from bridges_hip import ops
    base = None if form == "none" else pr["base"]
    base_row = pr["base_row"] if form == "rows" else None           # "row0": base WITHOUT base_row -- every row gets base row 0
    n, d = pr["row_a"].numel(), pr["wt_a"].shape[1]
    bits_a, row_a, bits_b, row_b = pr["bits"], pr["row_a"], pr["bits"], pr["row_b"]
    if identity:                                                    # no row index: raster r belongs to row r
        bits_a, row_a, bits_b, row_b = pr["bits"][row_a].contiguous(), None, pr["bits"][row_b].contiguous(), None
    poison(n, d)
    if two:
        return ops.bits_linear2(bits_a, pr["wt_a"], bits_b, pr["wt_b"], bits_row_a=row_a, bits_row_b=row_b, base=base, base_row=base_row)
    return ops.bits_linear(bits_a, pr["wt_a"], bits_row=row_a, base=base, base_row=base_row)


@pytest.mark.parametrize("d", A.BL_D)
def test_bits_linear_is_the_documented_sequence(d):
    """Bit for bit base first, then the weight rows of the set pixels in ascending p, operand a before operand b; inside the
    order-free bound of the float64 sum.  Base forms: none, ``base`` without ``base_row`` (every row gets base row 0) and ``base``
    with ``base_row``.  The case of 8193 rows checks rows >= 8192 -- the second grid-stride round -- by name (A.bl_check)."""
    for n, _, shift in [c for c in A.BL_CASES if c[1] == d]:
        pr = A.bl_probe(n, d, shift, DEV)
        for two in (False, True):
            name = "bits_linear2" if two else "bits_linear"
            for form in A.BL_BASE_FORMS:
                got = run_bits_linear(pr, two, form)
                A.bl_check(name, got.cpu(), n, d, shift, two, form, lib=A.bl_lib(n, d, shift, two, form, DEV).cpu())
                if n == 5:
                    assert A.same_bits(run_bits_linear(pr, two, form, identity=True), got), (name, n, d, shift, form)


@pytest.mark.parametrize("d", [4, 260])
def test_bits_linear_never_touches_a_weight_row_it_does_not_select(d):
    """NaN and inf in the weight rows of two pixels: every output row whose rasters select neither is finite and the sequence bit
    for bit (a product with the expanded raster would be NaN everywhere); the others are not finite."""
    pr, want, clean = A.bl_poison_probe(d, DEV)
    for two in (False, True):
        got = run_bits_linear(pr, two, "rows").cpu()
        ok = clean[int(two)]
        assert bool(torch.isfinite(got[ok]).all()) and A.same_bits(got[ok], want[int(two)][ok])
        assert not bool(torch.isfinite(got[~ok]).all(1).any())


def test_bits_linear_refusals():
    L = lib()
    pr = A.bl_probe(5, 8, 0, DEV)
    out = torch.full((5, 8), SENTINEL, device=DEV)
    b, ra, w, base, br, s = ptr(pr["bits"]), ptr(pr["row_a"]), ptr(pr["wt_a"]), ptr(pr["base"]), ptr(pr["base_row"]), stream()
    assert L.bridges_bits_linear(5, b, ra, w, 8, base, br, ptr(out), s) == 0
    torch.cuda.synchronize()
    assert A.same_bits(out.cpu(), A.bl_expected(5, 8, 0, False, "rows"))           # the arguments the refusals below vary are good
    out.fill_(SENTINEL)
    for rc in (L.bridges_bits_linear(5, b, ra, w, 6, base, br, ptr(out), s),                     # d % 4
               L.bridges_bits_linear(5, b, ra, w, 0, base, br, ptr(out), s),
               L.bridges_bits_linear(-1, b, ra, w, 8, base, br, ptr(out), s),
               L.bridges_bits_linear(5, b, ra, ptr(pr["wt_a"], 4), 8, base, br, ptr(out), s),    # one float off 16-byte alignment
               L.bridges_bits_linear(5, b, ra, w, 8, ptr(pr["base"], 4), br, ptr(out), s),
               L.bridges_bits_linear(5, b, ra, w, 8, base, br, ptr(out, 4), s),
               L.bridges_bits_linear(5, None, ra, w, 8, base, br, ptr(out), s),                  # null operands
               L.bridges_bits_linear(5, b, ra, None, 8, base, br, ptr(out), s),
               L.bridges_bits_linear(5, b, ra, w, 8, base, br, None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_bits_linear2_refusals():
    L = lib()
    pr = A.bl_probe(5, 8, 0, DEV)
    out = torch.full((5, 8), SENTINEL, device=DEV)
    b, ra, rb, wa, wb, base, br, s = (ptr(pr["bits"]), ptr(pr["row_a"]), ptr(pr["row_b"]), ptr(pr["wt_a"]), ptr(pr["wt_b"]), ptr(pr["base"]),
                                      ptr(pr["base_row"]), stream())
    o = ptr(out)
    for rc in (L.bridges_bits_linear2(5, b, ra, wa, b, rb, wb, 6, base, br, o, s),                # d % 4
               L.bridges_bits_linear2(-1, b, ra, wa, b, rb, wb, 8, base, br, o, s),
               L.bridges_bits_linear2(5, b, ra, ptr(pr["wt_a"], 4), b, rb, wb, 8, base, br, o, s),    # one float off 16-byte alignment
               L.bridges_bits_linear2(5, b, ra, wa, b, rb, ptr(pr["wt_b"], 4), 8, base, br, o, s),
               L.bridges_bits_linear2(5, b, ra, wa, b, rb, wb, 8, ptr(pr["base"], 4), br, o, s),
               L.bridges_bits_linear2(5, b, ra, wa, b, rb, wb, 8, base, br, ptr(out, 4), s),
               L.bridges_bits_linear2(5, None, ra, wa, b, rb, wb, 8, base, br, o, s),             # null operands
               L.bridges_bits_linear2(5, b, ra, None, b, rb, wb, 8, base, br, o, s),
               L.bridges_bits_linear2(5, b, ra, wa, None, rb, wb, 8, base, br, o, s),
               L.bridges_bits_linear2(5, b, ra, wa, b, rb, None, 8, base, br, o, s),
               L.bridges_bits_linear2(5, b, ra, wa, b, rb, wb, 8, base, br, None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# sigmoid_dot

@pytest.mark.parametrize("k", A.SD_K)
def test_sigmoid_dot_inside_the_bound(k):
    """Shared map and per-row maps, contiguous and as a view with row_stride = k + 64, at every n of the table (8193 rows at
    k = 260: the second grid-stride round); edge logits at the first and last column and the first column of the tail loop."""
    from bridges_hip import ops
    for n, _ in [s for s in A.SD_SHAPES if s[1] == k]:
        for strided in (False, True):
            pr = A.sd_probe(n, k, DEV, strided)
            x, w, maps, w_row = pr["x"], pr["w"], pr["maps"], pr["w_row"]
            assert x.stride(0) == (k + 64 if strided else k)
            shape = (n, k, "strided" if strided else "contiguous")
            poison(n)
            got = ops.sigmoid_dot(x, w)
            A.conform("sigmoid_dot", got, A.sd_lib(x, w), *A.sd_ref(x, w), shape, tight=n > A.FEW_ROWS)
            wr = maps[w_row.long()]
            poison(n)
            got_rows = ops.sigmoid_dot(x, maps, w_row=w_row)
            A.conform("sigmoid_dot.rows", got_rows, A.sd_lib(x, wr), *A.sd_ref(x, wr), shape, tight=n > A.FEW_ROWS)
            if n > A.launch_waves(n):
                late = slice(A.launch_waves(n), n)
                assert bool(torch.isfinite(got[late]).all()) and bool((got[late] != 0).all()) and bool((got_rows[late] != 0).all())
            for m in (0, A.SD_MAPS - 1, 3):                                 # every row naming map m: the shared-map call with w[m], bit for bit
                assert torch.equal(ops.sigmoid_dot(x, maps, w_row=torch.full((n,), m, dtype=torch.int32, device=DEV)),
                                   ops.sigmoid_dot(x, maps[m])), (shape, m)


def test_sigmoid_dot_few_rows_pooled():
    """The rows of the table with at most FEW_ROWS elements give either q as the largest of a few draws (kernel and library often
    return the same float, or neighbours): every element is inside its bound above; the two q are compared over all of them."""
    from bridges_hip import ops
    pool, pool_rows = [], []
    for n, k in [s for s in A.SD_SHAPES if s[0] <= A.FEW_ROWS]:
        for strided in (False, True):
            pr = A.sd_probe(n, k, DEV, strided)
            x, w, maps, w_row = pr["x"], pr["w"], pr["maps"], pr["w_row"]
            wr = maps[w_row.long()]
            pool.append((ops.sigmoid_dot(x, w), A.sd_lib(x, w), *A.sd_ref(x, w)))
            pool_rows.append((ops.sigmoid_dot(x, maps, w_row=w_row), A.sd_lib(x, wr), *A.sd_ref(x, wr)))
    A.conform_pooled("sigmoid_dot.few_rows", pool, len(pool))
    A.conform_pooled("sigmoid_dot.rows.few_rows", pool_rows, len(pool_rows))


@pytest.mark.parametrize("k", A.SD_K)
def test_sigmoid_dot_infinities_and_nan(k):
    """+inf contributes exactly w_j and -inf exactly 0; one NaN makes exactly its row NaN and every other row conforms."""
    from bridges_hip import ops
    x, w, want = A.sd_exact_probe(k, DEV)
    assert torch.equal(ops.sigmoid_dot(x, w), want)
    assert torch.equal(ops.sigmoid_dot(x, w.expand(2, k).contiguous(), w_row=torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=DEV)), want)
    pr = A.sd_probe(5, k, DEV)
    x = pr["x"].clone()
    x[2, k - 1] = math.nan
    got = ops.sigmoid_dot(x, pr["w"])
    assert torch.isnan(got).tolist() == [False, False, True, False, False]
    keep = torch.tensor([0, 1, 3, 4], device=DEV)
    ref, bound = A.sd_ref(x[keep], pr["w"])
    A.conform("sigmoid_dot.beside_nan", got[keep], A.sd_lib(x[keep], pr["w"]), ref, bound, (5, k), tight=False)


def test_sigmoid_dot_refusals():
    L = lib()
    pr = A.sd_probe(5, 256, DEV, strided=True)
    x, w, s = pr["x"], pr["w"], stream()
    out = torch.full((5,), SENTINEL, device=DEV)
    o = ptr(out)
    for rc in (L.bridges_sigmoid_dot(5, ptr(x), 320, ptr(w), 6, o, s),                           # k % 4
               L.bridges_sigmoid_dot(5, ptr(x), 318, ptr(w), 256, o, s),                         # row_stride % 4
               L.bridges_sigmoid_dot(5, ptr(x), 320, ptr(w), 0, o, s),
               L.bridges_sigmoid_dot(-1, ptr(x), 320, ptr(w), 256, o, s),
               L.bridges_sigmoid_dot(5, ptr(x, 4), 320, ptr(w), 256, o, s),                      # one float off 16-byte alignment
               L.bridges_sigmoid_dot(5, ptr(x), 320, ptr(w, 4), 252, o, s),
               L.bridges_sigmoid_dot(5, None, 320, ptr(w), 256, o, s),                           # null operands
               L.bridges_sigmoid_dot(5, ptr(x), 320, None, 256, o, s),
               L.bridges_sigmoid_dot(5, ptr(x), 320, ptr(w), 256, None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_sigmoid_dot_rows_refusals():
    L = lib()
    pr = A.sd_probe(5, 256, DEV, strided=True)
    x, maps, w_row, s = pr["x"], pr["maps"], pr["w_row"], stream()
    out = torch.full((5,), SENTINEL, device=DEV)
    o = ptr(out)
    for rc in (L.bridges_sigmoid_dot_rows(5, ptr(x), 320, ptr(maps), ptr(w_row), 6, o, s),       # k % 4
               L.bridges_sigmoid_dot_rows(5, ptr(x), 318, ptr(maps), ptr(w_row), 256, o, s),     # row_stride % 4
               L.bridges_sigmoid_dot_rows(-1, ptr(x), 320, ptr(maps), ptr(w_row), 256, o, s),
               L.bridges_sigmoid_dot_rows(5, ptr(x, 4), 320, ptr(maps), ptr(w_row), 256, o, s),  # one float off 16-byte alignment
               L.bridges_sigmoid_dot_rows(5, ptr(x), 320, ptr(maps, 4), ptr(w_row), 252, o, s),
               L.bridges_sigmoid_dot_rows(5, None, 320, ptr(maps), ptr(w_row), 256, o, s),       # null operands
               L.bridges_sigmoid_dot_rows(5, ptr(x), 320, None, ptr(w_row), 256, o, s),
               L.bridges_sigmoid_dot_rows(5, ptr(x), 320, ptr(maps), None, 256, o, s),
               L.bridges_sigmoid_dot_rows(5, ptr(x), 320, ptr(maps), ptr(w_row), 256, None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# head_sigmoid_dot

@pytest.mark.parametrize("N", A.HD_N_COLS)
def test_head_sigmoid_dot_inside_the_bound(N):
    """Shared map and per-row maps at every (n, N) of the table and every ``splits`` of A.hd_splits (N = 224: an odd first tile of
    a range, and more splits than ranges that hold a tile); h contiguous and as a view of a 320-wide buffer.  Rows form: the maps
    alternate inside a slab, the last row's map holds 1e30 -- the map and the column a dead row and a dead column are clamped to --
    and with every row naming one map the result is the shared-map kernel's bit for bit.  That last row is ONE element of a kind
    per launch (thousands of times the others' magnitude, no cancellation): it is held to its bound where it stands and the two q
    are compared over the last rows of all n and splits of this N."""
    from bridges_hip import ops
    big = []
    for n, _ in [s for s in A.HD_SHAPES if s[1] == N]:
        pr = A.hd_probe(n, N, DEV)
        h, Wd, bd, w, maps, w_row = (pr[k] for k in ("h", "Wd", "bd", "w", "maps", "w_row"))
        wr = maps[w_row.long()]
        ref, lb = A.hd_ref(h, Wd, bd, w), A.hd_lib(h, Wd, bd, w)
        ref_rows, lb_rows = A.hd_ref(h, Wd, bd, wr), A.hd_lib(h, Wd, bd, wr)
        padded = A.hd_probe(n, N, DEV, strided=True)["h"]
        assert padded.stride(0) == 320 and torch.equal(padded, h)
        for splits in A.hd_splits(N):
            shape = (n, N, splits)
            poison(n)
            got = ops.head_sigmoid_dot(h, Wd, bd, w, splits=splits)
            A.conform("head", got, lb, *ref, shape, tight=n > A.FEW_ROWS)
            poison(n)
            got_rows = ops.head_sigmoid_dot(h, Wd, bd, maps, splits=splits, w_row=w_row)
            if n > 1:
                A.conform("head.rows", got_rows[:-1], lb_rows[:-1], ref_rows[0][:-1], ref_rows[1][:-1], shape, tight=n - 1 > A.FEW_ROWS)
            big.append((got_rows[-1:], lb_rows[-1:], ref_rows[0][-1:], ref_rows[1][-1:]))
            A.conform("head.rows.big_map", *big[-1], shape, tight=False)
            assert torch.equal(ops.head_sigmoid_dot(padded, Wd, bd, w, splits=splits), got), shape
            assert torch.equal(ops.head_sigmoid_dot(padded, Wd, bd, maps, splits=splits, w_row=w_row), got_rows), shape
            one_map = torch.full((n,), 3, dtype=torch.int32, device=DEV)
            assert torch.equal(ops.head_sigmoid_dot(h, Wd, bd, maps, splits=splits, w_row=one_map), got), shape
    A.conform_pooled("head.rows.big_map", big, N)


def test_head_sigmoid_dot_few_rows_pooled():
    """The one-row shapes of the table, judged over all of them (see test_sigmoid_dot_few_rows_pooled)."""
    from bridges_hip import ops
    pool, pool_rows = [], []
    for n, N in [s for s in A.HD_SHAPES if s[0] <= A.FEW_ROWS]:
        pr = A.hd_probe(n, N, DEV)
        h, Wd, bd, w, maps, w_row = (pr[k] for k in ("h", "Wd", "bd", "w", "maps", "w_row"))
        wr = maps[w_row.long()]
        for splits in A.hd_splits(N):
            pool.append((ops.head_sigmoid_dot(h, Wd, bd, w, splits=splits), A.hd_lib(h, Wd, bd, w), *A.hd_ref(h, Wd, bd, w)))
            pool_rows.append((ops.head_sigmoid_dot(h, Wd, bd, maps, splits=splits, w_row=w_row), A.hd_lib(h, Wd, bd, wr), *A.hd_ref(h, Wd, bd, wr)))
    A.conform_pooled("head.few_rows", pool, len(pool))
    A.conform_pooled("head.rows.few_rows", pool_rows, len(pool_rows))


def head_refusal_probe():
    n, N = 33, 100
    pr = A.hd_probe(n, N, DEV, strided=True)
    return n, N, pr, torch.full((n,), SENTINEL, device=DEV), torch.full((4, n), SENTINEL, device=DEV)


def test_head_sigmoid_dot_refusals():
    L = lib()
    n, N, pr, out, part = head_refusal_probe()
    h, Wd, bd, w, s = ptr(pr["h"]), ptr(pr["Wd"]), ptr(pr["bd"]), ptr(pr["w"]), stream()
    o, p = ptr(out), ptr(part)
    for rc in (L.bridges_head_sigmoid_dot(n, 128, N, h, 320, Wd, bd, w, o, p, 1, s),             # K != 256
               L.bridges_head_sigmoid_dot(n, 256, N, h, 252, Wd, bd, w, o, p, 1, s),             # h_stride < 256
               L.bridges_head_sigmoid_dot(n, 256, N, h, 318, Wd, bd, w, o, p, 1, s),             # h_stride % 4
               L.bridges_head_sigmoid_dot(n, 256, N, ptr(pr["h"], 4), 320, Wd, bd, w, o, p, 1, s),   # one float off 16-byte alignment
               L.bridges_head_sigmoid_dot(n, 256, N - 1, h, 320, ptr(pr["Wd"], 4), bd, w, o, p, 1, s),
               L.bridges_head_sigmoid_dot(n, 256, N, None, 320, Wd, bd, w, o, p, 1, s),          # null operands
               L.bridges_head_sigmoid_dot(n, 256, N, h, 320, None, bd, w, o, p, 1, s),
               L.bridges_head_sigmoid_dot(n, 256, N, h, 320, Wd, None, w, o, p, 1, s),
               L.bridges_head_sigmoid_dot(n, 256, N, h, 320, Wd, bd, None, o, p, 1, s),
               L.bridges_head_sigmoid_dot(n, 256, N, h, 320, Wd, bd, w, None, p, 1, s),
               L.bridges_head_sigmoid_dot(n, 256, N, h, 320, Wd, bd, w, o, None, 2, s),          # splits > 1 without part
               L.bridges_head_sigmoid_dot(n, 256, N, h, 320, Wd, bd, w, o, p, 0, s),
               L.bridges_head_sigmoid_dot(n, 256, 0, h, 320, Wd, bd, w, o, p, 1, s),
               L.bridges_head_sigmoid_dot(-1, 256, N, h, 320, Wd, bd, w, o, p, 1, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((part == SENTINEL).all())


def test_head_sigmoid_dot_rows_refusals():
    L = lib()
    n, N, pr, out, part = head_refusal_probe()
    h, Wd, bd, maps, w_row, s = ptr(pr["h"]), ptr(pr["Wd"]), ptr(pr["bd"]), ptr(pr["maps"]), ptr(pr["w_row"]), stream()
    o, p, M = ptr(out), ptr(part), A.HD_MAPS
    for rc in (L.bridges_head_sigmoid_dot_rows(n, 128, N, h, 320, Wd, bd, maps, w_row, M, o, p, 1, s),                   # K != 256
               L.bridges_head_sigmoid_dot_rows(n, 256, N, h, 252, Wd, bd, maps, w_row, M, o, p, 1, s),                   # h_stride < 256
               L.bridges_head_sigmoid_dot_rows(n, 256, N, ptr(pr["h"], 4), 320, Wd, bd, maps, w_row, M, o, p, 1, s),     # misaligned
               L.bridges_head_sigmoid_dot_rows(n, 256, N - 1, h, 320, ptr(pr["Wd"], 4), bd, maps, w_row, M, o, p, 1, s),
               L.bridges_head_sigmoid_dot_rows(n, 256, N, None, 320, Wd, bd, maps, w_row, M, o, p, 1, s),                # null operands
               L.bridges_head_sigmoid_dot_rows(n, 256, N, h, 320, Wd, bd, None, w_row, M, o, p, 1, s),
               L.bridges_head_sigmoid_dot_rows(n, 256, N, h, 320, Wd, bd, maps, None, M, o, p, 1, s),
               L.bridges_head_sigmoid_dot_rows(n, 256, N, h, 320, Wd, bd, maps, w_row, M, None, p, 1, s),
               L.bridges_head_sigmoid_dot_rows(n, 256, N, h, 320, Wd, bd, maps, w_row, 0, o, p, 1, s),                   # no map
               L.bridges_head_sigmoid_dot_rows(n, 256, N, h, 320, Wd, bd, maps, w_row, M, o, None, 4, s)):               # splits > 1 without part
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((part == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# bits_dot

@pytest.mark.parametrize("n", A.BD_N)
def test_bits_dot_is_an_f64_sum_rounded_once(n):
    """Non-integer images: inside u |ref| + 4096 * 2**-53 * sum |terms| of the float64 sum; the empty raster gives exactly 0.0;
    the full raster, slots with repeats, ``bits_row`` given and absent."""
    from bridges_hip import ops
    pr = A.bd_probe(n, DEV)
    ref, bound = A.bd_ref(pr)
    poison(n)
    got = ops.bits_dot(pr["bits"], pr["img"], pr["slot"], bits_row=pr["rows"])
    A.conform("bits_dot", got, A.bd_lib(pr), ref, bound, n)
    empty = pr["rows"] == A.RASTER_NAMES.index("empty")
    assert bool((got[empty].view(torch.int32) == 0).all()) and int(empty.sum()) == (0 if n == 1 else A.ceil_div(n, A.N_RASTERS))
    assert bool((pr["rows"] == A.RASTER_NAMES.index("full")).any())
    poison(n)
    assert torch.equal(ops.bits_dot(pr["bits"][pr["rows"]].contiguous(), pr["img"], pr["slot"]), got)


def test_bits_dot_counts_up_to_two_to_the_24_are_exact():
    from bridges_hip import ops
    pr, want = A.bd_count_probe(DEV)
    got = ops.bits_dot(pr["bits"], pr["img"], pr["slot"], bits_row=pr["rows"])
    assert torch.equal(got.cpu().double(), want.double()) and float(got.max()) == 2.0 ** 24


def test_bits_dot_refusals():
    L = lib()
    pr = A.bd_probe(5, DEV)
    out = torch.full((5,), SENTINEL, device=DEV)
    b, r, img, sl, o, s = ptr(pr["bits"]), ptr(pr["rows"]), ptr(pr["img"]), ptr(pr["slot"]), ptr(out), stream()
    for rc in (L.bridges_bits_dot(-1, b, r, img, sl, o, s), L.bridges_bits_dot(5, None, r, img, sl, o, s),
               L.bridges_bits_dot(5, b, r, None, sl, o, s), L.bridges_bits_dot(5, b, r, img, None, o, s),
               L.bridges_bits_dot(5, b, r, img, sl, None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# bits_accumulate_

def test_bits_accumulate_under_contention_counts_exactly():
    """(a) 500 rows of the full raster onto one slot, weights in {1, 2}: every pixel holds the exact integer total, the slots
    beside it nothing."""
    from bridges_hip import ops
    bits, _ = A.raster_probe(DEV)
    rows, slot, weight, total = A.acc_contention_probe(DEV)
    img = torch.zeros((3, 64, 64), device=DEV)
    ops.bits_accumulate_(img, bits, slot, weight=weight, bits_row=rows)
    assert bool((img[1] == total).all()) and bool((img[[0, 2]].view(torch.int32) == 0).all())
    img.zero_()                                                         # no weights: one per row
    ops.bits_accumulate_(img, bits[rows].contiguous(), slot)
    assert bool((img[1] == float(rows.numel())).all()) and bool((img[[0, 2]].view(torch.int32) == 0).all())


def test_bits_accumulate_is_one_float32_add_and_touches_nothing_else():
    """(b) disjoint (slot, pixel) sets, arbitrary weights: every touched pixel is the single float32 add.  (c) the pixels and slots
    no row touches keep their bits: -0.0, NaN payloads, a subnormal, inf.  (d) rows of weight 0 change nothing."""
    from bridges_hip import ops
    bits, sel = A.raster_probe(DEV)
    rows, slot, weight = A.acc_disjoint_probe(DEV)
    touched = torch.zeros((6, A.PX), dtype=torch.bool, device=DEV)
    for r in range(rows.numel()):
        touched[int(slot[r])] |= sel[int(rows[r])]
    touched = touched.reshape(6, 64, 64)
    assert not bool(touched[3:].any()) and bool(touched[2].all())       # slot 3 gets the empty raster, slots 4 and 5 no row
    start = A.acc_pattern_image(6, DEV)
    g = torch.Generator().manual_seed(17)
    start[touched] = torch.randn(int(touched.sum()), generator=g).to(DEV)
    img = start.clone()
    ops.bits_accumulate_(img, bits, slot, weight=weight, bits_row=rows)
    want = A.acc_single_add(start.cpu(), sel.cpu(), rows.cpu(), slot.cpu(), weight.cpu())
    assert A.same_bits(img.cpu(), want)
    assert torch.equal(img.view(torch.int32)[~touched], start.view(torch.int32)[~touched])            # (c), stated on its own
    assert not torch.equal(img[touched], start[touched])
    # (d) weight 0: the patterned image -- NaN payloads and -0.0 under the rasters too -- keeps every bit
    img = A.acc_pattern_image(6, DEV)
    before = img.clone()
    n = 40
    ops.bits_accumulate_(img, bits, torch.arange(n, device=DEV) % 6, weight=torch.zeros(n, device=DEV), bits_row=torch.arange(n, device=DEV) % 16)
    assert torch.equal(img.view(torch.int32), before.view(torch.int32))


def test_bits_accumulate_refusals():
    L = lib()
    bits, _ = A.raster_probe(DEV)
    rows, slot, weight = A.acc_disjoint_probe(DEV)
    img = torch.full((4, 64, 64), SENTINEL, device=DEV)
    n = rows.numel()
    b, r, w, sl, s = ptr(bits), ptr(rows), ptr(weight), ptr(slot), stream()
    for rc in (L.bridges_bits_accumulate(-1, b, r, w, sl, ptr(img), s), L.bridges_bits_accumulate(n, None, r, w, sl, ptr(img), s),
               L.bridges_bits_accumulate(n, b, r, w, None, ptr(img), s), L.bridges_bits_accumulate(n, b, r, w, sl, None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((img == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the raster helpers

@pytest.mark.parametrize("n", A.BITS_TO_F32_N)
def test_bits_to_f32_is_the_shift_and_mask_expansion(n):
    from bridges_hip import ops
    bits, sel = A.raster_probe(DEV)
    for start in range(0, A.N_RASTERS, n):
        chunk = bits[start:start + n].contiguous()
        poison(chunk.shape[0], 64, 64)
        got = ops.bits_to_f32(chunk)
        assert A.same_bits(got.cpu(), A.raster_expand(chunk)), (n, start)
        assert torch.equal(got.reshape(-1, A.PX) != 0, sel[start:start + n])


def test_bits_or_over_several_groups():
    """bridges_bits_or with seven ranges in one launch: empty ranges (all-zero words), one raster, all sixteen, two that overlap."""
    L = lib()
    bits, _ = A.raster_probe(DEV)
    ranges = torch.tensor(A.BITS_OR_RANGES, dtype=torch.int32, device=DEV)
    G = len(A.BITS_OR_RANGES)
    out = torch.full((G + 1, 64), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    assert L.bridges_bits_or(G, ptr(ranges), ptr(bits), ptr(out), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:G].cpu(), A.bits_or_ref(bits, A.BITS_OR_RANGES)) and bool((out[G] == 0x5a5a5a5a).all())
    assert not bool(out[0].any()) and not bool(out[5].any())


def test_bits_or_refusals():
    L = lib()
    bits, _ = A.raster_probe(DEV)
    ranges = torch.tensor(A.BITS_OR_RANGES, dtype=torch.int32, device=DEV)
    out = torch.full((len(A.BITS_OR_RANGES), 64), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    s = stream()
    for rc in (L.bridges_bits_or(-1, ptr(ranges), ptr(bits), ptr(out), s), L.bridges_bits_or(3, None, ptr(bits), ptr(out), s),
               L.bridges_bits_or(3, ptr(ranges), None, ptr(out), s), L.bridges_bits_or(3, ptr(ranges), ptr(bits), None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a5a5a).all())


def test_bits_to_f32_refusals():
    L = lib()
    bits, _ = A.raster_probe(DEV)
    img = torch.full((16, 64, 64), SENTINEL, device=DEV)
    s = stream()
    for rc in (L.bridges_bits_to_f32(-1, ptr(bits), ptr(img), s), L.bridges_bits_to_f32(16, None, ptr(img), s),
               L.bridges_bits_to_f32(16, ptr(bits), None, s)):
        assert rc == E_ARG
    torch.cuda.synchronize()
    assert bool((img == SENTINEL).all())
