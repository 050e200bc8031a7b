"""GPU: k_conv_input / bridges_conv_input_rows / ops.conv_input against the torch formulation (ops.bits_to_f32, index_select,
stack), bit for bit on .view(torch.int32): row counts around one workgroup, index patterns, both strides, rasters that pin the bit
order, map values that arithmetic would change, out= inside a larger buffer, the argument checks, another stream."""
import ctypes as C
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = (1, 2, 5, 64, 257)
SOURCES = (3, 300)


def word(bits):
    """The int64 whose bit pattern has the given bits set."""
    v = 0
    for b in bits:
        v |= 1 << b
    return v - (1 << 64) if v >= 1 << 63 else v


def rasters(n, seed):
    """[n, 64] int64: the fixed rasters that pin the bit order first, random ones behind them."""
    fixed = torch.zeros((9, 64), dtype=torch.int64)
    fixed[1] = -1                                                          # all ones
    fixed[2, 0] = word([0])                                                # pixel (0, 0)
    fixed[3, 0] = word([63])                                               # pixel (0, 63)
    fixed[4, 63] = word([0])                                               # pixel (63, 0)
    fixed[5, 63] = word([63])                                              # pixel (63, 63)
    fixed[6, 17] = word([40])                                              # pixel (17, 40)
    fixed[7, 0::2], fixed[7, 1::2] = word(range(0, 64, 2)), word(range(1, 64, 2))      # alternating words
    fixed[8, 0::2] = -1                                                    # alternating rows
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(-2 ** 63, 2 ** 63 - 1, (max(n, 9), 64), generator=g, dtype=torch.int64)
    rnd[:9] = fixed
    order = torch.randperm(max(n, 9), generator=g)[:n] if n >= 9 else torch.tensor([6, 7, 3, 1, 0, 2, 4, 5, 8][:n])
    return rnd[order].contiguous().to(DEV)


def test_bit_order_and_exact_values():
    """Pixel (row, col) is bit col of word row, in every raster channel; the values are exactly 0.0f and 1.0f."""
    from bridges_hip import ops
    src = torch.zeros((9, 64), dtype=torch.int64)
    src[1] = -1
    src[2, 0], src[3, 0], src[4, 63], src[5, 63], src[6, 17] = word([0]), word([63]), word([0]), word([63]), word([40])
    src[7, 0::2], src[7, 1::2] = word(range(0, 64, 2)), word(range(1, 64, 2))
    src[8, 0::2] = -1
    src = src.to(DEV)
    rw = maps(9, 4)
    shift = lambda k: torch.roll(torch.arange(9, device=DEV), k)
    x = ops.conv_input(src, src, rw, src, block_row=shift(0), action_row=shift(1), obstacle_row=shift(2))
    assert same_bits(x, reference(src, src, rw, src, [shift(0), shift(1), None, shift(2)], 9))
    for ch, k in ((0, 0), (1, 1), (3, 2)):
        img = x[:, ch].index_select(0, torch.argsort(shift(k))).cpu()      # img[s] = the image of source raster s
        assert set(img.unique().tolist()) == {0.0, 1.0}
        assert float(img[0].sum()) == 0 and float(img[1].sum()) == 4096
        for s_, (r, c) in ((2, (0, 0)), (3, (0, 63)), (4, (63, 0)), (5, (63, 63)), (6, (17, 40))):
            assert float(img[s_].sum()) == 1 and float(img[s_, r, c]) == 1, (ch, s_)
        rr, cc = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
        assert torch.equal(img[7], ((rr + cc) % 2 == 0).float()) and torch.equal(img[8], (rr % 2 == 0).float().expand(64, 64))


def f32_bits(pattern):
    return struct.unpack("<f", struct.pack("<I", pattern))[0]


SPECIALS = (0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0x00000000)
#           quiet NaN + payload, signalling NaN (negative), +inf, -inf, -0.0, smallest denormal, negative denormal, float32 max, 0


def maps(n, seed):
    """[n, 64, 64] float32 whose first words (and a few in the middle and at the end) hold the special patterns, as raw bits."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn((n, 4096), generator=g, dtype=torch.float32)
    raw = m.view(torch.int32)
    pat = torch.tensor([p - (1 << 32) if p >= 1 << 31 else p for p in SPECIALS], dtype=torch.int32)
    for at in (0, 2045, 4096 - len(SPECIALS)):
        raw[:, at:at + len(SPECIALS)] = pat
    return m.reshape(n, 64, 64).to(DEV)


def index(kind, n, n_src, seed):
    if kind == "identity":
        return None
    if kind == "last":
        return torch.full((n,), n_src - 1, dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_src, (n,), generator=g, dtype=torch.int64).to(DEV)          # a choice with repeats


def reference(block_bits, action_bits, reward, obstacle_bits, rows, n):
    from bridges_hip import ops

    def pick(images, row):
        if row is not None:
            return images.index_select(0, row)
        return images.expand(n, -1, -1) if images.shape[0] == 1 else images[:n]
    chans = [pick(ops.bits_to_f32(block_bits), rows[0]), pick(ops.bits_to_f32(action_bits), rows[1]),
             pick(reward.reshape(-1, 64, 64), rows[2]), pick(ops.bits_to_f32(obstacle_bits), rows[3])]
    return torch.stack([c.view(torch.int32) for c in chans], dim=1)


def same_bits(x, want):
    return tuple(x.shape) == tuple(want.shape) and x.dtype == torch.float32 and x.is_contiguous() and torch.equal(x.view(torch.int32), want)


def test_maps_hold_the_special_values():
    m = maps(2, 0).cpu()
    flat = m.reshape(2, -1)
    assert torch.isnan(flat[0, 0]) and torch.isnan(flat[0, 1]) and flat[0, 2] == float("inf") and flat[0, 3] == -float("inf")
    assert flat[0, 4] == 0 and torch.signbit(flat[0, 4]) and 0 < float(flat[0, 5]) < 2 ** -126 and float(flat[0, 7]) == f32_bits(0x7F7FFFFF)
    assert [int(v) & 0xFFFFFFFF for v in flat.view(torch.int32)[1, :len(SPECIALS)]] == list(SPECIALS)


@pytest.mark.parametrize("n_src", SOURCES)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("kind", ["identity", "repeats", "last"])
def test_rows_equal_the_torch_formulation(n, n_src, kind):
    """Full strides for the map and the obstacle, every row index of one kind (identity needs n sources: n_src is raised to n; at
    n = 1 the wrapper passes the one map and raster with stride 0, which names the same row)."""
    from bridges_hip import ops
    m = max(n_src, n) if kind == "identity" else n_src
    bb, ab, ob, rw = rasters(m, 1), rasters(m, 2), rasters(m, 3), maps(m, 4)
    rows = [index(kind, n, m, 10 + c) for c in range(4)]
    if kind == "identity":
        bb, ab, ob, rw = bb[:n].contiguous(), ab[:n].contiguous(), ob[:n].contiguous(), rw[:n].contiguous()
    x = ops.conv_input(bb, ab, rw, ob, *rows)
    assert same_bits(x, reference(bb, ab, rw, ob, rows, n))


@pytest.mark.parametrize("n_src", SOURCES)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("shared_map,shared_obstacle", [(True, True), (True, False), (False, True)])
def test_strides(n, n_src, shared_map, shared_obstacle):
    """Stride 0 (one map / raster for every row) and the full stride, for the map and the obstacle independently; the block
    index is the identity where the sources allow it, the action index a choice with repeats."""
    from bridges_hip import ops
    bb, ab = rasters(max(n_src, n), 5), rasters(n_src, 6)
    rw = maps(1 if shared_map else n_src, 7)
    ob = rasters(n_src, 8)[n_src - 1:] if shared_obstacle else rasters(n_src, 8)
    rows = [None, index("repeats", n, n_src, 20), None if shared_map else index("last", n, n_src, 0),
            None if shared_obstacle else index("repeats", n, n_src, 21)]
    x = ops.conv_input(bb, ab, rw, ob, *rows)
    assert same_bits(x, reference(bb, ab, rw, ob, rows, n))


def test_mixed_identity_and_index():
    """An identity index beside given ones: n comes from the index that is given."""
    from bridges_hip import ops
    n = 5
    bb, ab, ob, rw = rasters(300, 1), rasters(3, 2), rasters(5, 3), maps(5, 4)
    rows = [index("repeats", n, 300, 1), index("last", n, 3, 0), None, None]
    assert same_bits(ops.conv_input(bb, ab, rw, ob, *rows), reference(bb, ab, rw, ob, rows, n))
    with pytest.raises(AssertionError):
        ops.conv_input(bb, ab, rw, ob, block_row=rows[0], action_row=rows[1][:3])         # indices of two lengths
    with pytest.raises(AssertionError):
        ops.conv_input(bb, ab, rw[:4], ob, block_row=rows[0])                             # 4 maps for 5 rows
    with pytest.raises(AssertionError):
        ops.conv_input(bb, ab.to(torch.int32), rw, ob, block_row=rows[0])


def test_out_is_written_in_place_and_nothing_else():
    from bridges_hip import ops
    n, lo = 5, 3
    bb, ab, ob, rw = rasters(5, 1), rasters(5, 2), rasters(1, 3), maps(5, 4)
    sentinel = -12345.5
    buf = torch.full((lo + n + 4, 4, 64, 64), sentinel, dtype=torch.float32, device=DEV)
    x = ops.conv_input(bb, ab, rw, ob, out=buf[lo:lo + n])
    assert x.data_ptr() == buf[lo].data_ptr() and same_bits(x, reference(bb, ab, rw, ob, [None] * 4, n))
    assert bool((buf[:lo] == sentinel).all()) and bool((buf[lo + n:] == sentinel).all())
    with pytest.raises(AssertionError):
        ops.conv_input(bb, ab, rw, ob, out=buf[:n + 1])
    # n == 0: success, out untouched
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    y = ops.conv_input(bb, ab, rw, ob, block_row=empty, action_row=empty, reward_row=empty, out=buf[:0])
    assert tuple(y.shape) == (0, 4, 64, 64) and bool((buf[:lo] == sentinel).all())


def raw_call(n, bb, br, ab, ar, rw, rr, rs, ob, orow, os_, x):
    from bridges_hip import abi, ops
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    return abi.lib().bridges_conv_input_rows(n, p(bb), p(br), p(ab), p(ar), p(rw), p(rr), rs, p(ob), p(orow), os_, p(x), ops._stream())


def test_argument_checks_are_made_on_the_host():
    """A refused call launches nothing: the output keeps its sentinel.  (Every refused argument list below would be harmless to
    launch as well -- the pointers are valid where they are not the argument under test.)"""
    from bridges_hip import abi
    abi.require_gpu()
    n = 4
    bb, ab, ob, rw = rasters(4, 1), rasters(4, 2), rasters(4, 3), maps(4, 4)
    x = torch.full((n, 4, 64, 64), 7.0, dtype=torch.float32, device=DEV)
    ok = lambda **kw: raw_call(**{**dict(n=n, bb=bb, br=None, ab=ab, ar=None, rw=rw, rr=None, rs=4096, ob=ob, orow=None, os_=64, x=x), **kw})
    for bad in (dict(rs=1), dict(rs=4095), dict(rs=128), dict(rs=64), dict(os_=1), dict(os_=128), dict(os_=4096), dict(rs=-4096),
                dict(bb=None), dict(ab=None), dict(rw=None), dict(ob=None), dict(x=None), dict(n=-1)):
        assert ok(**bad) == -1, bad
        assert b"bad argument" in abi.lib().bridges_last_error()
    assert ok(n=0) == 0
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())
    assert ok() == 0 and ok(rs=0, os_=0) == 0
    torch.cuda.synchronize()
    assert same_bits(x, reference(bb, ab, rw[:1], ob[:1], [None] * 4, n))


def test_on_another_stream():
    from bridges_hip import ops
    n = 64
    bb, ab, ob, rw = rasters(300, 1), rasters(300, 2), rasters(300, 3), maps(3, 4)
    rows = [index("repeats", n, 300, 1), index("repeats", n, 300, 2), index("repeats", n, 3, 3), index("last", n, 300, 0)]
    want = reference(bb, ab, rw, ob, rows, n)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = ops.conv_input(bb, ab, rw, ob, *rows)
    side.synchronize()
    assert same_bits(x, want)
