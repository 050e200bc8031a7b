"""GPU: conformance of the stand-alone geometry and raster operators -- k_place, k_create_block, k_pose_block, k_face_frames,
k_contains_points, k_raster_generic, k_render_blocks, k_action_features, k_bits_or -- through the C ABI (``abi.lib()``, a ShapeTable
of the five shapes).

Probe tables, references, the ``lin`` bound and the twins come from tests/geometry_conformance.py (checked without a GPU by
tests/test_cpu_geometry_conformance_refs.py, which also shows that a kernel wrong in one of eighteen ways would be rejected).  Poses,
vertices, frames, rasters and masks are compared bit for bit with oracle/geometry.py, oracle/shapes.py and oracle/raster.py; every
output buffer is longer than the call needs and filled with a sentinel first, which must survive past the call's last item; refusals
return BRIDGES_E_ARG, name their function in bridges_last_error() and leave the sentinel alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_conformance as Q

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E_ARG = -1                                          # BRIDGES_E_ARG
SENTINEL = -77.25
SENTINEL_U8 = 0xA5
SENTINEL_I64 = 0x5A5A5A5A5A5A5A5A
PAD = 3                                             # items of sentinel behind every output


def lib():
    from bridges_hip import abi
    return abi.require_gpu()


def stream():
    from bridges_hip import abi
    return abi.current_stream()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def dev(a):
    """numpy -> device tensor.  The caller keeps the tensor in a name until its kernel is launched: a temporary would go back to the
    caching allocator at once and the next upload could land in the block the kernel is about to read."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def out_f64(n, *shape):
    return torch.full((n + PAD,) + shape, SENTINEL, dtype=torch.float64, device=DEV)


def out_f32(n, *shape):
    return torch.full((n + PAD,) + shape, SENTINEL, dtype=torch.float32, device=DEV)


def out_u8(n, *shape):
    return torch.full((n + PAD,) + shape, SENTINEL_U8, dtype=torch.uint8, device=DEV)


def out_words(n):
    return torch.full((n + PAD, 64), SENTINEL_I64, dtype=torch.int64, device=DEV)


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def split(t, n):
    """(the call's n items, True if the sentinel behind them is intact) of an output tensor, on the host."""
    a = host(t)
    fill = {np.dtype(np.float64): SENTINEL, np.dtype(np.float32): SENTINEL, np.dtype(np.uint8): SENTINEL_U8,
            np.dtype(np.uint64): SENTINEL_I64}[a.dtype]
    return a[:n], bool((a[n:] == fill).all())


def ok(rc, what):
    assert rc == 0, (what, rc, lib().bridges_last_error().decode())


@pytest.fixture(scope="module")
def table():
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import ShapeTable
    return ShapeTable([load_urdf(f"shapes/{name}.urdf") for name in Q.SHAPE_NAMES])


# ---------------------------------------------------------------------------------------------------------------------------
# K1

BATCH_N = (1, 255, 256, 257, 1000)
CHUNK = 8192


def run_place(table, rows):
    P, n = Q.place_probe(), len(rows)
    pose, verts = out_f64(n, 4), out_f64(n, 6, 2)
    a = [dev(P[k][rows]) for k in ("frame1", "shape", "face", "ox", "oy")]
    ok(lib().bridges_place(table.ptr, n, *[ptr(t) for t in a], ptr(pose), ptr(verts), stream()), "bridges_place")
    return split(pose, n), split(verts, n)


def run_create_block(table, rows, want_frame=True):
    P, ref, n = Q.placement_probe(), Q.placement_reference(), len(rows)
    pose, verts, frame = out_f64(n, 4), out_f64(n, 6, 2), out_f64(n, 6)
    a = [dev(ref["target_verts"][rows])] + [dev(P[k][rows]) for k in ("target_shape", "target_face", "shape", "face", "ox", "oy")]
    ok(lib().bridges_create_block(table.ptr, n, *[ptr(t) for t in a], ptr(pose), ptr(verts), ptr(frame if want_frame else None),
                                  stream()), "bridges_create_block")
    return split(pose, n), split(verts, n), split(frame, n if want_frame else 0)


def run_pose_and_frames(table, sid, pose_in):
    n = len(sid)
    verts, frames = out_f64(n, 6, 2), out_f64(n, 6, 6)
    s, p = dev(sid), dev(pose_in)
    ok(lib().bridges_pose_block(table.ptr, n, ptr(s), ptr(p), ptr(verts), stream()), "bridges_pose_block")
    ok(lib().bridges_face_frames(table.ptr, n, ptr(s), ptr(verts[:n]), ptr(frames), stream()), "bridges_face_frames")
    return split(verts, n), split(frames, n)


@pytest.mark.parametrize("n", BATCH_N)
def test_place_batches(table, n):
    """Pose and vertices bit-equal to oracle.geometry.align + Block, slots >= nv exactly 0.0 (the reference holds +0.0 there and the
    comparison is bitwise), the sentinel intact past n; the batch's first, last and 256th item equal the item launched alone."""
    ref = Q.place_reference()
    total = len(ref["cy"])
    rows = Q.batch_rows(total, n, salt=total - 7 * n)            # the walk crosses the raw frames at the table's end
    (pose, p_ok), (verts, v_ok) = run_place(table, rows)
    assert p_ok and v_ok
    assert Q.same_bits(pose, ref["pose"][rows]) and Q.same_bits(verts, ref["verts"][rows])
    for i in sorted({0, n - 1, min(n - 1, 256)}):
        (p1, _), (v1, _) = run_place(table, rows[i:i + 1])
        assert Q.same_bits(p1, pose[i:i + 1]) and Q.same_bits(v1, verts[i:i + 1]), i


def test_place_whole_table(table):
    """Every row: both clamps, the sign band and both signs of cy (tests/test_cpu_geometry_conformance_refs.py counts them)."""
    ref = Q.place_reference()
    total = len(ref["cy"])
    for lo in range(0, total, CHUNK):
        rows = np.arange(lo, min(lo + CHUNK, total))
        (pose, p_ok), (verts, v_ok) = run_place(table, rows)
        assert p_ok and v_ok
        bad = np.nonzero((pose.view(np.uint64) != ref["pose"][rows].view(np.uint64)).any(1))[0]
        assert bad.size == 0, ("first differing probe row", lo + int(bad[0]), pose[bad[0]], ref["pose"][rows][bad[0]])
        assert Q.same_bits(verts, ref["verts"][rows])


@pytest.mark.parametrize("n", BATCH_N)
def test_create_block_batches(table, n):
    """Bit-equal to oracle.geometry.create_block; target_frame_out equal to the oracle's target frame (the floor's included), and
    NULL accepted without a change to pose or vertices; sentinel intact past n; items equal the item launched alone."""
    ref = Q.placement_reference()
    total = len(ref["pose"])
    rows = Q.batch_rows(total, n, salt=total - 5 * n)            # the walk crosses the floor rows at the table's end
    (pose, p_ok), (verts, v_ok), (frame, f_ok) = run_create_block(table, rows)
    assert p_ok and v_ok and f_ok
    assert Q.same_bits(pose, ref["pose"][rows]) and Q.same_bits(verts, ref["verts"][rows])
    assert Q.same_bits(frame, ref["frame1"][rows])
    (pose0, p_ok), (verts0, v_ok), (_, untouched) = run_create_block(table, rows, want_frame=False)
    assert p_ok and v_ok and untouched
    assert Q.same_bits(pose0, pose) and Q.same_bits(verts0, verts)
    for i in sorted({0, n - 1, min(n - 1, 256)}):
        (p1, _), (v1, _), (f1, _) = run_create_block(table, rows[i:i + 1])
        assert Q.same_bits(p1, pose[i:i + 1]) and Q.same_bits(v1, verts[i:i + 1]) and Q.same_bits(f1, frame[i:i + 1]), i


def test_create_block_whole_table(table):
    ref = Q.placement_reference()
    total = len(ref["pose"])
    for lo in range(0, total, CHUNK):
        rows = np.arange(lo, min(lo + CHUNK, total))
        (pose, p_ok), (verts, v_ok), (frame, f_ok) = run_create_block(table, rows)
        assert p_ok and v_ok and f_ok
        bad = np.nonzero((pose.view(np.uint64) != ref["pose"][rows].view(np.uint64)).any(1))[0]
        assert bad.size == 0, ("first differing probe row", lo + int(bad[0]), pose[bad[0]], ref["pose"][rows][bad[0]])
        assert Q.same_bits(verts, ref["verts"][rows]) and Q.same_bits(frame, ref["frame1"][rows])


@pytest.mark.parametrize("n", BATCH_N)
def test_pose_block_then_face_frames_is_block_frames(table, n):
    """The poses of the placement table (cos / sin as align leaves them, not renormalised) -> Block.verts, Block.frames; vertex and
    frame slots >= nv exactly 0.0; sentinel intact past n; items equal the item launched alone."""
    P, ref = Q.place_probe(), Q.place_reference()
    total = len(ref["cy"])
    rows = Q.batch_rows(total, n, salt=3 * n)
    (verts, v_ok), (frames, f_ok) = run_pose_and_frames(table, P["shape"][rows], ref["pose"][rows])
    assert v_ok and f_ok
    assert Q.same_bits(verts, ref["verts"][rows]) and Q.same_bits(frames, ref["frames"][rows])
    pad = np.arange(6)[None, :] >= Q.NV[P["shape"][rows]][:, None]
    assert pad.any() or n == 1
    assert (verts.view(np.uint64)[pad] == 0).all() and (frames.view(np.uint64)[pad] == 0).all()
    for i in sorted({0, n - 1, min(n - 1, 256)}):
        (v1, _), (f1, _) = run_pose_and_frames(table, P["shape"][rows[i:i + 1]], ref["pose"][rows[i:i + 1]])
        assert Q.same_bits(v1, verts[i:i + 1]) and Q.same_bits(f1, frames[i:i + 1]), i


# ---------------------------------------------------------------------------------------------------------------------------
# contains_points

def run_contains(table, verts_row, sid, pts):
    n = len(pts)
    inside, v, p = out_u8(n), dev(verts_row), dev(pts)
    ok(lib().bridges_contains_points(table.ptr, int(sid), ptr(v), n, ptr(p), ptr(inside), stream()), "bridges_contains_points")
    got, intact = split(inside, n)
    assert intact
    return got


@pytest.mark.parametrize("n", Q.POINT_N)
def test_contains_points(table, n):
    """Vertices, edge midpoints, the midpoints an ulp out and an ulp in, then grid points: uint8 equal to the oracle's pixel test."""
    for row, si, pts, _gx, _gz in Q.point_probe():
        got = run_contains(table, row, si, pts[:n])
        want = Q.contains_points_ref(row, si, pts[:n]).astype(np.uint8)
        assert Q.same_bits(got, want), (Q.SHAPE_NAMES[si], n, np.nonzero(got != want)[0][:5])


# ---------------------------------------------------------------------------------------------------------------------------
# raster_sized

def run_raster(table, g, S, want_bits=True, want_img=True, rows=None):
    verts, sid = (g["verts"], g["sid"]) if rows is None else (g["verts"][rows], g["sid"][rows])
    n = len(sid)
    bits = out_words(n) if want_bits else None
    img = out_f32(n, 64, 64) if want_img else None
    a = [dev(verts), dev(sid), dev(g["X"]), dev(g["Y"])]
    ok(lib().bridges_raster_sized(table.ptr, n, *[ptr(t) for t in a], S, ptr(bits), ptr(img), stream()), "bridges_raster_sized")
    out = []
    for t in (bits, img):
        if t is not None:
            got, intact = split(t, n)
            assert intact
            out.append(got)
        else:
            out.append(None)
    return out


@pytest.mark.parametrize("S", Q.RASTER_SIZES)
def test_raster_sized(table, S):
    """Bits only, img only and both: the words bit-equal to oracle.raster.contains_2d packed (so words and bits >= S are zero), img ==
    bits_to_f32(bits) on the whole 64 x 64 canvas -- on the wide grid (sample points on vertices, edge midpoints and centres; outlines
    over and outside every border) and on the tight grid (full images for prefix and for suffix runs)."""
    probe, ref = Q.raster_probe(S), Q.raster_reference(S)
    for name, g in probe.items():
        want = ref[name]
        bits, _ = run_raster(table, g, S, want_img=False)
        assert Q.accept_words(bits, want), (name, S, np.nonzero((bits != want).any(1))[0][:8])
        _, img = run_raster(table, g, S, want_bits=False)
        assert Q.same_bits(img, Q.bits_to_f32(want)), (name, S)
        bits2, img2 = run_raster(table, g, S)
        assert Q.accept_words(bits2, want) and Q.same_bits(img2, img), (name, S)


def test_raster_sized_grid_stride_round(table):
    """n = 8195 > 4 x 2048 waves: the second round of the capped grid.  The S = 64 probe outlines repeated cyclically, bits only."""
    g, want = Q.raster_probe(64)["wide"], Q.raster_reference(64)["wide"]
    rows = np.arange(8195) % len(g["sid"])
    bits, _ = run_raster(table, g, 64, want_img=False, rows=rows)
    bad = np.nonzero((bits != want[rows]).any(1))[0]
    assert bad.size == 0, ("first differing items", bad[:8])


# ---------------------------------------------------------------------------------------------------------------------------
# action_features

def run_features(table, g, rows=None, state=None, obstacle=None, prefix=None, want=("bits", "img", "mask", "lin"), S=64):
    verts, sid = (g["verts"], g["sid"]) if rows is None else (g["verts"][rows], g["sid"][rows])
    n = len(sid)
    outs = dict(bits=out_words(n) if "bits" in want else None, img=out_f32(n, 64, 64) if "img" in want else None,
                mask=out_u8(n) if "mask" in want else None, lin=out_f32(n) if "lin" in want else None)
    xlim, ylim = g.get("xlim", Q.XLIM), g.get("ylim", Q.YLIM)
    opt = [dev(a) if a is not None else None for a in (state, obstacle, prefix)]
    a = [dev(verts), dev(sid), dev(g["X"]), dev(g["Y"])]
    ok(lib().bridges_action_features(table.ptr, n, *[ptr(t) for t in a], S, xlim[0], xlim[1], ylim[0], ylim[1], *[ptr(t) for t in opt],
                                     ptr(outs["bits"]), ptr(outs["img"]), ptr(outs["mask"]), ptr(outs["lin"]), stream()),
       "bridges_action_features")
    res = {}
    for k, t in outs.items():
        if t is not None:
            res[k], intact = split(t, n)
            assert intact, k
    return res


def test_action_features_mask_and_rasters(table):
    """Every occupancy case on the wide group and the low group: mask bit-equal to the header's rule restated (vertices exactly on
    the 1e-6 bounds and an ulp beyond them; the z < -eps clause where ylim0 < 0), bits and img the oracle's rasters."""
    groups, words = Q.candidate_probe(), Q.candidate_words()
    cases = [("wide", name, s, o) for name, s, o in Q.occupancy_cases()] + [("low", "both_null", None, None)]
    for gname, name, state, obstacle in cases:
        g, w = groups[gname], words[gname]
        got = run_features(table, g, state=state, obstacle=obstacle, want=("bits", "img", "mask"))
        want = Q.mask_np(g, w, state, obstacle)
        assert Q.same_bits(got["mask"], want), (gname, name, np.nonzero(got["mask"] != want)[0])
        assert Q.accept_words(got["bits"], w) and Q.same_bits(got["img"], Q.bits_to_f32(w)), (gname, name)


@pytest.mark.parametrize("n", Q.CAND_N + (118,))
def test_action_features_lin_and_optional_outputs(table, n):
    """lin inside the derived bound around math.fsum of the float32 map under the raster (a map with 1e6 next to every run's end); lin
    and mask bit-equal whichever of bits / img is NULL; n of one wave, one workgroup, one more, and many."""
    g, words, m = Q.candidate_probe()["wide"], Q.candidate_words()["wide"], Q.reward_map()
    rows = (106 + np.arange(n)) % len(g["sid"])                 # from the last raster-probe outlines on into the bounds outlines
    name, state, obstacle = Q.occupancy_cases()[3]
    prefix = Q.reward_prefix(m)
    ref = Q.lin_reference(words, m)[rows]
    full = run_features(table, g, rows, state, obstacle, prefix)
    ratio = np.abs(full["lin"].astype(np.float64) - ref) / Q.lin_bound(ref, m)
    print(f"Q action_features lin n={n}: largest |lin - R| / bound = {ratio.max():.3g}")
    assert Q.accept_lin(full["lin"], ref, m), (n, ratio.max())
    assert Q.same_bits(full["mask"], Q.mask_np(g, words, state, obstacle)[rows])
    assert Q.accept_words(full["bits"], words[rows])
    for want in (("img", "mask", "lin"), ("bits", "mask", "lin"), ("mask", "lin"), ("lin",), ("mask",)):
        got = run_features(table, g, rows, state, obstacle, prefix, want=want)
        for k in want:
            assert Q.same_bits(got[k], full[k]), (n, want, k)
    got = run_features(table, g, rows, state, obstacle, None, want=("mask",))         # no prefix, no lin
    assert Q.same_bits(got["mask"], full["mask"])


def test_reward_prefix_wrapper_is_the_left_to_right_sum():
    from bridges_hip import ops
    m = Q.reward_map()
    assert Q.same_bits(ops.reward_prefix(torch.from_numpy(m)).cpu().numpy(), Q.reward_prefix(m))


# ---------------------------------------------------------------------------------------------------------------------------
# render_blocks, and the agreement of the four pixel paths

def run_render(table, verts, sid, X, Y, out=None):
    W, H = len(X), len(Y)
    n = len(sid)
    v = dev(verts if n else np.zeros((1, 6, 2)))
    s = dev(sid if n else np.zeros(1, dtype=np.int32))
    mine = out is None
    if mine:
        out = torch.full((H * W + 64,), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    gx, gy = dev(X), dev(Y)
    ok(lib().bridges_render_blocks(table.ptr, n, ptr(v), ptr(s), ptr(gx), W, ptr(gy), H, ptr(out), stream()), "bridges_render_blocks")
    if mine:
        a = out.cpu().numpy()
        assert (a[H * W:] == SENTINEL_U8).all()
        return a[:H * W].reshape(H, W)


def test_render_blocks_scene_probe(table):
    """0 .. 40 outlines (one, two and three LDS tiles; a full and a one-outline last tile) on five grids: equal to the OR of
    contains_2d per block.  Every outline is the only hit of some pixels, the last of the last tile included; in two scenes
    outlines 0..15 miss the image, so a pixel's first hit comes after a whole tile of misses."""
    for case in Q.scene_cases():
        verts, sid, X, Y = Q.scene_of(*case)
        got = run_render(table, verts, sid, X, Y)
        want = Q.render_reference(verts, sid, X, Y)
        assert Q.same_bits(got, want), (case, int((got != want).sum()))


@pytest.mark.parametrize("S", Q.RASTER_SIZES)
def test_four_pixel_paths_agree(table, S):
    """raster_sized, action_features, render_blocks of the single outline on the S x S grid and contains_points on the grid's points:
    the same pixels, which are the oracle's."""
    g, want = Q.raster_probe(S)["wide"], Q.raster_reference(S)["wide"]
    n = len(g["sid"])
    bits, _ = run_raster(table, g, S, want_img=False)
    feat = run_features(table, g, want=("bits",), S=S)["bits"]
    assert Q.accept_words(bits, want) and Q.accept_words(feat, want)
    pts = np.stack(np.meshgrid(g["X"], g["Y"]), axis=2).reshape(-1, 2)              # point r * S + q = (X[q], Y[r])
    L, s = lib(), stream()
    rendered = torch.full((n + PAD, S * S), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    inside = torch.full((n + PAD, S * S), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    v, sid, X, Y, p = dev(g["verts"]), dev(g["sid"]), dev(g["X"]), dev(g["Y"]), dev(pts)
    for i in range(n):
        ok(L.bridges_render_blocks(table.ptr, 1, ptr(v[i]), ptr(sid[i:]), ptr(X), S, ptr(Y), S, ptr(rendered[i]), s), "bridges_render_blocks")
        ok(L.bridges_contains_points(table.ptr, int(g["sid"][i]), ptr(v[i]), S * S, ptr(p), ptr(inside[i]), s), "bridges_contains_points")
    pixels = Q.unpack(want)[:, :S, :S].reshape(n, S * S).astype(np.uint8)
    for name, t in (("render_blocks", rendered), ("contains_points", inside)):
        got, intact = split(t, n)
        assert intact, name
        assert Q.same_bits(got, pixels), (name, S, np.nonzero((got != pixels).any(1))[0][:8])


# ---------------------------------------------------------------------------------------------------------------------------
# bits_or

def test_bits_or(table):
    bits, ranges = Q.bits_or_probe()
    want = Q.bits_or_reference(bits, ranges)
    L, s = lib(), stream()
    b, r = dev(bits), dev(ranges)
    out = out_words(len(ranges))
    ok(L.bridges_bits_or(len(ranges), ptr(r), ptr(b), ptr(out), s), "bridges_bits_or")
    got, intact = split(out, len(ranges))
    assert intact and Q.accept_words(got, want)
    out = out_words(1)
    ok(L.bridges_bits_or(0, ptr(r), ptr(b), ptr(out), s), "n_groups = 0")
    ok(L.bridges_bits_or(0, None, None, None, s), "n_groups = 0, no arrays")
    assert split(out, 0)[1]
    for rc in (L.bridges_bits_or(2, None, ptr(b), ptr(out), s), L.bridges_bits_or(2, ptr(r), None, ptr(out), s),
               L.bridges_bits_or(2, ptr(r), ptr(b), None, s), L.bridges_bits_or(-1, ptr(r), ptr(b), ptr(out), s)):
        assert rc == E_ARG and "bridges_bits_or" in L.bridges_last_error().decode()
    assert split(out, 0)[1]


# ---------------------------------------------------------------------------------------------------------------------------
# refusals

def refused(L, rc, names, not_names=()):
    msg = L.bridges_last_error().decode()
    assert rc == E_ARG, (names, rc)
    assert msg.startswith("bad argument") and all(n in msg for n in names) and not any(n in msg for n in not_names), msg


def each_null(args, nullable):
    """args with each position of ``nullable`` replaced by NULL in turn."""
    for k in nullable:
        yield k, [None if i == k else a for i, a in enumerate(args)]


def test_k1_refusals(table):
    """n < 0, and with n > 0 a NULL for every array the kernel dereferences unconditionally (api.hip checks each before the launch);
    n == 0 is BRIDGES_OK before any array is looked at; nothing is written."""
    L, s, n = lib(), stream(), 2
    P, ref = Q.placement_probe(), Q.placement_reference()
    rows = np.array([0, 5])
    tv = dev(ref["target_verts"][rows])
    ts, tf, sh, fc, ox, oy = (dev(P[k][rows]) for k in ("target_shape", "target_face", "shape", "face", "ox", "oy"))
    f1, pose_in = dev(ref["frame1"][rows]), dev(ref["pose"][rows])
    pose, verts, frame, frames = out_f64(n, 4), out_f64(n, 6, 2), out_f64(n, 6), out_f64(n, 6, 6)
    outs = (pose, verts, frame, frames)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in outs)

    calls = {                                       # name -> (function, arguments after (table, n), positions that must not be NULL)
        "bridges_place": (L.bridges_place, [f1, sh, fc, ox, oy, pose, verts], range(7)),
        "bridges_create_block": (L.bridges_create_block, [tv, ts, tf, sh, fc, ox, oy, pose, verts, frame], range(2, 9)),
        "bridges_pose_block": (L.bridges_pose_block, [sh, pose_in, verts], range(3)),
        "bridges_face_frames": (L.bridges_face_frames, [sh, tv, frames], range(3)),
    }
    for name, (fn, args, nullable) in calls.items():
        good = [ptr(a) for a in args]
        refused(L, fn(table.ptr, -1, *good, s), [name])
        refused(L, fn(None, n, *good, s), [name])
        for k, bad in each_null(args, nullable):
            refused(L, fn(table.ptr, n, *[ptr(a) for a in bad], s), [name, "NULL"])
        assert fn(table.ptr, 0, *[None] * len(args), s) == 0, name
        assert untouched(), name
        ok(fn(table.ptr, n, *good, s), name)      # the arguments the refusals varied are good
        assert not untouched()
        for t in outs:
            t.fill_(SENTINEL)


def test_contains_points_refusals(table):
    L, s = lib(), stream()
    row, si, pts, _gx, _gz = Q.point_probe()[0]
    v, p, n = dev(row), dev(pts[:5]), 5
    inside = out_u8(n)
    refused(L, L.bridges_contains_points(table.ptr, si, ptr(v), -1, ptr(p), ptr(inside), s), ["bridges_contains_points"])
    refused(L, L.bridges_contains_points(None, si, ptr(v), n, ptr(p), ptr(inside), s), ["bridges_contains_points"])
    refused(L, L.bridges_contains_points(table.ptr, -1, ptr(v), n, ptr(p), ptr(inside), s), ["bridges_contains_points", "shape_id"])
    refused(L, L.bridges_contains_points(table.ptr, si, None, n, ptr(p), ptr(inside), s), ["bridges_contains_points", "NULL"])
    refused(L, L.bridges_contains_points(table.ptr, si, ptr(v), n, None, ptr(inside), s), ["bridges_contains_points", "NULL"])
    refused(L, L.bridges_contains_points(table.ptr, si, ptr(v), n, ptr(p), None, s), ["bridges_contains_points", "NULL"])
    assert L.bridges_contains_points(table.ptr, si, None, 0, None, None, s) == 0
    assert split(inside, 0)[1]
    ok(L.bridges_contains_points(table.ptr, si, ptr(v), n, ptr(p), ptr(inside), s), "bridges_contains_points")
    assert Q.same_bits(split(inside, n)[0], Q.contains_points_ref(row, si, pts[:5]).astype(np.uint8))


def test_raster_refusals(table):
    """bridges_raster_sized names itself (not bridges_raster) and bridges_raster names itself; sizes 1 and 65; NULL inputs; n < 0."""
    L, s = lib(), stream()
    g = Q.raster_probe(64)["wide"]
    n = 3
    v, sid, X, Y = dev(g["verts"][:n]), dev(g["sid"][:n]), dev(g["X"]), dev(g["Y"])
    bits, img = out_words(n), out_f32(n, 64, 64)
    ins = [v, sid, X, Y]

    def sized(nn, a, size, tab=table.ptr):
        return L.bridges_raster_sized(tab, nn, *[ptr(t) for t in a], size, ptr(bits), ptr(img), s)

    def plain(nn, a, tab=table.ptr):
        return L.bridges_raster(tab, nn, *[ptr(t) for t in a], ptr(bits), ptr(img), s)

    for size in (1, 65, 0, -3):
        refused(L, sized(n, ins, size), ["bridges_raster_sized", "2..64"])
    refused(L, sized(-1, ins, 64), ["bridges_raster_sized"])
    refused(L, sized(n, ins, 64, tab=None), ["bridges_raster_sized"])
    refused(L, plain(-1, ins), ["bridges_raster"], not_names=["bridges_raster_sized"])
    refused(L, plain(n, ins, tab=None), ["bridges_raster"], not_names=["bridges_raster_sized"])
    for k, bad in each_null(ins, range(4)):
        refused(L, sized(n, bad, 64), ["bridges_raster_sized", "NULL"])
        refused(L, plain(n, bad), ["bridges_raster", "NULL"], not_names=["bridges_raster_sized"])
    assert sized(0, [None] * 4, 64) == 0 and plain(0, [None] * 4) == 0
    torch.cuda.synchronize()
    assert split(bits, 0)[1] and split(img, 0)[1]
    ok(plain(n, ins), "bridges_raster")
    assert Q.accept_words(split(bits, n)[0], Q.raster_reference(64)["wide"][:n])


def test_render_and_action_features_refusals(table):
    L, s = lib(), stream()
    g, n = Q.candidate_probe()["wide"], 3
    v, sid, X, Y = dev(g["verts"][:n]), dev(g["sid"][:n]), dev(g["X"]), dev(g["Y"])
    out = torch.full((64 * 64 + 64,), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    for W, H in ((0, 64), (64, 0), (-1, 64), (0, 0)):
        refused(L, L.bridges_render_blocks(table.ptr, n, ptr(v), ptr(sid), ptr(X), W, ptr(Y), H, ptr(out), s), ["bridges_render_blocks"])
    refused(L, L.bridges_render_blocks(table.ptr, -1, ptr(v), ptr(sid), ptr(X), 64, ptr(Y), 64, ptr(out), s), ["bridges_render_blocks"])
    for k, bad in each_null([v, sid, X, None, Y, None, out], (0, 1, 2, 4, 6)):      # (W and H sit between the arrays)
        a = [ptr(t) for t in bad]
        refused(L, L.bridges_render_blocks(table.ptr, n, a[0], a[1], a[2], 64, a[4], 64, a[6], s), ["bridges_render_blocks"])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL_U8).all())

    prefix = dev(Q.reward_prefix(Q.reward_map()))
    bits, mask, lin = out_words(n), out_u8(n), out_f32(n)

    def features(nn, size, pre, a=(v, sid, X, Y), lin_out=lin):
        return L.bridges_action_features(table.ptr, nn, *[ptr(t) for t in a], size, -3.0, 7.0, 0.0, 10.0, None, None, ptr(pre), ptr(bits), None,
                                         ptr(mask), ptr(lin_out), s)

    for size in (1, 65):
        refused(L, features(n, size, prefix), ["bridges_action_features", "2..64"])
    refused(L, features(n, 64, None), ["bridges_action_features", "reward_prefix"])
    refused(L, features(-1, 64, prefix), ["bridges_action_features"])
    for k, bad in each_null([v, sid, X, Y], range(4)):
        refused(L, features(n, 64, prefix, a=bad), ["bridges_action_features"])
    torch.cuda.synchronize()
    assert split(bits, 0)[1] and split(mask, 0)[1] and split(lin, 0)[1]
    ok(features(n, 64, prefix), "bridges_action_features")
    assert Q.accept_words(split(bits, n)[0], Q.candidate_words()["wide"][:n])
