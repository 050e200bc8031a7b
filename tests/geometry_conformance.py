"""Probe tables, references, bounds and defective twins for the stand-alone geometry and raster operators of
csrc/ops_kernels.hip -- k_place / k_create_block / k_pose_block / k_face_frames, k_contains_points, k_raster_generic,
k_render_blocks, k_action_features, k_bits_or (not a test module; no GPU needed).

* References come from oracle/geometry.py, oracle/shapes.py and oracle/raster.py only: ``create_block`` / ``align`` / ``Block``,
  ``edge_frame`` and ``contains_2d``.  Poses, vertices, frames, rasters and masks are exact and compared bit for bit
  (``same_bits``: the float64 bit patterns, or uint8 / uint64 words).  All five shapes are used.
* The numpy restatements (``align_np``, ``pose_np``, ``frames_np``, ``pixels_np``, ``render_np``, ``mask_np``, ``lin_np``) state
  the same operations batch-wise; tests/test_cpu_geometry_conformance_refs.py shows that they reproduce the oracle on every probe
  row.  Each DEFECTIVE TWIN is such a restatement wrong in one way a kernel could be; the CPU test shows that the acceptance
  function rejects every one of them on the probe alone.
* ``lin`` (sum of a reward map under a raster) is not exact: ``lin_bound`` is derived next to its constant.
"""
import fractions
import functools
import math
import types

import numpy as np

from oracle import geometry as G
from oracle import raster as R
from oracle import shapes as SH

SHAPE_NAMES = ("cube06", "cube1", "trapezoid", "hexagon", "block")
SHAPES = [SH.get_shape(name) for name in SHAPE_NAMES]
MAXV = 6
NV = np.array([len(s.verts) for s in SHAPES], dtype=np.int64)
XLIM, YLIM = (-3.0, 7.0), (0.0, 10.0)


def _table(fn, width=1):
    out = np.zeros((len(SHAPES), MAXV) + ((width,) if width > 1 else ()))
    for i, s in enumerate(SHAPES):
        for k in range(len(s.verts)):
            out[i, k] = fn(s, k)
    return out


VLOC = _table(lambda s, k: s.verts[k], 2)                                  # local vertices
FA = _table(lambda s, k: s.faces[k][0]).astype(np.int64)
FB = _table(lambda s, k: s.faces[k][1]).astype(np.int64)
FC = _table(lambda s, k: s.face_frame_local(k)[0], 2)                      # local face centres
FN = _table(lambda s, k: s.face_frame_local(k)[2], 2)                      # local face normals


def same_bits(a, b):
    """Equal shapes and equal bit patterns (float64 compared as uint64: -0.0 is not 0.0, NaN equals itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    elif a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return bool(np.array_equal(a, b))


def exact_cs(angle):
    """(cos, sin) of an angle; the four right angles exactly."""
    for a, cs in ((0.0, (1.0, 0.0)), (math.pi / 2, (0.0, 1.0)), (-math.pi / 2, (0.0, -1.0)), (math.pi, (-1.0, 0.0)),
                  (3 * math.pi / 2, (0.0, -1.0))):
        if angle == a:
            return cs
    return (math.cos(angle), math.sin(angle))


def pad_verts(rows):
    """list of vertex lists -> float64 [n, 6, 2], slots >= nv zero."""
    out = np.zeros((len(rows), MAXV, 2))
    for i, v in enumerate(rows):
        out[i, :len(v)] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# bit rasters: word r = image row r (row 0 = top), bit q of it = column q

def pack(img):
    """bool [H <= 64, W <= 64] -> uint64 [64]."""
    H, W = img.shape
    words = np.zeros(64, dtype=np.uint64)
    weights = np.uint64(1) << np.arange(W, dtype=np.uint64)
    words[:H] = (img.astype(np.uint64) * weights[None, :]).sum(axis=1, dtype=np.uint64)
    return words


def unpack(words):
    """uint64 [..., 64] -> bool [..., 64, 64]."""
    words = np.asarray(words, dtype=np.uint64)
    return ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def bits_to_f32(words):
    return unpack(words).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# placement probe (K1)

# the hexagon's own symmetry angles follow the issue's five: posed there, parallel normals differ by rounding noise only, which is
# what puts cy inside the sign band [-1e-6, 0) on create_block's path too
PLACE_FIXED_ANGLES = (0.0, math.pi / 2, -math.pi / 2, math.pi, math.pi / 4, math.pi / 3, -math.pi / 3, 2 * math.pi / 3, -2 * math.pi / 3)
PLACE_RANDOM_ANGLES = 40
OFFSETS = [(ox, oy) for ox in (0.0, 1.0 / 3.0, -1.0 / 3.0, 0.6) for oy in (0.0, 0.25)]
SHAPE_FACES = [(si, f) for si, s in enumerate(SHAPES) for f in range(len(s.verts))]        # 22
# raw target normals for bridges_place: posed blocks only produce unit normals, with which neither clamp of align can fire
RAW_NORMALS = ((0.0, 1.0 + 2.0 ** -52), (0.0, 2.0), (0.0, -2.0), (0.0, float(np.nextafter(1.0, 0.0))),
               (float(np.nextafter(1.0, 0.0)), 0.0), (-2.0, 0.0))
RAW_ULP_STEPS = ((0, +1), (0, -1), (1, +1), (1, -1))      # and, per shape face, its opposite normal with one coordinate an ulp off


@functools.lru_cache(maxsize=None)
def placement_probe():
    """The create_block table: target shape x target face x shape x face over 49 target rotations, the offsets cycling, then every
    shape face on the floor with every offset.  Returns arrays: target_shape, target_face (-1 = floor), target_pose [n,4], shape,
    face, ox, oy."""
    rng = np.random.default_rng(20260101)
    angles = list(PLACE_FIXED_ANGLES) + [float(a) for a in rng.uniform(-math.pi, math.pi, PLACE_RANDOM_ANGLES)]
    positions = np.stack([rng.uniform(-2.0, 6.0, len(angles)), rng.uniform(0.0, 4.0, len(angles))], axis=1)
    rows, k = [], 0
    for ai, a in enumerate(angles):
        c, s = exact_cs(a)
        for ts, tf in SHAPE_FACES:
            for sh, f in SHAPE_FACES:
                ox, oy = OFFSETS[k % len(OFFSETS)]
                k += 1
                rows.append((ts, tf, positions[ai, 0], positions[ai, 1], c, s, sh, f, ox, oy))
    for sh, f in SHAPE_FACES:
        for ox, oy in OFFSETS:
            rows.append((sh, -1, 0.0, 0.0, 1.0, 0.0, sh, f, ox, oy))
    a = np.array(rows, dtype=np.float64)
    return dict(target_shape=a[:, 0].astype(np.int32), target_face=a[:, 1].astype(np.int32), target_pose=np.ascontiguousarray(a[:, 2:6]),
                shape=a[:, 6].astype(np.int32), face=a[:, 7].astype(np.int32), ox=np.ascontiguousarray(a[:, 8]),
                oy=np.ascontiguousarray(a[:, 9]))


def _flat_frame(fr):
    (cx, cz), (tx, tz), (nx, nz) = fr
    return (cx, cz, tx, tz, nx, nz)


def _block_arrays(b):
    nv = len(b.shape.verts)
    verts, frames = np.zeros((MAXV, 2)), np.zeros((MAXV, 6))
    verts[:nv] = b.verts
    frames[:nv] = [_flat_frame(fr) for fr in b.frames]
    return verts, frames


@functools.lru_cache(maxsize=None)
def placement_reference():
    """oracle.geometry.create_block on every row of placement_probe(): target_verts [n,6,2], frame1 [n,6] (the target frame), pose
    [n,4], verts [n,6,2], frames [n,6,6] (Block.frames of the new block), all zero in slots >= nv."""
    P = placement_probe()
    n = len(P["shape"])
    out = dict(target_verts=np.zeros((n, MAXV, 2)), frame1=np.zeros((n, 6)), pose=np.zeros((n, 4)), verts=np.zeros((n, MAXV, 2)),
               frames=np.zeros((n, MAXV, 6)))
    targets = {}
    for i in range(n):
        ts, tf = int(P["target_shape"][i]), int(P["target_face"][i])
        if tf < 0:
            blocks, action, frame1 = [], (-1, 0), G.FLOOR_FRAME
        else:
            key = (ts, tuple(P["target_pose"][i]))
            if key not in targets:
                targets[key] = G.Block(SHAPES[ts], key[1][:2], key[1][2:])
            tb = targets[key]
            blocks, action, frame1 = [tb], (0, tf), tb.face_frame(tf)
            out["target_verts"][i, :len(tb.verts)] = tb.verts
        b = G.create_block(SHAPES, blocks, action + (int(P["shape"][i]), int(P["face"][i]), P["ox"][i], P["oy"][i]))
        out["frame1"][i] = _flat_frame(frame1)
        out["pose"][i] = b.pos + b.cs
        out["verts"][i], out["frames"][i] = _block_arrays(b)
    return out


@functools.lru_cache(maxsize=None)
def place_probe():
    """The bridges_place table: the target frames of the placement probe, then raw frames against every shape face: RAW_NORMALS (both clamps) and
    the face's opposite normal an ulp off (the sign band).
    Returns frame1 [n,6], shape, face, ox, oy."""
    P, ref = placement_probe(), placement_reference()
    raw = []
    for k, (nx, nz) in enumerate(RAW_NORMALS):
        for j, (sh, f) in enumerate(SHAPE_FACES):
            ox, oy = OFFSETS[(k + j) % len(OFFSETS)]
            raw.append((0.5, 1.0, nz, -nx, nx, nz, sh, f, ox, oy))
    for j, (sh, f) in enumerate(SHAPE_FACES):
        n2 = SHAPES[sh].face_frame_local(f)[2]
        for k, (axis, sign) in enumerate(RAW_ULP_STEPS):
            n1 = [-n2[0], -n2[1]]
            n1[axis] = float(np.nextafter(n1[axis], sign * math.inf))
            ox, oy = OFFSETS[(k + j) % len(OFFSETS)]
            raw.append((0.5, 1.0, n1[1], -n1[0], n1[0], n1[1], sh, f, ox, oy))
    raw = np.array(raw, dtype=np.float64)
    return dict(frame1=np.concatenate([ref["frame1"], raw[:, :6]]), shape=np.concatenate([P["shape"], raw[:, 6].astype(np.int32)]),
                face=np.concatenate([P["face"], raw[:, 7].astype(np.int32)]), ox=np.concatenate([P["ox"], raw[:, 8]]),
                oy=np.concatenate([P["oy"], raw[:, 9]]))


@functools.lru_cache(maxsize=None)
def place_reference():
    """oracle.geometry.align + Block on every row of place_probe(): pose, verts, frames, and the branch operands c_raw = -dot (before
    the clamps) and cy."""
    P = place_probe()
    n = len(P["shape"])
    out = dict(pose=np.zeros((n, 4)), verts=np.zeros((n, MAXV, 2)), frames=np.zeros((n, MAXV, 6)), c_raw=np.zeros(n), cy=np.zeros(n))
    for i in range(n):
        fr = P["frame1"][i]
        frame1 = ((fr[0], fr[1]), (fr[2], fr[3]), (fr[4], fr[5]))
        shape = SHAPES[int(P["shape"][i])]
        c2, _t2, n2 = shape.face_frame_local(int(P["face"][i]))
        pos, cs = G.align(frame1, c2, n2, float(P["ox"][i]), float(P["oy"][i]))
        b = G.Block(shape, pos, cs)
        out["pose"][i] = b.pos + b.cs
        out["verts"][i], out["frames"][i] = _block_arrays(b)
        out["c_raw"][i] = -(fr[4] * n2[0] + fr[5] * n2[1])
        out["cy"][i] = fr[5] * n2[0] - fr[4] * n2[1]
    return out


def place_branches(ref):
    """How often each branch of align is taken on the bridges_place table."""
    c, cy = ref["c_raw"], ref["cy"]
    band = (cy < 0) & (cy + 1e-6 >= 0)
    return dict(clamp_hi=int((c > 1.0).sum()), clamp_lo=int((c < -1.0).sum()), band=int(band.sum()),
                negative=int(((cy < 0) & ~band).sum()), non_negative=int((cy >= 0).sum()))


def batch_rows(total, n, salt=0):
    """Row indices of a batch of n cut from a table of ``total`` rows: a stride that walks the whole table, offset by ``salt``."""
    stride = max(total // n, 1)
    return (salt + stride * np.arange(n)) % total


# numpy restatements (and their twins) ---------------------------------------------------------------------------------------

def align_np(frame1, sid, face, ox, oy, clamps=True, sign_eps=1e-6):
    n2x, n2z = FN[sid, face, 0], FN[sid, face, 1]
    c2x, c2z = FC[sid, face, 0], FC[sid, face, 1]
    c1x, c1z, t1x, t1z, n1x, n1z = (frame1[:, k] for k in range(6))
    dot = n1x * n2x + n1z * n2z
    c = -dot
    if clamps:
        c = np.where(c > 1.0, 1.0, c)
        c = np.where(c < -1.0, -1.0, c)
    cy = n1z * n2x - n1x * n2z
    s = np.where(cy + sign_eps >= 0, np.abs(cy), -np.abs(cy))
    r2x = c2x * c + c2z * s
    r2z = c2z * c - c2x * s
    px = ((c1x + ox * t1x) + oy * n1x) - r2x
    pz = ((c1z + ox * t1z) + oy * n1z) - r2z
    return np.stack([px, pz, c, s], axis=1)


def pose_np(sid, pose, transposed=False, pad=0.0):
    vx, vz = VLOC[sid, :, 0], VLOC[sid, :, 1]                               # [n,6]
    px, pz, c, s = (pose[:, k, None] for k in range(4))
    if transposed:
        rx, rz = vx * c - vz * s, vz * c + vx * s
    else:
        rx, rz = vx * c + vz * s, vz * c - vx * s
    out = np.stack([px + rx, pz + rz], axis=2)
    out[np.arange(MAXV)[None, :] >= NV[sid][:, None]] = pad
    return out


def frames_np(sid, verts, pad=0.0):
    n = len(sid)
    idx = np.arange(n)[:, None]
    a, b = verts[idx, FA[sid]], verts[idx, FB[sid]]                         # [n,6,2]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (a + b) * 0.5
        d = b - a
        L = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        t = d / L[..., None]
    out = np.concatenate([c, t, np.stack([-t[..., 1], t[..., 0]], axis=2)], axis=2)
    out[np.arange(MAXV)[None, :] >= NV[sid][:, None]] = pad
    return out


def place_np(P, **kw):
    """(pose, verts) of the bridges_place table; kw: clamps, sign_eps (align), transposed, pad (pose)."""
    pose = align_np(P["frame1"], P["shape"], P["face"], P["ox"], P["oy"], **{k: v for k, v in kw.items() if k in ("clamps", "sign_eps")})
    return pose, pose_np(P["shape"], pose, **{k: v for k, v in kw.items() if k in ("transposed", "pad")})


def accept_place(got, ref):
    """K1's acceptance: pose and vertices bit for bit."""
    return same_bits(got[0], ref["pose"]) and same_bits(got[1], ref["verts"])


PLACE_TWINS = {
    "align_without_clamps": dict(clamps=False),
    "align_sign_cy_ge_0": dict(sign_eps=0.0),
    "transposed_rotation": dict(transposed=True),
    "padding_not_zeroed": dict(pad=-77.25),
}


# ---------------------------------------------------------------------------------------------------------------------------
# outlines, the pixel test and its twins

def outline(verts_row, sid):
    """A posed outline as oracle.raster.contains_2d takes it: ``frames`` by oracle.shapes.edge_frame from the world vertices."""
    v = [(float(x), float(z)) for x, z in np.asarray(verts_row)[:NV[sid]]]
    return types.SimpleNamespace(frames=[SH.edge_frame(v[a], v[b]) for a, b in SHAPES[sid].faces], verts=v)


def contains_points_ref(verts_row, sid, pts):
    """The pixel test of oracle.raster.contains_2d on arbitrary points [n,2] (operation for operation; the CPU test compares it
    with contains_2d on the probe's grid points)."""
    inside = np.ones(len(pts), dtype=bool)
    for (c, _t, n) in outline(verts_row, sid).frames:
        d = (pts[:, 0] - c[0]) * n[0] + (pts[:, 1] - c[1]) * n[1]
        inside &= d <= 0
    return inside


def _fma_le0(a, b, c):
    """fma(a, b, c) <= 0, the fused result formed exactly and rounded once."""
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c)) <= 0.0


def pixels_np(verts_row, sid, X, Y, op="le", drop_last=False):
    """contains_2d restated, with the twins' switches.  op: "le" (the contract), "lt", "fma" (d = fma(X - c.x, n.x, (Y - c.z) * n.z):
    what a compiler contracts the expression to).  The fused result can differ in sign from the separately rounded one only
    where |d| <= 2**-50 * |(X - c.x) * n.x|, so only those pixels are recomputed exactly."""
    frames = outline(verts_row, sid).frames
    if drop_last:
        frames = frames[:-1]
    inside = np.ones((len(Y), len(X)), dtype=bool)
    for (c, _t, n) in frames:
        ax = X - c[0]
        tx = ax * n[0]
        tz = (Y - c[1]) * n[1]
        d = tx[None, :] + tz[:, None]
        if op == "lt":
            ok = d < 0
        else:
            ok = d <= 0
            if op == "fma":
                for r, q in zip(*np.nonzero(np.abs(d) <= 2.0 ** -50 * np.abs(tx)[None, :])):
                    ok[r, q] = _fma_le0(float(ax[q]), float(n[0]), float(tz[r]))
        inside &= ok
    return inside


def near_edge_counts(verts_row, sid, X, Y):
    """(sample points with d == 0 for some face, sample points with 0 < |d| < 1e-15 for some face)."""
    zero = np.zeros((len(Y), len(X)), dtype=bool)
    near = np.zeros_like(zero)
    for (c, _t, n) in outline(verts_row, sid).frames:
        d = ((X - c[0]) * n[0])[None, :] + ((Y - c[1]) * n[1])[:, None]
        zero |= d == 0
        near |= (d != 0) & (np.abs(d) < 1e-15)
    return int(zero.sum()), int(near.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# raster probe (K4)

RASTER_SIZES = (2, 3, 16, 17, 31, 32, 33, 63, 64)
RASTER_ANGLES = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), exact_cs(math.pi / 4), exact_cs(0.3), exact_cs(2.0), exact_cs(-1.1))
BORDER_CENTRES = ((-3.2, 5.0), (7.2, 5.3), (2.0, 10.1), (2.2, -0.1), (-6.0, -4.0), (10.5, 14.0))   # four overhangs, two outside
TIGHT_CENTRE, TIGHT_HALF = (2.0, 5.0), 0.2
TIGHT_OUTLINES = ((1, 0), (1, 2), (1, 1), (1, 3), (3, 0), (3, 2), (0, 0), (4, 0), (2, 0), (1, 4))   # (shape, angle)


def _feature(shape, k, kind):
    nv = len(shape.verts)
    if kind == 0:
        return shape.verts[k % nv]
    if kind == 1:
        return shape.face_frame_local(k % nv)[0]
    return (0.0, 0.0)


@functools.lru_cache(maxsize=None)
def raster_probe(S):
    """Two groups of posed outlines for S x S images, each a dict(X, Y, verts [n,6,2], sid [n]):

    * "wide": the grid of XLIM x YLIM.  Per shape 16 poses over the eight RASTER_ANGLES, each with a vertex, an edge midpoint or
      the centre put on a sample point of THIS grid (pos = sample - R(feature): exactly on it or an ulp off), then six poses that
      hang over or lie outside a border -- 110 outlines;
    * "tight": a grid of half-width 0.2 around the centre of a cube1, the cube at the four right angles (its normals change sign,
      so prefix and suffix runs both cover the whole image) and a few other outlines around the same centre."""
    X, Y = R.pixel_grid(XLIM, YLIM, (S, S))
    verts, sid = [], []
    for si, shape in enumerate(SHAPES):
        for k in range(16):
            c, s = RASTER_ANGLES[k % 8]
            feat = _feature(shape, k, (k // 8 + k + si) % 3)
            px, pz = float(X[(3 + 5 * k + 2 * si) % S]), float(Y[(1 + 7 * k + 3 * si) % S])
            rx, rz = G.rot(feat, c, s)
            verts.append(G.Block(shape, (px - rx, pz - rz), (c, s)).verts)
            sid.append(si)
        for k, centre in enumerate(BORDER_CENTRES):
            verts.append(G.Block(shape, centre, RASTER_ANGLES[(k + si) % 8]).verts)
            sid.append(si)
    wide = dict(X=X, Y=Y, verts=pad_verts(verts), sid=np.array(sid, dtype=np.int32))
    (cx, cz), h = TIGHT_CENTRE, TIGHT_HALF
    Xt, Yt = R.pixel_grid((cx - h, cx + h), (cz - h, cz + h), (S, S))
    tv = [G.Block(SHAPES[si], TIGHT_CENTRE, RASTER_ANGLES[ai]).verts for si, ai in TIGHT_OUTLINES]
    tight = dict(X=Xt, Y=Yt, verts=pad_verts(tv), sid=np.array([si for si, _ in TIGHT_OUTLINES], dtype=np.int32))
    return dict(wide=wide, tight=tight)


def raster_words(group, pixel_fn=None, **kw):
    """uint64 [n,64] words of a group's outlines: oracle.raster.contains_2d (default) or a restatement, packed; rows and bits >= S zero."""
    out = np.zeros((len(group["sid"]), 64), dtype=np.uint64)
    for i, si in enumerate(group["sid"]):
        if pixel_fn is None:
            img = R.contains_2d(outline(group["verts"][i], int(si)), group["X"], group["Y"])
        else:
            img = pixel_fn(group["verts"][i], int(si), group["X"], group["Y"], **kw)
        out[i] = pack(img)
    return out


@functools.lru_cache(maxsize=None)
def raster_reference(S):
    return {name: raster_words(g) for name, g in raster_probe(S).items()}


def _shifted(g):                                                             # the grid one sample on: pixel q samples X[q + 1]
    X, Y = g["X"], g["Y"]
    return dict(g, X=np.append(X[1:], X[-1] + (X[-1] - X[-2])), Y=np.append(Y[1:], Y[-1] + (Y[-1] - Y[-2])))


def _dirty(g):                                                               # lanes >= S repeat the last sample and are kept
    S = len(g["X"])
    return dict(g, X=np.append(g["X"], np.full(64 - S, g["X"][-1])), Y=np.append(g["Y"], np.full(64 - S, g["Y"][-1])))


def _flip_rows(words, S):
    out = np.zeros_like(words)
    out[:, :S] = words[:, :S][:, ::-1]
    return out


def _reverse_columns(words, S):
    img = unpack(words)[:, :S, :S][:, :, ::-1]
    return np.stack([pack(i) for i in img]) if len(img) else words


RASTER_TWINS = {
    "pixel_test_lt": lambda g, S: raster_words(g, pixels_np, op="lt"),
    "pixel_test_fma": lambda g, S: raster_words(g, pixels_np, op="fma"),
    "last_face_dropped": lambda g, S: raster_words(g, pixels_np, drop_last=True),
    "row_order_flipped": lambda g, S: _flip_rows(raster_words(g, pixels_np), S),
    "column_bits_reversed": lambda g, S: _reverse_columns(raster_words(g, pixels_np), S),
    "grid_shifted_one_sample": lambda g, S: raster_words(_shifted(g), pixels_np),
    "beyond_S_not_cleared": lambda g, S: raster_words(_dirty(g), pixels_np),
}


def accept_words(got, want):
    """The rasters' acceptance: every word of the 64-word canvas, so rows and bits >= S must be zero."""
    return same_bits(np.asarray(got, dtype=np.uint64), want)


# ---------------------------------------------------------------------------------------------------------------------------
# point probe (contains_points)

POINT_N = (1, 255, 256, 257, 4099)
POINT_POSES = (0, 4, 5, 7, 9)                                                # indices into a shape's 16 wide poses: five angles


def _ulp_step(p, n, sign):
    """p moved one ulp along sign * n in every coordinate n is non-zero in."""
    return tuple(float(np.nextafter(p[k], math.copysign(math.inf, sign * n[k]))) if n[k] != 0 else p[k] for k in range(2))


@functools.lru_cache(maxsize=None)
def point_probe():
    """Per shape and pose (verts_row, sid, points [4096 + 4 nv, 2]): the vertices, the edge midpoints, the midpoints one ulp out and
    one ulp in along the normal, then a 64 x 64 grid over the outline's bounding box widened by a tenth."""
    wide = raster_probe(64)["wide"]
    cases = []
    for si in range(len(SHAPES)):
        for k in POINT_POSES:
            row = wide["verts"][22 * si + k]
            o = outline(row, si)
            pts = list(o.verts) + [c for c, _t, _n in o.frames]
            for c, _t, n in o.frames:
                pts += [_ulp_step(c, n, +1), _ulp_step(c, n, -1)]
            v = np.array(o.verts)
            lo, hi = v.min(0), v.max(0)
            m = 0.1 * (hi - lo)
            gx, gz = np.linspace(lo[0] - m[0], hi[0] + m[0], 64), np.linspace(lo[1] - m[1], hi[1] + m[1], 64)
            grid = np.stack(np.meshgrid(gx, gz), axis=2).reshape(-1, 2)
            cases.append((row, si, np.ascontiguousarray(np.concatenate([np.array(pts), grid])), gx, gz))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# scene probe (render_blocks)

SCENE_N = (0, 1, 15, 16, 17, 33, 40)
SCENE_GRIDS = ((1, 1), (64, 64), (65, 65), (200, 120), (17, 300))           # (W, H)
RENDER_TILE = 16


def scene(n, first_tile_misses=False, corner=False):
    """n outlines, outline k in cell k of an 8 x 5 partition of XLIM x YLIM (so each is the only hit of some pixels -- the last
    outline of the last tile included).  first_tile_misses: outlines 0..15 lie 20 to the left of the image.  corner: the last
    outline is centred on (XLIM[0], YLIM[1]), the only sample of a 1 x 1 grid."""
    verts, sid = [], []
    for k in range(n):
        centre = (-3.0 + 0.625 + 1.25 * (k % 8), 1.0 + 2.0 * (k // 8))
        if first_tile_misses and k < RENDER_TILE:
            centre = (centre[0] - 20.0, centre[1])
        if corner and k == n - 1:
            centre = (XLIM[0], YLIM[1])
        verts.append(G.Block(SHAPES[k % 5], centre, RASTER_ANGLES[(3 * k) % 8]).verts)
        sid.append(k % 5)
    return pad_verts(verts), np.array(sid, dtype=np.int32)


def scene_grid(W, H):
    return np.linspace(XLIM[0], XLIM[1], W), np.linspace(YLIM[1], YLIM[0], H)


def render_reference(verts, sid, X, Y):
    """The OR of oracle.raster.contains_2d per block: uint8 [H, W]."""
    img = np.zeros((len(Y), len(X)), dtype=bool)
    for i, si in enumerate(sid):
        img |= R.contains_2d(outline(verts[i], int(si)), X, Y)
    return img.astype(np.uint8)


def render_np(verts, sid, X, Y, skip=None, forget_tile0=False):
    img = np.zeros((len(Y), len(X)), dtype=bool)
    for i, si in enumerate(sid):
        if i == skip or (forget_tile0 and i < RENDER_TILE and len(sid) > RENDER_TILE):
            continue
        img |= pixels_np(verts[i], int(si), X, Y)
    return img.astype(np.uint8)


RENDER_TWINS = {"outline_16_skipped": dict(skip=16), "tile_0_forgotten": dict(forget_tile0=True)}


def scene_cases():
    """(n, W, H, first_tile_misses) of every scene of the probe."""
    cases = [(n, W, H, False) for n in SCENE_N for W, H in SCENE_GRIDS]
    return cases + [(33, 64, 64, True), (17, 200, 120, True)]


def scene_of(n, W, H, miss):
    verts, sid = scene(n, first_tile_misses=miss, corner=(W == 1 and n > 0))
    X, Y = scene_grid(W, H)
    return verts, sid, X, Y


# ---------------------------------------------------------------------------------------------------------------------------
# candidate probe (action_features)

CAND_N = (1, 4, 5, 300)
EPS = 1e-6
LOW_YLIM = (-2.0, 8.0)        # with ylim0 = 0 the rule  z < ylim0 - eps  and the rule  z < -eps  coincide; below zero they do not


def _cube1_at(x_min, z_min):
    return [(x_min, z_min), (x_min, z_min + 1.0), (x_min + 1.0, z_min + 1.0), (x_min + 1.0, z_min)]     # cube1's vertex order


def _edge_pairs(t, outward):
    return t, float(np.nextafter(t, math.copysign(math.inf, outward)))


@functools.lru_cache(maxsize=None)
def candidate_probe():
    """Two groups, each dict(xlim, ylim, X, Y, verts, sid), S = 64:

    * "wide" (XLIM, YLIM): the 110 outlines of the raster probe, then cube1 outlines with a vertex exactly on xlim0 - 1e-6, on
      z = -1e-6, on xlim1 + 1e-6, on ylim1 + 1e-6 (in bounds) and one ulp further out (not);
    * "low" (XLIM, LOW_YLIM): cube1 outlines with the lowest vertex at z = -1e-6, one ulp lower, at -1 (in bounds but for the
      z < -eps clause), at ylim0 - 1e-6 and one ulp lower, and one well inside."""
    wide = raster_probe(64)["wide"]
    edge = []
    for t in _edge_pairs(XLIM[0] - EPS, -1):
        edge.append(_cube1_at(t, 3.0))
    for t in _edge_pairs(-EPS, -1):
        edge.append(_cube1_at(1.0, t))
    for t in _edge_pairs(XLIM[1] + EPS, +1):
        edge.append(_cube1_at(t - 1.0, 3.0))
        edge[-1][2] = (t, edge[-1][2][1])
        edge[-1][3] = (t, edge[-1][3][1])
    for t in _edge_pairs(YLIM[1] + EPS, +1):
        edge.append(_cube1_at(1.0, t - 1.0))
        edge[-1][1] = (edge[-1][1][0], t)
        edge[-1][2] = (edge[-1][2][0], t)
    groups = dict(wide=dict(xlim=XLIM, ylim=YLIM, X=wide["X"], Y=wide["Y"], verts=np.concatenate([wide["verts"], pad_verts(edge)]),
                            sid=np.concatenate([wide["sid"], np.full(len(edge), 1, dtype=np.int32)])))
    low = [_cube1_at(0.0, t) for t in _edge_pairs(-EPS, -1)] + [_cube1_at(2.0, -1.0)]
    low += [_cube1_at(4.0, t) for t in _edge_pairs(LOW_YLIM[0] - EPS, -1)] + [_cube1_at(0.5, 3.0)]
    X, Y = R.pixel_grid(XLIM, LOW_YLIM, (64, 64))
    groups["low"] = dict(xlim=XLIM, ylim=LOW_YLIM, X=X, Y=Y, verts=pad_verts(low), sid=np.full(len(low), 1, dtype=np.int32))
    return groups


@functools.lru_cache(maxsize=None)
def candidate_words():
    return {name: raster_words(g) for name, g in candidate_probe().items()}


def mask_np(group, words, state=None, obstacle=None, eps=EPS, z_clause=True, state_only=False):
    """filter_actions as include/bridges_hip.h states it: every vertex inside [xlim, ylim] and above z = 0 within eps, and no pixel in
    common with state | obstacle (uint64 [64] each or None)."""
    x0, x1, y0, y1 = group["xlim"] + group["ylim"]
    vx, vz = group["verts"][..., 0], group["verts"][..., 1]
    out = (vx < x0 - eps) | (vx > x1 + eps) | (vz < y0 - eps) | (vz > y1 + eps)
    if z_clause:
        out |= vz < -eps
    out &= np.arange(MAXV)[None, :] < NV[group["sid"]][:, None]
    occ = np.zeros(64, dtype=np.uint64)
    if state is not None:
        occ |= state
    if obstacle is not None and not state_only:
        occ |= obstacle
    overlap = ((words & occ[None, :]) != 0).any(axis=1)
    return (~out.any(axis=1) & ~overlap).astype(np.uint8)


MASK_TWINS = {"bounds_eps_0": dict(eps=0.0), "bounds_without_z_clause": dict(z_clause=False), "overlap_state_only": dict(state_only=True)}


def _one_pixel(r, q):
    w = np.zeros(64, dtype=np.uint64)
    w[r] = np.uint64(1) << np.uint64(q)
    return w


@functools.lru_cache(maxsize=None)
def occupancy_cases():
    """(name, state, obstacle) for the wide group: both NULL; one given; both given, sharing exactly one pixel with a candidate (the
    obstacle's -- the state's pixels touch no candidate); both given, sharing none."""
    words = candidate_words()["wide"]
    img = unpack(words)
    union = img.any(axis=0)
    ok = np.nonzero(mask_np(candidate_probe()["wide"], words) & img.any(axis=(1, 2)))[0]     # in bounds, with pixels
    hit_a = tuple(int(v) for v in np.argwhere(img[ok[0]])[0])                # a pixel of the first of them
    hit_b = tuple(int(v) for v in np.argwhere(img[ok[-1]])[-1])              # and one of the last
    free = [tuple(int(v) for v in p) for p in np.argwhere(~union)]
    assert len(free) >= 2 and hit_a != hit_b
    return (("both_null", None, None),
            ("state_only", _one_pixel(*hit_a), None),
            ("obstacle_only", None, _one_pixel(*hit_b)),
            ("both_one_shared", _one_pixel(*free[0]), _one_pixel(*hit_b) | _one_pixel(*free[-1])),
            ("both_none_shared", _one_pixel(*free[0]), _one_pixel(*free[-1])))


@functools.lru_cache(maxsize=None)
def reward_map():
    """float32 [64,64] for the wide group, mixed signs: magnitude in [2e-4, 1e-3) wherever some candidate has a pixel, 1e6 on the
    pixels next to those in their row (just outside every run that ends there), magnitude in [0.5, 2) elsewhere.  A sum that
    takes one pixel too many is off by 1e6; one that takes one too few is off by >= 2e-4, over ten times lin_bound here."""
    rng = np.random.default_rng(7)
    union = unpack(candidate_words()["wide"]).any(axis=0)
    sign = np.where(rng.random((64, 64)) < 0.5, -1.0, 1.0)
    m = sign * rng.uniform(0.5, 2.0, (64, 64))
    beside = np.zeros_like(union)
    beside[:, 1:] |= union[:, :-1]
    beside[:, :-1] |= union[:, 1:]
    m[beside] = sign[beside] * 1e6
    m[union] = (sign * rng.uniform(2e-4, 1e-3, (64, 64)))[union]
    return m.astype(np.float32)


def reward_prefix(m):
    """float64 row prefix sums [64,65], accumulated left to right (bridges_hip.ops.reward_prefix)."""
    pre = np.zeros((64, 65), dtype=np.float64)
    pre[:, 1:] = np.cumsum(m.astype(np.float64), axis=1)
    return pre


def lin_reference(words, m):
    """R: math.fsum of the float32 map values under each raster (exact, rounded once)."""
    img = unpack(words)
    return np.array([math.fsum(float(v) for v in m[i]) for i in img], dtype=np.float64)


# |lin - R| <= 2**-24 |R| + 2**-44 sum|map| + 2**-149, derived (u = 2**-53):
#  * entry j of a row's float64 prefix is a left-to-right sum of j <= 64 terms: its error is at most 64 u A_r, A_r = the row's
#    absolute sum (first order; the float32 -> float64 conversions are exact);
#  * the row's part prefix[hi] - prefix[lo] subtracts two entries, 128 u A_r, and rounds once more: + u |part| <= u A_r;
#  * the 64 parts are added in float64, any order: at most 63 roundings of partial sums <= sum_r A_r, so <= 64 u sum|map|;
#  * in all (128 + 1 + 64) u sum|map| = 193 * 2**-53 sum|map| < 2**-45.4 sum|map|; 2**-44 leaves a factor 2.6 of room for the
#    second-order terms;
#  * the result is rounded to float32 once: 2**-24 |R| (plus 2**-24 of the error above, inside the room), or half the smallest
#    float32 subnormal, 2**-149 with room, when it underflows.
LIN_REL, LIN_ABS, LIN_TINY = 2.0 ** -24, 2.0 ** -44, 2.0 ** -149


def lin_bound(ref, m):
    return LIN_REL * np.abs(ref) + LIN_ABS * float(np.abs(m.astype(np.float64)).sum()) + LIN_TINY


def accept_lin(lin, ref, m):
    assert lin.dtype == np.float32
    return bool((np.abs(lin.astype(np.float64) - ref) <= lin_bound(ref, m)).all())


def lin_np(words, prefix, hi_shift=0, lo_shift=0):
    """The kernel's own summation in float64: per row prefix[hi] - prefix[lo] of the row's run [lo, hi), the 64 parts added in a
    tree, one float32 rounding.  hi_shift / lo_shift: the twins' wrong indices."""
    out = np.zeros(len(words), dtype=np.float32)
    for i, cand in enumerate(words):
        parts = np.zeros(64)
        for r, w in enumerate(cand):
            w = int(w)
            if w:
                lo, hi = (w & -w).bit_length() - 1, w.bit_length()
                parts[r] = prefix[r, hi + hi_shift] - prefix[r, lo + lo_shift]
        while len(parts) > 1:
            parts = parts[0::2] + parts[1::2]
        out[i] = np.float32(parts[0])
    return out


LIN_TWINS = {"lin_from_prefix_hi_minus_1": dict(hi_shift=-1), "lin_from_prefix_lo_plus_1": dict(lo_shift=+1)}


# ---------------------------------------------------------------------------------------------------------------------------
# bits_or

def bits_or_probe():
    """bits uint64 [12,64] and ranges int32 [g,2]: empty ranges (lo == hi, at either end and inside, and hi < lo), one-row ranges,
    the whole table, and overlapping ranges."""
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2 ** 63, size=(12, 64), dtype=np.uint64) & rng.integers(0, 2 ** 63, size=(12, 64), dtype=np.uint64)
    bits[3] |= np.uint64(1) << np.uint64(63)
    ranges = np.array([[0, 0], [0, 1], [11, 12], [12, 12], [0, 12], [5, 5], [3, 4], [2, 9], [7, 3], [4, 12]], dtype=np.int32)
    return bits, ranges


def bits_or_reference(bits, ranges):
    out = np.zeros((len(ranges), 64), dtype=np.uint64)
    for g, (lo, hi) in enumerate(ranges):
        for i in range(lo, hi):
            out[g] |= bits[i]
    return out
