"""Probes and references for the conformance tests of the contact detector and the equilibrium solver (not a test module, no
GPU import): ``k_stability`` (the tail of csrc/ops_kernels.hip) with csrc/rbe_device.h behind it, and the two env-side
producers of the contact list, ``k_step`` and ``k_rebuild_contacts``.

References: oracle/rbe.py (face_pair_contact, find_interfaces, equilibrium_system, infeasibility, is_stable_rbe,
is_stable_rbe_penalty) and oracle/shapes.py (edge_frame).  find_interfaces reads only ``verts``, ``frames``, ``shape.faces`` and
``shape.depth`` of a block, equilibrium_system only ``centroid`` and ``weight_per_density``: ``Posed`` is a stand-in with
hand-written vertices for the faces no placement produces.

Three things live here:
  * the probes -- the boundary table of the detector (one face pair per assembly, at the three decision boundaries), the
    assemblies (golden structures, every ninth record of large_assemblies.json, the degenerate ones), the certificate probes
    (tipping, sliding, mu = 0, densities, fixed sets) and the capacity edges (coincident cubes, the LDS limit);
  * a restatement of the detector in the kernel's loop order and of the certificate, each with switches for the defective twins;
  * the bounds of the certificate, derived beside ``LP_VERIFY_TOL``.
"""
import functools
import json
import math
import os

import numpy as np

from oracle.geometry import Block, create_block
from oracle.rbe import (AMIN, FEAS_TOL, S_MAX, TOL_COPLANAR, TOL_PARALLEL, equilibrium_system, face_pair_contact,
                        find_interfaces, infeasibility, is_stable_rbe_penalty)
from oracle.shapes import edge_frame, get_shape

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# compiled limits of the library (include/bridges_hip.h, csrc/rbe_device.h), restated
MAXV, MAX_BLOCKS, MAX_IF, WAVE = 6, 16, 64, 64
LP_MAX_COLS = 4 * MAX_IF
LP_TAB_LDS = 2048
LP_VERIFY_TOL = 1e-4
FLOOR_HW, FLOOR_DEPTH = 5.0, 10.0                    # oracle.rbe.floor_body of the default bounds
BOUNDS = ((-3.0, -3.0, -1.0), (7.0, 7.0, 9.0))
TABLE = ("trapezoid", "hexagon", "cube", "cube06")   # the shape table every probe is launched with
TOP = dict(cube=3, cube06=3, hexagon=4, trapezoid=1)     # face whose outward normal is +z in the local frame
BOTTOM = dict(cube=0, cube06=0, hexagon=0, trapezoid=3)  # ... -z
U = 2.0 ** -53
GAP = (1e-6, 1e-4)                                   # x density: no oracle optimum of a probe may lie in between


class Posed:
    """What find_interfaces and equilibrium_system read of a block, with hand-written world vertices.  ``pose`` is what the
    kernel takes the centroid from (pose position + rotated local centroid); a Posed block is never rotated."""

    def __init__(self, shape, verts, pos):
        self.shape = shape
        self.verts = [(float(x), float(z)) for x, z in verts]
        self.frames = [edge_frame(self.verts[a], self.verts[b]) for a, b in shape.faces]
        self.pos, self.cs = (float(pos[0]), float(pos[1])), (1.0, 0.0)
        self.centroid = (self.pos[0] + shape.centroid[0], self.pos[1] + shape.centroid[1])

    @property
    def weight_per_density(self):
        return self.shape.area * self.shape.depth


def pose_of(b):
    return (b.pos[0], b.pos[1], b.cs[0], b.cs[1])


def shape_id(b):
    return TABLE.index(b.shape.name)


# ---- the kernel's order ----------------------------------------------------------------------------------------------

def kernel_order(interfaces):
    """The oracle lists interfaces by (A, B, face A, face B); the kernel appends, block by block, the contacts of the new block B
    with every earlier body A: (B, A, face A, face B).  A stable sort by (B, A) turns one into the other."""
    out = sorted(interfaces, key=lambda it: (it[1], it[0]))
    keys = [(it[1], it[0]) for it in out]
    assert keys == sorted(keys) and len(out) == len(interfaces)
    for pair in set(keys):                                          # within a body pair the oracle's (face A, face B) order stays
        assert [it for it in out if (it[1], it[0]) == pair] == [it for it in interfaces if (it[1], it[0]) == pair]
    assert all(it[0] < it[1] for it in out)
    return out


def contact_words(interfaces):
    """-> (int32 [n,2] body A / body B, float64 [n,8] p_lo.xz, p_hi.xz, n.xz, t.xz): the words of if_body / if_geom."""
    body = np.array([[it[0], it[1]] for it in interfaces], dtype=np.int32).reshape(-1, 2)
    geom = np.array([[it[2][0], it[2][1], it[3][0], it[3][1], it[4][0], it[4][1], it[5][0], it[5][1]] for it in interfaces],
                    dtype=np.float64).reshape(-1, 8)
    return body, geom


def same_words(a, b):
    """Bit equality of two float64 arrays (-0.0 != 0.0, NaN == NaN of the same payload)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def reference_contacts(blocks, bounds=BOUNDS):
    return kernel_order(find_interfaces(blocks, bounds))


# ---- restatement of the detector, in the kernel's loop order, with the defective twins -----------------------------------

DETECTOR_TWINS = ("parallel_ge", "coplanar_ge", "amin_le", "depth_of_a", "depth_max", "project_on_tb", "swap_lo_hi",
                  "normal_of_b", "swap_bodies", "floor_depth_everywhere", "order_ab", "chunk_drop")


def pair_detail(fa, fb, depth_a, depth_b, twin=None):
    """face_pair_contact restated.  -> (category, contact or None, detail) with category in {'parallel', 'coplanar', 'amin',
    'accept'} and detail = dict(lo_from, hi_from, L) once the projections exist."""
    vaA, vbA, (cA, tA, nA) = fa
    vaB, vbB, (cB, tB, nB) = fb
    depth = min(depth_a, depth_b)
    if twin == "depth_of_a":
        depth = depth_a
    elif twin == "depth_max":
        depth = max(depth_a, depth_b)
    elif twin == "floor_depth_everywhere":
        depth = FLOOR_DEPTH
    dotn = nA[0] * nB[0] + nA[1] * nB[1]
    if (dotn >= -1.0 + TOL_PARALLEL) if twin == "parallel_ge" else (dotn > -1.0 + TOL_PARALLEL):
        return "parallel", None, dict(dotn=dotn)
    gap = (cB[0] - cA[0]) * nA[0] + (cB[1] - cA[1]) * nA[1]
    if (abs(gap) >= TOL_COPLANAR) if twin == "coplanar_ge" else (abs(gap) > TOL_COPLANAR):
        return "coplanar", None, dict(dotn=dotn, gap=gap)
    tP = tB if twin == "project_on_tb" else tA

    def proj(v):
        return (v[0] - cA[0]) * tP[0] + (v[1] - cA[1]) * tP[1]

    a0, a1, b0, b1 = proj(vaA), proj(vbA), proj(vaB), proj(vbB)
    lo = max(min(a0, a1), min(b0, b1))
    hi = min(max(a0, a1), max(b0, b1))
    detail = dict(dotn=dotn, gap=gap, a=(a0, a1), b=(b0, b1), lo=lo, hi=hi,
                  lo_from="A" if min(a0, a1) > min(b0, b1) else ("B" if min(b0, b1) > min(a0, a1) else "AB"),
                  hi_from="A" if max(a0, a1) < max(b0, b1) else ("B" if max(b0, b1) < max(a0, a1) else "AB"))
    area = (hi - lo) * depth
    if (area <= AMIN) if twin == "amin_le" else (area < AMIN):
        return "amin", None, detail
    p_lo = (cA[0] + lo * tA[0], cA[1] + lo * tA[1])
    p_hi = (cA[0] + hi * tA[0], cA[1] + hi * tA[1])
    if twin == "swap_lo_hi":
        p_lo, p_hi = p_hi, p_lo
    return "accept", (p_lo, p_hi, nB if twin == "normal_of_b" else nA, tA), detail


def _faces(block):
    return [(block.verts[ia], block.verts[ib], fr) for (ia, ib), fr in zip(block.shape.faces, block.frames)]


FLOOR_FACE = ((-FLOOR_HW, 0.0), (FLOOR_HW, 0.0), ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)))


def detect(blocks, twin=None, lanes=None):
    """append_interfaces for block 0, 1, ..: face pair p = qa * MAXV + fn (qa = 0 the floor, 1 + 6 A + fA otherwise; fn the face of
    the new block), 64 pairs per chunk, hits compacted in p order.  ``lanes``: a list that receives p % 64 of every hit."""
    out = []
    for b, blk in enumerate(blocks):
        fb_all = _faces(blk)
        for qa in range(1 + b * MAXV):
            if qa == 0:
                A, fa, depth_a = -1, FLOOR_FACE, FLOOR_DEPTH
            else:
                A, f = (qa - 1) // MAXV, (qa - 1) % MAXV
                fa_all = _faces(blocks[A])
                if f >= len(fa_all):
                    continue
                fa, depth_a = fa_all[f], blocks[A].shape.depth
            for fn in range(len(fb_all)):
                p = qa * MAXV + fn
                cat, c, _ = pair_detail(fa, fb_all[fn], depth_a, blk.shape.depth, twin)
                if c is None:
                    continue
                if lanes is not None:
                    lanes.append((p % WAVE, p // WAVE))
                if twin == "chunk_drop" and p % WAVE == WAVE - 1:       # the last lane of a chunk loses its hit
                    continue
                out.append(((b, A) if twin == "swap_bodies" else (A, b)) + c)
    if twin == "order_ab":
        out = sorted(out, key=lambda it: (it[0], it[1]))
    return out


def words_equal(got, ref):
    gb, gg = contact_words(got)
    rb, rg = contact_words(ref)
    return np.array_equal(gb, rb) and same_words(gg, rg)


# ---- boundary table: one face pair per assembly ---------------------------------------------------------------------------

KINDS = (("cube", "cube"), ("cube", "cube06"), ("cube06", "cube"), ("floor", "cube"), ("floor", "cube06"),
         ("cube", "hexagon"), ("hexagon", "cube"), ("floor", "hexagon"), ("hexagon", "hexagon"))
Z_TOP = 2.0                                          # body A hangs above the floor: its top face is the only face B can meet


def _face_width(shape, f):
    (ax, az), (bx, bz) = shape.verts[shape.faces[f][0]], shape.verts[shape.faces[f][1]]
    return math.hypot(bx - ax, bz - az)


def widths(kind_a, kind_b):
    wa = 2.0 * FLOOR_HW if kind_a == "floor" else _face_width(get_shape(kind_a), TOP[kind_a])
    return wa, _face_width(get_shape(kind_b), BOTTOM[kind_b])


def pair_row(kind_a, kind_b, x=0.0, gap=0.0, delta=0.0):
    """Body A (or the floor) with its top face at z = Z_TOP (0), body B with its bottom face on it: shifted by x along the face,
    lifted by ``gap`` along the normal, then rotated by ``delta`` about the centre of its bottom face.
    -> (blocks, (face pair A, face pair B, depth A, depth B))."""
    blocks, zc = [], 0.0
    if kind_a != "floor":
        sa = get_shape(kind_a)
        top = sa.verts[sa.faces[TOP[kind_a]][0]][1]
        blocks.append(Posed(sa, [(vx, vz - top + Z_TOP) for vx, vz in sa.verts], (0.0, Z_TOP - top)))
        zc = Z_TOP
    sb = get_shape(kind_b)
    bot = sb.verts[sb.faces[BOTTOM[kind_b]][0]][1]
    vb = [(vx + x, vz - bot + zc + gap) for vx, vz in sb.verts]
    if delta != 0.0:
        ia, ib = sb.faces[BOTTOM[kind_b]]
        cx, cz = (vb[ia][0] + vb[ib][0]) * 0.5, (vb[ia][1] + vb[ib][1]) * 0.5
        c, s = math.cos(delta), math.sin(delta)
        vb = [(cx + (px - cx) * c - (pz - cz) * s, cz + (px - cx) * s + (pz - cz) * c) for px, pz in vb]
    blocks.append(Posed(sb, vb, (x, zc + gap - bot)))
    return blocks


def target_pair(kind_a, kind_b, blocks):
    fb = _faces(blocks[-1])[BOTTOM[kind_b]]
    if kind_a == "floor":
        return FLOOR_FACE, fb, FLOOR_DEPTH, blocks[-1].shape.depth
    return _faces(blocks[0])[TOP[kind_a]], fb, blocks[0].shape.depth, blocks[-1].shape.depth


def oracle_accepts(kind_a, kind_b, **kw):
    blocks = pair_row(kind_a, kind_b, **kw)
    fa, fb, da, db = target_pair(kind_a, kind_b, blocks)
    return face_pair_contact(fa, fb, min(da, db)) is not None


def straddle(pred, a, b):
    """Bisection on the doubles between a and b (pred(a) != pred(b)) -> adjacent doubles (u, v), pred(u) == pred(a),
    pred(v) == pred(b)."""
    pa, pb = pred(a), pred(b)
    assert pa != pb, (a, b, pa)
    while True:
        m = a + (b - a) * 0.5
        if m == a or m == b:
            break
        if pred(m) == pa:
            a = m
        else:
            b = m
    assert b == math.nextafter(a, b) and pred(a) == pa and pred(b) == pb
    return a, b


def thin_rows():
    """(hi - lo) * depth == 0.001 EXACTLY: body B is a 'cube' (depth 1) squeezed to half-width h about the centre of A's top
    face, whose tangent is exactly (1, 0): the projections are -h and h, hi - lo = 2 h without rounding, and 2 * 0.0005 is the
    double 0.001.  The next double below is rejected."""
    rows = []
    for name, h in (("thin_equal", 0.0005), ("thin_below", math.nextafter(0.0005, 0.0)), ("thin_above", math.nextafter(0.0005, 1.0))):
        a = pair_row("cube", "cube")[0]
        cube = get_shape("cube")
        b = Posed(cube, [(-h, Z_TOP), (-h, Z_TOP + 1.0), (h, Z_TOP + 1.0), (h, Z_TOP)], (0.0, Z_TOP + 0.5))
        rows.append(dict(name=name, kinds=("cube", "cube"), blocks=[a, b], group="thin"))
    return rows


@functools.lru_cache(maxsize=None)
def boundary_table():
    """-> list of dict(name, kinds, blocks, group, category, detail, pair=(name of the straddling partner or None))."""
    rows = []

    def add(kinds, group, name, partner=None, **kw):
        rows.append(dict(name=f"{kinds[0]}/{kinds[1]}/{name}", kinds=kinds, blocks=pair_row(*kinds, **kw), group=group,
                         partner=None if partner is None else f"{kinds[0]}/{kinds[1]}/{partner}"))

    for kinds in KINDS:
        wa, wb = widths(*kinds)
        # --- parallelism: B rotated about the centre of its own face
        for d in (0.0, 1e-7, -1e-7, 2e-3, -2e-3):
            add(kinds, "parallel", f"delta={d!r}", delta=d)
        for sgn in (1.0, -1.0):
            u, v = straddle(lambda d: oracle_accepts(*kinds, delta=d), 0.0, sgn * 2e-3)
            add(kinds, "parallel", f"delta_in{sgn:+.0f}", partner=f"delta_out{sgn:+.0f}", delta=u)
            add(kinds, "parallel", f"delta_out{sgn:+.0f}", partner=f"delta_in{sgn:+.0f}", delta=v)
        # --- coplanarity: a gap along the normal
        for sgn in (1.0, -1.0):
            u, v = straddle(lambda g: oracle_accepts(*kinds, gap=g), 0.0, sgn * 2e-6)
            add(kinds, "coplanar", f"gap_in{sgn:+.0f}", partner=f"gap_out{sgn:+.0f}", gap=u)
            add(kinds, "coplanar", f"gap_out{sgn:+.0f}", partner=f"gap_in{sgn:+.0f}", gap=v)
        # --- overlap: L * min(depth) straddles 0.001 on either side (lo from B and hi from A on the right, the reverse on the left)
        touch = (wa + wb) * 0.5
        for sgn in (1.0, -1.0):
            u, v = straddle(lambda x: oracle_accepts(*kinds, x=x), sgn * (touch - 0.05), sgn * touch)
            add(kinds, "overlap", f"x_in{sgn:+.0f}", partner=f"x_out{sgn:+.0f}", x=u)
            add(kinds, "overlap", f"x_out{sgn:+.0f}", partner=f"x_in{sgn:+.0f}", x=v)
        add(kinds, "overlap", "contained", x=0.0625 if wa != wb else 0.0)     # the narrower face inside the wider one
        add(kinds, "overlap", "shared_vertex", x=touch)
        add(kinds, "overlap", "disjoint", x=touch + 0.25)
    rows += [dict(r, name="cube/cube/" + r["name"], partner=None) for r in thin_rows()]
    for r in rows:
        fa, fb, da, db = (target_pair(r["kinds"][0], r["kinds"][1], r["blocks"]))
        r["category"], _, r["detail"] = pair_detail(fa, fb, da, db)
        r["reference"] = reference_contacts(r["blocks"])
    return rows


# ---- assemblies ---------------------------------------------------------------------------------------------------------------

def _case(name, blocks, fixed, mu=0.8, density=1.0, mask_extra=0, tags=()):
    return dict(name=name, blocks=list(blocks), fixed=set(fixed), mu=float(mu), density=float(density),
                mask_extra=int(mask_extra), tags=set(tags))


def fixed_mask(case):
    return (sum(1 << b for b in case["fixed"]) | case["mask_extra"]) & 0xFFFFFFFF


def structure_blocks(name, structs=None):
    st = (structs or json.load(open(os.path.join(GOLDEN, "structures.json"))))[name]
    shapes = [get_shape(s) for s in st["shapes"]]
    blocks = []
    for a in st["actions"]:
        blocks.append(create_block(shapes, blocks, a[:6]))
    return blocks


STRUCTURES = ("hexagon", "trapezoid_bridge", "hexagon_bridge_3", "hexagon_bridge_5", "horizontal_bridge", "tower", "levitating_block")


def record_blocks(r):
    shapes = [get_shape(n) for n in r["shapes"]]
    return [Block(shapes[s], (p[0], p[1]), (p[2], p[3])) for s, p in zip(r["shape_ids"], r["poses"])]


def cubes(xs, lift=0.0):
    cube = get_shape("cube")
    return [Block(cube, (float(x), 0.5 + lift)) for x in xs]


def incline_pair():
    """A trapezoid resting with its long face on the right incline of a fixed trapezoid, shifted up the slope so that its weight
    passes through the contact: whether it stays is decided by friction alone, at mu = tan(theta)."""
    trap = get_shape("trapezoid")
    base = create_block([trap], [], (-1, 0, 0, 3, 0.0, 0.0))
    n = base.frames[2][2]
    tan_theta = abs(n[0] / n[1])
    out = []
    for ox in (0.5, -0.5):
        top = create_block([trap], [base], (0, 2, 0, 3, ox, 0.0))
        out.append(([base, top], tan_theta))
    return out


@functools.lru_cache(maxsize=None)
def assembly_cases():
    """Every assembly the contact list and the certificate are checked on, as dict(name, blocks, fixed, mu, density, mask_extra,
    tags)."""
    cases = []
    structs = json.load(open(os.path.join(GOLDEN, "structures.json")))
    for name in STRUCTURES:
        blocks = structure_blocks(name, structs)
        for k in range(1, len(blocks) + 1):
            for fixed in (set(), {k - 1}):
                cases.append(_case(f"{name}[:{k}]/fixed={sorted(fixed)}", blocks[:k], fixed, tags={"structure"}))
    fixture = json.load(open(os.path.join(GOLDEN, "large_assemblies.json")))
    for i, r in list(enumerate(fixture))[::9]:
        blocks = record_blocks(r)
        for c in r["cases"]:
            cases.append(_case(f"large[{i}]/fixed={c['fixed']}", blocks, c["fixed"], mu=r["mu"], tags={"large"}))
    cases.append(_case("empty", [], set(), tags={"degenerate"}))
    cases.append(_case("levitating_cube", cubes([0.0], lift=2.5), set(), tags={"degenerate"}))
    cases.append(_case("levitating_cube/fixed", cubes([0.0], lift=2.5), {0}, tags={"degenerate"}))
    cases.append(_case("cube+levitating_cube", cubes([0.0]) + cubes([2.0], lift=2.5), set(), tags={"degenerate"}))
    # --- certificate probes
    for d in TIP_OFFSETS:
        cases.append(_case(f"tipping/d={d!r}", [Block(get_shape("cube"), (0.0, 0.5)), Block(get_shape("cube"), (0.5 + d, 1.5))], {0},
                           tags={"tipping"}))
    (blocks, tan_theta) = sliding_pair()
    r = sliding_r()
    for sgn in (1.0, -1.0):
        cases.append(_case(f"sliding/mu=tan(1{sgn:+.0f}*{r!r})", blocks, {0}, mu=tan_theta * (1.0 + sgn * r), tags={"sliding"}))
    for name in ("tower", "trapezoid_bridge", "hexagon_bridge_3"):
        blocks = structure_blocks(name, structs)
        cases.append(_case(f"{name}/mu=0", blocks, set(), mu=0.0, tags={"mu0"}))
        cases.append(_case(f"{name}/mu=0/fixed=last", blocks, {len(blocks) - 1}, mu=0.0, tags={"mu0"}))
    cases.append(_case("sliding/mu=0", blocks_of_sliding(), {0}, mu=0.0, tags={"mu0"}))
    # --- fixed sets: none / last are everywhere above; all, and masks with bits at or above n_blocks
    for name in ("trapezoid_bridge", "hexagon_bridge_5", "tower"):
        blocks = structure_blocks(name, structs)
        n = len(blocks)
        cases.append(_case(f"{name}/fixed=all", blocks, set(range(n)), tags={"fixedsets"}))
        cases.append(_case(f"{name}/fixed=none+high", blocks, set(), mask_extra=(0xFFFFFFFF << n), tags={"fixedsets"}))
        cases.append(_case(f"{name}/fixed=last+high", blocks, {n - 1}, mask_extra=(1 << 31) | (1 << n), tags={"fixedsets"}))
    # --- densities, on the certificate probes and three structures
    base = [c for c in cases if c["tags"] & {"tipping", "sliding"}]
    base += [c for c in cases if c["name"] in ("trapezoid_bridge[:9]/fixed=[8]", "hexagon_bridge_5[:5]/fixed=[]", "tower[:10]/fixed=[]")]
    for c in base:
        for dens in (1e-3, 1e3):
            cases.append(dict(c, name=f"{c['name']}/density={dens!r}", density=dens, tags=c["tags"] | {"density"}, twin_of=c["name"]))
    return cases


TIP_OFFSETS = (-1e-2, -1e-3, 1e-3, 1e-2)


@functools.lru_cache(maxsize=None)
def sliding_pair():
    """The incline pair that holds at mu = 3 (the up-slope shift; the other one tips whatever the friction)."""
    ok = [(blocks, tan_theta) for blocks, tan_theta in incline_pair() if oracle_v(blocks, {0}, 3.0, 1.0)[1] < GAP[0]]
    assert len(ok) == 1
    return ok[0]


def blocks_of_sliding():
    return sliding_pair()[0]


R_LADDER = tuple(2.0 ** -k for k in range(1, 24))


@functools.lru_cache(maxsize=None)
def sliding_r():
    """The smallest r of the ladder 2**-k for which the oracle's optimum stays outside the gap on both sides of tan(theta)."""
    blocks, tan_theta = sliding_pair()

    def outside(r):
        return (oracle_v(blocks, {0}, tan_theta * (1.0 - r), 1.0)[1] > GAP[1]
                and oracle_v(blocks, {0}, tan_theta * (1.0 + r), 1.0)[1] < GAP[0])
    good = [r for r in R_LADDER if outside(r)]
    return min(good)


def oracle_v(blocks, fixed, mu, density):
    """-> (interfaces in the kernel's order, v*): is_stable_rbe's decision quantity (None -> no interface: 0 iff nothing is free)."""
    fixed = {b for b in fixed if 0 <= b < len(blocks)}
    itf = reference_contacts(blocks)
    n_free = len(blocks) - len(fixed)
    if not itf:
        return itf, (0.0 if n_free == 0 else math.inf)
    M, w = equilibrium_system(blocks, itf, fixed, mu, density)
    return itf, infeasibility(M, w, S_MAX * density)


_ORACLE = {}


def oracle_of(case, tols=()):
    """Cached oracle results of a case: interfaces (kernel order), v, stable, and per tension tolerance the penalty optimum and
    boolean."""
    key = case["name"]
    o = _ORACLE.get(key)
    if o is None:
        itf, v = oracle_v(case["blocks"], case["fixed"], case["mu"], case["density"])
        o = _ORACLE[key] = dict(interfaces=itf, v=v, stable=v <= FEAS_TOL * case["density"], pen={})
    for tol in tols:
        if tol not in o["pen"]:
            fixed = {b for b in case["fixed"] if 0 <= b < len(case["blocks"])}
            if tol == 0.0:
                o["pen"][tol] = (o["stable"], o["v"])
            elif not o["interfaces"] or len(fixed) == len(case["blocks"]):
                o["pen"][tol] = (len(fixed) == len(case["blocks"]), o["v"])
            else:
                st, info = _penalty(case["blocks"], fixed, case["mu"], case["density"], tol)
                o["pen"][tol] = (st, info)
    return o


def _penalty(blocks, fixed, mu, density, tol):
    """is_stable_rbe_penalty and its optimum (one LP: return_info=True would solve a second one for the minimum tension)."""
    from scipy.optimize import linprog
    itf = find_interfaces(blocks, BOUNDS)
    M, w = equilibrium_system(blocks, itf, fixed, mu, density)
    N = tension_columns(blocks, itf, fixed)
    m, n, nt = M.shape[0], M.shape[1], N.shape[1]
    s_max = S_MAX * density
    res = linprog(np.concatenate([np.zeros(n + nt), np.ones(2 * m)]), A_eq=np.hstack([M, N, np.eye(m), -np.eye(m)]), b_eq=w,
                  A_ub=np.concatenate([np.ones(n), np.full(nt, s_max / tol), np.zeros(2 * m)])[None, :], b_ub=[s_max],
                  bounds=(0, None), method="highs")
    assert res.status == 0
    v = float(res.fun)
    st = v <= FEAS_TOL * density
    assert st == is_stable_rbe_penalty(blocks, fixed, mu, density, tol, BOUNDS)      # the restated LP is the oracle's
    return st, v


def tension_columns(blocks, interfaces, fixed):
    """The tension columns of is_stable_rbe_penalty: one per contact point, a force along -n on B (and +n on A)."""
    free = [i for i in range(len(blocks)) if i not in fixed]
    row = {b: 3 * k for k, b in enumerate(free)}
    N = np.zeros((3 * len(free), 2 * len(interfaces)))
    for k, (A, B, p_lo, p_hi, nrm, _t) in enumerate(interfaces):
        for ip, p in enumerate((p_lo, p_hi)):
            for body, sign in ((B, -1.0), (A, 1.0)):
                if body in row:
                    r = row[body]
                    gx, gz = sign * nrm[0], sign * nrm[1]
                    cx, cz = blocks[body].centroid
                    N[r, 2 * k + ip] += gx
                    N[r + 1, 2 * k + ip] += gz
                    N[r + 2, 2 * k + ip] += (p[0] - cx) * gz - (p[1] - cz) * gx
    return N


# ---- capacity edges ---------------------------------------------------------------------------------------------------------

def coincident_cubes(order, lift=0.0):
    """Cubes on the floor at x = 0 ('L') and x = 1 ('R'), in the given order: every L touches every R (and the floor)."""
    return cubes([0.0 if c == "L" else 1.0 for c in order], lift)


# (4, 12): block 3 is an R and block 4 an L, so their pair is p = (1 + 18 + 2) * 6 + 1 = 127: the LAST lane of a chunk
ORDER_64 = "RRRRLLLLRRRRRRRR"
ORDER_80 = "RLRLRLRLLRLRLRLR"
ORDER_42 = "LLLLLLRRRRRRR"


@functools.lru_cache(maxsize=None)
def capacity_cases():
    c64 = _case("cubes4x12", coincident_cubes(ORDER_64), set(), tags={"capacity"})
    c80 = _case("cubes8x8", coincident_cubes(ORDER_80), set(), tags={"capacity"})
    c42 = _case("lifted6x7", coincident_cubes(ORDER_42, lift=1.0), set(), tags={"capacity"})
    # 43: a 14th cube, on the floor and away from the others (coincident cubes share every face, so nothing can touch one of
    # them alone: the extra interface is the new cube's own floor contact)
    c43 = _case("lifted6x7+1", coincident_cubes(ORDER_42, lift=1.0) + cubes([3.0]), set(), tags={"capacity"})
    return dict(c64=c64, c80=c80, c42=c42, c43=c43)


def lp_cells(n_free, n_if, n_tens=0):
    """lp_dims of csrc/rbe_device.h: (3 n_free + 2) rows x an odd stride of 4 n_if + 2 n_tens + 2 columns."""
    stride = 4 * n_if + 2 * n_tens + 2
    if stride % 2 == 0:
        stride += 1
    return (3 * n_free + 2) * stride


@functools.lru_cache(maxsize=None)
def lds_pair():
    """One fixture assembly whose tableau fits the 2048-double LDS area with the last block fixed and does not with nothing
    fixed.  -> (case last fixed, case nothing fixed)."""
    fixture = json.load(open(os.path.join(GOLDEN, "large_assemblies.json")))
    # a record whose LDS-side verdict is 'stable' first: that one has an equilibrium to certify (no record is stable on both sides)
    for i, r in sorted(enumerate(fixture), key=lambda ir: not any(c["stable"] for c in ir[1]["cases"])):
        nb, n_if = len(r["poses"]), r["cases"][0]["n_if"]
        if lp_cells(nb - 1, n_if) <= LP_TAB_LDS < lp_cells(nb, n_if):
            blocks = record_blocks(r)
            a = _case(f"lds[{i}]/fixed=last", blocks, {nb - 1}, mu=r["mu"], tags={"lds"})
            b = _case(f"lds[{i}]/fixed=none", blocks, set(), mu=r["mu"], tags={"lds"})
            if all(not (GAP[0] < oracle_of(c)["v"] < GAP[1]) for c in (a, b)):
                return a, b
    raise AssertionError("no fixture record straddles the LDS limit")


# ---- the certificate ----------------------------------------------------------------------------------------------------------

CERT_TWINS = ("moment_about_pose", "friction_flip_second", "tension_along_n")
TENSION_TOLS = (0.0, 1e-3, 50.0)

# Bounds, derived (u = 2**-53, first order).
#
# Balance.  lp_verify accepts a verdict when the L1 residual of the equilibrium rows, evaluated by the kernel from the contact
# list as  acc_i = sum_j coef_ij x_j  (coef_ij built in <= 6 rounded operations: mu * t, n +- mu t, p - g, two products and a
# difference for a moment; one product and one addition per term), is at most LP_VERIFY_TOL * density.  The test evaluates the
# same rows from (c_np, c_nn, f_t) = (a + b, t, mu (a - b)) -- the kernel's outputs, one rounding each -- as
# c_np n + f_t t - c_nn n, again <= 6 rounded operations per term and one addition per term.  Either evaluation of row i with
# T_i terms therefore differs from the exact value of the row at the kernel's x by at most (T_i + 8) u A_i, where
# A_i = sum_j |coef_ij| |x_j| + |w_i| is the row's absolute sum (majorised below with |n| + mu |t| for a generator and the
# absolute lever arms); the two differ by at most twice that.  BALANCE_OPS = 8 covers the six operations, the rounding of the
# kernel's outputs and the final subtraction of the weight.
BALANCE_OPS = 8


def balance_rounding(abs_sum, terms):
    return 2.0 * (terms + BALANCE_OPS) * U * abs_sum


def balance_bound(density, abs_sum, terms):
    return LP_VERIFY_TOL * density + balance_rounding(abs_sum, terms)


# Cone.  a, b >= 0 are clipped basic values, so c_np = fl(a + b) >= 0 and c_nn >= 0 hold exactly.  |f_t| = fl(mu fl(a - b)) <=
# mu |a - b| (1 + u)^2 and mu c_np >= mu (a + b)(1 - u) (1 - u) once the test's own product is counted: |f_t| - mu c_np <=
# 4 u mu c_np.
def cone_slack(mu, cnp):
    return 4.0 * U * mu * cnp


# Budget.  sum c_np + (S_MAX density / tol) sum c_nn <= S_MAX density (the oracle's budget row, is_stable_rbe_penalty; at
# density 1 the coefficient is S_MAX / tol).  When the tension budget binds, the slack of this row is non-basic and the row holds
# with equality in exact arithmetic, so its rounding decides the sign.  The tension t of a contact point is a basic value: it is
# fixed by the equilibrium rows, whose coefficients are O(1), and is therefore known only to the absolute precision those rows
# have -- the rounding term R = 2 (T + 8) u A of the balance above (A = the rows' absolute sum, a force).  The budget row
# multiplies it by C = S_MAX density / tol (1e7 at tol = 1e-3): the row is determined to C R and no solver in binary64 can do
# better.  (A first version of this bound counted u S_MAX density per pivot and entry and overlooked C; the kernel's tension on
# trapezoid_bridge[:4], last block fixed, tol = 1e-3 is 1.5e-15 above the row: 1.5e-8 in the row's units, 1.5e-12 of S_MAX.)
# Evaluating the row itself costs one rounding per term on a running sum of at most the row's value V: (6 n_if + 8) u V.
def budget_slack(coef, rounding, n_if, value):
    return max(coef, 1.0) * rounding + (6.0 * n_if + BALANCE_OPS) * U * value


def certificate(blocks, interfaces, fixed, mu, density, tol, forces, twin=None):
    """forces [n_if, 2, 3] = (c_np, c_nn, f_t) per contact point -> dict of the figures the certificate asserts on.
    Contact point force on B:  c_np n + f_t t - c_nn n;  its negative on A."""
    n_if = len(interfaces)
    forces = np.asarray(forces, dtype=np.float64).reshape(n_if, 2, 3)
    free = [b for b in range(len(blocks)) if b not in fixed]
    acc = {b: [0.0, 0.0, 0.0] for b in free}
    mag = {b: [0.0, 0.0, 0.0] for b in free}
    terms = {b: 0 for b in free}
    for k, (A, B, p_lo, p_hi, n, t) in enumerate(interfaces):
        for ip, p in enumerate((p_lo, p_hi)):
            cnp, cnn, ft = (float(v) for v in forces[k, ip])
            if twin == "friction_flip_second" and ip == 1:
                ft = -ft
            tens = cnn if twin == "tension_along_n" else -cnn
            fx = cnp * n[0] + ft * t[0] + tens * n[0]
            fz = cnp * n[1] + ft * t[1] + tens * n[1]
            ax = (cnp + cnn) * abs(n[0]) + abs(ft) * abs(t[0])
            az = (cnp + cnn) * abs(n[1]) + abs(ft) * abs(t[1])
            for body, sign in ((B, 1.0), (A, -1.0)):
                if body in acc:
                    cx, cz = blocks[body].pos if twin == "moment_about_pose" else blocks[body].centroid
                    rx, rz = p[0] - cx, p[1] - cz
                    acc[body][0] += sign * fx
                    acc[body][1] += sign * fz
                    acc[body][2] += sign * (rx * fz - rz * fx)
                    mag[body][0] += ax
                    mag[body][1] += az
                    mag[body][2] += abs(rx) * az + abs(rz) * ax
                    terms[body] += 3                         # c_np, c_nn, f_t: up to three kernel columns' worth per point
    residual, abs_sum, n_terms = 0.0, 0.0, 0
    for b in free:
        w = density * blocks[b].weight_per_density
        residual += abs(acc[b][0]) + abs(acc[b][1] - w) + abs(acc[b][2])
        abs_sum += mag[b][0] + mag[b][1] + mag[b][2] + abs(w)
        n_terms = max(n_terms, terms[b])
    cnp, cnn, ft = forces[:, :, 0], forces[:, :, 1], forces[:, :, 2]
    coef = S_MAX * density / tol if tol > 0.0 else 0.0
    budget = float(cnp.sum()) + (coef * float(cnn.sum()) if tol > 0.0 else 0.0)
    rounding = balance_rounding(abs_sum, n_terms)
    return dict(residual=residual, residual_bound=balance_bound(density, abs_sum, n_terms),
                min_cnp=float(cnp.min()) if n_if else 0.0, min_cnn=float(cnn.min()) if n_if else 0.0,
                max_cnn=float(cnn.max()) if n_if else 0.0,
                cone_excess=float((np.abs(ft) - mu * cnp - cone_slack(mu, cnp)).max()) if n_if else -0.0,
                budget=budget, budget_bound=S_MAX * density + budget_slack(coef, rounding, n_if, budget))


def certificate_ok(c, tol):
    return (c["residual"] <= c["residual_bound"] and c["min_cnp"] >= 0.0 and c["min_cnn"] >= 0.0 and c["cone_excess"] <= 0.0
            and c["budget"] <= c["budget_bound"] and (tol > 0.0 or c["max_cnn"] == 0.0))


def clean_equilibrium(case, tol, seed=0):
    """An equilibrium of the oracle's system found by HiGHS (a random linear objective over a budget of 100 x density, so that
    friction and -- with tol > 0 -- tension are in use): forces [n_if, 2, 3] in the kernel's layout, or None when there is none."""
    from scipy.optimize import linprog
    blocks, fixed, mu, density = case["blocks"], {b for b in case["fixed"] if b < len(case["blocks"])}, case["mu"], case["density"]
    itf = oracle_of(case)["interfaces"]
    if not itf or len(fixed) == len(blocks):
        return None
    M, w = equilibrium_system(blocks, itf, fixed, mu, density)
    n = M.shape[1]
    cols, budget = [M], [np.ones(n)]
    if tol > 0.0:
        N = tension_columns(blocks, itf, fixed)
        cols.append(N)
        budget.append(np.full(N.shape[1], S_MAX * density / tol))
    A = np.hstack(cols)
    rng = np.random.default_rng(seed)
    cost = rng.uniform(-1.0, 1.0, A.shape[1])
    cost[n:] = -np.abs(cost[n:])                                    # tension is rewarded: the tension twin must meet some
    res = linprog(cost, A_eq=A, b_eq=w, A_ub=np.stack([np.concatenate(budget), np.concatenate([np.ones(n), np.zeros(A.shape[1] - n)])]),
                  b_ub=[0.5 * S_MAX * density, 100.0 * density], bounds=(0, None), method="highs")   # half the budget: HiGHS' own 1e-7 stays inside
    if res.status != 0:
        return None
    x = np.maximum(res.x, 0.0)
    forces = np.zeros((len(itf), 2, 3))
    for k in range(len(itf)):
        for ip in range(2):
            a, b = x[4 * k + 2 * ip], x[4 * k + 2 * ip + 1]
            forces[k, ip] = (a + b, x[n + 2 * k + ip] if tol > 0.0 else 0.0, mu * (a - b))
    return forces
