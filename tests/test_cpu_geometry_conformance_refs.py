"""CPU: the probes, references, bound and twins of tests/geometry_conformance.py checked without a GPU.

* The probe tables reach what they are built to reach: every branch of ``align``, sample points exactly on edges at every image
  size, empty, full and single-pixel rasters, scenes whose hits lie in one tile only, vertices on either side of the 1e-6 bounds.
* The numpy restatements the twins are built from reproduce oracle/geometry.py, oracle/shapes.py and oracle/raster.py bit for bit
  on every probe row, and the shape table the library uploads is the oracle's.
* ``lin_bound`` holds for the float64 restatement of the kernel's own summation.
* Every defective twin is rejected by the acceptance function on the probe alone (``-s`` prints where and how often)."""
import numpy as np
import pytest

import geometry_conformance as Q
from oracle import geometry as G
from oracle import raster as R


def test_shape_table_of_the_library_is_the_oracles():
    from bridges_hip.shapes import load_urdf
    for si, name in enumerate(Q.SHAPE_NAMES):
        g, s = load_urdf(f"shapes/{name}.urdf"), Q.SHAPES[si]
        assert g.verts == s.verts and g.faces == s.faces, name
        st, nv = g.to_struct(), len(s.verts)
        assert st.nv == nv
        assert Q.same_bits(np.array([st.fcx[:nv], st.fcz[:nv]]).T, Q.FC[si, :nv]), name
        assert Q.same_bits(np.array([st.fnx[:nv], st.fnz[:nv]]).T, Q.FN[si, :nv]), name
        assert Q.same_bits(np.array([st.vx[:nv], st.vz[:nv]]).T, Q.VLOC[si, :nv]), name


# ---------------------------------------------------------------------------------------------------------------------------
# K1

def test_placement_probe_takes_every_branch_of_align():
    P = Q.placement_probe()
    assert set(P["shape"]) == set(P["target_shape"]) == set(range(5)) and int((P["target_face"] < 0).sum()) == 22 * 8
    br = Q.place_branches(Q.place_reference())
    print("align branches on the bridges_place table:", br)
    assert br["clamp_hi"] >= 1 and br["clamp_lo"] >= 1
    assert br["band"] >= 20
    assert br["negative"] >= 1000 and br["non_negative"] >= 1000
    n = len(P["shape"])                                     # create_block's own rows: posed targets, so no clamp, but the band
    own = Q.place_branches({k: Q.place_reference()[k][:n] for k in ("c_raw", "cy")})
    assert own["clamp_hi"] == own["clamp_lo"] == 0 and own["band"] >= 20


def test_k1_restatements_reproduce_the_oracle():
    P, ref, place, cref = Q.place_probe(), Q.place_reference(), Q.placement_probe(), Q.placement_reference()
    assert Q.accept_place(Q.place_np(P), ref)
    assert Q.same_bits(Q.frames_np(P["shape"], ref["verts"]), ref["frames"])
    n = len(place["shape"])
    # create_block = align on the target's face frame: the same rows through both oracle entries
    for k in ("pose", "verts", "frames"):
        assert Q.same_bits(cref[k], ref[k][:n]), k
    on_block = place["target_face"] >= 0
    fr = Q.frames_np(place["target_shape"], cref["target_verts"])[np.arange(n), np.maximum(place["target_face"], 0)]
    assert Q.same_bits(fr[on_block], cref["frame1"][on_block])
    assert Q.same_bits(cref["frame1"][~on_block], np.tile(np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 1.0]]), (int((~on_block).sum()), 1)))
    assert Q.same_bits(Q.pose_np(place["target_shape"], place["target_pose"])[on_block], cref["target_verts"][on_block])
    # one row spelled out against oracle.geometry.create_block
    i = 12345
    tb = G.Block(Q.SHAPES[place["target_shape"][i]], place["target_pose"][i, :2], place["target_pose"][i, 2:])
    b = G.create_block(Q.SHAPES, [tb], (0, int(place["target_face"][i]), int(place["shape"][i]), int(place["face"][i]),
                                        place["ox"][i], place["oy"][i]))
    assert Q.same_bits(np.array(b.verts), cref["verts"][i, :len(b.verts)])


@pytest.mark.parametrize("twin", sorted(Q.PLACE_TWINS))
def test_defective_k1_twins_are_rejected(twin):
    P, ref = Q.place_probe(), Q.place_reference()
    pose, verts = Q.place_np(P, **Q.PLACE_TWINS[twin])
    rows = int(((pose.view(np.uint64) != ref["pose"].view(np.uint64)).any(1)
                | (verts.view(np.uint64) != ref["verts"].view(np.uint64)).any((1, 2))).sum())
    print(f"twin {twin}: rejected, {rows} of {len(pose)} rows differ")
    assert not Q.accept_place((pose, verts), ref) and rows >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# rasters

@pytest.mark.parametrize("S", Q.RASTER_SIZES)
def test_raster_probe_conditions(S):
    probe, ref = Q.raster_probe(S), Q.raster_reference(S)
    assert len(probe["wide"]["sid"]) == 110 and set(probe["wide"]["sid"]) == set(range(5))
    zero = near = 0
    for g in probe.values():
        for i, si in enumerate(g["sid"]):
            z, m = Q.near_edge_counts(g["verts"][i], int(si), g["X"], g["Y"])
            zero, near = zero + z, near + m
    count = np.concatenate([Q.unpack(w).sum((1, 2)) for w in ref.values()])
    tight = Q.unpack(ref["tight"]).sum((1, 2))
    print(f"S={S}: d == 0 at {zero} sample points, 0 < |d| < 1e-15 at {near}, {int((count == 0).sum())} empty, "
          f"{int((count == S * S).sum())} full, {int((count == 1).sum())} single-pixel rasters of {len(count)}")
    assert zero >= 50
    assert int((count == 0).sum()) >= 1
    assert int((tight[:4] == S * S).all()) and int((count == S * S).sum()) >= 1     # the cube at 0, pi (and +-pi/2): prefix and suffix runs
    assert int((count == 1).sum()) >= 1
    for name, g in probe.items():                                                    # the restatement is contains_2d
        assert Q.accept_words(Q.raster_words(g, Q.pixels_np), ref[name]), name
        assert not Q.unpack(ref[name])[:, S:, :].any() and not Q.unpack(ref[name])[:, :, S:].any()


@pytest.mark.parametrize("twin", sorted(Q.RASTER_TWINS))
def test_defective_raster_twins_are_rejected(twin):
    fn = Q.RASTER_TWINS[twin]
    for S in Q.RASTER_SIZES:
        if twin == "beyond_S_not_cleared" and S == 64:
            continue                                                                 # nothing lies beyond a 64 x 64 image
        probe, ref = Q.raster_probe(S), Q.raster_reference(S)
        got = {name: fn(g, S) for name, g in probe.items()}
        outlines = sum(int((got[k] != ref[k]).any(1).sum()) for k in ref)
        pixels = sum(int(Q.unpack(got[k] ^ ref[k]).sum()) for k in ref)
        print(f"twin {twin}: S={S} rejected, {outlines} outlines / {pixels} pixels differ")
        assert not all(Q.accept_words(got[k], ref[k]) for k in ref), (twin, S)


def test_point_probe():
    cases = Q.point_probe()
    assert len(cases) == 25 and {si for _, si, *_ in cases} == set(range(5))
    corners = []
    for row, si, pts, gx, gz in cases:
        assert len(pts) >= max(Q.POINT_N)
        want = Q.contains_points_ref(row, si, pts)
        nv = int(Q.NV[si])
        assert want[nv:2 * nv].all()                                                  # an edge midpoint has d == 0 on its own face: inside
        corners += [int(want[:nv].sum()), nv]                                         # a vertex sits on two faces, either way by an ulp
        grid = R.contains_2d(Q.outline(row, si), gx, gz)                              # [64 (z), 64 (x)], as the probe's meshgrid
        assert np.array_equal(want[4 * nv:].reshape(64, 64), grid)
        assert 0 < int(grid.sum()) < grid.size
        assert want[2 * nv:4 * nv].any() and not want[2 * nv:4 * nv].all()            # an ulp out / an ulp in along the normal
    print(f"point probe: {sum(corners[0::2])} of {sum(corners[1::2])} vertices test inside")
    assert 0 < sum(corners[0::2]) < sum(corners[1::2])


# ---------------------------------------------------------------------------------------------------------------------------
# scenes

def test_scene_probe_and_render_twins():
    rejected = {k: 0 for k in Q.RENDER_TWINS}
    last_only = first_tile_empty = False
    for case in Q.scene_cases():
        n, W, H, miss = case
        verts, sid, X, Y = Q.scene_of(*case)
        want = Q.render_reference(verts, sid, X, Y)
        assert want.shape == (H, W) and np.array_equal(Q.render_np(verts, sid, X, Y), want)
        if W == H and n:                                                              # the oracle's own (square) renderer
            blocks = [Q.outline(verts[i], int(sid[i])) for i in range(n)]
            assert np.array_equal(R.render_blocks_2d(blocks, Q.XLIM, Q.YLIM, (W, H)).astype(np.uint8), want)
        if n > Q.RENDER_TILE:
            without_last = Q.render_np(verts, sid, X, Y, skip=n - 1)
            last_only |= bool((want != without_last).any())       # the last outline of the last tile is some pixels' only hit
        if miss:
            first_tile_empty |= not Q.render_reference(verts[:16], sid[:16], X, Y).any() and bool(want.any())
        for k, kw in Q.RENDER_TWINS.items():
            rejected[k] += int(not np.array_equal(Q.render_np(verts, sid, X, Y, **kw), want))
    print("render twins rejected on", rejected, "of", len(Q.scene_cases()), "scenes")
    assert last_only and first_tile_empty
    assert all(v >= 1 for v in rejected.values())
    # n = 17: outline 16, the last of the last tile, is the only hit of some pixels
    verts, sid, X, Y = Q.scene_of(17, 64, 64, False)
    assert (Q.render_reference(verts, sid, X, Y) != Q.render_reference(verts[:16], sid[:16], X, Y)).any()


# ---------------------------------------------------------------------------------------------------------------------------
# candidates

def mask_cases():
    groups, words = Q.candidate_probe(), Q.candidate_words()
    for name, state, obstacle in Q.occupancy_cases():
        yield "wide/" + name, groups["wide"], words["wide"], state, obstacle
    yield "low/both_null", groups["low"], words["low"], None, None


def test_candidate_probe_conditions():
    groups, words = Q.candidate_probe(), Q.candidate_words()
    m = Q.mask_np(groups["wide"], words["wide"])
    assert m[110:].tolist() == [1, 0] * 4                    # on the 1e-6 bound: in; one ulp further out: not
    assert Q.mask_np(groups["low"], words["low"]).tolist() == [1, 0, 0, 0, 0, 1]
    assert 20 <= int(m.sum()) <= len(m) - 20
    base = Q.mask_np(groups["wide"], words["wide"])
    shared = {name: int((base != Q.mask_np(groups["wide"], words["wide"], s, o)).sum()) for name, s, o in Q.occupancy_cases()}
    print("candidates refused by the occupancy alone:", shared)
    assert shared["both_null"] == shared["both_none_shared"] == 0
    assert shared["state_only"] >= 1 and shared["obstacle_only"] >= 1 and shared["both_one_shared"] == shared["obstacle_only"]
    for name, s, o in Q.occupancy_cases():                   # "exactly one pixel": the occupancy meets the union of the rasters once
        occ = np.zeros(64, dtype=np.uint64)
        for w in (s, o):
            occ |= w if w is not None else np.uint64(0)
        hits = int((Q.unpack(occ) & Q.unpack(words["wide"]).any(0)).sum())
        assert hits == (0 if name in ("both_null", "both_none_shared") else 1), name


@pytest.mark.parametrize("twin", sorted(Q.MASK_TWINS))
def test_defective_mask_twins_are_rejected(twin):
    where = [name for name, g, w, s, o in mask_cases()
             if not Q.same_bits(Q.mask_np(g, w, s, o, **Q.MASK_TWINS[twin]), Q.mask_np(g, w, s, o))]
    print(f"twin {twin}: rejected on {where}")
    assert where


def test_reward_map_and_lin_bound():
    words, m = Q.candidate_words()["wide"], Q.reward_map()
    union = Q.unpack(words).any(0)
    a = np.abs(m)
    assert a[union].max() < 1e-3 and a[union].min() >= 2e-4 * (1 - 2.0 ** -23) and (m < 0).any() and (m > 0).any()
    beside = np.zeros_like(union)
    beside[:, 1:] |= union[:, :-1]
    beside[:, :-1] |= union[:, 1:]
    beside &= ~union
    assert beside.sum() >= 64 and (a[beside] == 1e6).all() and (a[~union] >= 0.5).all()
    ref = Q.lin_reference(words, m)
    bound = Q.lin_bound(ref, m)
    lin = Q.lin_np(words, Q.reward_prefix(m))
    ratio = np.abs(lin.astype(np.float64) - ref) / bound
    print(f"float64 restatement: largest |lin - R| / bound = {ratio.max():.3g}; bound {bound.min():.3g} .. {bound.max():.3g}")
    assert Q.accept_lin(lin, ref, m)
    assert bound.max() < 2e-4 / 10                           # a sum one pixel short is off by >= 2e-4: the bound cannot hide it
    empty = ~Q.unpack(words).any((1, 2))
    assert empty.any() and (lin[empty] == 0).all() and (ref[empty] == 0).all()


@pytest.mark.parametrize("twin", sorted(Q.LIN_TWINS))
def test_defective_lin_twins_are_rejected(twin):
    words, m = Q.candidate_words()["wide"], Q.reward_map()
    ref = Q.lin_reference(words, m)
    lin = Q.lin_np(words, Q.reward_prefix(m), **Q.LIN_TWINS[twin])
    out = int((np.abs(lin.astype(np.float64) - ref) > Q.lin_bound(ref, m)).sum())
    print(f"twin {twin}: rejected, {out} of {len(lin)} candidates outside the bound")
    assert not Q.accept_lin(lin, ref, m)
    assert 2 * out > int(Q.unpack(words).any((1, 2)).sum())  # (mixed signs: the dropped pixels of a few candidates may cancel)


def test_every_twin_of_the_issue_is_listed():
    names = set(Q.PLACE_TWINS) | set(Q.RASTER_TWINS) | set(Q.RENDER_TWINS) | set(Q.MASK_TWINS) | set(Q.LIN_TWINS)
    assert len(names) == 18


def test_bits_or_probe():
    bits, ranges = Q.bits_or_probe()
    want = Q.bits_or_reference(bits, ranges)
    assert not want[0].any() and not want[3].any() and not want[5].any() and not want[8].any()
    assert np.array_equal(want[1], bits[0]) and np.array_equal(want[4], np.bitwise_or.reduce(bits, axis=0))
