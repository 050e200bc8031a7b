"""No GPU: the probes of tests/stability_conformance.py hold what tests/test_gpu_stability_conformance.py relies on, the
restated detector and certificate agree with oracle/rbe.py, and every defective twin is rejected by the probes alone.
Run with -s for the counts (docs/MEASUREMENT_LOG.md quotes them)."""
import collections
import math

import pytest

import stability_conformance as sc
from oracle.rbe import AMIN


def all_block_lists():
    rows = [(r["name"], r["blocks"], r["reference"]) for r in sc.boundary_table()]
    seen = set()
    for c in list(sc.assembly_cases()) + list(sc.capacity_cases().values()) + list(sc.lds_pair()):
        key = id(c["blocks"][0]) if c["blocks"] else 0, len(c["blocks"])
        if key not in seen:                                      # one row per distinct block list (fixed sets do not matter here)
            seen.add(key)
            rows.append((c["name"], c["blocks"], sc.oracle_of(c)["interfaces"]))
    return rows


def test_restated_detector_equals_the_oracle_in_kernel_order():
    rows = all_block_lists()
    for name, blocks, ref in rows:
        assert sc.words_equal(sc.detect(blocks), ref), name
    print(f"\nrestated detector == oracle (kernel order) on {len(rows)} block lists, "
          f"{sum(len(r[2]) for r in rows)} interfaces")


def test_boundary_table_conditions():
    rows = {r["name"]: r for r in sc.boundary_table()}
    cats = collections.Counter(r["category"] for r in rows.values())
    assert all(cats[c] > 0 for c in ("parallel", "coplanar", "amin", "accept")), cats
    # every straddling pair: adjacent doubles, one accepted and one rejected, the rejection being the boundary's own
    pairs = 0
    for r in rows.values():
        if r["partner"] and "_in" in r["name"]:
            q = rows[r["partner"]]
            assert r["category"] == "accept" and q["category"] == dict(parallel="parallel", coplanar="coplanar", overlap="amin")[r["group"]], (r["name"], q["category"])
            pairs += 1
    assert pairs == 6 * len(sc.KINDS)
    # lo and hi each taken from face A and from face B
    prov = collections.Counter((r["detail"]["lo_from"], r["detail"]["hi_from"]) for r in rows.values() if r["category"] == "accept")
    assert any(k[0] == "A" for k in prov) and any(k[0] == "B" for k in prov), prov
    assert any(k[1] == "A" for k in prov) and any(k[1] == "B" for k in prov), prov
    assert prov[("A", "A")] > 0 and prov[("B", "B")] > 0                        # full containment, either way
    withproj = [r for r in rows.values() if "a" in r["detail"]]
    # a face's own end points project to -L/2, +L/2 on its own tangent (frames come from the edge: a0 > a1 cannot be fed through
    # the entry point); the end points of an anti-parallel face B always arrive reversed, so min / max of B's pair decide
    assert all(r["detail"]["a"][0] < r["detail"]["a"][1] for r in withproj)
    assert all(r["detail"]["b"][0] > r["detail"]["b"][1] for r in withproj)
    shared = [r for r in withproj if r["detail"]["hi"] == r["detail"]["lo"]]
    disjoint = [r for r in withproj if r["detail"]["hi"] < r["detail"]["lo"]]
    assert shared and disjoint and all(r["category"] == "amin" for r in shared + disjoint)
    # the three depth pairings and the floor decide through min(depthA, depthB): the straddling x differs by the depth ratio
    L = {k: rows[f"{k[0]}/{k[1]}/x_in+1"]["detail"] for k in sc.KINDS}
    for k, want in ((("cube", "cube"), 1.0), (("cube", "cube06"), 0.6), (("cube06", "cube"), 0.6), (("floor", "cube"), 1.0), (("floor", "cube06"), 0.6)):
        width = L[k]["hi"] - L[k]["lo"]
        assert width * want >= AMIN > math.nextafter(width, 0.0) * want * (1 - 1e-12), (k, width)
    # exact equality on each boundary
    eq = rows["cube/cube/thin_equal"]["detail"]
    assert (eq["hi"] - eq["lo"]) * 1.0 == AMIN and rows["cube/cube/thin_equal"]["category"] == "accept"
    assert rows["cube/cube/thin_below"]["category"] == "amin" and rows["cube/cube/thin_above"]["category"] == "accept"
    assert any(abs(r["detail"].get("gap", 0.0)) == 1e-6 for r in rows.values() if r["category"] == "accept")
    assert any(r["detail"]["dotn"] == -1.0 + 1e-6 for r in rows.values() if r["category"] == "accept")
    nfaces = collections.Counter((len(r["blocks"][0].shape.faces) if r["kinds"][0] != "floor" else 1, len(r["blocks"][-1].shape.faces))
                                 for r in rows.values())
    assert {(4, 6), (6, 4), (1, 6), (1, 4), (4, 4)} <= set(nfaces)
    print(f"\nboundary table: {len(rows)} rows, categories {dict(cats)}, {pairs} straddling pairs, provenance (lo, hi) {dict(prov)}, "
          f"{len(shared)} shared-vertex, {len(disjoint)} disjoint, faces (A, B) {dict(nfaces)}")


def test_every_detector_twin_is_rejected_by_the_probes():
    rows = all_block_lists()
    lanes = []
    for _, blocks, _ in rows:
        sc.detect(blocks, lanes=lanes)
    assert any(lane == sc.WAVE - 1 for lane, _ in lanes) and any(chunk >= 2 for _, chunk in lanes)
    print()
    for twin in sc.DETECTOR_TWINS:
        bad = [name for name, blocks, ref in rows if not sc.words_equal(sc.detect(blocks, twin), ref)]
        print(f"detector twin {twin}: differs on {len(bad)} of {len(rows)} block lists")
        assert bad, twin


def test_assembly_probe_conditions():
    cases = sc.assembly_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    n_st = n_un = 0
    for c in cases:
        o = sc.oracle_of(c, sc.TENSION_TOLS)
        d = c["density"]
        assert not (sc.GAP[0] * d < o["v"] <= sc.GAP[1] * d), (c["name"], o["v"])      # stable: < 1e-6 d; unstable: > 1e-4 d
        assert o["stable"] == (o["v"] < sc.GAP[0] * d)
        n_st += o["stable"]
        n_un += not o["stable"]
        for tol in sc.TENSION_TOLS[1:]:
            st, v = o["pen"][tol]
            assert not (sc.GAP[0] * d < v <= sc.GAP[1] * d), (c["name"], tol, v)
            assert st or not o["stable"], c["name"]                                       # plain-stable => penalty-stable
    by = {c["name"]: c for c in cases}
    for dd, want in zip(sc.TIP_OFFSETS, (0.0, 0.0, 1e-3, 1e-2)):
        assert sc.oracle_of(by[f"tipping/d={dd!r}"])["v"] == pytest.approx(want, abs=1e-9)
    r = sc.sliding_r()
    blocks, tan_theta = sc.sliding_pair()
    lo, hi = (sc.oracle_v(blocks, {0}, tan_theta * (1.0 + s * r / 2), 1.0)[1] for s in (-1.0, 1.0))
    assert not (lo > sc.GAP[1] and hi < sc.GAP[0]), "r / 2 would do as well"
    sl = [sc.oracle_of(c) for c in cases if c["tags"] == {"sliding"}]
    assert [o["stable"] for o in sl] == [True, False]
    for c in cases:
        if "density" in c["tags"]:
            assert sc.oracle_of(c)["stable"] == sc.oracle_of(by[c["twin_of"]])["stable"], c["name"]
    for c in cases:
        if c["mask_extra"]:
            assert c["mask_extra"] & ((1 << len(c["blocks"])) - 1) == 0 and sc.fixed_mask(c) >> len(c["blocks"])
    assert all(sc.oracle_of(c)["stable"] for c in cases if c["name"].endswith("fixed=all"))
    ks = collections.Counter(len(c["blocks"]) for c in cases)
    # stable verdicts (the ones lp_verify and the certificate see) on both sides of the LDS limit
    cells = [sc.lp_cells(len(c["blocks"]) - len({b for b in c["fixed"] if b < len(c["blocks"])}), len(sc.oracle_of(c)["interfaces"]))
             for c in cases if sc.oracle_of(c)["stable"] and sc.oracle_of(c)["interfaces"]]
    assert sum(x > sc.LP_TAB_LDS for x in cells) >= 5 and sum(x <= sc.LP_TAB_LDS for x in cells) >= 5
    assert ks[0] == 1 and ks[1] > 3 and any(2 <= k <= 5 for k in ks) and max(ks) >= 12
    print(f"\nassemblies: {len(cases)} cases ({n_st} stable, {n_un} unstable under the oracle), sizes {dict(sorted(ks.items()))}, "
          f"{sum(x > sc.LP_TAB_LDS for x in cells)} stable tableaux beyond LDS, sliding r = {r!r} (tan theta = {tan_theta!r}); optima "
          f"max stable v*/density = {max(sc.oracle_of(c)['v'] / c['density'] for c in cases if sc.oracle_of(c)['stable']):.3g}, "
          f"min unstable = {min(sc.oracle_of(c)['v'] / c['density'] for c in cases if not sc.oracle_of(c)['stable']):.3g}")


def test_capacity_probe_conditions():
    cap = sc.capacity_cases()
    n = {k: len(sc.oracle_of(c)["interfaces"]) for k, c in cap.items()}
    assert n == dict(c64=64, c80=80, c42=42, c43=43)
    assert 6 * n["c42"] <= sc.LP_MAX_COLS < 6 * n["c43"]
    lanes = []
    sc.detect(cap["c64"]["blocks"], lanes=lanes)
    assert (sc.WAVE - 1, 1) in lanes                                      # a hit in the last lane of chunk 1
    o64, o42, o43 = (sc.oracle_of(cap[k], sc.TENSION_TOLS) for k in ("c64", "c42", "c43"))
    assert o64["stable"] and o64["v"] < sc.GAP[0]
    assert o42["v"] == pytest.approx(13.0, abs=1e-6) and o43["v"] == pytest.approx(13.0, abs=1e-6)
    for o in (o42, o43):
        for tol in sc.TENSION_TOLS[1:]:
            assert not (sc.GAP[0] < o["pen"][tol][1] <= sc.GAP[1])
    a, b = sc.lds_pair()
    nif = len(sc.oracle_of(a)["interfaces"])
    nb = len(a["blocks"])
    assert sc.lp_cells(nb - 1, nif) <= sc.LP_TAB_LDS < sc.lp_cells(nb, nif)
    v80 = sc.oracle_of(cap["c80"])["v"]
    print(f"\ncapacity: interfaces {n}; v* 64: {o64['v']:.3g}, 80: {v80:.3g}, 42: {o42['v']:.6g}, 43: {o43['v']:.6g}; penalty optima "
          f"42: {[o42['pen'][t][1] for t in sc.TENSION_TOLS[1:]]}, 43: {[o43['pen'][t][1] for t in sc.TENSION_TOLS[1:]]}; LDS pair {a['name']}: "
          f"{nb} blocks, {nif} interfaces, cells {sc.lp_cells(nb - 1, nif)} <= 2048 < {sc.lp_cells(nb, nif)}, "
          f"v* {sc.oracle_of(a)['v']:.3g} / {sc.oracle_of(b)['v']:.3g}")


def test_certificate_accepts_clean_equilibria_and_rejects_every_twin():
    cases = [c for c in sc.assembly_cases() if "density" not in c["tags"] or "tipping" in c["tags"]] + list(sc.lds_pair())
    rejected = collections.Counter()
    n = 0
    worst = 0.0
    for c in cases:
        for tol in sc.TENSION_TOLS:
            if not sc.oracle_of(c, (tol,))["pen"][tol][0]:
                continue
            forces = sc.clean_equilibrium(c, tol)
            if forces is None:
                continue
            itf = sc.oracle_of(c)["interfaces"]
            fixed = {b for b in c["fixed"] if b < len(c["blocks"])}
            # HiGHS leaves a primal residual of its own (feasibility tolerance 1e-7 per row): far inside the 1e-4 the kernel may use
            cert = sc.certificate(c["blocks"], itf, fixed, c["mu"], c["density"], tol, forces)
            assert sc.certificate_ok(cert, tol), (c["name"], tol, cert)
            worst = max(worst, cert["residual"] / cert["residual_bound"])
            n += 1
            for twin in sc.CERT_TWINS:
                t = sc.certificate(c["blocks"], itf, fixed, c["mu"], c["density"], tol, forces, twin=twin)
                rejected[twin] += not sc.certificate_ok(t, tol)
    print(f"\ncertificate: {n} clean equilibria accepted (largest residual / bound {worst:.3g})")
    for twin in sc.CERT_TWINS:
        print(f"certificate twin {twin}: rejected on {rejected[twin]} of {n}")
        assert rejected[twin] > 0, twin
