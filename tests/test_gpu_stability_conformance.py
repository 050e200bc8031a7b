"""GPU: the contact detector and the equilibrium solver against oracle/rbe.py, through the C ABI (bridges_stability,
bridges_stability_penalty, bridges_pose_block) and, for the two env-side producers of the contact list, through the lock-step env.

  * the contact list -- info[1], every if_body pair and every if_geom word, read from the head of the lp_ws row -- bit for bit
    (the build is -ffp-contract=off and face_pair_contact_v keeps the oracle's operation order): the boundary table, the
    assemblies at K in {1, 5, 16} and n in {1, >= 130}, k_step's incremental list and k_rebuild_contacts' list;
  * the equilibrium a stable verdict reports, as a certificate: balance of every free block, friction cone, budget and tension
    bound re-evaluated in float64 on the host from the ORACLE's interfaces, centroids and weights, against the bounds derived in
    tests/stability_conformance.py;
  * the capacity edges of the stand-alone entry point: 64 and 80 interfaces, the penalty variant at 42 / 43, the LDS limit.

Probes, references and bounds: tests/stability_conformance.py (conditions asserted by tests/test_cpu_stability_conformance_refs.py)."""
import numpy as np
import pytest
import torch

import stability_conformance as sc

pytestmark = pytest.mark.gpu

FIGURES = {}                                          # variant -> largest residual / bound (printed by the last test; -s shows it)


@pytest.fixture(scope="module")
def gpu():
    from bridges_hip import abi
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import ShapeTable
    L = abi.require_gpu()
    return L, ShapeTable([load_urdf(f"shapes/{n}.urdf") for n in sc.TABLE])


def launch(gpu, rows, K, mu, density=1.0, tol=None):
    """rows = [(blocks, fixed mask)] -> dict(stable bool [n], info [n,8], body int32 [n,64,2], geom f64 [n,64,8], forces [n,64,2,3]
    or None).  tol None: bridges_stability; otherwise bridges_stability_penalty with forces.  Vertices of posed oracle Blocks come
    from bridges_pose_block, those of hand-written stand-ins are uploaded as they are."""
    from bridges_hip import abi
    from bridges_hip.vec_env import _ptr, _stream
    L, table = gpu
    dev = torch.device("cuda")
    n = len(rows)
    pose = np.zeros((n, K, 4))
    pose[:, :, 2] = 1.0
    shape = np.zeros((n, K), dtype=np.int32)
    nb = np.zeros(n, dtype=np.int32)
    mask = np.zeros(n, dtype=np.uint32)
    hand = np.zeros((n, K, sc.MAXV, 2))
    is_hand = np.zeros((n, K), dtype=bool)
    for i, (blocks, m) in enumerate(rows):
        assert len(blocks) <= K
        nb[i], mask[i] = len(blocks), m
        for j, b in enumerate(blocks):
            pose[i, j], shape[i, j] = sc.pose_of(b), sc.shape_id(b)
            if isinstance(b, sc.Posed):
                is_hand[i, j] = True
                hand[i, j, :len(b.verts)] = b.verts
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pose_d, shape_d, nb_d, mask_d = t(pose), t(shape), t(nb), t(mask.view(np.int32))
    verts = torch.zeros((n, K, sc.MAXV, 2), dtype=torch.float64, device=dev)
    abi.check(L.bridges_pose_block(table.ptr, n * K, _ptr(shape_d.reshape(-1)), _ptr(pose_d), _ptr(verts), _stream()), "bridges_pose_block")
    verts = torch.where(t(is_hand)[:, :, None, None], t(hand), verts).contiguous()
    stride = abi.lp_ws_stride(K)
    ws = torch.full((n, stride), float("nan"), dtype=torch.float64, device=dev)
    stable = torch.zeros(n, dtype=torch.uint8, device=dev)
    info = torch.full((n, 8), float("nan"), dtype=torch.float64, device=dev)
    forces = None
    if tol is None:
        abi.check(L.bridges_stability(table.ptr, n, K, _ptr(pose_d), _ptr(verts), _ptr(shape_d), _ptr(nb_d), _ptr(mask_d), float(mu),
                                      float(density), sc.FLOOR_HW, sc.FLOOR_DEPTH, _ptr(stable), _ptr(info), _ptr(ws), stride, _stream()),
                  "bridges_stability")
    else:
        forces = torch.full((n, sc.MAX_IF, 2, 3), float("nan"), dtype=torch.float64, device=dev)
        abi.check(L.bridges_stability_penalty(table.ptr, n, K, _ptr(pose_d), _ptr(verts), _ptr(shape_d), _ptr(nb_d), _ptr(mask_d),
                                              float(mu), float(density), sc.FLOOR_HW, sc.FLOOR_DEPTH, float(tol), _ptr(stable), _ptr(info),
                                              _ptr(forces), _ptr(ws), stride, _stream()), "bridges_stability_penalty")
    torch.cuda.synchronize()
    head = ws[:, :9 * sc.MAX_IF].cpu().numpy()
    return dict(stable=stable.cpu().numpy().astype(bool), info=info.cpu().numpy(),
                geom=head[:, :8 * sc.MAX_IF].reshape(n, sc.MAX_IF, 8),
                body=np.ascontiguousarray(head[:, 8 * sc.MAX_IF:]).view(np.int32).reshape(n, sc.MAX_IF, 2),
                forces=None if forces is None else forces.cpu().numpy())


def assert_contacts(out, i, ref, name, limit=None):
    """info[1], the if_body pairs and the if_geom words of row i equal the oracle's list (its first ``limit`` entries)."""
    want = ref if limit is None else ref[:limit]
    n_if = int(out["info"][i, 1])
    assert n_if == len(want), (name, n_if, len(want))
    rb, rg = sc.contact_words(want)
    assert np.array_equal(out["body"][i, :n_if], rb), (name, out["body"][i, :n_if].tolist(), rb.tolist())
    assert sc.same_words(out["geom"][i, :n_if], rg), (name, np.argwhere(out["geom"][i, :n_if] != rg).tolist()[:4])


def same_rows(a, i, b, j):
    """Everything a launch reports of one assembly, bit for bit (the cycle counters of info[4:6] aside)."""
    n_if = int(a["info"][i, 1])
    ok = n_if == int(b["info"][j, 1]) and a["stable"][i] == b["stable"][j] and sc.same_words(a["info"][i, :4], b["info"][j, :4])
    ok = ok and np.array_equal(a["body"][i, :n_if], b["body"][j, :n_if]) and sc.same_words(a["geom"][i, :n_if], b["geom"][j, :n_if])
    if a["forces"] is not None:
        ok = ok and sc.same_words(a["forces"][i], b["forces"][j])
    return ok


# ---- 1. the contact list, bit for bit ---------------------------------------------------------------------------------------

def test_boundary_table_contact_lists(gpu):
    rows = sc.boundary_table()
    out = launch(gpu, [(r["blocks"], 0) for r in rows], 2, 0.8)
    for i, r in enumerate(rows):
        assert_contacts(out, i, r["reference"], r["name"])
    assert not out["info"][:, 3].any()


@pytest.mark.parametrize("K", [1, 5, 16])
def test_assembly_contact_lists_at_every_stride(gpu, K):
    cases = [c for c in sc.assembly_cases() if "density" not in c["tags"]] + list(sc.lds_pair()) + [sc.capacity_cases()["c64"]]
    cases = [c for c in cases if len(c["blocks"]) <= K]
    assert len(cases) > 10 and any(len(c["blocks"]) == K for c in cases) and any(not c["blocks"] for c in cases)
    out = launch(gpu, [(c["blocks"], sc.fixed_mask(c)) for c in cases], K, 0.8)
    for i, c in enumerate(cases):
        assert_contacts(out, i, sc.oracle_of(c)["interfaces"], c["name"])     # the count included: nothing overflowed


def test_same_assembly_alone_and_at_both_ends_of_a_long_launch(gpu):
    cases = list(sc.assembly_cases())                             # every row at mu = 0.8, density 1: only x's verdict is read
    x = next(c for c in cases if c["name"] == "trapezoid_bridge[:9]/fixed=[8]")
    rows = [x] + cases + [x]
    assert len(rows) >= 130
    for tol in (None, 1e-3):
        many = launch(gpu, [(c["blocks"], sc.fixed_mask(c)) for c in rows], 16, 0.8, tol=tol)
        one = launch(gpu, [(x["blocks"], sc.fixed_mask(x))], 16, 0.8, tol=tol)
        assert_contacts(one, 0, sc.oracle_of(x)["interfaces"], x["name"])
        assert same_rows(one, 0, many, 0) and same_rows(one, 0, many, len(rows) - 1)
        assert one["stable"][0] == sc.oracle_of(x, (tol or 0.0,))["pen"][tol or 0.0][0]


ENV_TASKS = {
    "tower": (dict(num_stories=2), "bridge_setup", 10, 3, ["trapezoid"], {}),
    "hexbridge": (dict(num_obstacles=3, trapezoid=False, hexagon=True), "horizontal_bridge_setup", 15, 11, ["hexagon"], dict(mu=0.8)),
    "mixed": (dict(num_obstacles=4, trapezoid=True, hexagon=True), "horizontal_bridge_setup", 12, 21, ["trapezoid", "hexagon"], dict(mu=2.0)),
}


@pytest.mark.parametrize("task", list(ENV_TASKS))
def test_env_side_contact_lists(task):
    """k_step's incremental list after every lock-step and k_rebuild_contacts' list of the same states, against the oracle env's
    find_interfaces and against each other."""
    import oracle.env as oenv
    from oracle.env import policy_draw
    from oracle.rbe import find_interfaces
    from test_gpu_env_parity import make_pair
    kwargs, setup, max_steps, seed, names, kw = ENV_TASKS[task]
    E, n_lock = 8, 10
    vec, oracles = make_pair(kwargs, getattr(oenv, setup), E, max_steps, seed, names, **kw)
    second, _ = make_pair(kwargs, getattr(oenv, setup), E, max_steps, seed, names, **kw)
    counters = [0] * E
    total = most = 0
    for it in range(n_lock):
        vec.select_random()
        for e, o in enumerate(oracles):
            def pick(nv, e=e):
                r = policy_draw(seed, e, counters[e]) % nv
                counters[e] += 1
                return r
            o.lockstep(pick)
        vec.step()
        assert not vec.flags()["lp_error"].any()
        second.load_states(vec.buf["n_blocks"], vec.buf["blk_shape"], vec.buf["blk_pose"], vec.buf["blk_occ"])
        second.rebuild_contacts()
        got = [{k: env.buf[k].cpu().numpy() for k in ("n_blocks", "n_if", "if_body", "if_geom")} for env in (vec, second)]
        for e, o in enumerate(oracles):
            ref = sc.kernel_order(find_interfaces(o.gym.blocks, o.gym.bounds))
            rb, rg = sc.contact_words(ref)
            for g, producer in zip(got, ("k_step", "k_rebuild_contacts")):
                assert g["n_blocks"][e] == len(o.gym.blocks)
                assert g["n_if"][e] == len(ref), (producer, it, e, g["n_if"][e], len(ref))
                assert np.array_equal(g["if_body"][e, :len(ref)], rb), (producer, it, e)
                assert sc.same_words(g["if_geom"][e, :len(ref)], rg), (producer, it, e)
            assert np.array_equal(got[0]["if_body"][e, :len(ref)], got[1]["if_body"][e, :len(ref)])
            assert sc.same_words(got[0]["if_geom"][e, :len(ref)], got[1]["if_geom"][e, :len(ref)])
            total += len(ref)
            most = max(most, len(ref))
    assert total > 100 and most >= 5, (total, most)


# ---- 2. the reported equilibrium as a certificate ---------------------------------------------------------------------------

def certificate_cases():
    return list(sc.assembly_cases()) + list(sc.lds_pair())


def check_certificate(c, out, i, tol, variant):
    """The forces row of one verdict: a certificate when stable, exactly zero beyond n_if and for every other verdict."""
    o = sc.oracle_of(c, (tol,))
    itf = o["interfaces"]
    n_if = len(itf)
    f = out["forces"][i]
    assert not f[n_if:].any() and not np.isnan(f).any(), c["name"]
    if not out["stable"][i] or out["info"][i, 3] != 0:
        assert not f.any(), c["name"]
        return None
    fixed = {b for b in c["fixed"] if b < len(c["blocks"])}
    if not f[:n_if].any() and (n_if == 0 or len(fixed) == len(c["blocks"])):
        return None                                              # nothing is free (or nothing touches): no equilibrium to report
    cert = sc.certificate(c["blocks"], itf, fixed, c["mu"], c["density"], tol, f[:n_if])
    ratio = cert["residual"] / cert["residual_bound"]
    FIGURES[variant] = max(FIGURES.get(variant, 0.0), ratio)
    slack = cert["budget_bound"] - sc.S_MAX * c["density"]
    if slack > 0.0:
        FIGURES[variant + " budget"] = max(FIGURES.get(variant + " budget", -np.inf), (cert["budget"] - sc.S_MAX * c["density"]) / slack)
    assert cert["residual"] <= cert["residual_bound"], (c["name"], tol, cert)
    assert cert["min_cnp"] >= 0.0 and cert["min_cnn"] >= 0.0, (c["name"], tol, cert)
    assert cert["cone_excess"] <= 0.0, (c["name"], tol, cert)
    assert cert["budget"] <= cert["budget_bound"], (c["name"], tol, cert)
    if tol == 0.0:
        assert cert["max_cnn"] == 0.0, (c["name"], cert)
    return f[:n_if]


@pytest.mark.parametrize("tol", sc.TENSION_TOLS)
def test_reported_equilibrium_is_a_certificate(gpu, tol):
    cases = certificate_cases()
    groups = {}
    for c in cases:
        groups.setdefault((c["mu"], c["density"]), []).append(c)
    forces_of, stable_of = {}, {}
    n_cert = 0
    for (mu, density), cs in groups.items():
        rows = [(c["blocks"], sc.fixed_mask(c)) for c in cs]
        out = launch(gpu, rows, 16, mu, density, tol=tol)
        plain = launch(gpu, rows, 16, mu, density) if tol == 0.0 else None
        for i, c in enumerate(cs):
            o = sc.oracle_of(c, (tol,))
            assert out["info"][i, 3] == 0, (c["name"], "solver error")
            assert_contacts(out, i, o["interfaces"], c["name"])
            assert out["stable"][i] == o["pen"][tol][0], (c["name"], tol, out["info"][i, 0], o["pen"][tol][1])
            if plain is not None:                                 # tension_tol = 0 is plain RBE: the other entry point, same bits
                assert plain["stable"][i] == o["stable"] and sc.same_words(plain["info"][i, :4], out["info"][i, :4]), c["name"]
            f = check_certificate(c, out, i, tol, f"tension_tol={tol!r}")
            stable_of[c["name"]] = bool(out["stable"][i])
            if f is not None:
                forces_of[c["name"]] = f
                n_cert += 1
    assert n_cert > 60
    # densities: the plain boolean does not change (tension_tol is an absolute force, so the penalty boolean may: it was compared
    # with the oracle at its own density above), and the forces scale: divided by the density they certify the density-1
    # assembly, under the tension bound divided likewise
    n_scaled = 0
    for c in cases:
        if "density" in c["tags"]:
            base = next(b for b in cases if b["name"] == c["twin_of"])
            if tol == 0.0:
                assert stable_of[c["name"]] == stable_of[base["name"]], c["name"]
            if c["name"] in forces_of:
                fixed = {b for b in base["fixed"] if b < len(base["blocks"])}
                cert = sc.certificate(base["blocks"], sc.oracle_of(base)["interfaces"], fixed, base["mu"], 1.0, tol / c["density"],
                                      forces_of[c["name"]] / c["density"])
                assert sc.certificate_ok(cert, tol), (c["name"], cert)
                n_scaled += 1
    assert n_scaled >= 8
    print(f"\ntension_tol={tol!r}: {n_cert} certificates, largest residual / bound {FIGURES[f'tension_tol={tol!r}']:.4g}, "
          f"largest (budget row - S_MAX density) / slack {FIGURES.get(f'tension_tol={tol!r} budget', float('nan')):.4g}")


def test_plain_stable_implies_penalty_stable(gpu):
    cases = [c for c in certificate_cases() if c["density"] == 1.0 and c["mu"] == 0.8]
    rows = [(c["blocks"], sc.fixed_mask(c)) for c in cases]
    plain = launch(gpu, rows, 16, 0.8)
    for tol in sc.TENSION_TOLS[1:]:
        pen = launch(gpu, rows, 16, 0.8, tol=tol)
        assert not (plain["stable"] & ~pen["stable"]).any()
    assert plain["stable"].any() and not plain["stable"].all()


# ---- 3. capacity edges ----------------------------------------------------------------------------------------------------

def test_sixty_four_interfaces_fit(gpu):
    c = sc.capacity_cases()["c64"]
    o = sc.oracle_of(c)
    for tol in (None, 0.0):
        out = launch(gpu, [(c["blocks"], 0)], 16, c["mu"], tol=tol)
        assert_contacts(out, 0, o["interfaces"], c["name"])
        assert int(out["info"][0, 1]) == 64
        assert out["info"][0, 3] == 0, "64 interfaces are not an overflow"
        assert out["stable"][0] == o["stable"], (out["info"][0], o["v"])       # v* = 0: outside the gap
        if tol is not None:
            assert check_certificate(c, out, 0, 0.0, "64 interfaces") is not None


@pytest.mark.parametrize("tol", [0.0, 1e-3])
def test_eighty_interfaces_overflow_and_leave_the_neighbours_alone(gpu, tol):
    cap = sc.capacity_cases()
    by = {c["name"]: c for c in sc.assembly_cases()}
    a, b = by["trapezoid_bridge[:9]/fixed=[8]"], by["hexagon_bridge_5[:5]/fixed=[]"]
    with_it = launch(gpu, [(a["blocks"], sc.fixed_mask(a)), (cap["c80"]["blocks"], 0), (b["blocks"], 0)], 16, 0.8, tol=tol)
    without = launch(gpu, [(a["blocks"], sc.fixed_mask(a)), (b["blocks"], 0)], 16, 0.8, tol=tol)
    assert with_it["info"][1, 3] == 1 and int(with_it["info"][1, 1]) == 64
    assert_contacts(with_it, 1, sc.oracle_of(cap["c80"])["interfaces"], "cubes8x8", limit=64)
    assert not with_it["stable"][1] and not with_it["forces"][1].any()
    assert same_rows(with_it, 0, without, 0) and same_rows(with_it, 2, without, 1)
    assert_contacts(with_it, 0, sc.oracle_of(a)["interfaces"], a["name"])
    assert_contacts(with_it, 2, sc.oracle_of(b)["interfaces"], b["name"])
    assert with_it["stable"][0] == sc.oracle_of(a)["stable"] and with_it["stable"][2] == sc.oracle_of(b)["stable"]


def test_penalty_variant_at_its_column_limit(gpu):
    cap = sc.capacity_cases()
    c42, c43 = cap["c42"], cap["c43"]
    rows = [(c42["blocks"], 0), (c43["blocks"], 0)]
    plain = launch(gpu, rows, 16, 0.8)
    for i, c in enumerate((c42, c43)):
        assert_contacts(plain, i, sc.oracle_of(c)["interfaces"], c["name"])
        assert plain["info"][i, 3] == 0 and plain["stable"][i] == sc.oracle_of(c)["stable"]
    for tol in sc.TENSION_TOLS[1:]:
        pen = launch(gpu, rows, 16, 0.8, tol=tol)
        assert pen["info"][0, 3] == 0 and pen["stable"][0] == sc.oracle_of(c42, (tol,))["pen"][tol][0]      # 252 columns: solved
        assert pen["info"][1, 3] == 1 and not pen["stable"][1]                                                # 258 > 256: refused
        assert int(pen["info"][0, 1]) == 42 and int(pen["info"][1, 1]) == 43
        assert not pen["forces"].any()
        assert_contacts(pen, 1, sc.oracle_of(c43)["interfaces"], c43["name"])


def test_both_sides_of_the_lds_limit(gpu):
    a, b = sc.lds_pair()
    for tol in sc.TENSION_TOLS:
        out = launch(gpu, [(a["blocks"], sc.fixed_mask(a)), (b["blocks"], sc.fixed_mask(b))], 16, a["mu"], tol=tol)
        for i, c in enumerate((a, b)):
            assert out["info"][i, 3] == 0
            assert out["stable"][i] == sc.oracle_of(c, (tol,))["pen"][tol][0], (c["name"], tol)
            check_certificate(c, out, i, tol, f"LDS pair tol={tol!r}")
