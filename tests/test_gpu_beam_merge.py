"""GPU: bridges_beam_merge against the numpy statement of its rule (tests/beam_merge_ref.py), exactly and on sentinel-filled outputs:
the probe tables, seeded tables at G in {1, 5} x B in {1, 2, 8, 16} x K in {1, 6, 64} under both key_last values, the same bits on a
second call, the refusals, which leave the outputs untouched -- and the premise on the real env: ground placements that commute
leave two envs the operator calls equivalent."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_merge_ref as MR

pytestmark = pytest.mark.gpu
ARRAYS = ("n_blocks", "blk_shape", "blk_pose", "blk_occ", "targets_left", "live", "ret")


def _dev(case):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in ARRAYS}


def _run(case):
    """One call on sentinel-filled outputs -> the outputs as numpy arrays."""
    from bridges_hip import ops
    c = _dev(case)
    out = {k: torch.from_numpy(v).cuda() for k, v in MR.sentinels(len(case["n_blocks"]), case["B"]).items()}
    ops.beam_merge(c["n_blocks"], c["blk_shape"], c["blk_pose"], c["blk_occ"], c["targets_left"], case["B"], c["live"], c["ret"],
                   key_last=case["key_last"], out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_exact(got, want, what):
    for k in MR.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


@pytest.mark.parametrize("name", sorted(MR.probe_tables()))
def test_probe_tables_exactly(name):
    case = MR.probe_tables()[name]
    _assert_exact(_run(case), MR.reference(case), name)


@pytest.mark.parametrize("K", [1, 6, 64])
@pytest.mark.parametrize("B", [1, 2, 8, 16])
@pytest.mark.parametrize("G", [1, 5])
def test_seeded_tables_exactly_and_the_same_on_a_second_call(G, B, K):
    merged = 0
    for key_last in (0, 1):
        case = MR.random_case(G, B, K, seed=100 * G + 10 * B + K + key_last, key_last=key_last)
        got, want = _run(case), MR.reference(case)
        _assert_exact(got, want, (G, B, K, key_last))
        assert MR.same(_run(case), got)
        merged += int(want["n_merged"].sum())
    assert B == 1 or G * B <= 2 or merged > 0                            # (the tables hold classes to find)


def test_refusals_leave_the_outputs_untouched():
    from bridges_hip import abi
    L = abi.require_gpu()
    case = MR.random_case(3, 4, 6, seed=1)
    c = _dev(case)
    E = 12
    out = {k: torch.from_numpy(v).cuda() for k, v in MR.sentinels(E, 4).items()}
    stream = abi.current_stream()

    def call(E=E, B=4, K=6, **swap):
        a = dict(c, rep=out["rep"], live_out=out["live"], n_merged=out["n_merged"])
        a.update(swap)
        p = {k: (v if isinstance(v, C.c_void_p) else C.c_void_p(v.data_ptr() if v is not None else 0)) for k, v in a.items()}
        return L.bridges_beam_merge(E, B, K, p["n_blocks"], p["blk_shape"], p["blk_pose"], p["blk_occ"], p["targets_left"], p["live"],
                                    p["ret"], 1, p["rep"], p["live_out"], p["n_merged"], stream)
    assert call(B=0) == -1 and call(B=17) == -1 and b"1..16" in L.bridges_last_error()
    assert call(E=11) == -1 and call(E=-4) == -1                         # E % B != 0, a negative count
    assert call(K=0) == -1 and call(K=65) == -1 and b"1..64" in L.bridges_last_error()
    for name in ARRAYS + ("rep", "live_out", "n_merged"):
        assert call(**{name: None}) == -1, name
    assert call(E=0) == 0                                                # nothing to do, nothing launched
    torch.cuda.synchronize()
    want = MR.sentinels(E, 4)
    for k in MR.OUTPUTS:
        assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert call() == 0                                                   # and the call they guard goes through
    torch.cuda.synchronize()
    _assert_exact({k: v.cpu().numpy() for k, v in out.items()}, MR.reference(case), "after the refusals")


# ---- the premise on the real env ----------------------------------------------------------------------------------------------------
def _ground_candidates(env, e):
    """The valid ground candidates of env e: a list of (x, pose bytes, shape id), by x."""
    off, n = env.cand_offset.cpu().numpy(), env.n_cand.cpu().numpy()
    rows = slice(int(off[e]), int(off[e]) + int(n[e]))
    desc, pose, mask = env.cand_desc[rows].cpu().numpy(), env.cand_pose[rows].cpu().numpy(), env.cand_mask[rows].cpu().numpy()
    out = [(float(pose[j, 0]), pose[j].tobytes(), int(desc[j, 2])) for j in range(len(desc)) if mask[j] and desc[j, 0] == -1]
    return sorted(out)


def _find(env, e, cand):
    """The candidate index, within env e's set, of the valid ground candidate with these pose bits and this shape."""
    off, n = env.cand_offset.cpu().numpy(), env.n_cand.cpu().numpy()
    rows = slice(int(off[e]), int(off[e]) + int(n[e]))
    desc, pose, mask = env.cand_desc[rows].cpu().numpy(), env.cand_pose[rows].cpu().numpy(), env.cand_mask[rows].cpu().numpy()
    hits = [j for j in range(len(desc)) if pose[j].tobytes() == cand[1] and desc[j, 2] == cand[2] and desc[j, 0] == -1 and mask[j]]
    assert hits, f"env {e}: the ground candidate at x = {cand[0]} is not valid any more"
    return hits[0]


def _classes(env, B, key_last):
    from bridges_hip import ops
    E = env.E
    live = torch.ones(E, dtype=torch.uint8, device="cuda")
    ret = torch.zeros(E, dtype=torch.float64, device="cuda")
    out = ops.beam_merge(env.n_blocks, env.blk_shape, env.blk_pose, env.blk_occ, env.targets_left, B, live, ret, key_last=key_last)
    torch.cuda.synchronize()
    return out["rep"].cpu().numpy(), out["n_merged"].cpu().numpy()


def test_ground_placements_that_commute_leave_equivalent_envs():
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    from robotoddler.training.vec_dqn import beam_env_like
    # ground positions 2.5 apart and all on the floor (it ends at x = 5): the trapezoid's diameter is 2, so a ground block never
    # touches its neighbour's; a target out of the ground blocks' reach
    fixed = VecAssemblyGym(4, [load_urdf("shapes/trapezoid.urdf")], [], [(0.5, 0, 5.0)], max_steps=6, seed=3, f32_rasters=False,
                           x_discr_ground=[-1.9, 0.6, 3.1])
    env = beam_env_like(fixed, 2)                                        # 4 groups of 2, one task: any grouping shares it
    E = env.E
    assert E == 8 and env.K <= 64
    env.reset()
    torch.cuda.synchronize()
    nb0 = int(env.n_blocks[0])
    turns = {}
    for g in _ground_candidates(env, 0):                                 # by (rotation, shape): the three positions of one of them
        turns.setdefault((g[1][16:], g[2]), []).append(g)
    flat = min(turns, key=lambda k: (abs(np.frombuffer(k[0], np.float64)[1]), -np.frombuffer(k[0], np.float64)[0]))
    assert len(turns[flat]) == 3                                         # lying flat: stable whether frozen or not
    a, c, b = turns[flat]
    assert len({a[1], b[1], c[1]}) == 3
    # slots 0 and 3: a, b, c;  slot 1: b, a, c;  slot 2: a, b, c' (another valid ground candidate than c);  the others: a, b, c
    script = {e: [a, b, c] for e in range(E)}
    script[1] = [b, a, c]
    for d in range(3):
        if d == 2:
            script[2][2] = [g for g in _ground_candidates(env, 2) if g[1] != c[1]][0]
        sel = torch.tensor([_find(env, e, script[e][d]) for e in range(E)], dtype=torch.int32, device="cuda")
        env.step(sel)
        torch.cuda.synchronize()
        assert env.n_blocks.tolist() == [nb0 + d + 1] * E and bool(env.step_flags[:, 0].all())
        assert not bool(env.step_flags[:, 5].any() | env.step_flags[:, 6].any())       # nobody's episode ended
        if d == 1:                                                       # depth 2: the same two blocks, another last block
            rep1, _ = _classes(env, 2, key_last=1)
            rep0, _ = _classes(env, 2, key_last=0)
            assert rep1[0] != rep1[1] and rep1[:2].tolist() == [0, 1]
            assert rep0[0] == rep0[1] == 0
            assert rep1[2] == rep1[3] == 2                               # (an exact copy is equivalent under either)
    # depth 3: the slot order differs, the structure does not
    assert not torch.equal(env.blk_pose[0], env.blk_pose[1])
    for key_last in (0, 1):
        rep, n_merged = _classes(env, 2, key_last)
        assert rep[0] == rep[1] == 0 and n_merged[0] == 1
        assert rep[2] == 2 and rep[3] == 3 and n_merged[1] == 0          # a, b, c' is another structure than a, b, c
        rep, n_merged = _classes(env, 4, key_last)                       # ... also inside one group of four
        assert rep[:4].tolist() == [0, 0, 2, 0] and n_merged.tolist() == [2, 3]
