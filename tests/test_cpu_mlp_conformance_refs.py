"""CPU: the references, bounds and acceptance rule of tests/mlp_conformance.py checked without a GPU.

* At every row of every table torch's own float32 CPU result passes ``conform`` against the float64 reference (with itself as the
  yardstick): the references and bounds alone stay inside the conditions the GPU tests put on the kernels.
* Every defective twin -- a float32 evaluation wrong in one way a kernel could be -- is rejected at every row where its defect
  applies, and applies to at least one row: the evidence that tests/test_gpu_mlp_conformance.py would notice such a kernel.
* The tables reach the branches they are there for (the split counts, grid rounds and rider counts csrc/api.hip would choose).
* The middle stack (k_mid_fwd, k_mid_bwd with its riders, k_rows2) has the same three kinds of test at the end of the module."""
import pytest
import torch

import mlp_conformance as M

CPU = torch.device("cpu")


def rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def lin_conform_all(shape, fwd, bwd):
    """conform over everything a layer computes; fwd(x, w, b, relu) and bwd(dz, a, w, act) produce the results under test."""
    pr = M.lin_probe(*shape, CPU)
    x, w, b, dz, act = (pr[k] for k in ("x", "w", "b", "dz", "act"))
    for relu in (False, True):
        ref, bound = M.lin_forward_ref(x, w, b, relu)
        M.conform(f"lin.fwd.relu{int(relu)}", fwd(x, w, b, relu), M.lin_forward_lib(x, w, b, relu), ref, bound, shape)
    for tag, a in (("mask", act), ("nomask", None)):
        refs, got, lib = M.lin_backward_ref(dz, x, w, a), bwd(dz, x, w, a), M.lin_backward_lib(dz, x, w, a)
        for k in ("dW", "db", "dx"):
            M.conform(f"lin.{k}.{tag}", got[k], lib[k], *refs[k], shape)


@pytest.mark.parametrize("shape", M.LIN_SHAPES)
def test_float32_linear_layers_pass(shape):
    lin_conform_all(shape, M.lin_forward_lib, M.lin_backward_lib)


LIN_TWINS = {          # name -> (fwd, bwd, applies(rows, K, N))
    "k_tail_dropped": (M.twin_fwd_k_tail_dropped, M.lin_backward_lib, lambda r, K, N: K % 8 != 0),
    "last_column_shifted": (M.twin_fwd_last_column_shifted, M.lin_backward_lib, lambda r, K, N: N >= 2),
    "last_k_split_left_out": (M.twin_fwd_last_split_left_out, M.lin_backward_lib, lambda r, K, N: M.fwd_plan(r, K, N)[0] > 1),
    "last_n_split_left_out": (M.lin_forward_lib, M.twin_dx_last_split_left_out, lambda r, K, N: M.bwd_plan(r, K, N)[0] > 1),
    "mask_ge_zero": (M.lin_forward_lib, M.twin_dx_mask_ge_zero, lambda r, K, N: True),
}


@pytest.mark.parametrize("twin", sorted(LIN_TWINS))
def test_defective_linear_twins_are_rejected(twin):
    fwd, bwd, applies = LIN_TWINS[twin]
    hit = [s for s in M.LIN_SHAPES if applies(*s)]
    assert hit, twin
    for shape in hit:
        assert rejected(lin_conform_all, shape, fwd, bwd), (twin, shape)


def test_linear_table_reaches_its_branches():
    S = M.LIN_SHAPES
    assert {K for r, K, N in S if r == 32} >= {1, 3, 7, 8, 9, 31, 33, 65} and {K % 8 for _, K, _ in S} == set(range(8))
    assert {N for _, _, N in S} >= {1, 31, 32, 33}
    assert M.fwd_plan(32, 1030, 40) == (17, 64) and M.fwd_plan(64, 1030, 40)[0] > 1 and M.bwd_plan(64, 1030, 40)[0] == 1
    for shape, tiles in (((32, 70, 1100), 1), ((64, 200, 1100), 2), ((96, 33, 515), 3), ((64, 257, 515), 2)):
        assert shape in S and M.bwd_plan(*shape)[0] > 1 and shape[0] // 32 == tiles
    assert (32, 4102, 64) in S and (4102 * 4) % 16 == 8
    # a workspace of two splits' partial sums cuts the split count; none at all means one split; too little is refused
    assert M.fwd_plan(32, 1030, 40, 2 * 32 * 40)[0] == 2 and M.fwd_plan(32, 1030, 40, 0)[0] == 1
    assert M.bwd_plan(32, 70, 1100, 2 * 32 * 70)[0] == 2 and M.bwd_plan(32, 70, 1100, 32 * 70 - 1) == (0, 0)
    # every split of every row holds at least one value
    for r, K, N in S:
        splits, kchunk = M.fwd_plan(r, K, N)
        nsplit, nchunk = M.bwd_plan(r, K, N)
        assert (splits - 1) * kchunk < K <= splits * kchunk and (nsplit - 1) * nchunk < N <= nsplit * nchunk


def loss_conform_all(shape, counter, fn):
    batch, px, nf, use_q, use_sf, per_row = shape
    pr = M.loss_probe(batch, px, nf, per_row, CPU)
    args = (pr["y"], *M.loss_batch(pr, batch, px, counter), batch, px, nf, use_q, use_sf)
    refs, got, lib = M.loss_ref(*args), fn(*args), M.loss_lib(*args)
    for k in ("q", "loss_rows", "dy"):
        M.conform(f"loss.{k}", got[k], lib[k], *refs[k], shape)


@pytest.mark.parametrize("shape", M.LOSS_SHAPES)
def test_float32_head_and_loss_pass(shape):
    for counter in (0, 2):
        loss_conform_all(shape, counter, M.loss_lib)


def test_loss_table_reaches_its_branches():
    S = M.LOSS_SHAPES
    assert {s[1] for s in S} >= {64, 1024, 4096, 4100, 5184, 9000} and {s[0] for s in S} >= {1, 7, 32, 33}
    assert {s[2] for s in S} == {0, 6} and {s[3:5] for s in S} == {(True, True), (True, False), (False, True)}
    assert {s[5] for s in S} == {False, True}
    assert {s[5] for s in S if s[1] > 4096} == {False, True}


def test_loss_that_ignores_pixels_beyond_the_cache_is_rejected():
    hit = [s for s in M.LOSS_SHAPES if s[1] > 4096]
    assert hit
    for shape in hit:
        assert rejected(loss_conform_all, shape, 0, M.twin_loss_cache_only), shape
    for shape in [s for s in M.LOSS_SHAPES if s[1] <= 4096][:2]:          # where the defect does not apply the twin IS the operator
        loss_conform_all(shape, 0, M.twin_loss_cache_only)


def adam_conform_all(n, t, fn):
    p, g, m, v = M.adam_probe(n, CPU)
    refs, got, lib = M.adam_ref(p, g, m, v, t), fn(p, g, m, v, t), M.adam_lib(p, g, m, v, t)
    for k in ("p", "m", "v"):
        M.conform(f"adam.{k}", got[k], lib[k], *refs[k], (n, t))


@pytest.mark.parametrize("t", M.ADAM_STEPS)
def test_float32_adam_passes_and_a_stale_tail_is_rejected(t):
    sizes = sorted(set(M.ADAM_FLAT_N + M.ADAM_MULTI_N))
    for n in sizes:
        adam_conform_all(n, t, M.adam_lib)
    hit = [n for n in sizes if n % 4]
    assert hit
    for n in hit:
        assert rejected(adam_conform_all, n, t, M.twin_adam_tail_not_updated), (n, t)


@pytest.mark.parametrize("sf_dim", M.TD_SF_DIMS)
def test_float32_td_target_passes_and_the_last_maximum_is_rejected(sf_dim):
    pr = M.td_probe(sf_dim, CPU)
    for gamma in (1.0, 0.8):
        ref, rows = M.td_ref(pr, gamma)
        plain = M.td_plain(pr, gamma)
        M.td_conform("td", plain, plain, ref, rows, (sf_dim, gamma))
        assert rejected(M.td_conform, "td", M.td_plain(pr, gamma, last=True), plain, ref, rows, (sf_dim, gamma))
    # the planted ties: the first maximum, whichever thread or stride holds the later one
    lo = pr["lo"]
    assert rows[:7] == [0, rows[1], rows[2], lo[3] + 200, lo[4] + 44, lo[5] + 5, lo[6]] and rows[7] == M.NO_ROW
    assert rows[8] == lo[3] + 200 and rows[9] == lo[5] + 5 + 256          # the shared ranges: the second starts behind lo + 5
    assert [h - l for l, h in zip(lo, pr["hi"])][:6] == list(M.TD_LENGTHS)


# ---------------------------------------------------------------------------------------------------------------------------
# the middle stack: k_mid_fwd, k_mid_bwd with its riders, k_rows2

MID_SEEDS = (0, 1)
ROWS_CPU_N = tuple(n for n in M.MID_ROWS_N if n <= 8193)       # 16389 adds a grid round, not a numerical case: left to the GPU


def mid_forward_conform_all(seed, fwd):
    pr = M.mid_probe(CPU, seed)
    M.mid_forward_conform("mid_fwd", pr["x"], fwd(pr["W"], pr["b"], pr["x"]), pr["W"], pr["b"], seed)


def rows_conform_all(n, fn):
    pr = M.mid_probe(CPU)
    x = M.rows_probe(n, CPU)
    mid, y = fn(pr["W"], pr["b"], x)
    M.rows_conform("mid_rows", x, mid, y, pr["W"], pr["b"], n)


def mid_backward_conform_all(seed, bwd):
    pr = M.mid_probe(CPU, seed)
    M.mid_backward_conform("mid_bwd", bwd(pr["W"], pr["acts"], pr["dz4"]), pr["W"], pr["acts"], pr["dz4"], seed)


def rider_conform_all(n, t, fn):
    p, g, m, v = M.adam_probe(n, CPU, seed=3)
    refs, got, lib = M.adam_ref(p, g, m, v, t), fn(p, g, m, v, t), M.adam_lib(p, g, m, v, t)
    for k in ("p", "m", "v"):
        M.conform(f"rider.{k}", got[k], lib[k], *refs[k], (n, t))


@pytest.mark.parametrize("seed", MID_SEEDS)
def test_float32_middle_stack_passes(seed):
    mid_forward_conform_all(seed, M.mid_forward_lib)
    mid_backward_conform_all(seed, M.mid_backward_lib)


@pytest.mark.parametrize("n", ROWS_CPU_N)
def test_float32_two_layer_chains_pass(n):
    rows_conform_all(n, M.rows_lib)


@pytest.mark.parametrize("t", M.ADAM_STEPS)
def test_float32_rider_adam_passes_and_a_single_stride_round_is_rejected(t):
    hit = []
    for n in M.MID_REST_N:
        if n:
            rider_conform_all(n, t, M.adam_lib)
        if M.rider_plan(n)[1] > 1:
            hit.append(n)
            assert rejected(rider_conform_all, n, t, M.twin_rider_first_round_only), (n, t)
    assert len(hit) >= 3


MID_FWD_TWINS = {"quarter_left_out": M.twin_mid_fwd_quarter_left_out, "last_tile_without_bias": M.twin_mid_fwd_last_tile_without_bias,
                 "bf16_operands": M.twin_mid_fwd_bf16_operands}
MID_BWD_TWINS = {"inner_mask_ge_zero": M.twin_mid_bwd_inner_mask_ge_zero, "dw_from_unmasked_gradient": M.twin_mid_bwd_dw_from_unmasked_gradient,
                 "db_even_rows_only": M.twin_mid_bwd_db_even_rows_only}
MID_ROWS_TWINS = {          # name -> (twin, applies(n))
    "relu_in_forgotten": (M.twin_rows_relu_in_forgotten, lambda n: True),
    "last_tile_from_row_n_minus_1": (M.twin_rows_last_tile_from_row_n_minus_1, lambda n: n % 32 >= 2),
    **{k: (M.rows_from(f), lambda n: True) for k, f in MID_FWD_TWINS.items()},
}


@pytest.mark.parametrize("twin", sorted(MID_FWD_TWINS))
def test_defective_forward_stack_twins_are_rejected(twin):
    for seed in MID_SEEDS:
        assert rejected(mid_forward_conform_all, seed, MID_FWD_TWINS[twin]), (twin, seed)


@pytest.mark.parametrize("twin", sorted(MID_BWD_TWINS))
def test_defective_backward_stack_twins_are_rejected(twin):
    for seed in MID_SEEDS:
        assert rejected(mid_backward_conform_all, seed, MID_BWD_TWINS[twin]), (twin, seed)


@pytest.mark.parametrize("twin", sorted(MID_ROWS_TWINS))
def test_defective_two_layer_chain_twins_are_rejected(twin):
    fn, applies = MID_ROWS_TWINS[twin]
    hit = [n for n in ROWS_CPU_N if n < 8193 and applies(n)]
    assert hit, twin
    for n in hit:
        assert rejected(rows_conform_all, n, fn), (twin, n)
    for n in [n for n in ROWS_CPU_N if not applies(n)][:2]:                # where the defect does not apply the twin IS the operator
        rows_conform_all(n, fn)


def test_middle_stack_tables_reach_their_branches():
    """From the launch arithmetic of csrc/api.hip (M.rows_plan, M.rider_plan)."""
    plans = {n: M.rows_plan(n) for n in M.MID_ROWS_N}
    assert plans[1] == (1, 1) and plans[32] == (1, 1) and plans[33] == (2, 1) and plans[63] == (2, 1)
    assert plans[8193] == (256, 2) and 8193 == 256 * 32 + 1               # 257 tiles on the clamped grid: one row in round two
    assert plans[16389] == (256, 3)                                        # a second round with a `next` to prefetch
    assert any(M.ceil_div(n, 32) > 256 for n in M.MID_ROWS_N)
    assert {n % 32 for n in M.MID_ROWS_N} >= {0, 1, 31} and any(n % 32 >= 2 and n > 8192 for n in M.MID_ROWS_N)
    assert set(M.MID_ROWS_STRIDED_N) <= set(M.MID_ROWS_N) and max(M.MID_ROWS_STRIDED_N) > 8192
    assert {s[0] for s in M.MID_ROWS_STRIDES} == {256, 260, 320} and {s[1] for s in M.MID_ROWS_STRIDES} == {256, 257, 300}
    assert all(s[0] % 4 == 0 for s in M.MID_ROWS_STRIDES)
    riders = {n: M.rider_plan(n) for n in M.MID_REST_N}
    assert riders[0] == (0, 0, 0) and riders[4] == (1, 1, 1)
    assert riders[4100] == (1, 2, 1)                                       # one rider, a ragged second round
    assert riders[16388] == (2, 3, 1)                                      # two riders, three rounds, the last ragged
    big = max(M.MID_REST_N)
    assert M.ceil_div(big >> 2, 4096) > 248 and riders[big][0] == 248 and riders[big][1] > 4 and riders[big][2] < 248 * 1024
    assert all(n % 4 == 0 for n in M.MID_REST_N)
    assert [M.T(K) for K in (256, 128, 64)] == [264, 134, 69]
