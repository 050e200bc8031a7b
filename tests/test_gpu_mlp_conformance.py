"""GPU: conformance of the SuccessorMLP step kernels (csrc/mlp_kernels.hip: k_lin_fwd, k_lin_bwd, k_successor_loss, the folded
Adam update, and the middle stack's k_mid_fwd, k_mid_bwd with its Adam riders and k_rows2) and of the scalar-ish DQN kernels
(csrc/dqn_kernels.hip: k_td_target, k_adam_flat, k_adam_multi, k_soft_update) at the entry points of include/bridges_hip.h.

Tables, probe data, float64 references, bounds and the acceptance rule come from tests/mlp_conformance.py (checked without a GPU
by tests/test_cpu_mlp_conformance_refs.py, which also shows that a kernel wrong in one of sixteen ways would be rejected):

* every element inside the first-order float32 bound around the float64 result, exact zeros where the kernel must write them;
* q_kernel <= FACTOR * q_library, the library being torch's float32 result on the same inputs (``Q ...`` lines are printed;
  docs/MEASUREMENT_LOG.md records a run);
* what an entry point promises beside the numbers: blocks addressed through a device word, workspaces that cut the split count,
  refusals that name their reason and leave the output alone, results that repeat bit for bit, counters and tickets."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mlp_conformance as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -77.25


def lib():
    from bridges_hip import abi
    return abi.require_gpu()


def call(name, *args):
    from bridges_hip import abi
    abi.check(getattr(lib(), name)(*args), name)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    from bridges_hip import abi
    return abi.current_stream()


def word(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


WS = None


def workspace():
    global WS
    if WS is None:
        WS = torch.empty(M.WS_FLOATS, device=DEV)
    return WS


def forward(x, w, b, relu, rows=None, ws_floats=M.WS_FLOATS, x_block=None):
    rows, (N, K) = (x.shape[0] if rows is None else rows), w.shape
    y = torch.full((rows, N), SENTINEL, device=DEV)
    call("bridges_linear_forward", rows, K, N, ptr(x), ptr(w), ptr(b), int(relu), ptr(y), ptr(workspace() if ws_floats else None),
         ws_floats, ptr(x_block), stream())
    return y


def backward(dz, a, w, act=None, need_dx=True, rows=None, ws_floats=M.WS_FLOATS, a_block=None, a_block_bias=0):
    rows, (N, K) = (dz.shape[0] if rows is None else rows), w.shape
    dW, db = torch.full((N, K), SENTINEL, device=DEV), torch.full((N,), SENTINEL, device=DEV)
    dx = torch.full((rows, K), SENTINEL, device=DEV) if need_dx else None
    call("bridges_linear_backward", rows, K, N, ptr(dz), ptr(a), ptr(w), ptr(dW), ptr(db), ptr(act), ptr(dx),
         ptr(workspace() if ws_floats else None), ws_floats, ptr(a_block), a_block_bias, stream())
    return dict(dW=dW, db=db, dx=dx)


def poisoned_blocks(t, block, n_blocks=3):
    """t as block ``block`` of ``n_blocks``; every other block NaN (a read of a wrong block poisons the result)."""
    out = torch.full((n_blocks, *t.shape), math.nan, device=DEV)
    out[block] = t
    return out.reshape(n_blocks * t.shape[0], *t.shape[1:])


# ---------------------------------------------------------------------------------------------------------------------------
# linear layers

@pytest.mark.parametrize("shape", M.LIN_SHAPES)
def test_linear_forward_inside_the_bound(shape):
    """k_lin_fwd, and behind a split-K launch k_lin_fwd_finish, at bridges_linear_forward against lin_forward_ref's float64 result:
    with the full workspace, without one (one split) and with room for two splits; x_block addressing; repeats bit for bit."""
    rows, K, N = shape
    pr = M.lin_probe(rows, K, N, DEV)
    x, w, b = pr["x"], pr["w"], pr["b"]
    splits = M.fwd_plan(rows, K, N)[0]
    for relu in (False, True):
        ref, bound = M.lin_forward_ref(x, w, b, relu)
        lb = M.lin_forward_lib(x, w, b, relu)
        y = forward(x, w, b, relu)
        M.conform(f"lin.fwd.relu{int(relu)}", y, lb, ref, bound, shape)
        # no workspace: one split whatever K; a workspace of two splits' partial sums: two splits
        M.conform(f"lin.fwd.relu{int(relu)}.no_ws", forward(x, w, b, relu, ws_floats=0), lb, ref, bound, shape)
        if splits > 2:
            assert M.fwd_plan(rows, K, N, 2 * rows * N)[0] == 2
            M.conform(f"lin.fwd.relu{int(relu)}.ws2", forward(x, w, b, relu, ws_floats=2 * rows * N), lb, ref, bound, shape)
        assert torch.equal(forward(x, w, b, relu), y)                                  # deterministic
    # x_block: the layer's input is block *x_block of a [3 rows, K] array; the other blocks are never read
    y = forward(x, w, b, False)
    for blk in (1, 2):
        assert torch.equal(forward(poisoned_blocks(x, blk), w, b, False, rows=rows, x_block=word(blk)), y), blk


@pytest.mark.parametrize("shape", M.LIN_SHAPES)
def test_linear_backward_inside_the_bound(shape):
    """k_lin_bwd<false>, and behind a split-N launch k_lin_dx_finish, at bridges_linear_backward against lin_backward_ref's float64
    dW, db and masked dx: with and without a mask, with a workspace that cuts the split count, without an input gradient, and
    through a_block addressing; repeats bit for bit."""
    rows, K, N = shape
    pr = M.lin_probe(rows, K, N, DEV)
    x, w, dz, act = pr["x"], pr["w"], pr["dz"], pr["act"]
    nsplit = M.bwd_plan(rows, K, N)[0]
    first = None
    for tag, a in (("mask", act), ("nomask", None)):
        refs, lb, got = M.lin_backward_ref(dz, x, w, a), M.lin_backward_lib(dz, x, w, a), backward(dz, x, w, a)
        for k in ("dW", "db", "dx"):
            M.conform(f"lin.{k}.{tag}", got[k], lb[k], *refs[k], shape)
        if a is not None:
            assert bool((got["dx"][~(act > 0)] == 0).all())                            # +0, -0.0 and negatives switch an element off
            first = got
            again = backward(dz, x, w, a)
            assert all(torch.equal(again[k], got[k]) for k in got)                     # deterministic over two calls
            if nsplit > 2:                                                              # a workspace that forces fewer N splits
                assert M.bwd_plan(rows, K, N, 2 * rows * K)[0] == 2
                M.conform("lin.dx.mask.ws2", backward(dz, x, w, a, ws_floats=2 * rows * K)["dx"], lb["dx"], *refs["dx"], shape)
    only = backward(dz, x, w, None, need_dx=False, ws_floats=0)                         # no input gradient: no workspace needed
    assert only["dx"] is None and torch.equal(only["dW"], first["dW"]) and torch.equal(only["db"], first["db"])
    # a_block: the layer's input is block *a_block + a_block_bias of a [3 rows, K] array
    for blk, bias in ((1, 0), (2, -1), (0, 0)):
        got = backward(dz, poisoned_blocks(x, blk + bias), w, act, rows=rows, a_block=word(blk), a_block_bias=bias)
        assert all(torch.equal(got[k], first[k]) for k in got), (blk, bias)


def refused(rc, reason):
    """A non-zero status, ``reason`` in bridges_last_error() and in what abi.check raises."""
    from bridges_hip import abi
    assert rc != 0
    msg = lib().bridges_last_error().decode()
    assert reason in msg, msg
    with pytest.raises(abi.BridgesHipError, match=reason):
        abi.check(rc, "entry point")


def test_linear_refusals_name_their_reason_and_leave_the_output_alone():
    L = lib()
    pr = M.lin_probe(64, 70, 33, DEV)
    x, w, b, dz, act = (pr[k] for k in ("x", "w", "b", "dz", "act"))
    y = torch.full((64, 33), SENTINEL, device=DEV)
    dW, db, dx = torch.full((33, 70), SENTINEL, device=DEV), torch.full((33,), SENTINEL, device=DEV), torch.full((64, 70), SENTINEL, device=DEV)
    ws = workspace()
    refused(L.bridges_linear_forward(48, 70, 33, ptr(x), ptr(w), ptr(b), 0, ptr(y), ptr(ws), ws.numel(), None, stream()), "multiple of 32")
    refused(L.bridges_linear_backward(48, 70, 33, ptr(dz), ptr(x), ptr(w), ptr(dW), ptr(db), ptr(act), ptr(dx), ptr(ws), ws.numel(), None, 0,
                                      stream()), "multiple of 32")
    refused(L.bridges_linear_backward(64, 70, 33, ptr(dz), ptr(x), ptr(w), ptr(dW), ptr(db), ptr(act), ptr(dx), None, 0, None, 0, stream()),
            "workspace needed")
    refused(L.bridges_linear_backward(64, 70, 33, ptr(dz), ptr(x), ptr(w), ptr(dW), ptr(db), ptr(act), ptr(dx), ptr(ws), 64 * 70 - 1, None, 0,
                                      stream()), "workspace too small")
    torch.cuda.synchronize()
    for t in (y, dW, db, dx):
        assert bool((t == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# Adam folded into the first layer's weight-gradient tiles

@pytest.mark.parametrize("shape", [(32, 70, 33), (32, 523, 257), (32, 256, 128)])
def test_folded_adam_equals_backward_then_flat_adam(shape):
    """k_lin_bwd<true> claims `the same arithmetic as k_adam_flat`: W, bias, their four moment tensors and the rest range after
    bridges_linear_backward_adam equal bridges_linear_backward followed by bridges_adam_step on copies, bit for bit."""
    rows, K, N = shape
    pr = M.lin_probe(rows, K, N, DEV)
    x, w, b, dz = pr["x"], pr["w"], pr["b"], pr["dz"]
    lr, b1, b2, eps = M.ADAM_HYPER
    grads = backward(dz, x, w, None, need_dx=False, ws_floats=0)
    for rest_n in (0, 4, 4100):
        for t in M.ADAM_STEPS:
            step = torch.full((), float(t), device=DEV)                                # the number of THIS update
            _, _, mW, vW = M.adam_probe(N * K, DEV, seed=1)
            _, _, mb, vb = M.adam_probe(N, DEV, seed=2)
            rp, rg, rm, rv = M.adam_probe(max(rest_n, 4), DEV, seed=3)
            rp0 = rp.clone()
            want = dict(W=w.clone().reshape(-1), b=b.clone(), mW=mW.clone(), vW=vW.clone(), mb=mb.clone(), vb=vb.clone(), rp=rp.clone(),
                        rm=rm.clone(), rv=rv.clone())
            for p_, g_, m_, v_, n_ in ((want["W"], grads["dW"], want["mW"], want["vW"], N * K), (want["b"], grads["db"], want["mb"], want["vb"], N),
                                       (want["rp"], rg, want["rm"], want["rv"], rest_n)):
                call("bridges_adam_step", ptr(p_), ptr(g_), ptr(m_), ptr(v_), n_, ptr(step), lr, b1, b2, eps, stream())
            got = dict(W=w.clone().reshape(-1), b=b.clone(), mW=mW, vW=vW, mb=mb, vb=vb, rp=rp, rm=rm, rv=rv)
            call("bridges_linear_backward_adam", rows, K, N, ptr(dz), ptr(x), ptr(got["W"]), ptr(got["b"]), ptr(got["mW"]), ptr(got["vW"]),
                 ptr(got["mb"]), ptr(got["vb"]), ptr(got["rp"]), ptr(rg), ptr(got["rm"]), ptr(got["rv"]), rest_n, ptr(step), lr, b1, b2, eps,
                 None, 0, stream())
            for k in want:
                same = torch.equal(got[k], want[k])
                worst = float((got[k].double() - want[k].double()).abs().max())
                print(f"FOLD {shape} rest={rest_n} t={t} {k}: {'bit-identical' if same else f'max difference {worst:.3e}'}")
                assert same, (shape, rest_n, t, k, worst)
            assert not torch.equal(got["W"], w.reshape(-1)) and (rest_n == 0 or not torch.equal(got["rp"], rp0))      # something moved


# ---------------------------------------------------------------------------------------------------------------------------
# head and loss

def run_loss(shape, pr, counter_value, losses=None, n_losses=0, counter_inc=None, ticket=None, adam_step=None, counter=None):
    batch, px, nf, use_q, use_sf, per_row = shape
    rows, N = M.rows_of(batch), 2 * px + 2 * nf
    counter = word(counter_value) if counter is None else counter
    dy, loss_rows, q_out = (torch.full(s, math.nan, device=DEV) for s in ((rows, N), (rows,), (rows,)))
    head = (batch, rows, px, nf, ptr(pr["y"]), ptr(pr["reward"]))
    tail = (ptr(counter), ptr(pr["q_t"] if use_q else None), ptr(pr["sf_t"] if use_sf else None), int(use_q), int(use_sf), ptr(dy),
            ptr(loss_rows), ptr(q_out), ptr(losses), n_losses, ptr(counter_inc), ptr(ticket), ptr(adam_step), stream())
    if per_row:
        call("bridges_successor_loss_rows", *head, px, *tail)
    else:
        call("bridges_successor_loss", *head, *tail)
    return dict(q=q_out, loss_rows=loss_rows, dy=dy)


def row_order_sum(loss_rows, batch):
    total = np.float32(0.0)
    for v in loss_rows[:batch].cpu().numpy():
        total = np.float32(total + v)
    return float(total)


@pytest.mark.parametrize("shape", M.LOSS_SHAPES)
def test_successor_loss_inside_the_bound(shape):
    """k_successor_loss<PER_ROW> at bridges_successor_loss / _rows against loss_ref's float64 q, per-row loss and gradient, at two
    positions of the per-call arrays; exact zeros in padding rows and behind column 2 px."""
    batch, px, nf, use_q, use_sf, per_row = shape
    pr = M.loss_probe(batch, px, nf, per_row, DEV)
    for c in (0, 2):                                                                    # addressing into the per-call arrays
        args = (pr["y"], *M.loss_batch(pr, batch, px, c), batch, px, nf, use_q, use_sf)
        refs, lb, got = M.loss_ref(*args), M.loss_lib(*args), run_loss(shape, pr, c)
        for k in ("q", "loss_rows", "dy"):
            M.conform(f"loss.{k}.c{c}", got[k], lb[k], *refs[k], shape)
        assert bool((got["dy"][batch:] == 0).all()) and bool((got["dy"][:, 2 * px:] == 0).all())
        assert bool((got["q"][batch:] == 0).all()) and bool((got["loss_rows"][batch:] == 0).all())


@pytest.mark.parametrize("shape", [M.LOSS_SHAPES[0], M.LOSS_SHAPES[1], M.LOSS_SHAPES[4], M.LOSS_SHAPES[7]])
def test_successor_loss_logging_forms(shape):
    """No log, the k_loss_log launch and the ticket form (the last row workgroup to arrive logs inside the loss kernel) give the
    same q, loss rows and gradient; a log entry is the row-order float32 sum of the loss rows; counter and step advance by one a
    call; the ticket is re-armed; a counter at or beyond n_losses drops the entry and still advances."""
    batch, px, nf, use_q, use_sf, per_row = shape
    pr = M.loss_probe(batch, px, nf, per_row, DEV)
    plain = [run_loss(shape, pr, c) for c in range(3)]
    sums = [row_order_sum(p["loss_rows"], batch) for p in plain]
    # k_loss_log behind the loss kernel; n_losses = 2, so the third call (c = 2 >= n_losses) logs nothing
    counter, losses = word(0), torch.full((3,), SENTINEL, device=DEV)
    for c in range(3):
        got = run_loss(shape, pr, None, losses=losses, n_losses=2, counter_inc=counter, counter=counter)
        assert all(torch.equal(got[k], plain[c][k]) for k in got) and int(counter) == c + 1
    assert losses.tolist() == [sums[0], sums[1], SENTINEL]
    # the ticket form: three consecutive calls on one ticket word
    counter, losses = word(0), torch.full((3,), SENTINEL, device=DEV)
    ticket, adam_step = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros((), device=DEV)
    for c in range(3):
        got = run_loss(shape, pr, None, losses=losses, n_losses=3, counter_inc=counter, ticket=ticket, adam_step=adam_step, counter=counter)
        assert all(torch.equal(got[k], plain[c][k]) for k in got)
        assert float(losses[c]) == sums[c] and int(counter) == c + 1 and float(adam_step) == c + 1.0 and int(ticket) == 0
    assert losses.tolist() == sums
    # ... and beyond n_losses
    counter, losses = word(2), torch.full((2,), SENTINEL, device=DEV)
    run_loss(shape, pr, None, losses=losses, n_losses=2, counter_inc=counter, ticket=ticket, adam_step=adam_step, counter=counter)
    assert losses.tolist() == [SENTINEL, SENTINEL] and int(counter) == 3 and float(adam_step) == 4.0 and int(ticket) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# TD target

def run_td(pr, gamma):
    from bridges_hip import dqn_ops
    seg = (torch.tensor(pr["lo"], dtype=torch.int32, device=DEV), torch.tensor(pr["hi"], dtype=torch.int32, device=DEV))
    q, sf, rows = dqn_ops.td_target(seg, pr["next_q"], pr["lin"], torch.tensor(pr["done"], device=DEV), gamma, next_sf=pr["next_sf"],
                                    action_raster=pr["act"])
    return q, sf, rows.cpu().tolist()


@pytest.mark.parametrize("strided", [True, False])
@pytest.mark.parametrize("sf_dim", M.TD_SF_DIMS)
def test_td_target_on_the_segment_probes(sf_dim, strided):
    """Segments of 1 .. 700 rows (the strided loop over 256 threads), planted ties in one thread's strides and across the tree,
    an all -inf segment, an empty done one, (lo, hi) pairs that share rows; sf_dim 0 .. 4096, contiguous and as the psi[:, 0]
    view.  The rows exact, the targets within 2 u (|a| + |gamma s|) of the oracle's, exactly lin / the raster where done."""
    if sf_dim == 0 and not strided:
        strided = True                                                                  # nothing to stride: the same case once more
    pr = M.td_probe(sf_dim, DEV, strided=strided)
    assert sf_dim == 0 or (pr["next_sf"].stride(0) == (2 if strided else 1) * sf_dim)
    live_done = [i in (0, 3, 5, 7, 9) for i in range(len(pr["lo"]))]                   # a second mask; the empty segment stays done
    for done in (pr["done"], live_done):
        case = dict(pr, done=done)
        for gamma in (1.0, 0.8):
            ref, rows = M.td_ref(case, gamma)
            got = run_td(case, gamma)
            M.td_conform("td", got, M.td_plain(case, gamma), ref, rows, (sf_dim, strided, gamma))
            dn = torch.tensor(done, device=DEV)
            assert torch.equal(got[0][dn], pr["lin"][dn])
            if sf_dim:
                assert torch.equal(got[1][dn], pr["act"].reshape(len(done), -1)[dn])


def test_td_target_empty_segment_that_is_not_done_reads_no_row():
    """include/bridges_hip.h: an empty segment of a transition that is not done is the caller's error and is marked, not
    followed -- q = -inf, argmax_row = 0x7fffffff, the successor-feature part taken as zero."""
    g = torch.Generator().manual_seed(0)
    next_q = torch.tensor([1.0, 3.0], device=DEV)
    next_sf = M.dense(g, 2, 2, 8, 8).to(DEV)[:, 0]
    act = (torch.rand(2, 1, 8, 8, generator=g) > 0.5).float().to(DEV)
    pr = dict(lo=[0, 2], hi=[2, 2], done=[False, False], next_q=next_q, lin=torch.tensor([0.5, 0.25], device=DEV), next_sf=next_sf, act=act,
              sf_dim=64)
    q, sf, rows = run_td(pr, 0.8)
    assert rows == [1, M.NO_ROW] and float(q[1]) == -math.inf
    assert torch.equal(sf[1], act[1].reshape(-1))
    ref, ref_rows = M.td_ref(pr, 0.8)
    M.td_conform("td.empty", (q, sf, rows), M.td_plain(pr, 0.8), ref, ref_rows, (64, "empty"))


# ---------------------------------------------------------------------------------------------------------------------------
# Adam launches

GUARD = 4            # floats on either side of a tensor (16 bytes: the view behind them keeps the allocation's alignment)


def guarded(t, shift=0):
    """A copy of t [n] at float offset GUARD + shift of a buffer full of SENTINEL -> (buffer, view)."""
    buf = torch.full((t.numel() + 2 * GUARD + shift,), SENTINEL, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + t.numel()]
    view.copy_(t)
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + view.numel():] == SENTINEL).all())


def adam_conform(name, got, inputs, t, shape, pool):
    """Every element of a row inside the bound; the row joins ``pool``, over which the caller compares kernel and library: the
    update is elementwise, a row of 1 .. 5 elements gives one draw of either q (measured 0.41 against 0.09 at n = 5 where the
    rows of 1023 .. 4099 agree within a factor two), and nothing but its position tells one element of the table from another."""
    p, g, m, v = inputs
    refs, lb = M.adam_ref(p, g, m, v, t), M.adam_lib(p, g, m, v, t, fused=True)
    for k in ("p", "m", "v"):
        M.conform(f"{name}.{k}", got[k], lb[k], *refs[k], shape, tight=False)
        pool.setdefault(k, []).append((got[k], lb[k], *refs[k]))


def adam_pool_conform(name, pool, shape):
    for k in ("p", "m", "v"):
        M.conform_pooled(f"{name}.{k}.pooled", pool[k], shape)


@pytest.mark.parametrize("t", M.ADAM_STEPS)
def test_flat_adam_inside_the_bound(t):
    lr, b1, b2, eps = M.ADAM_HYPER
    step, pool = torch.full((), float(t), device=DEV), {}
    for n in M.ADAM_FLAT_N:
        inputs = M.adam_probe(n, DEV)
        bufs = [guarded(x) for x in inputs]
        (p, g, m, v) = [view for _, view in bufs]
        assert all(x.data_ptr() % 16 == 0 for x in (p, g, m, v))
        call("bridges_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(step), lr, b1, b2, eps, stream())
        adam_conform("adam_flat", dict(p=p.clone(), m=m.clone(), v=v.clone()), inputs, t, (n, t), pool)
        assert all(guards_intact(*bv) for bv in bufs) and torch.equal(g, inputs[1]), n
    adam_pool_conform("adam_flat", pool, (M.ADAM_FLAT_N, t))


@pytest.mark.parametrize("t", M.ADAM_STEPS)
def test_multi_tensor_adam_inside_the_bound(t):
    """Hand-built slots in ONE launch: aligned tensors, the same sizes as views that start 4 bytes into an allocation (the scalar
    path of a chunk) and one slot whose gradient alone is misaligned; guard words on both sides of every tensor."""
    from bridges_hip.dqn_ops import MultiTensorAdam
    lr, b1, b2, eps = M.ADAM_HYPER
    plan = [(n, (0, 0, 0, 0)) for n in M.ADAM_MULTI_N] + [(n, (1, 1, 1, 1)) for n in M.ADAM_MULTI_N] + [(1025, (0, 1, 0, 0))]
    slots, table, chunk_slot, chunk_off = [], np.zeros(len(plan), dtype=MultiTensorAdam._SLOT), [], []
    for i, (n, shifts) in enumerate(plan):
        inputs = M.adam_probe(n, DEV, seed=i)
        bufs = [guarded(x, s) for x, s in zip(inputs, shifts)]
        views = [view for _, view in bufs]
        assert [x.data_ptr() % 16 for x in views] == [4 * s for s in shifts]
        step_word = torch.full((), SENTINEL, device=DEV)
        table[i] = (*[x.data_ptr() for x in views], step_word.data_ptr(), n)
        chunks = M.ceil_div(n, MultiTensorAdam.CHUNK)
        chunk_slot += [i] * chunks
        chunk_off += list(range(chunks))
        slots.append((n, shifts, inputs, bufs, views, step_word))
    table_dev = torch.from_numpy(table.view(np.uint8)).to(DEV)
    done_so_far = torch.full((), float(t - 1), device=DEV)                              # this update is number *step + 1
    slot_dev, off_dev = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (chunk_slot, chunk_off))
    call("bridges_adam_multi", ptr(table_dev), len(plan), ptr(slot_dev), ptr(off_dev), len(chunk_slot), ptr(done_so_far), lr, b1, b2, eps,
         stream())
    pool = {}
    assert float(done_so_far) == t - 1                                                 # the caller advances it
    for n, shifts, inputs, bufs, (p, g, m, v), step_word in slots:
        adam_conform("adam_multi", dict(p=p.clone(), m=m.clone(), v=v.clone()), inputs, t, (n, shifts, t), pool)
        assert float(step_word) == t                                                   # the per-tensor step words are written
        assert all(guards_intact(*bv) for bv in bufs) and torch.equal(g, inputs[1]), (n, shifts)
    adam_pool_conform("adam_multi", pool, (len(plan), t))


# ---------------------------------------------------------------------------------------------------------------------------
# soft update

@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_soft_update_bitwise_below_two_float4(n):
    """n >> 2 == 0 (the scalar tail alone) and one float4 with a tail of three; tests/test_gpu_dqn.py holds n = 5."""
    from bridges_hip import dqn_ops
    from oracle import dqn as O
    g = torch.Generator().manual_seed(n)
    p, t = M.dense(g, n), M.dense(g, n)
    ref = O.update_target_net(dict(w=p), dict(w=t), 0.01)["w"]
    td = t.to(DEV)
    dqn_ops.soft_update_(td, p.to(DEV), 0.01)
    assert torch.equal(td.cpu(), ref)


# ---------------------------------------------------------------------------------------------------------------------------
# the middle stack, straight through the C ABI: host pointer tables as mlp_ops builds them, outputs full of SENTINEL

MID_DIMS_C = (C.c_int32 * 5)(*M.MID_DIMS)
F_MID, B_MID, R_MID = "bridges_mlp_mid_forward", "bridges_mlp_mid_backward", "bridges_mlp_mid_rows"


def table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def fresh(*shape):
    return torch.full(shape, SENTINEL, device=DEV)


def untouched(*tensors):
    return all(bool((t == SENTINEL).all()) for t in tensors)


def same_bits(a, b):
    """Equal bit for bit (so +0 differs from -0.0); a NaN equals any NaN: its payload is no value of the operator."""
    na, nb = torch.isnan(a), torch.isnan(b)
    bits = lambda t, n: torch.where(n, torch.zeros_like(t), t).contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(bits(a, na), bits(b, nb))


def off4(t):
    """A copy of t that starts 4 bytes into an allocation."""
    buf = fresh(t.numel() + 4)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def mid_forward(W, b, x):
    acts = [x.clone()] + [fresh(32, d) for d in M.MID_DIMS[1:]]
    call(F_MID, 32, 4, MID_DIMS_C, table(W), table(b), table(acts), stream())
    return acts


def mid_backward(W, acts, dz4, rest=(None, None, None, None), rest_n=0, step=None, hyper=M.ADAM_HYPER):
    """-> ({dW0..3, db0..3, dz0}, the dz table's five tensors)."""
    D = M.MID_DIMS
    dW, db = [fresh(D[l + 1], D[l]) for l in range(4)], [fresh(D[l + 1]) for l in range(4)]
    dz = [fresh(32, d) for d in D[:4]] + [dz4]
    call(B_MID, 32, 4, MID_DIMS_C, table(W), table(dW), table(db), table(acts), table(dz), *[ptr(r) for r in rest], rest_n, ptr(step),
         *hyper, stream())
    out = {f"dW{l}": dW[l] for l in range(4)}
    out.update({f"db{l}": db[l] for l in range(4)}, dz0=dz[0])
    return out, dz


def test_mid_forward_inside_the_bound_and_equal_to_the_layer_launches():
    """k_mid_fwd<256,128,64,128,256> at bridges_mlp_mid_forward on the lin_probe stack: every element of acts[1..4] within the
    one-layer float64 bound of lin_forward_ref on the kernel's own acts[l], q_kernel <= FACTOR q_library; acts[l + 1] bit for bit
    what bridges_linear_forward gives on acts[l] (the header's claim); a second call repeats; acts[0] is not written; a NaN in
    one input row makes that row NaN in all four outputs, leaves the 31 others bit-identical and matches the library's pattern."""
    pr = M.mid_probe(DEV)
    W, b, x = pr["W"], pr["b"], pr["x"]
    acts = mid_forward(W, b, x)
    M.mid_forward_conform("mid_fwd", acts[0], acts[1:], W, b)
    for l in range(4):
        assert same_bits(acts[l + 1], forward(acts[l], W[l], b[l], True)), l
    again = mid_forward(W, b, x)
    assert all(same_bits(p, q) for p, q in zip(again, acts)) and torch.equal(acts[0], x)
    xn = x.clone()
    xn[5, 17] = math.nan
    got, lb = mid_forward(W, b, xn), M.mid_forward_lib(W, b, xn)
    others = torch.arange(32, device=DEV) != 5
    for l in range(4):
        assert bool(torch.isnan(got[l + 1][5]).all()) and same_bits(got[l + 1][others], acts[l + 1][others]), l
        assert torch.equal(torch.isnan(got[l + 1]), torch.isnan(lb[l])), l


def test_mid_backward_inside_the_propagated_bounds_and_equal_to_the_layer_launches():
    """k_mid_bwd<256,128,64,128,256> at bridges_mlp_mid_backward, no riders, activations that are masks with +0, -0.0 and
    negatives: dz[0], dW[0..3] and db[0..3] within the bounds mid_backward_ref carries down the chain, q_kernel <= FACTOR
    q_library; dz[0] exactly 0 wherever acts[0] is not positive; bit for bit four chained bridges_linear_backward calls; dz[1..3]
    keep their sentinel, acts, W and dz[4] are not written; a second call repeats; with a NaN and an Inf in dz[4] every output
    is non-finite exactly where the library chain's is."""
    pr = M.mid_probe(DEV)
    W, acts, dz4 = pr["W"], pr["acts"], pr["dz4"]
    keep = [t.clone() for t in W + acts + [dz4]]
    a0 = acts[0]
    assert all(bool(c.any()) for c in ((a0 == 0) & ~torch.signbit(a0), (a0 == 0) & torch.signbit(a0), a0 < 0, a0 > 0))
    got, dz = mid_backward(W, acts, dz4)
    M.mid_backward_conform("mid_bwd", got, W, acts, dz4)
    assert bool((got["dz0"][~(a0 > 0)] == 0).all())
    z = dz4
    for l in (3, 2, 1, 0):
        one = backward(z, acts[l], W[l], acts[l])
        assert same_bits(one["dW"], got[f"dW{l}"]) and same_bits(one["db"], got[f"db{l}"]), l
        z = one["dx"]
    assert same_bits(z, got["dz0"])
    assert untouched(*dz[1:4]) and all(torch.equal(p, q) for p, q in zip(W + acts + [dz4], keep))
    again, _ = mid_backward(W, acts, dz4)
    assert all(same_bits(again[k], got[k]) for k in M.MID_BWD_KEYS)
    dzn = dz4.clone()
    dzn[3, 40], dzn[20, 200] = math.nan, math.inf
    gotn, dzs = mid_backward(W, acts, dzn)
    lb = M.mid_backward_lib(W, acts, dzn)
    for k in M.MID_BWD_KEYS:
        fin = torch.isfinite(lb[k])
        assert not bool(fin.all()), k
        assert torch.equal(torch.isfinite(gotn[k]), fin), (k, int((~torch.isfinite(gotn[k])).sum()), int((~fin).sum()))
    assert untouched(*dzs[1:4])


@pytest.mark.parametrize("t", M.ADAM_STEPS)
def test_mid_backward_riders_equal_the_flat_adam(t):
    """The rider workgroups of k_mid_bwd for every range of MID_REST_N (none, one float4, one ragged rider, two riders over three
    stride rounds, more than the cap of 248 over five): parameters and both moments bit for bit what bridges_adam_step gives on
    copies (one Adam struct) and within adam_ref's float64 bound; the chain's outputs bit for bit those of the call
    without riders; the gradient, *step and the four floats behind the range are not written."""
    pr = M.mid_probe(DEV)
    clean, _ = mid_backward(pr["W"], pr["acts"], pr["dz4"])
    step, pool = torch.full((), float(t), device=DEV), {}
    for rest_n in M.MID_REST_N:
        inputs = tuple(x[:rest_n] for x in M.adam_probe(max(rest_n, 4), DEV, seed=3))
        bufs = [torch.cat([x, fresh(4)]) for x in inputs]
        want = [x.clone() for x in bufs]
        call("bridges_adam_step", *[ptr(x) for x in want], rest_n, ptr(step), *M.ADAM_HYPER, stream())
        got, _ = mid_backward(pr["W"], pr["acts"], pr["dz4"], rest=bufs, rest_n=rest_n, step=step)
        for k, a, w in zip("pgmv", bufs, want):
            assert torch.equal(a, w), (rest_n, t, k, float((a.double() - w.double()).abs().max()))
        assert torch.equal(bufs[1][:rest_n], inputs[1]) and float(step) == t and untouched(*[x[rest_n:] for x in bufs]), rest_n
        assert all(same_bits(got[k], clean[k]) for k in M.MID_BWD_KEYS), rest_n
        if rest_n:
            adam_conform("mid_bwd.rider", dict(p=bufs[0][:rest_n], m=bufs[2][:rest_n], v=bufs[3][:rest_n]), inputs, t, (rest_n, t), pool)
    adam_pool_conform("mid_bwd.rider", pool, (M.MID_REST_N, t))


@pytest.mark.parametrize("n", M.MID_ROWS_N)
def test_mid_rows_inside_the_chain_bounds_and_equal_to_the_layer_launches(n):
    """k_rows2<256,128,64,true> and k_rows2<64,128,256,false> at bridges_mlp_mid_rows: ``mid`` (the first launch) and ``y`` (the
    second, from the kernel's own mid) within chain2_ref's propagated float64 bounds, q_kernel <= FACTOR q_library; both bit for
    bit bridges_linear_forward layer by layer on relu(x) in zero-padded rows.  The input holds negatives, -0.0 and (n >= 31) a
    row of NaN, which comes out as NaN.  Rows >= n of y and of mid (allocated to the next multiple of 32 plus a tile) and the
    columns of y between 256 and y_stride keep their sentinel; the columns of x beyond 256 hold NaN and are never read: every
    strided call gives the contiguous result.  n = 8193 and 16389 take a workgroup through a second and a third tile."""
    pr = M.mid_probe(DEV)
    W, b = pr["W"], pr["b"]
    nan_row = n - 2 if n >= 31 else None
    x = M.rows_probe(n, DEV, nan_row=nan_row)
    assert bool((x < 0).any()) and bool(((x == 0) & torch.signbit(x)).any())
    rows = M.rows_of(n)

    def run(xs, ys):
        xb = torch.full((n, xs), math.nan, device=DEV)
        xb[:, :256] = x
        yb, mb = fresh(rows + 32, ys), fresh(rows + 32, 64)
        call(R_MID, n, 4, MID_DIMS_C, table(W), table(b), ptr(xb), xs, ptr(yb), ys, ptr(mb), stream())
        assert untouched(yb[n:], yb[:n, 256:], mb[n:]) and same_bits(xb[:, :256], x), (xs, ys)
        return yb[:n, :256].contiguous(), mb[:n].clone()

    y, mid = run(256, 256)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    if nan_row is not None:
        keep[nan_row] = False
        assert bool(torch.isnan(y[nan_row]).all()) and bool(torch.isnan(mid[nan_row]).all())
    assert bool(torch.isfinite(y[keep]).all()) and bool(torch.isfinite(mid[keep]).all())
    M.rows_conform("mid_rows", x, mid, y, W, b, n, keep)
    a = torch.zeros((rows, 256), device=DEV)
    a[:n] = torch.relu(x)
    for l in range(4):
        a = forward(a, W[l], b[l], True)
        assert l != 1 or same_bits(mid, a[:n])
    assert same_bits(y, a[:n])
    for xs, ys in (M.MID_ROWS_STRIDES if n in M.MID_ROWS_STRIDED_N else M.MID_ROWS_STRIDES[:1]):       # (the first: a repeat)
        y2, mid2 = run(xs, ys)
        assert same_bits(y2, y) and same_bits(mid2, mid), (xs, ys)


def test_mid_stack_refusals_name_the_entry_point_and_leave_the_outputs_alone():
    """What csrc/api.hip refuses on the host, before any launch: rows != 32, another layer count or width, no bias table, a W[l],
    acts[l] or dz[4] that starts 4 bytes into an allocation; an Adam range that is no multiple of 4, has no step or a misaligned
    buffer, beta1 = 1, lr = NaN; for the many-rows call a stride below the width, an x stride that is no multiple of 4, no
    scratch, a misaligned x, n_rows < 0.  n_rows = 0 is BRIDGES_OK and writes nothing.  bridges_mlp_mid_supported is 1 for
    (32, 4, MID_DIMS) alone."""
    L = lib()
    pr = M.mid_probe(DEV)
    W, b, acts, dz4, D = pr["W"], pr["b"], pr["acts"], pr["dz4"], M.MID_DIMS
    facts = [pr["x"]] + [fresh(32, d) for d in D[1:]]
    dW, db = [fresh(D[l + 1], D[l]) for l in range(4)], [fresh(D[l + 1]) for l in range(4)]
    dz = [fresh(32, d) for d in D[:4]] + [dz4]
    rest, step = [fresh(8) for _ in range(4)], torch.ones((), device=DEV)
    rest_off, out_off = fresh(12)[1:9], off4(facts[4])
    bad_dims, swapped = (C.c_int32 * 5)(256, 128, 32, 128, 256), (C.c_int32 * 5)(128, 256, 64, 128, 256)
    swap = lambda seq, l, t: [t if i == l else s for i, s in enumerate(seq)]

    def fwd(rows=32, nl=4, dims=MID_DIMS_C, W_=W, b_=b, acts_=facts):
        return L.bridges_mlp_mid_forward(rows, nl, dims, table(W_), table(b_) if b_ is not None else None, table(acts_), stream())

    def bwd(rows=32, nl=4, dims=MID_DIMS_C, W_=W, acts_=acts, dz_=dz, rest_=rest, rest_n=0, step_=step, hyper=M.ADAM_HYPER):
        return L.bridges_mlp_mid_backward(rows, nl, dims, table(W_), table(dW), table(db), table(acts_), table(dz_), *[ptr(r) for r in rest_],
                                          rest_n, ptr(step_), *hyper, stream())

    for fn, who in ((fwd, F_MID), (bwd, B_MID)):
        refused(fn(rows=64), who)
        refused(fn(nl=3), who)
        refused(fn(dims=bad_dims), who)
        for l in (0, 2):
            refused(fn(W_=swap(W, l, off4(W[l]))), who)
    refused(fwd(b_=None), F_MID)
    refused(fwd(acts_=swap(facts, 0, off4(facts[0]))), F_MID)
    refused(fwd(acts_=swap(facts, 4, out_off)), F_MID)
    refused(bwd(acts_=swap(acts, 1, off4(acts[1]))), B_MID)
    refused(bwd(dz_=swap(dz, 4, off4(dz4))), B_MID)
    lr, b1, b2, eps = M.ADAM_HYPER
    refused(bwd(rest_n=6), B_MID)
    refused(bwd(rest_n=4, step_=None), B_MID)
    refused(bwd(rest_n=4, rest_=swap(rest, 2, rest_off)), B_MID)
    refused(bwd(rest_n=4, hyper=(lr, 1.0, b2, eps)), B_MID)
    refused(bwd(rest_n=4, hyper=(math.nan, b1, b2, eps)), B_MID)

    x = M.rows_probe(33, DEV)
    xw = torch.zeros((33, 260), device=DEV)
    yb, mb = fresh(96, 256), fresh(96, 64)

    def rows_call(n=33, x_=x, xs=256, ys=256, mid_=mb):
        return L.bridges_mlp_mid_rows(n, 4, MID_DIMS_C, table(W), table(b), ptr(x_), xs, ptr(yb), ys, ptr(mid_), stream())

    refused(rows_call(xs=252), R_MID)
    refused(rows_call(x_=xw, xs=258), R_MID)
    refused(rows_call(ys=255), R_MID)
    refused(rows_call(mid_=None), R_MID)
    refused(rows_call(x_=off4(x)), R_MID)
    refused(rows_call(n=-1), R_MID)
    assert rows_call(n=0) == 0
    torch.cuda.synchronize()
    assert untouched(*facts[1:], out_off, *dW, *db, *dz[:4], *rest, rest_off, yb, mb) and float(step) == 1.0

    S = L.bridges_mlp_mid_supported
    assert S(32, 4, MID_DIMS_C) == 1
    assert [S(64, 4, MID_DIMS_C), S(0, 4, MID_DIMS_C), S(31, 4, MID_DIMS_C), S(32, 3, MID_DIMS_C), S(32, 5, MID_DIMS_C), S(32, 4, bad_dims),
            S(32, 4, swapped), S(32, 4, None)] == [0] * 8
