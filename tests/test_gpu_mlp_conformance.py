"""GPU: conformance of the SuccessorMLP step kernels (csrc/mlp_kernels.hip: k_lin_fwd, k_lin_bwd, k_successor_loss and the
folded Adam update) and of the scalar-ish DQN kernels (csrc/dqn_kernels.hip: k_td_target, k_adam_flat, k_adam_multi,
k_soft_update) at the entry points of include/bridges_hip.h.

Tables, probe data, float64 references, bounds and the acceptance rule come from tests/mlp_conformance.py (checked without a GPU
by tests/test_cpu_mlp_conformance_refs.py, which also shows that a kernel wrong in one of seven ways would be rejected):

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


def test_linear_refusals_name_their_reason_and_leave_the_output_alone():
    from bridges_hip import abi
    L = lib()
    pr = M.lin_probe(64, 70, 33, DEV)
    x, w, b, dz, act = (pr[k] for k in ("x", "w", "b", "dz", "act"))
    y = torch.full((64, 33), SENTINEL, device=DEV)
    dW, db, dx = torch.full((33, 70), SENTINEL, device=DEV), torch.full((33,), SENTINEL, device=DEV), torch.full((64, 70), SENTINEL, device=DEV)
    ws = workspace()

    def refused(rc, reason):
        assert rc != 0
        msg = L.bridges_last_error().decode()
        assert reason in msg, msg
        with pytest.raises(abi.BridgesHipError, match=reason):
            abi.check(rc, "entry point")

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
