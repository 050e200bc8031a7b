"""The captured optimiser step shared by both training loops, train_policy_net (successor_dqn.py) and VecDQN.train_steps
(vec_dqn.py): which body a step runs, when it is captured as a HIP graph and replayed, how it warms up, when it is switched
off, and how Adam's step count goes back to the torch optimiser.  One driver per policy net, ``net._fused_trainer``
(the name of the attribute since the hand-written step was its first body)."""
import gc
import os
import warnings

import numpy as np
import torch

from bridges_hip import dqn_ops, ops


def graph_enabled(default):
    """BRIDGES_TRAIN_GRAPH=0/1 overrides a loop's default: optimiser steps as replays of a captured graph, or eager.

    VecDQN: on for SuccessorMLP, whose step has no multi-workgroup reduction left in it and is verified against the eager run
    at the bench size (tests/test_gpu_vec_dqn.py); on for ConvNet: its ConvBlocks run forward and backward on the hand-written
    kernels (deterministic partial-sum reductions, csrc/conv_train_kernels.hip), what is left of the library in its step are
    single-workgroup reductions over the 32 batch rows, the eager step is bound by the host (1.2 ms of Python and launches for
    0.57 ms of GPU work), and the replays run under the on-device restore guard (_guard_restore); on for the U-Net policy as
    well: its 3x3 convolutions are the hand-written ones, its transposed and 1x1 convolutions run on
    dqn_ops.UpConv2x2Function / Conv1x1O1Function, deterministic partial sums as well.  train_policy_net: on."""
    return os.environ.get("BRIDGES_TRAIN_GRAPH", "1" if default else "0") == "1"


def fused_step_enabled(net, loss_parts):
    """The hand-written step (bridges_hip/mlp_ops.py FusedSuccessorStep) applies to a float32 SuccessorMLP with the two MSE
    losses of the CLI (BRIDGES_FUSED_MLP_STEP=0: the autograd body, as before it)."""
    from robotoddler.models.cv import SuccessorMLP
    return (isinstance(net, SuccessorMLP) and os.environ.get("BRIDGES_FUSED_MLP_STEP", "1") != "0"
            and set(loss_parts) <= {'mse_q_values', 'mse_block_features'}
            and all(p.dtype == torch.float32 for p in net.parameters()))


def conv_task_net(net):
    """True for the conv Q-networks that take a task as image channels at 64x64: a ConvNet(in_channels=4, img_size=(64, 64)) or
    the U-Net Policy -- the nets whose input rows ops.conv_input builds."""
    from robotoddler.models.cv import ConvNet, Policy
    if isinstance(net, Policy):
        return True
    return (isinstance(net, ConvNet) and net.layers[0].layers[0].in_channels == 4
            and net.bottleneck_size == 128 * (64 // 16) * (64 // 16))


def sync_optimizer(policy_net):
    """Hand Adam's step count back to the torch optimiser (the hand-written step counts it itself; its moments already are the
    optimiser's state tensors): call before optimizer.state_dict() / optimizer.step() after either loop trained the net."""
    drv = getattr(policy_net, "_fused_trainer", None)
    if drv is not None:
        drv.sync()


def release(policy_net):
    """Sync and drop the net's driver: the next call builds and captures the step afresh (e.g. after the optimiser's
    hyper-parameters changed, which a captured step holds as constants)."""
    sync_optimizer(policy_net)
    policy_net._fused_trainer = None


def _put(dst, src):
    """src into the leading elements of the static buffer dst (one copy)."""
    dst.view(-1)[:src.numel()].view(src.shape).copy_(src)


class CapturedTrainStep:
    """n optimiser steps of a policy net on the n batches of one call.

    Two bodies.  The hand-written SuccessorMLP step (FusedSuccessorStep.launch: forward, both MSE losses, backward and Adam as
    ~11 launches on the f32 matrix cores instead of ~60 library / element-wise ones) reads its batch from a device-side
    counter, so the n steps of a call are captured as ONE graph per step count n: inside a graph consecutive kernels follow
    each other without the ~9 us gap between two graph launches.  The autograd body (forward, loss, backward, Adam of the conv
    nets, and of the MLP with BRIDGES_FUSED_MLP_STEP=0) is one single-step graph replayed n times; it is not chained, because
    it holds library reductions (see check_losses) and runs under the restore guard.  Either way the per-call inputs go into
    static buffers first (``prepared``: the hand-written step's first-layer rows of all batches are built by one launch
    instead), the losses land in a device buffer, and a call has no host wait.

    Warm-up: the first ``warmup`` calls run eagerly -- the body's launches queued one by one (``eager_body``), or ``run``
    returns None and the caller takes its own eager step (VecDQN: it initialises the optimiser state and the library
    workspaces a capture needs).  A call with more batches than the buffers hold rebuilds the buffers and the body and
    captures again; a failed capture (RuntimeError) or an invalid logged loss switches the driver to eager for good."""

    def __init__(self, net, optimizer, batch, loss_parts, img, fused, graph_default=True, warmup=1, eager_body=True,
                 prepared=False, task=None, owner=None, task_rows=False, obstacle_rows=False, weights=False):
        self.net, self.opt, self.B, self.img = net, optimizer, int(batch), tuple(int(s) for s in img)
        # weights (importance-sampling weights of prioritised replay): ``run`` takes weights [n * B] float32 and copies them into
        # the static w [n_max * B]; the hand-written step scales row b's loss share and gradient coefficients by w_b
        # (bridges_successor_loss_weighted), the autograd body its per-row terms before the reduction over the batch rows.  Part
        # of the key: a net is never replayed with a graph captured for the other form
        self.weights = bool(weights)
        self.key = (optimizer, self.B, tuple(loss_parts), owner, self.weights)
        self.use_q, self.use_sf = 'mse_q_values' in loss_parts, 'mse_block_features' in loss_parts
        self.fused, self.graph_default, self.warmup, self.eager_body = fused, graph_default, warmup, eager_body
        self.prepared, self.task = prepared, task         # task: the (reward, obstacle) maps of every call (None: per call)
        # task_rows (per-env tasks; the hand-written step only): every transition has a reward map of its own -- ``run`` takes
        # them as reward [n * B, px] and copies them into a static [n_max * B, px] buffer the captured launches read with a
        # row stride, so the graph replays unchanged; task = (None, obstacle): the obstacle map stays shared
        # obstacle_rows (per-env obstacles; with task_rows only): every transition has an obstacle raster of its own too --
        # ``run`` takes them bit-packed as obstacle [n * B, 64] int64 and copies them into a static [n_max * B, 64] buffer the
        # captured launches read (bridges_mlp_input_task_rows / _batches_task_rows); task = (None, None)
        # task_rows with the autograd body (fused=False; the conv nets at 64x64 only): ``run`` takes block / action BIT-PACKED
        # ([n * B, 64] int64 each), and ONE ops.conv_input launch per call writes the stacked rows of all n * B transitions into
        # the static x_all [n_max * B, 4, 64, 64] -- no f32 block / action images, no staging copies; the captured step takes
        # batch `counter` of x_all.  task = (None, obstacle_bits [64] int64): the shared obstacle raster, bit-packed as well
        self.task_rows, self.obstacle_rows = bool(task_rows), bool(obstacle_rows)
        self.conv_rows = self.task_rows and not fused and conv_task_net(net) and self.img == (64, 64)
        if self.task_rows and not ((fused or self.conv_rows) and task is not None and task[0] is None):
            raise ValueError("per-transition reward maps need the hand-written step (fused=True) -- or, with the autograd body, a "
                             "conv net that takes the task as image channels (ConvNet(in_channels=4, img_size=(64, 64)) or Policy "
                             "at 64x64) -- and task=(None, obstacle)")
        if self.obstacle_rows and not (self.task_rows and task[1] is None):
            raise ValueError("per-transition obstacle rasters need per-transition reward maps (task_rows=True) and task=(None, None)")
        if self.task_rows and not self.obstacle_rows and task[1] is None:
            raise ValueError("task=(None, None) needs obstacle_rows=True: without it the obstacle map is the shared task[1]")
        self.calls, self.disabled, self.n_max = 0, False, 0
        self.step = self.adam = self.state = None
        self._graphs = {}

    @classmethod
    def of(cls, net, optimizer, batch, loss_parts, n, owner=None, **config):
        """The net's driver for this optimiser / batch size / loss / owner, built on first use after the previous one handed
        its state back: one driver per net, so no two hand-written steps adopt the same Adam state.  A driver with an eager
        body builds it here (for n batches): ValueError if the hand-written step does not take the optimiser over."""
        drv = getattr(net, "_fused_trainer", None)
        if drv is None or drv.key != (optimizer, int(batch), tuple(loss_parts), owner, bool(config.get("weights", False))):
            release(net)
            drv = cls(net, optimizer, batch, loss_parts, owner=owner, **config)
            if drv.eager_body:
                drv._build(n)
            net._fused_trainer = drv
        return drv

    def _build(self, n):
        """Static buffers for n batches and a fresh body; every graph is dropped (after Adam's step count went back)."""
        self.sync()
        B, S, dev = self.B, self.img, next(self.net.parameters()).device
        N, px = n * B, S[0] * S[1]
        z = lambda *s: torch.zeros(s, device=dev)
        self._graphs, self.n_max = {}, n
        self.state = dict(n_max=n, fused=self.fused)        # of this build; the guard keeps its snapshot here
        self.binary, self.q = z(N, 6), z(N)
        self.block, self.action = (None, None) if self.conv_rows else (z(N, 1, *S), z(N, 1, *S))
        self.x_all = z(N, 4, *S) if self.conv_rows else None
        self.sf = z(N, px) if self.use_sf else None
        self.w = z(N) if self.weights else None
        self.counter, self.losses = torch.zeros((), dtype=torch.int64, device=dev), z(n)
        self.lane, self.iota = torch.arange(B, device=dev), torch.arange(n, device=dev)
        if self.conv_rows:                                 # read from the caller's tensors by the one launch of a call
            self.reward, self.obstacle = None, (None if self.obstacle_rows else self.task[1].reshape(1, 64).contiguous())
        elif self.obstacle_rows:
            self.reward, self.obstacle = z(N, px), torch.zeros((N, 64), dtype=torch.int64, device=dev)
        elif self.task_rows:
            self.reward, self.obstacle = z(N, px), self.task[1].reshape(-1).contiguous()
        else:
            self.reward, self.obstacle = (z(px), z(px)) if self.task is None else (t.reshape(-1).contiguous() for t in self.task)
        self.net.train()
        self.opt.zero_grad(set_to_none=True)
        self.step = self.adam = None
        if self.fused:
            from bridges_hip.mlp_ops import FusedSuccessorStep
            self.step = FusedSuccessorStep(self.net, B, self.use_q, self.use_sf, optimizer=self.opt)
            if self.eager_body and not self.step.fused_adam:
                raise ValueError("the optimiser is not a plain Adam over the net's flattened parameters")
            if self.prepared:
                # the first layer's input rows of all batches of a call are built by ONE launch before the replays (run), a
                # replayed step reads batch `counter` of them: one launch per optimiser step less
                self.step.allocate_inputs(n)
                self.step._prepared = True               # captured in the form that reads the pre-built rows
        else:
            self.reduce = dqn_ops.ReduceTables(dev)
            try:
                self.adam = dqn_ops.MultiTensorAdam(self.opt)
            except ValueError:
                pass                                       # another optimiser, or one with options the launch does not cover

    def _fused_body(self, block, action, binary, reward, obstacle, q, sf, w=None):
        self.step.launch(self.counter, block, action, binary, reward, obstacle, q, sf, self.losses, weight_all=w)
        if not self.step.fused_adam:                       # else the Adam update is the last launch of the sequence
            self.opt.step()

    def _autograd_body(self):
        B, S = self.B, self.img
        idx = self.lane + self.counter * B
        if self.conv_rows:
            x = self.x_all.index_select(0, idx)            # the four channel views: the net stacks them back without a copy
            q, sf, _ = self.net(x[:, 0:1], self.binary.index_select(0, idx), x[:, 1:2], x[:, 2:3], x[:, 3:4])
        else:
            reward = self.reward.view(1, 1, *S).expand(B, -1, -1, -1)
            obstacle = self.obstacle.view(1, 1, *S).expand(B, -1, -1, -1)
            q, sf, _ = self.net(self.block.index_select(0, idx), self.binary.index_select(0, idx), self.action.index_select(0, idx),
                                reward, obstacle)
        # the MSE losses, but the 131 072-element mean is reduced row-wise and then over the 32 rows: the multi-workgroup
        # (semaphore) reduction nn.MSELoss launches for it returned garbage on some replays (negative "MSE", ROCm 7.2 + torch
        # 2.10; eager never) while every single-workgroup reduction was right.  The value is logged through a one-hot of the
        # step counter (pure elementwise arithmetic).
        loss = 0.
        if self.weights:                                   # every row's term times its weight, before the reduction over the rows
            w = self.w.index_select(0, idx)
            if self.use_q:
                loss = loss + (w * (q - self.q.index_select(0, idx)) ** 2).mean()
            if self.use_sf:
                loss = loss + (w * ((sf[:, 0].reshape(B, -1) - self.sf.index_select(0, idx)) ** 2).mean(dim=1)).mean()
        else:
            if self.use_q:
                loss = loss + ((q - self.q.index_select(0, idx)) ** 2).mean()
            if self.use_sf:
                loss = loss + ((sf[:, 0].reshape(B, -1) - self.sf.index_select(0, idx)) ** 2).mean(dim=1).mean()
        self.losses.add_((self.iota == self.counter).to(torch.float32) * loss.detach())
        with dqn_ops.deferred_wgrad_reduce(self.reduce):   # the conv layers' weight-gradient reductions as one launch
            loss.backward()
        if self.adam is not None:
            self.adam.step()                               # one launch of 1024-element chunks over all parameter tensors
        else:
            self.opt.step()
        self.counter.add_(1)

    def _capture(self, m):
        # No garbage collection between capture_begin and capture_end: a dead reference cycle that holds GPU objects (an earlier
        # agent with its env, its captured graphs and their memory pool) would be destroyed inside the capture, where freeing
        # device memory is not permitted -- the process aborted there.  torch.cuda.graph no longer collects before it begins a
        # capture, so collect here, and keep the collector off until the capture has ended.
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(m):
                    if self.fused:
                        N = self.n_max * self.B
                        self._fused_body(self.block.view(N, -1), self.action.view(N, -1), self.binary, self.reward, self.obstacle,
                                         self.q, self.sf, self.w)
                    else:
                        self._autograd_body()
        finally:
            if collecting:
                gc.enable()
        return graph

    def _check_hyperparameters(self):
        body = self.step if self.fused else self.adam
        if body is not None:
            body.check_hyperparameters()

    def run(self, n, block, action, binary, reward, obstacle, q, sf, weights=None):
        """n optimiser steps on batches 0 .. n-1 of the per-call arrays (rows b * B .. b * B + B - 1 of block / action /
        binary / q / sf; reward / obstacle: one map for all rows, unused with ``task`` -- except with ``task_rows``, where
        reward [n * B, px] holds the map of every transition, and with ``obstacle_rows``, where obstacle [n * B, 64] int64 holds
        the bit-packed obstacle raster of every transition; ``task_rows`` with the autograd body: block / action [n * B, 64]
        int64 are the bit-packed rasters of every transition too; a driver built with ``weights=True``: weights [n * B] float32,
        the importance-sampling weight of every transition) -> the device tensor of the n losses
        (a view of the driver's buffer, valid until its next call), or None: the caller steps eagerly."""
        if self.weights != (weights is not None):
            raise ValueError("CapturedTrainStep.run: weights are given exactly to a driver built with weights=True")
        graphs = not self.disabled and graph_enabled(self.graph_default)
        if not graphs or self.calls < self.warmup:
            self.calls += graphs
            if not self.eager_body:
                return None
            if n > self.n_max:
                self._build(n)
            self._check_hyperparameters()
            self.counter.zero_()
            self.losses.zero_()
            if self.task_rows:
                reward = reward.reshape(n * self.B, -1).contiguous()
                obstacle = obstacle.reshape(n * self.B, 64).contiguous() if self.obstacle_rows else self.obstacle
            if self.weights:
                weights = weights.reshape(-1).contiguous()
            for _ in range(n):
                self._fused_body(block, action, binary, reward, obstacle, q, sf, weights)
            return self.losses[:n]
        if n > self.n_max:                                 # the first capture, or more batches than the buffers hold
            self._build(n)
        self._check_hyperparameters()
        m = n if self.fused else 1
        graph = self._graphs.get(m)
        if graph is None:
            try:
                graph = self._graphs[m] = self._capture(m)
            except RuntimeError as e:                      # same arithmetic either way: keep training eagerly
                warnings.warn(f"train-step graph capture failed, staying eager: {e}")
                self._disable()
                return self.run(n, block, action, binary, reward, obstacle, q, sf, weights)
        N = n * self.B
        if self.task_rows and not self.conv_rows:
            _put(self.reward, reward.reshape(N, -1))       # before the first-layer rows are built from it
            if self.obstacle_rows:
                _put(self.obstacle, obstacle.reshape(N, 64))
        if self.conv_rows:
            # the stacked rows of all n batches in one launch, straight from the caller's bit rasters and maps
            ops.conv_input(block, action, reward.reshape(N, -1).contiguous(), obstacle if self.obstacle_rows else self.obstacle,
                           out=self.x_all[:N])
            _put(self.binary, binary)
        elif self.fused and self.prepared:
            # the first layer's input rows of all n batches in one launch, straight from the caller's tensors (no staging
            # copy of the block / action images: a replayed step reads only x_all, q and sf)
            self.step.prepare_inputs(n, block.reshape(N, -1).contiguous(), action.reshape(N, -1).contiguous(),
                                     binary.contiguous(), self.reward, self.obstacle)
        else:
            _put(self.block, block); _put(self.binary, binary); _put(self.action, action)
            if self.task is None:
                _put(self.reward, reward); _put(self.obstacle, obstacle)
        if not self.fused:
            self._guard_snapshot(self.state)
        if q is not None:
            _put(self.q, q)
        if sf is not None:
            _put(self.sf, sf)
        if self.weights:
            _put(self.w, weights.reshape(-1))
        self.counter.zero_()
        self.losses.zero_()
        for _ in range(n // m):
            graph.replay()
        if not self.fused:
            self._guard_restore(self.state, self.losses[:n])
        return self.losses[:n]

    # The replayed autograd step of the conv nets holds library reductions; one of that kind once returned garbage inside a
    # replayed graph (see check_losses).  The host learns of a bad loss one lock-step late (deferred read-back), so the
    # weights are protected ON THE DEVICE: parameters and Adam state are copied before the replays of a call and put back --
    # a torch.where on a device flag, no host decision -- when any of the call's losses is negative or not finite.  The
    # call's optimiser steps are then lost, not applied as garbage; the host switches to the eager step when it sees the loss.
    def _guard_tensors(self):
        flat = getattr(self.net, "_flat_params", None)
        ts = [flat.flat] if flat is not None else [p.data for p in self.net.parameters()]
        for s in self.opt.state.values():
            ts += [t for t in s.values() if torch.is_tensor(t) and t.is_cuda]
        if self.adam is not None:
            ts.append(self.adam.step_count)
        return ts

    def _guard_snapshot(self, st):
        ts = self._guard_tensors()
        snap = st.get("guard")
        if snap is None or len(snap) != len(ts) or any(a.shape != b.shape for a, b in zip(snap, ts)):
            st["guard"] = [t.clone() for t in ts]
        else:
            torch._foreach_copy_(snap, ts)

    def _guard_restore(self, st, losses):
        bad = ~(torch.isfinite(losses).all() & (losses >= 0).all())
        for t, s in zip(self._guard_tensors(), st["guard"]):
            torch.where(bad, s, t, out=t)

    def check_losses(self, losses):
        """Guard for the anomaly recorded in DESIGN.md: a multi-workgroup reduction inside a replayed graph once returned
        garbage (a negative "MSE"; ROCm 7.2 + torch 2.10, cause not established).  The graph holds only single-workgroup
        reductions since, and every replay's loss is checked here: a sum of squares that is negative or not finite
        means a kernel in the graph misbehaved -- from then on the step runs eagerly."""
        if not all(np.isfinite(l) and l >= 0.0 for l in losses):
            warnings.warn(f"train-step graph produced an invalid loss {losses}; switching to the eager step")
            self._disable()
        return losses

    def _disable(self):
        self.sync()
        self.disabled, self.n_max, self._graphs = True, 0, {}
        self.step = self.adam = self.state = None

    def sync(self):
        if self.step is not None:
            self.step.export_state()                       # (a no-op unless the step runs Adam itself)
