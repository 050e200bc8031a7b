"""Helpers shared by the GPU parity tests (not a test module)."""
import ctypes as C

import torch

from bridges_hip import abi


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def candidate_stability_unfused(env, chunk=8192):
    """The round-1 way of deciding is_action_stable_rbe for every valid candidate: gather a padded copy of the env's
    block list per candidate in torch, append the candidate, and let the stand-alone ``bridges_stability`` operator
    re-detect every interface from scratch.  Kept as an independent second path to cross-check the fused kernel at
    sizes the CPU oracle cannot reach.  Returns (rows, stable bool, error bool)."""
    L = abi.require_gpu()
    idx, row_env = env.valid_rows()
    n = idx.numel()
    K16 = abi.MAX_BLOCKS
    out = torch.zeros(n, dtype=torch.bool, device=env.device)
    errs = torch.zeros(n, dtype=torch.bool, device=env.device)
    if n == 0:
        return idx, out, errs
    ws_stride = abi.lp_ws_stride(K16)
    stab_ws = torch.empty((min(chunk, n), ws_stride), dtype=torch.float64, device=env.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lo in range(0, n, chunk):
        ii, ee = idx[lo:lo + chunk], row_env[lo:lo + chunk]
        m = ii.numel()
        nb = env.buf["n_blocks"][ee].long()
        pose = torch.zeros((m, K16, 4), dtype=torch.float64, device=env.device)
        verts = torch.zeros((m, K16, 6, 2), dtype=torch.float64, device=env.device)
        shape = torch.zeros((m, K16), dtype=torch.int32, device=env.device)
        pose[:, :env.K] = env.buf["blk_pose"][ee]
        verts[:, :env.K] = env.buf["blk_verts"][ee]
        shape[:, :env.K] = env.buf["blk_shape"][ee]
        r = torch.arange(m, device=env.device)
        pose[r, nb] = env.buf["cand_pose"][ii]
        verts[r, nb] = env.buf["cand_verts"][ii]
        shape[r, nb] = env.buf["cand_desc"][ii, 2]
        nblocks = (nb + 1).to(torch.int32)
        fixed = torch.where(nb > 0, torch.ones_like(nb) << (nb - 1).clamp(min=0), torch.zeros_like(nb)).to(torch.int32)
        stable = torch.zeros(m, dtype=torch.uint8, device=env.device)
        info = torch.zeros((m, 8), dtype=torch.float64, device=env.device)
        fh, fd = env._create_args
        abi.check(L.bridges_stability(env.table.ptr, m, K16, _ptr(pose), _ptr(verts), _ptr(shape), _ptr(nblocks),
                                      _ptr(fixed), env.mu, env.density, fh, fd, _ptr(stable), _ptr(info),
                                      _ptr(stab_ws), ws_stride, stream), "bridges_stability")
        torch.cuda.synchronize()
        out[lo:lo + m] = stable.bool() & (info[:, 3] == 0)
        errs[lo:lo + m] = info[:, 3] != 0
    return idx, out, errs


# ---- conformance of the conv kernels against float64 (tests/test_gpu_conv_conformance.py) ----------------------------------
import contextlib
import copy

U32 = 2.0 ** -24                                   # unit roundoff of float32
PREDICATES = ("conv3x3_supported", "conv3x3_relu_o16_applies", "upconv2x2_applies", "upconv2x2_train_applies",
              "conv1x1_o1_applies", "maxpool2_of_relu_applies")


def ref64(fn, *tensors):
    """fn on the float64 copies of the tensors (same device): the plain torch.nn.functional statement of an operator."""
    return fn(*[t.double() if torch.is_tensor(t) and t.is_floating_point() else t for t in tensors])


def dot_bound(K, abs_terms):
    """Forward-error bound of a float32 dot product of K terms summed in ANY order: gamma_K * sum |x_k w_k| with
    gamma_K = K u / (1 - K u), u = 2**-24 (Higham, Accuracy and Stability, eq. 3.5), plus K * 2**-126 so that a product flushed
    to zero is no error.  ``abs_terms``: the operator applied to |x|, |w|, |b| in float64."""
    assert K * U32 < 0.5
    return abs_terms.double() * (K * U32 / (1.0 - K * U32)) + K * 2.0 ** -126


def library_twin(net):
    """A float64 copy of the net: every predicate of dqn_ops / cv.py demands float32, so the copy runs plain nn layers."""
    return copy.deepcopy(net).double()


@contextlib.contextmanager
def all_predicates_off():
    """The float32 LIBRARY path of the conv nets: every ``*_applies`` / ``*_supported`` predicate of dqn_ops answers False, the
    fused inference epilogues of cv.py are off and the bias of a transposed / 1x1 convolution stays with the library (no
    bridges_bias_grad), so no hand-written conv kernel is left on a forward or backward pass.  Restored on exit."""
    from bridges_hip import dqn_ops
    from robotoddler.models import cv
    saved = {name: getattr(dqn_ops, name) for name in PREDICATES + ("conv_bias_train",)}
    saved_fused = cv._fused_inference
    try:
        for name in PREDICATES:
            setattr(dqn_ops, name, lambda *a, **k: False)
        dqn_ops.conv_bias_train = lambda module, x: module(x)
        cv._fused_inference = lambda x: False
        yield
    finally:
        for name, fn in saved.items():
            setattr(dqn_ops, name, fn)
        cv._fused_inference = saved_fused


def hand_written_nodes(*outputs):
    """Names of the dqn_ops autograd Functions in the graphs of the given tensors (the backward nodes ``<Name>Backward``)."""
    from bridges_hip import dqn_ops
    names = {n + "Backward" for n in dir(dqn_ops) if n.endswith("Function")}
    seen, found, todo = set(), set(), [t.grad_fn for t in outputs if torch.is_tensor(t) and t.grad_fn is not None]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__ in names:
            found.add(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return sorted(found)
