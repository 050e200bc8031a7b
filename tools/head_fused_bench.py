"""Fused head (bridges_head_sigmoid_dot) against the library GEMM + bridges_sigmoid_dot on the acting forward's row count.
With --maps M also the per-row-map head (bridges_head_sigmoid_dot_rows: per-env tasks) on the same rows, spread over M maps
env-major (a 128-row workgroup touches a handful of maps, as candidate rows do) and shuffled (16 different maps per lane).
Usage: python tools/head_fused_bench.py [--rows 45056] [--reps 20] [--maps 4096]"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = importlib.import_module("bridges-with-reinforcement-learning_amd")
from importlib import import_module

ops = import_module("bridges-with-reinforcement-learning_amd.bridges_hip.ops")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45056)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=0, help="> 0: also time the per-row-map head with this many reward maps")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    n, K, N = a.rows, 256, 4096
    h = torch.relu(torch.randn(n, K, device=dev, generator=g))
    Wd = torch.randn(N, K, device=dev, generator=g) * 0.05
    bd = torch.randn(N, device=dev, generator=g) * 0.1
    w = torch.randn(N, device=dev, generator=g)

    def two_pass():
        d = torch.addmm(bd, h, Wd.T)
        return ops.sigmoid_dot(d, w)

    def fused(splits=None):
        return ops.head_sigmoid_dot(h, Wd, bd, w, splits=splits)

    ref = (torch.sigmoid(h.double() @ Wd.double().T + bd.double()) * w.double()).sum(1)
    import functools
    cases = [("gemm+sigmoid_dot", two_pass), ("fused (auto)", fused)]
    cases += [(f"fused splits={s}", functools.partial(fused, s)) for s in (1, 2, 4, 8, 16, 32)]
    refs = {}
    if a.maps > 0:
        w_all = torch.randn(a.maps, N, device=dev, generator=g)
        rows_of = dict(env_major=(torch.arange(n, device=dev) * a.maps // n).to(torch.int32),
                       shuffled=torch.randint(0, a.maps, (n,), device=dev, generator=g).to(torch.int32))
        for order, w_row in rows_of.items():
            sig = torch.sigmoid(h.double() @ Wd.double().T + bd.double())
            r = torch.empty(n, dtype=torch.float64, device=dev)
            for o in range(0, n, 4096):                    # in chunks: [n, N] float64 maps would be 1.5 GB
                r[o:o + 4096] = (sig[o:o + 4096] * w_all[w_row[o:o + 4096].long()].double()).sum(1)
            for s_ in (None, 8):
                name = f"rows {order} " + ("(auto)" if s_ is None else f"splits={s_}")
                cases.append((name, functools.partial(ops.head_sigmoid_dot, h, Wd, bd, w_all, s_, w_row)))
                refs[name] = r
    for name, fn in cases:
        out = fn()
        err = (out.double() - refs.get(name, ref)).abs().max().item()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        print(f"{name:26s} {ms:8.3f} ms  {2.0 * n * K * N / ms / 1e9:7.1f} TFLOP/s  max |err| vs f64 {err:.3e}", flush=True)


if __name__ == "__main__":
    main()
