"""k_conv_input against the torch formulation it replaces, on identical inputs in one process: the stacked [n, 4, 64, 64] input of
the conv Q-networks from bit-packed rasters and a map index (ops.conv_input, one launch) beside two index_selects out of f32
rasters, an expand and a cat.  HIP events around single launches, both sides alternating, warm-up first; prints one JSON line
with the medians, the spread (min, max, inter-quartile range) and the achieved bytes per second.
    python tools/conv_input_bench.py [--rows 2048] [--envs 1024] [--cands 40000] [--reps 40] [--shared_obstacle]
Bytes the kernel moves per row: 64 KiB written, 16 KiB of map + 3 x 512 B of rasters + 4 indices read.  The formulation moves
about 192 KiB per row by the sizes of its tensors: two gathers (16 KiB read + 16 KiB written each), and the cat (64 KiB read, 64
KiB written)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")]
import numpy as np
import torch
from bridges_hip import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2048)
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--cands", type=int, default=40000)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--shared_obstacle", action="store_true", help="targets only: one obstacle raster for every row (stride 0)")
a = ap.parse_args()
assert a.reps >= 20
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
n, E, Cn = a.rows, a.envs, a.cands
# rasters as sparse as the env's (a block covers ~35 pixels): a few rows of a few bits
def sparse_bits(m):
    b = torch.zeros((m, 64), dtype=torch.int64)
    rows = torch.randint(0, 58, (m,), generator=g)
    cols = torch.randint(0, 58, (m,), generator=g)
    for k in range(6):
        b[torch.arange(m), rows + k] = (63 << cols)
    return b.to(dev)
state_bits, cand_bits, obst_bits = sparse_bits(E), sparse_bits(Cn), sparse_bits(1 if a.shared_obstacle else E)
maps = torch.rand((E, 64, 64), generator=g).to(dev)
row_env = torch.sort(torch.randint(0, E, (n,), generator=g)).values.to(dev)       # rows come grouped by env
idx = torch.sort(torch.randint(0, Cn, (n,), generator=g)).values.to(dev)
# what the formulation reads: the f32 rasters the rollout env would hold
state_raster, cand_raster, obst_raster = ops.bits_to_f32(state_bits), ops.bits_to_f32(cand_bits), ops.bits_to_f32(obst_bits)


def kernel():
    if a.shared_obstacle:
        return ops.conv_input(state_bits, cand_bits, maps, obst_bits, block_row=row_env, action_row=idx, reward_row=row_env)
    return ops.conv_input(state_bits, cand_bits, maps, obst_bits, block_row=row_env, action_row=idx, reward_row=row_env,
                          obstacle_row=row_env)


def formulation():
    block = state_raster.index_select(0, row_env).unsqueeze(1)
    action = cand_raster.index_select(0, idx).unsqueeze(1)
    reward = maps.index_select(0, row_env).unsqueeze(1)
    obstacle = (obst_raster.unsqueeze(0).expand(n, -1, -1, -1) if a.shared_obstacle
                else obst_raster.index_select(0, row_env).unsqueeze(1))
    return torch.cat([block, action, reward, obstacle], dim=1)


assert torch.equal(kernel().view(torch.int32), formulation().view(torch.int32))
for _ in range(a.warmup):
    kernel(); formulation()
torch.cuda.synchronize()
times = dict(kernel=[], formulation=[])
for _ in range(a.reps):
    for name, fn in (("kernel", kernel), ("formulation", formulation)):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        times[name].append(start.elapsed_time(stop) * 1e3)              # us
        del out
summary = {}
for name, t in times.items():
    t = np.array(t)
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    summary[name] = dict(median_us=float(med), min_us=float(t.min()), max_us=float(t.max()), iqr_us=float(q3 - q1), launches=len(t))
kernel_bytes = n * (4 * 16384 + 16384 + 3 * 512 + (3 if a.shared_obstacle else 4) * 8)
k, f = summary["kernel"], summary["formulation"]
print(json.dumps(dict(config=vars(a), **summary, ratio_of_medians=f["median_us"] / k["median_us"],
                      kernel_bytes=kernel_bytes, kernel_TB_per_s=kernel_bytes / (k["median_us"] * 1e-6) / 1e12,
                      kernel_write_TB_per_s=n * 65536 / (k["median_us"] * 1e-6) / 1e12,
                      faster_by_more_than_the_formulations_spread=bool(f["median_us"] - k["median_us"] > f["max_us"] - f["min_us"]),
                      note="HIP events around single calls (host launch gaps of the formulation's several launches included), both "
                           "sides alternating in one process; spread = max - min of the timed launches")))
