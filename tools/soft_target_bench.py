"""bridges_soft_expect alone against a torch formulation, on the segments the vectorised loop really feeds it.

A VecDQN(target_temperature=T) on the tower task rolls out a few lock-steps, samples --transitions records (800 = 25 batches of
32, the loop's default) and runs its target pass once; the segments, q vectors and last-hidden rows that pass handed to
next_targets are kept.  Then the operator is timed alone with HIP events on those very inputs, for dim = the hidden width (the
factored SuccessorMLP's feature rows) and for dim = 4096 (channel 0 of a module-forward net's output; random rows of the same
count), alternating with the torch formulation: scatter_reduce(amax) and index_add_ over (transition, row) pairs for m, Z, the
value and the entropy in float64, and one index_add_ of p * feat[row] in float32 for the feature mean (float64 there would cost
torch a [pairs, dim] float64 temporary; the kernel sums in float64).  --relative adds a third leg, alternating with the two:
dqn_ops.soft_expect(relative=True) (bridges_soft_expect_rel: the same grid with the spread pass and temp_out), and says whether
its median lies inside the scalar operator's own max - min spread.  Prints one JSON line per dim: medians with min-max in
microseconds.
--munchausen builds the loop with munchausen_alpha = 0.9 and, behind the lines above, times the three pieces of the Munchausen path
alone on what that target pass fed them, each alternating with a torch formulation, HIP events around single calls:
dqn_ops.soft_value with the taken rows over the segments of s (torch: a scatter-amax / index_add_ logsumexp in float64 and a
gather of the taken row), dqn_ops.action_row (torch: a masked compare of every (transition, row) pair's descriptor and pose words
with the record's and a scatter-amin of the row), and load_records(prev=True) (torch: records.unpack_states + load_states).  One
JSON line each."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")]
import torch
from bridges_hip import dqn_ops
from bridges_hip.shapes import load_urdf
from bridges_hip.vec_env import VecAssemblyGym
from robotoddler.training.successor_dqn import build_parser, make_nets
from robotoddler.training.vec_dqn import VecDQN

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--tower", type=int, default=4)
ap.add_argument("--max_steps", type=int, default=15)
ap.add_argument("--locksteps", type=int, default=12, help="rollout lock-steps before the sample")
ap.add_argument("--transitions", type=int, default=800)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--relative", action="store_true", help="one more leg: the relative-temperature operator")
ap.add_argument("--spread_floor", type=float, default=1e-3)
ap.add_argument("--munchausen", action="store_true", help="three more lines: soft_value, action_row and the prev-unpack")
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
pol, tgt = make_nets(vars(build_parser().parse_args(["--model", "SuccessorMLP", "--loss_function", "mse_block_features"])), dev)
H = 0.8
env = VecAssemblyGym(a.envs, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(a.tower)],
                     [(0.5, 0, a.tower * H + H / 2)], max_steps=a.max_steps, seed=0, device=dev, f32_rasters=False)
agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 200000, 32, 0.95, 0.01, "mse_block_features",
               target_temperature=a.temperature, **(dict(munchausen_alpha=0.9) if a.munchausen else {}))
for _ in range(a.locksteps):
    agent.lockstep(0)
seen, inner = {}, dqn_ops.next_targets


def keep(seg, next_q, done, gamma, **kw):
    seen.update(seg=seg, next_q=next_q, feat=kw["next_feat"], cur_seg=kw.get("cur_seg"), cur_q=kw.get("cur_q"), taken=kw.get("taken_row"))
    return inner(seg, next_q, done, gamma, **kw)


dqn_ops.next_targets = keep
sampled = agent.ring.sample(a.transitions, agent.sample_gen, False)
agent._targets(sampled)
dqn_ops.next_targets = inner
lo, hi = (t.to(torch.int64) for t in seen["seg"])
nq = seen["next_q"].contiguous().float()
B, R, T = lo.numel(), nq.numel(), a.temperature
length = (hi - lo).clamp_(min=0)
ids = torch.repeat_interleave(torch.arange(B, device=dev), length)                 # the transition of every (transition, row) pair
start = torch.cumsum(length, 0) - length
rows = lo[ids] + (torch.arange(ids.numel(), device=dev) - start[ids])               # ... and its row


def torch_leg(feat):
    q = nq.double()[rows]
    m = torch.full((B,), -float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, ids, q, "amax")
    x = (q - m[ids]) / T
    w = torch.exp(x)
    Z = torch.zeros(B, dtype=torch.float64, device=dev).index_add_(0, ids, w)
    p = w / Z[ids]
    value = torch.zeros(B, dtype=torch.float64, device=dev).index_add_(0, ids, p * q)
    entropy = torch.log(Z) - torch.zeros(B, dtype=torch.float64, device=dev).index_add_(0, ids, p * x)
    mean = torch.zeros((B, feat.shape[1]), dtype=torch.float32, device=dev).index_add_(0, ids, p.float().unsqueeze(1) * feat[rows])
    return value.float(), mean, entropy.float()


def kernel_leg(feat):
    return dqn_ops.soft_expect(seen["seg"], nq, nq, T, feat=feat)


def relative_leg(feat):
    return dqn_ops.soft_expect(seen["seg"], nq, nq, T, feat=feat, relative=True, spread_floor=a.spread_floor)


def timed(fn, feat):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(feat)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(xs):
    xs = sorted(xs)
    return dict(median_us=round(xs[len(xs) // 2], 1), min_us=round(xs[0], 1), max_us=round(xs[-1], 1))


for name, feat in (("hidden", seen["feat"]), ("4096", torch.randn((R, 4096), device=dev))):
    v_t, m_t, e_t = torch_leg(feat)
    v_k, m_k, e_k, _ = kernel_leg(feat)
    live = length > 0
    agree = dict(value=float((v_t - v_k)[live].abs().max()), feat_mean=float((m_t - m_k)[live].abs().max()),
                 entropy=float((e_t - e_k)[live].abs().max()))
    for _ in range(3):                                                              # warm both legs
        timed(torch_leg, feat), timed(kernel_leg, feat)
        if a.relative:
            timed(relative_leg, feat)
    t_torch, t_kernel, t_rel = [], [], []
    for _ in range(a.reps):                                                         # legs alternating
        t_torch.append(timed(torch_leg, feat))
        t_kernel.append(timed(kernel_leg, feat))
        if a.relative:
            t_rel.append(timed(relative_leg, feat))
    rel = {}
    if a.relative:
        k, r = stats(t_kernel), stats(t_rel)
        rel = dict(relative=r, relative_over_kernel=round(r["median_us"] / k["median_us"], 3),
                   relative_inside_kernels_own_spread=bool(abs(r["median_us"] - k["median_us"]) <= k["max_us"] - k["min_us"]))
    print(json.dumps(dict(bench="soft_expect", dim=int(feat.shape[1]), transitions=B, rows=R, pairs=int(ids.numel()),
                          longest_segment=int(length.max()), temperature=T, kernel=stats(t_kernel), torch=stats(t_torch),
                          max_abs_difference=agree, **rel)), flush=True)


def alternate(name, kernel_fn, torch_fn, **extra):
    for _ in range(3):
        timed(torch_fn, None), timed(kernel_fn, None)
    t_torch, t_kernel = [], []
    for _ in range(a.reps):
        t_torch.append(timed(torch_fn, None))
        t_kernel.append(timed(kernel_fn, None))
    print(json.dumps(dict(bench=name, transitions=B, kernel=stats(t_kernel), torch=stats(t_torch), **extra)), flush=True)


if a.munchausen:
    from robotoddler.training import records as R
    renv_s = agent.replay_env_s
    E = renv_s.E
    rec = sampled[:, :R.RECORD_WIDTH].contiguous()
    rec = rec if rec.shape[0] == E else torch.cat([rec, rec[:1].expand(E - rec.shape[0], -1)]).contiguous()
    slo, shi = (t.to(torch.int64) for t in seen["cur_seg"])
    cq, taken = seen["cur_q"], seen["taken"]
    slen = (shi - slo).clamp_(min=0)
    sids = torch.repeat_interleave(torch.arange(E, device=dev), slen)
    sstart = torch.cumsum(slen, 0) - slen
    srows = slo[sids] + (torch.arange(sids.numel(), device=dev) - sstart[sids])
    alpha, clip = agent.munchausen

    def value_kernel(_):
        return dqn_ops.soft_value(seen["cur_seg"], cq, T, taken_row=taken, alpha=alpha, clip_lo=clip)

    def value_torch(_):
        q = cq.double()[srows]
        m = torch.full((E,), -float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, sids, q, "amax")
        Z = torch.zeros(E, dtype=torch.float64, device=dev).index_add_(0, sids, torch.exp((q - m[sids]) / T))
        V = m + T * torch.log(Z)
        L = (cq.double()[taken.long().clamp(max=cq.numel() - 1)] - V).clamp(max=0.0)
        return V.float(), L.float(), (alpha * L.clamp(min=clip)).float()

    v_k, l_k, b_k, miss = value_kernel(None)
    v_t, l_t, b_t = value_torch(None)
    ok = miss == 0
    alternate("soft_value", value_kernel, value_torch, rows=int(cq.numel()), pairs=int(sids.numel()), missed=int(miss.sum()),
              max_abs_difference=dict(value=float((v_k - v_t)[ok].abs().max()), tlogp=float((l_k - l_t)[ok].abs().max()),
                                      bonus=float((b_k - b_t)[ok].abs().max())))
    idx_s = renv_s.valid_rows(renv_s._valid_rows[5])[0]          # (cached: the rows of the target pass)
    desc, pose = renv_s.buf["cand_desc"], renv_s.buf["cand_pose"]
    want_desc = rec[:, [R.O_ATB, R.O_ATF, R.O_ASHAPE, R.O_AFACE]].to(torch.int32)
    want_pose = rec[:, R.O_APOSE:R.O_APOSE + 4].contiguous().view(torch.int64)

    def row_kernel(_):
        return dqn_ops.action_row(renv_s, seen["cur_seg"], idx_s, rec)

    def row_torch(_):
        c = idx_s[srows]
        same = (desc[c] == want_desc[sids]).all(dim=1) & (pose[c].view(torch.int64) == want_pose[sids]).all(dim=1)
        cand = torch.where(same, srows, torch.full_like(srows, 0x7fffffff))
        return torch.full((E,), 0x7fffffff, dtype=torch.int64, device=dev).scatter_reduce(0, sids, cand, "amin").to(torch.int32)

    alternate("action_row", row_kernel, row_torch, rows=int(idx_s.numel()), pairs=int(sids.numel()),
              equal=bool((row_kernel(None) == row_torch(None)).all()))

    def unpack_kernel(_):
        return renv_s.load_records(rec, prev=True)

    def unpack_torch(_):
        return renv_s.load_states(*R.unpack_states(rec, renv_s.K)[0])

    alternate("load_records_prev", unpack_kernel, unpack_torch, envs=E)
