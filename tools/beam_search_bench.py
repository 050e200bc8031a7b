"""What beam-search evaluation costs, part by part, on identical inputs in one process:
  fork      bridges_env_fork alone (the two copy launches, no candidate refresh) against the torch formulation
            t.copy_(t.index_select(0, src)) over the same state arrays, at --fork_envs envs of a tower env advanced a few random
            lock-steps; bytes moved = 4 x the scratch (read the source rows, write the scratch, read it, write the rows)
  select    ops.beam_select (bridges_beam_select: one launch) against a torch top-k formulation (scores in float64, scattered into a
            padded [G, rows] matrix, torch.topk, gathers) at --groups groups of --width beams
  search    one VecDQN.beam_search(width) call for every --widths next to one VecDQN.evaluate() call on --tasks held-out tasks
            (wall clock around the whole call, its host waits included)
HIP events around single calls (fork, select), the legs alternating, warm-up first; one JSON line per shape with medians and spread.
--merge times beam merging instead of the parts above:
  merge     ops.beam_merge (bridges_beam_merge: one launch) alone at --tasks groups of --width beams whose envs hold permutations of
            a few structures, HIP events around single calls after warm-up
  search    one VecDQN.beam_search(--width) call without and with merge=True on the same --tasks held-out tasks, alternating (wall
            clock around the whole call), and the beams merging closed
--syncs lists the host waits of one evaluate() and one beam_search() call instead (tools/find_syncs.py's counting, plus explicit
stream / event / device synchronisations): per depth the search must wait only where acting waits
(with --merge: of the search with and without merging -- merging must add none).
--trace times the tracing of the best beams' records instead:
  trace     ops.beam_trace (bridges_beam_trace: two launches) alone at --groups groups of --width beams and --max_steps depths,
            n_step 1 and 3, against a torch formulation of the same rows -- a [E, K, W] path buffer gathered by the depth's parents
            at every depth, the episodes picked and cut to their lengths by a masked select --, HIP events around single calls that
            write into given outputs, the legs alternating
  search    one VecDQN.beam_search(--width) call without and with trace=True on the same --tasks held-out tasks, alternating
(--trace --syncs: the host waits of both searches -- tracing must add none).
--particles times the particle search against the beam search instead:
  select    ops.particle_select (bridges_particle_select: one launch) against ops.beam_select on the same rows at --groups groups of
            --width envs, HIP events around single calls that write into given outputs, the two alternating in one process
  search    one VecDQN.particle_search(--width, --particle_temperature) against one VecDQN.beam_search(--width) next to one
            VecDQN.evaluate() on the same --tasks held-out tasks, alternating (wall clock around the whole call)
(--particles --syncs: the host waits of both searches -- per depth the particle search must wait exactly where the beam search does).
    python tools/beam_search_bench.py [--fork_envs 512 4096] [--groups 64 512] [--width 8] [--tasks 64] [--widths 1 4 8] [--syncs]
    python tools/beam_search_bench.py --merge [--tasks 64] [--width 8] [--syncs]
    python tools/beam_search_bench.py --trace [--groups 64 512] [--tasks 64] [--width 8] [--syncs]
    python tools/beam_search_bench.py --particles [--groups 64 512] [--tasks 64] [--width 8] [--particle_temperature 1.0] [--syncs]"""
import argparse, ctypes as C, json, os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd")]
import numpy as np
import torch
from bridges_hip import abi, ops
from bridges_hip.shapes import load_urdf
from bridges_hip.vec_env import RandomTargets, VecAssemblyGym
from robotoddler.training.successor_dqn import build_parser, make_nets
from robotoddler.training.vec_dqn import VecDQN, beam_env_like

ap = argparse.ArgumentParser()
ap.add_argument("--fork_envs", type=int, nargs="*", default=[512, 4096])
ap.add_argument("--groups", type=int, nargs="*", default=[64, 512])
ap.add_argument("--width", type=int, default=8, help="beams per group of the select legs")
ap.add_argument("--rows_per_env", type=int, default=40)
ap.add_argument("--tasks", type=int, default=64, help="held-out tasks of the search legs (0: skip them)")
ap.add_argument("--widths", type=int, nargs="*", default=[1, 4, 8])
ap.add_argument("--max_steps", type=int, default=10)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--search_reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--syncs", action="store_true")
ap.add_argument("--merge", action="store_true", help="time bridges_beam_merge and a search with / without merging at --tasks x --width")
ap.add_argument("--trace", action="store_true", help="time bridges_beam_trace and a search with / without tracing at --tasks x --width")
ap.add_argument("--particles", action="store_true",
                help="time bridges_particle_select against bridges_beam_select and a particle search against a beam search at --tasks x --width")
ap.add_argument("--particle_temperature", type=float, default=1.0, help="with --particles: the temperature of both draws")
a = ap.parse_args()
assert a.merge + a.trace + a.particles <= 1, "--merge, --trace and --particles are three modes"
assert a.reps >= 20 and a.search_reps >= 5
dev = torch.device("cuda:0")
HBM_PEAK = 8.0e12                                             # bytes / s, the card's specification


def summarise(times):
    out = {}
    for name, t in times.items():
        t = np.array(t)
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        out[name] = dict(median_us=float(med), min_us=float(t.min()), max_us=float(t.max()), iqr_us=float(q3 - q1), calls=len(t))
    return out


def alternate(legs, reps, warmup, wall=False):
    for _ in range(warmup):
        for _name, fn in legs:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, fn in legs:
            if wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
            else:
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                out = fn()
                stop.record()
                stop.synchronize()
                times[name].append(start.elapsed_time(stop) * 1e3)
            del out
    return summarise(times)


def tower_env(E, **kw):
    H = 0.8
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)], [(0.5, 0, 2 * H + H / 2)],
                          max_steps=a.max_steps, seed=1, device=dev, f32_rasters=False, **kw)


def waits(fn):
    seen = []
    saved = (torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize)

    def counting(name, inner):
        def f(*args, **kw):
            seen.append(name)
            return inner(*args, **kw)
        return f
    torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize = counting("stream", saved[0]), counting("event", saved[1])
    torch.cuda.synchronize = counting("device", saved[2])
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        seen += ["op"] * sum("synchroniz" in str(x.message) for x in w)
    finally:
        torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize = saved
    return seen


# ---- fork ---------------------------------------------------------------------------------------------------------------------
for E in ([] if a.syncs or a.merge or a.trace or a.particles else a.fork_envs):
    env = tower_env(E)
    for _ in range(4):
        env.select_random()
        env.step()
    arrays = [t for t in ([env.buf[n] for n in abi.FORK_ENV_FIELDS if n != "lp_snap"] + [env.lp_snap]) if t is not None]
    n = C.c_int64(0)
    abi.check(env.L.bridges_env_fork_scratch(env._env, C.byref(n)), "bridges_env_fork_scratch")
    scratch = torch.empty(n.value, dtype=torch.uint8, device=dev)
    src = torch.randint(0, E, (E,), generator=torch.Generator().manual_seed(E), dtype=torch.int32).to(dev)
    src_l = src.long()

    def fork_op():
        abi.check(env.L.bridges_env_fork(env._env, src.data_ptr(), scratch.data_ptr(), n.value, abi.current_stream()), "bridges_env_fork")

    def formulation():
        for t in arrays:
            t.copy_(t.index_select(0, src_l))
    s = alternate((("fork", fork_op), ("torch", formulation)), a.reps, a.warmup)
    moved = 4 * n.value
    bw = moved / (s["fork"]["median_us"] * 1e-6)
    print(json.dumps(dict(part="fork", envs=E, scratch_bytes=n.value, scratch_bytes_per_env=n.value / E, bytes_moved=moved,
                          bandwidth_TB_s=bw / 1e12, share_of_hbm_peak=bw / HBM_PEAK, **s,
                          torch_over_fork=s["torch"]["median_us"] / s["fork"]["median_us"],
                          note="the two copy launches alone (no candidate refresh); HIP events around single calls, legs alternating")),
          flush=True)
    del env, arrays, scratch

# ---- select -------------------------------------------------------------------------------------------------------------------
for G in ([] if a.syncs or a.merge or a.trace else a.groups):   # (--particles: its own legs below)
    B = a.width
    E = G * B
    g = torch.Generator().manual_seed(G)
    lengths = torch.randint(1, 2 * a.rows_per_env + 1, (E,), generator=g)
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)]).to(torch.int32).to(dev)
    nrows = int(seg[-1])
    row_env = torch.repeat_interleave(torch.arange(E), lengths).to(dev)
    q = torch.randn(nrows, generator=g).to(dev)
    idx = torch.arange(nrows, device=dev)
    cand_offset = seg[:-1].contiguous()
    live = (torch.rand(E, generator=g) < 0.9).to(torch.uint8).to(dev)
    ret, disc = torch.randn(E, generator=g, dtype=torch.float64).to(dev), (0.95 ** torch.randint(0, 8, (E,), generator=g).double()).to(dev)
    # the torch formulation's static part: every row's group and its position among the group's rows
    row_group = row_env // B
    group_start = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    group_start[1:] = torch.bincount(row_group, minlength=G).cumsum(0)
    pos = idx - group_start[row_group]
    width = int((group_start[1:] - group_start[:-1]).max())
    own = torch.arange(E, device=dev, dtype=torch.int32)

    def select():
        return ops.beam_select(seg, q, B, live, ret, disc, idx, cand_offset)

    def formulation():
        S = ret[row_env] + disc[row_env] * q.double()
        S = torch.where(live[row_env].bool() & ~torch.isnan(q) & (q != -torch.inf), S, -torch.inf)
        pad = torch.full((G, width), -torch.inf, dtype=torch.float64, device=dev)
        pad[row_group, pos] = S
        top, col = torch.topk(pad, B, dim=1)
        row = (group_start[:-1, None] + col).clamp(max=nrows - 1).reshape(-1)
        ok = (top > -torch.inf).reshape(-1)
        e = row_env[row]
        return (torch.where(ok, e.to(torch.int32), own), torch.where(ok, idx[row], 0),
                torch.where(ok, (idx[row] - cand_offset[e]).to(torch.int32), 0), torch.where(ok, q[row], 0.0), top.reshape(-1), ok)
    if a.particles:                                          # the sampled sibling against the operator it stands beside
        gen = torch.Generator(device=dev).manual_seed(G)
        u_act, u_res = torch.rand(E, generator=gen, device=dev), torch.rand(G, generator=gen, device=dev)
        q32, idx64 = q.float().contiguous(), idx.contiguous()
        out_b = ops.beam_select(seg, q32, B, live, ret, disc, idx64, cand_offset)
        out_p = ops.particle_select(seg, q32, B, live, ret, disc, idx64, cand_offset, u_act, u_res, a.particle_temperature,
                                    a.particle_temperature)
        legs = (("particle_select", lambda: ops.particle_select(seg, q32, B, live, ret, disc, idx64, cand_offset, u_act, u_res,
                                                                a.particle_temperature, a.particle_temperature, out=out_p)),
                ("beam_select", lambda: ops.beam_select(seg, q32, B, live, ret, disc, idx64, cand_offset, out=out_b)))
        s = alternate(legs, a.reps, a.warmup)
        print(json.dumps(dict(part="particle_select", groups=G, width=B, rows=nrows, temperature=a.particle_temperature,
                              mean_ess=float(out_p["ess"].mean()), moved=float((out_p["src"] != own).float().mean()), **s,
                              particle_over_beam=s["particle_select"]["median_us"] / s["beam_select"]["median_us"],
                              note="HIP events around single calls that write into given outputs (host launch gap included), the two "
                                   "alternating")), flush=True)
        continue
    k, f = select(), formulation()
    same = (k["sel_compact"] == f[1]).float().mean().item()   # topk breaks exact ties its own way: random q has none to speak of
    assert same > 0.999, same
    s = alternate((("select", select), ("torch", formulation)), a.reps, a.warmup)
    print(json.dumps(dict(part="select", groups=G, width=B, rows=nrows, same_rows_as_torch=same, **s,
                          torch_over_select=s["torch"]["median_us"] / s["select"]["median_us"],
                          note="HIP events around single calls (host launch gaps included), legs alternating")), flush=True)

# ---- merge --------------------------------------------------------------------------------------------------------------------
if a.merge and not a.syncs:
    G, B, K = max(a.tasks, 1), a.width, a.max_steps
    E = G * B
    rng = np.random.default_rng(G)
    pool_shape, pool_occ, pool_pose = rng.integers(0, 2, 12), rng.integers(0, 4, 12), rng.normal(size=(12, 4))
    n_blocks = np.zeros(E, np.int32)
    pick = np.zeros((E, K), np.int64)
    for g in range(G):                                       # a group: permutations of two or three structures of one depth
        nb = int(rng.integers(1, K + 1))
        bases = [rng.integers(0, 12, nb) for _ in range(3)]
        for e in range(g * B, (g + 1) * B):
            n_blocks[e] = nb
            pick[e, :nb] = rng.permutation(bases[int(rng.integers(0, 3))])
    to = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    st = dict(n_blocks=to(n_blocks, torch.int32), blk_shape=to(pool_shape[pick], torch.int32), blk_pose=to(pool_pose[pick], torch.float64),
              blk_occ=to(pool_occ[pick], torch.uint8), targets_left=torch.full((E,), 3, dtype=torch.int32, device=dev))
    live = to(rng.random(E) < 0.9, torch.uint8)
    ret = to(rng.normal(size=E), torch.float64)
    out = ops.beam_merge(st["n_blocks"], st["blk_shape"], st["blk_pose"], st["blk_occ"], st["targets_left"], B, live, ret)

    def merge_op():
        return ops.beam_merge(st["n_blocks"], st["blk_shape"], st["blk_pose"], st["blk_occ"], st["targets_left"], B, live, ret, out=out)
    s = alternate((("merge", merge_op),), a.reps, a.warmup)
    print(json.dumps(dict(part="merge", groups=G, width=B, slots=K, live=int(live.sum()), closed=int(out["n_merged"].sum()), **s,
                          note="HIP events around single calls (host launch gap included), after warm-up")), flush=True)

# ---- trace --------------------------------------------------------------------------------------------------------------------
for G, n_step in ([(G, n) for G in a.groups for n in (1, 3)] if a.trace and not a.syncs else []):
    from robotoddler.training import records as R
    B, D, W, n_tail, gamma, priority = a.width, a.max_steps, R.RECORD_WIDTH, 9, 0.95, 1.0
    E = G * B
    g = torch.Generator().manual_seed(G + n_step)
    rec = torch.randn((D, E, W), generator=g, dtype=torch.float64).to(dev)
    valid = torch.ones((D, E), dtype=torch.uint8, device=dev)
    # every depth permutes the slots of every group
    parent = (torch.rand((D, G, B), generator=g).argsort(dim=2) + torch.arange(G)[None, :, None] * B).reshape(D, E).to(torch.int32).to(dev)
    end_depth = torch.where(torch.rand(G, generator=g) < 0.1, -1, torch.randint(0, D, (G,), generator=g)).to(torch.int32).to(dev)
    end_env = (torch.arange(G) * B + torch.randint(0, B, (G,), generator=g)).to(torch.int32).to(dev)
    tail = torch.randn((E, n_tail), generator=g, dtype=torch.float64).to(dev)
    out = ops.beam_trace(rec, valid, parent, end_env, end_depth, B, gamma, n_step=n_step, tail=tail, priority=priority)
    parent_l, end_env_l, L = parent.long(), end_env.long(), (end_depth + 1).long()
    steps = torch.arange(D, device=dev)
    ends_at = (end_depth[None] == steps[:, None])[:, :, None, None]        # [D, G, 1, 1]

    def trace_op():
        return ops.beam_trace(rec, valid, parent, end_env, end_depth, B, gamma, n_step=n_step, tail=tail, priority=priority,
                              out=out["rows"], offset=out["offset"], status=out["status"])

    def formulation():
        path = torch.zeros((E, D, W), dtype=torch.float64, device=dev)
        for d in range(D):                                   # what the search would do per depth: the history follows the fork
            if d:
                path = path[parent_l[d]]
            path[:, d] = rec[d]
            # ... and the group's best episode is kept where it ends (the slot is forked over at the next depth)
            ep = torch.where(ends_at[d], path[end_env_l], ep) if d else path[end_env_l]
        task = tail[end_env_l][:, None].expand(-1, D, -1)
        if n_step > 1:
            h = torch.minimum(torch.full((), n_step, device=dev), L[:, None] - steps[None]).clamp(min=1)
            last = (steps[None] + h - 1).clamp(max=D - 1)
            rows = torch.gather(ep, 1, last[..., None].expand(-1, -1, W)).clone()
            rows[..., R.O_STABLE_S] = ep[..., R.O_STABLE_S]
            lin = torch.nn.functional.pad(ep[..., R.O_LIN], (0, n_step - 1))
            acc, disc = torch.zeros_like(ep[..., 0]), 1.0
            for k in range(n_step):
                acc = acc + torch.where(k < h, disc * lin[:, k:k + D], 0.0)
                disc *= gamma
            rows[..., R.O_LIN] = torch.where(h > 1, acc, rows[..., R.O_LIN])
            rows = torch.cat([rows, task, h.double()[..., None]], dim=2)
        else:
            rows = torch.cat([ep, task], dim=2)
        rows[..., R.O_TD] = priority
        return rows[steps[None] < L[:, None]]                # the masked select: the one host wait of the formulation
    f = formulation()
    torch.cuda.synchronize()
    n = int(out["offset"][-1])
    assert f.shape[0] == n and int(out["status"].sum()) == 0
    assert torch.equal(out["rows"][:n], f) if n_step == 1 else torch.allclose(out["rows"][:n], f, rtol=1e-12, atol=1e-12)
    s = alternate((("trace", trace_op), ("torch", formulation)), a.reps, a.warmup)
    print(json.dumps(dict(part="trace", groups=G, width=B, depths=D, n_step=n_step, n_tail=n_tail, rows=n, bytes_written=n * out["rows"].shape[1] * 8,
                          **s, torch_over_trace=s["torch"]["median_us"] / s["trace"]["median_us"],
                          note="HIP events around single calls (host launch gaps included), legs alternating; the torch leg ends in a "
                               "masked select, which waits for the device")), flush=True)

# ---- search -------------------------------------------------------------------------------------------------------------------
if a.tasks > 0:
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    torch.manual_seed(0)
    pol, tgt = make_nets(args, dev)
    mk = lambda E, seed: VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [], RandomTargets(3), max_steps=a.max_steps, seed=seed,
                                        device=dev, f32_rasters=False)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), mk(256, 0), 20000, 32, 0.95, 0.01,
                   "mse_q_values+mse_block_features", per_env_tasks=True)
    eval_env = mk(a.tasks, 1)
    beams = {B: beam_env_like(eval_env, B) for B in ([a.width] if a.merge or a.trace or a.particles else a.widths)}
    legs = [("evaluate", lambda: agent.evaluate(eval_env))] + [(f"beam_{B}", (lambda B=B: agent.beam_search(beams[B], B))) for B in beams]
    if a.merge:
        legs.append((f"beam_{a.width}_merge", lambda: agent.beam_search(beams[a.width], a.width, merge=True)))
    if a.trace:
        legs.append((f"beam_{a.width}_trace", lambda: agent.beam_search(beams[a.width], a.width, trace=True)))
        legs.append((f"beam_{a.width}_trace3", lambda: agent.beam_search(beams[a.width], a.width, trace=True, trace_n_step=3)))
    if a.particles:
        T = a.particle_temperature
        legs.append((f"particle_{a.width}", lambda: agent.particle_search(beams[a.width], a.width, T)))
        legs.append((f"best_of_{a.width}", lambda: agent.particle_search(beams[a.width], a.width, T, float("inf"), elite=False)))
    if a.syncs:
        for name, fn in legs:
            fn()
        for name, fn in legs:
            w = waits(fn)
            print(json.dumps(dict(part="syncs", call=name, depths=eval_env.K, waits=len(w), kinds={k: w.count(k) for k in sorted(set(w))})),
                  flush=True)
    else:
        s = alternate(legs, a.search_reps, 2, wall=True)
        res = {name: {k: v for k, v in fn().items() if not torch.is_tensor(v)} for name, fn in legs}
        print(json.dumps(dict(part="search", tasks=a.tasks, max_steps=a.max_steps, **s,
                              over_evaluate={name: s[name]["median_us"] / s["evaluate"]["median_us"] for name, _ in legs[1:]},
                              success_rate={name: r["success_rate"] for name, r in res.items()},
                              lin_reward={name: r["lin_reward"] for name, r in res.items()},
                              merged_beams={name: sum(r["merged_beams"]) for name, r in res.items() if "merged_beams" in r},
                              **(dict(merge_minus_plain_us=s[f"beam_{a.width}_merge"]["median_us"] - s[f"beam_{a.width}"]["median_us"])
                                 if a.merge else {}),
                              **(dict(trace_minus_plain_us=s[f"beam_{a.width}_trace"]["median_us"] - s[f"beam_{a.width}"]["median_us"],
                                      plain_spread_us=s[f"beam_{a.width}"]["max_us"] - s[f"beam_{a.width}"]["min_us"],
                                      trace_rows=res[f"beam_{a.width}_trace"]["trace_count"]) if a.trace else {}),
                              note="wall clock around whole calls on an UNTRAINED net (cost only), legs alternating")), flush=True)
