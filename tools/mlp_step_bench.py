"""Times one SuccessorMLP optimiser step at batch 32 (BASELINE.json configs[2] shape: 64x64 images, hidden
256-128-64-128-256) as a replayed HIP graph: the hand-written forward / loss / backward (bridges_hip/mlp_ops.py) + torch's
fused Adam, against the autograd step + fused Adam.  Under rocprofv3 --kernel-trace the kernel list of either is visible.
Usage: python tools/mlp_step_bench.py [--autograd] [--replays 400] [--batch 32]
       python tools/mlp_step_bench.py --obstacle_bits     (times the two kernels of per-env obstacles alone, see obstacle_bits_lines)
       python tools/mlp_step_bench.py --td_select         (times bridges_td_target and bridges_td_target_select, see td_select_lines)"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bridges-with-reinforcement-learning_amd"))


def obstacle_bits_lines(dev, B=32, n_b=25, E=4096, hidden=256, reps=50):
    """The two kernels of per-env obstacles beside the ones they stand in for, device time per launch: the input rows of 25
    batches with a reward map per transition and the obstacle as one f32 map (k_mlp_input<rows>) against a bit-packed raster
    per transition (k_mlp_input<rows, obstacle bits>); the per-env base of the first layer on E state rasters
    (k_bits_linear) against state + obstacle rasters (k_bits_linear2)."""
    from bridges_hip import ops
    from bridges_hip.mlp_ops import FusedSuccessorStep
    from robotoddler.models.cv import SuccessorMLP
    px, n = 4096, n_b * B
    net = SuccessorMLP(img_size=(64, 64), hidden_dims=[hidden, 128, 64, 128, 256]).to(dev)
    step = FusedSuccessorStep(net, B, True, True)
    step.allocate_inputs(n_b)
    block, action = (torch.rand(n, px, device=dev) < 0.05).float(), (torch.rand(n, px, device=dev) < 0.01).float()
    binary, maps, one = (torch.rand(n, 6, device=dev) < 0.5).float(), torch.rand(n, px, device=dev), (torch.rand(px, device=dev) < 0.03).float()

    def rasters(m, k):                                                  # m rasters of a k x k square each, somewhere on the canvas
        bits = torch.zeros((m, 64), dtype=torch.int64, device=dev)
        y, x = torch.randint(0, 64 - k, (m,), device=dev), torch.randint(0, 64 - k, (m,), device=dev)
        for j in range(k):
            bits[torch.arange(m, device=dev), y + j] = ((1 << k) - 1) << x
        return bits
    obst = rasters(n, 8)
    state, env_obst = rasters(E, 6), rasters(E, 8)
    wa, wb = torch.randn(px, hidden, device=dev), torch.randn(px, hidden, device=dev)
    table, base_row = torch.randn(2 * E, hidden, device=dev), torch.arange(E, device=dev) * 2

    def timed(name, fn):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"{name}: {a.elapsed_time(b) / reps * 1e3:.1f} us per call (host launch path included)", flush=True)
    timed(f"k_mlp_input<rows> x {n_b} batches, one f32 obstacle map   ", lambda: step.prepare_inputs(n_b, block, action, binary, maps, one))
    timed(f"k_mlp_input<rows, obstacle bits> x {n_b} batches          ", lambda: step.prepare_inputs(n_b, block, action, binary, maps, obst))
    timed(f"k_bits_linear  E = {E}, d = {hidden}                      ", lambda: ops.bits_linear(state, wa, base=table, base_row=base_row))
    timed(f"k_bits_linear2 E = {E}, d = {hidden}                      ", lambda: ops.bits_linear2(state, wa, env_obst, wb, base=table, base_row=base_row))
    timed(f"k_bits_linear chained twice E = {E}, d = {hidden}         ",
          lambda: ops.bits_linear(env_obst, wb, base=ops.bits_linear(state, wa, base=table, base_row=base_row), base_row=torch.arange(E, device=dev)))


def td_select_lines(dev, B=32, n_b=25, rounds=15, per_graph=20):
    """bridges_td_target_select (dqn_ops.td_target(select_q=...)) beside bridges_td_target (the same call without select_q) on
    the same segments, device time per launch.  BOTH COLUMNS TIME ONE KERNEL, k_td_target<false> (the plain entry point passes
    next_q as select_q): the tool serves to compare a tree with its parent -- run it in both checkouts, alternating, and hold
    a column against the same column of the other -- and the difference between its own two columns is its noise.  Shapes: n_b * B transitions whose segments are the candidate sets of a tower-4 rollout
    (an env of n_b * B envs after 6 lock-steps of random actions), and the same number of transitions on 700-row segments
    (the longest of the conformance probe, tests/mlp_conformance.td_probe), eight distinct ones shared as (lo, hi) pairs; each
    with sf_dim = 0 (the launch the loop makes: rows only, the successor features follow for the selected rows) and with
    sf_dim = 4096.  A launch is timed as 1 / per_graph of a replayed HIP graph of per_graph launches, between HIP events; the two
    calls ALTERNATE for `rounds` rounds and the line gives the median and the range over the rounds of each -- the range is the
    run-to-run spread to hold a difference between two trees against."""
    import statistics
    from bridges_hip import dqn_ops
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    n, H = n_b * B, 0.8
    env = VecAssemblyGym(n, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(4)], [(0.5, 0, 4 * H + H / 2)],
                         max_steps=15, seed=0, device=dev, f32_rasters=False, candidate_snapshots=False)
    for _ in range(6):
        env.select_random()
        env.step()
    counts = env.n_valid[:n].to(torch.int32)
    hi = torch.cumsum(counts, 0).to(torch.int32)
    rollout = (hi - counts, hi)
    lo8 = 700 * (torch.arange(n, device=dev, dtype=torch.int32) % 8)
    longest = (lo8, lo8 + 700)
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (lo, hi) in (("tower-4 rollout segments", rollout), ("700-row segments", longest)):
        R = int(hi.max())
        lens = (hi - lo).float()
        print(f"{name}: {n} transitions, {R} rows, segment length mean {float(lens.mean()):.1f} max {int(lens.max())}", flush=True)
        next_q, select_q = torch.randn(R, device=dev, generator=g), torch.randn(R, device=dev, generator=g)
        lin, done = torch.randn(n, device=dev, generator=g), (torch.rand(n, device=dev, generator=g) < 0.1).to(torch.uint8)
        for sf_dim in (0, 4096):
            if sf_dim and R * sf_dim * 4 > (2 << 30):
                print(f"  sf_dim {sf_dim}: skipped, next_sf would hold {R * sf_dim * 4 / 2 ** 30:.1f} GiB", flush=True)
                continue
            kw = {}
            if sf_dim:
                kw = dict(next_sf=torch.randn(R, sf_dim, device=dev, generator=g), action_raster=torch.rand(n, sf_dim, device=dev, generator=g))
            calls = dict(td_target=lambda: dqn_ops.td_target((lo, hi), next_q, lin, done, 0.95, **kw),
                         td_target_select=lambda: dqn_ops.td_target((lo, hi), next_q, lin, done, 0.95, select_q=select_q, **kw))
            graphs = {}
            for k, fn in calls.items():
                fn()
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    fn()
                torch.cuda.current_stream().wait_stream(st)
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k]):
                    for _ in range(per_graph):
                        fn()
                for _ in range(3):
                    graphs[k].replay()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(rounds):
                for k in calls:                                         # alternate: both see the same minutes of the machine
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(5):
                        graphs[k].replay()
                    b.record()
                    torch.cuda.synchronize()
                    times[k].append(a.elapsed_time(b) / (5 * per_graph) * 1e3)
            for k, t in times.items():
                print(f"  sf_dim {sf_dim:4d} {k:17s}: median {statistics.median(t):7.2f} us  min {min(t):7.2f}  max {max(t):7.2f} "
                      f"per launch over {rounds} rounds", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--td_select", action="store_true",
                    help="time bridges_td_target and bridges_td_target_select (one kernel, k_td_target) at the same shapes and exit")
    ap.add_argument("--obstacle_bits", action="store_true",
                    help="time the two kernels of per-env obstacles (k_bits_linear2, k_mlp_input with obstacle bits) alone and exit")
    ap.add_argument("--autograd", action="store_true")
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-adam", action="store_true")
    ap.add_argument("--per-step-inputs", action="store_true", help="build the first layer's input rows inside every step (round 2)")
    ap.add_argument("--torch-adam", action="store_true", help="hand-written step + torch's fused Adam launch (the round-2 step)")
    args = ap.parse_args()
    if args.obstacle_bits:
        torch.manual_seed(0)
        return obstacle_bits_lines(torch.device("cuda:0"), B=args.batch)
    if args.td_select:
        torch.manual_seed(0)
        return td_select_lines(torch.device("cuda:0"), B=args.batch)
    from bridges_hip.mlp_ops import FusedSuccessorStep
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.utils.utils import init_weights
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    size, B, n_b = 64, args.batch, 25
    px = size * size
    net = SuccessorMLP(img_size=(size, size), hidden_dims=[256, 128, 64, 128, 256]).to(dev)
    net.apply(init_weights)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True, capturable=True)
    n = n_b * B
    block = (torch.rand(n, 1, size, size, device=dev) < 0.05).float()
    action = (torch.rand(n, 1, size, size, device=dev) < 0.01).float()
    binary = (torch.rand(n, 6, device=dev) < 0.5).float()
    reward, obstacle = torch.rand(1, size, size, device=dev), (torch.rand(1, size, size, device=dev) < 0.03).float()
    q_t, sf_t = torch.randn(n, device=dev), torch.rand(n, px, device=dev)
    counter = torch.zeros((), dtype=torch.int64, device=dev)
    losses = torch.zeros(n_b, device=dev)
    lane = torch.arange(B, device=dev)

    def autograd_body():
        idx = lane + counter * B
        q, sf, _ = net(block.index_select(0, idx), binary.index_select(0, idx), action.index_select(0, idx),
                       reward.unsqueeze(0).expand(B, -1, -1, -1), obstacle.unsqueeze(0).expand(B, -1, -1, -1))
        loss = ((q - q_t.index_select(0, idx)) ** 2).mean() + ((sf[:, 0].reshape(B, -1) - sf_t.index_select(0, idx)) ** 2).mean(dim=1).mean()
        loss.backward()
        if not args.no_adam:
            opt.step()
        counter.add_(1)

    # eager steps first: optimiser state, library workspaces
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        autograd_body()
    counter.zero_()
    opt.zero_grad(set_to_none=True)
    if args.autograd:
        body = autograd_body
    else:
        from bridges_hip.dqn_ops import FlatParameters
        net._flat_params = FlatParameters(net)
        step = FusedSuccessorStep(net, B, True, True, optimizer=None if (args.torch_adam or args.no_adam) else opt)
        rw, ob = reward.reshape(px).contiguous(), obstacle.reshape(px).contiguous()
        if not args.per_step_inputs:                     # as VecDQN.train_steps does: all batches' input rows in one launch
            step.allocate_inputs(n_b)
            step.prepare_inputs(n_b, block.view(n, px), action.view(n, px), binary, rw, ob)

        def body():
            step.launch(counter, block.view(n, px), action.view(n, px), binary, rw, ob, q_t, sf_t, losses)
            if not args.no_adam and not step.fused_adam:
                opt.step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    counter.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for _ in range(20):
        counter.zero_()
        graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(args.replays):
        if i % n_b == 0:
            counter.zero_()
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    kind = "autograd" if args.autograd else ("hand-written + torch Adam" if args.torch_adam else "hand-written incl. Adam")
    print(f"{kind} step{'' if not args.no_adam else ' (no Adam)'}: "
          f"{a.elapsed_time(b) / args.replays * 1e3:.1f} us per optimiser step (batch {B})", flush=True)


if __name__ == "__main__":
    main()
