"""GPU: the vectorised DQN loop -- transition records re-rasterise to exactly the states they were recorded from,
the loop trains without errors, and the single-environment reference-style rollout runs on the drop-in API."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def make_env(E, seed=0, tower=2, max_steps=10):
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    H = 0.8
    return VecAssemblyGym(E, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., i * H + H / 2) for i in range(tower)],
                          [(0.5, 0, tower * H + H / 2)], max_steps=max_steps, seed=seed)


def test_records_rebuild_the_recorded_states():
    from robotoddler.training import records as R
    E = 32
    env, renv = make_env(E, seed=4), make_env(E, seed=99)
    for it in range(6):
        env.select_random()
        snap = R.snapshot(env)
        state_bits_before = env.state_bits.clone()
        sel = env.cand_offset[:E].long() + env.sel_index.long()
        sel_rows = (env.cand_desc[sel].clone(), env.cand_pose[sel].clone())
        env.step()
        rec, valid = R.make_records(env, snap, sel_rows)
        (nb, shape, pose, occ), (nnb, nshape, npose, nocc) = R.unpack_states(rec, env.K)
        renv.load_states(nb, shape, pose, occ)
        assert torch.equal(renv.state_bits[valid], state_bits_before[valid])
        renv.load_states(nnb, nshape, npose, nocc)
        assert torch.equal(renv.prefix_state_bits(nb)[valid], state_bits_before[valid])       # s is a prefix of s'
        cont = valid & ~env.step_flags[:, 5].bool()                 # not done: env now holds s' with its candidates
        assert cont.any()
        assert torch.equal(renv.state_bits[cont], env.state_bits[cont])
        assert torch.equal(renv.n_cand[cont], env.n_cand[cont])
        assert torch.equal(renv.n_valid[cont], env.n_valid[cont])
        for e in torch.nonzero(cont).squeeze(1).tolist()[:8]:
            a, b, n = int(renv.cand_offset[e]), int(env.cand_offset[e]), int(env.n_cand[e])
            assert torch.equal(renv.cand_mask[a:a + n], env.cand_mask[b:b + n])
            assert torch.equal(renv.cand_bits[a:a + n], env.cand_bits[b:b + n])
            assert torch.equal(renv.cand_pose[a:a + n], env.cand_pose[b:b + n])


@pytest.mark.parametrize("shape,E,n_rec", [("trapezoid", 48, 48), ("trapezoid", 48, 17), ("hexagon", 40, 40)])
def test_record_kernels_equal_the_torch_formulation(shape, E, n_rec):
    """bridges_record_state / _result write the very rows snapshot + make_records build, and bridges_replay_unpack (load_records)
    leaves the scratch env in the very state unpack_states + load_states + prefix_state_bits do (all arrays bit-identical)."""
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    from robotoddler.training import records as R
    H = 0.8
    mk = lambda seed: VecAssemblyGym(E, [load_urdf(f"shapes/{shape}.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)],
                                     [(0.5, 0, 2 * H + H / 2)], max_steps=12, seed=seed)
    env, renv_a, renv_b = mk(7), mk(1), mk(2)
    for it in range(8):
        env.select_random()
        sel = env.cand_offset[:E].long() + env.sel_index.long()
        snap = R.snapshot(env)
        sel_rows = (env.cand_desc[sel].clone(), env.cand_pose[sel].clone())
        rec = R.pack_state(env, sel)
        env.step()
        valid = R.pack_result(env, rec)
        want, want_valid = R.make_records(env, snap, sel_rows)
        assert torch.equal(valid, want_valid)
        assert torch.equal(rec, want), torch.nonzero(rec != want)[:5]
        # records of padded / unpadded batches into the scratch envs
        part = rec[:n_rec].contiguous()
        padded = torch.cat([part, part[:1].expand(E - n_rec, -1)]) if n_rec < E else part
        (nb, sh, po, oc), (nnb, nsh, npo, noc) = R.unpack_states(padded, renv_a.K)
        renv_a.load_states(nnb, nsh, npo, noc)
        bits_s_a = renv_a.prefix_state_bits(nb)
        bits_s, lin, stable_s, done, stable_n = renv_b.load_records(part)
        assert torch.equal(bits_s, bits_s_a)
        assert torch.equal(lin, padded[:, R.O_LIN].float()) and torch.equal(stable_s, padded[:, R.O_STABLE_S].float())
        assert torch.equal(done.bool(), padded[:, R.O_DONE] > 0.5) and torch.equal(stable_n.bool(), padded[:, R.O_STABLE_N] > 0.5)
        for name in ("n_blocks", "blk_shape", "blk_pose", "blk_occ", "n_cand", "n_valid", "state_bits", "blk_verts"):
            assert torch.equal(renv_a.buf[name], renv_b.buf[name]), name
        tot = int(renv_a.cand_offset[E])
        assert tot == int(renv_b.cand_offset[E])
        for name in ("cand_mask", "cand_bits", "cand_pose", "cand_desc", "cand_lin"):
            assert torch.equal(renv_a.buf[name][:tot], renv_b.buf[name][:tot]), name


@pytest.mark.parametrize("shape,E", [("trapezoid", 50), ("hexagon", 1100)])
def test_valid_rows_operator_equals_nonzero(shape, E):
    """bridges_valid_rows (scan of n_valid + ballot compaction per env) against torch.nonzero over the mask bytes: same rows in
    the same order, their envs, the per-env ranges; the alternating buffers keep the previous call's rows intact."""
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    H = 0.8
    env = VecAssemblyGym(E, [load_urdf(f"shapes/{shape}.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)],
                         [(0.5, 0, 2 * H + H / 2)], max_steps=12, seed=3)
    prev = None
    for it in range(5):
        idx, row_env = env.valid_rows()
        total = env.total_candidates()
        want = torch.nonzero(env.buf["cand_mask"][:total]).squeeze(1)
        assert torch.equal(idx, want)
        assert torch.equal(row_env, env.buf["cand_env"][want].long())
        lo, hi = env.valid_segments()
        assert lo.dtype == hi.dtype == torch.int32 and int(lo[0]) == 0 and int(hi[E - 1]) == idx.numel()
        assert torch.equal(hi - lo, env.n_valid[:E]) and torch.equal(lo[1:], hi[:-1])
        assert env.valid_rows()[0] is idx                                  # cached until the candidate set changes
        if prev is not None:
            assert torch.equal(prev[0], prev[1])                           # the rows of the call before are untouched
        prev = (idx, idx.clone())
        env.select_random()
        env.step()


TOWER2 = ["--tower_height", "2"]
HEX_BRIDGE =["--shapes", "hexagon", "--bridge_length", "3", "--max_steps", "15"]       # BASELINE.json configs[4]


@pytest.mark.parametrize("model,loss,task", [("SuccessorMLP", "mse_q_values+mse_block_features", TOWER2),
                                             ("ConvNet", "mse_q_values", TOWER2),
                                             ("UNet", "mse_block_features", TOWER2),
                                             ("UNet", "mse_q_values+mse_block_features", HEX_BRIDGE),
                                             ("SuccessorMLP", "mse_q_values", TOWER2 + ["--prioritized_replay"]),
                                             ("SuccessorMLP", "mse_q_values+mse_block_features", TOWER2 + ["--image_size", "32x32"]),
                                             ("ConvNet", "mse_q_values", TOWER2 + ["--image_size", "32x32"])])
def test_vectorised_training_runs(model, loss, task):
    from robotoddler.training.successor_dqn import build_parser, main
    hist = main(["--model", model, "--loss_function", loss, *task, "--num_envs", "64", "--num_episodes", "150",
                 "--num_training_steps", "2", "--batch_size", "16", "--seed", "1", "--learning_rate", "1e-4"])
    assert hist[-1]["episodes"] >= 150
    losses = [h["avg_loss"] for h in hist if h["avg_loss"] is not None]
    assert losses and all(np.isfinite(losses))


def test_bit_packed_acting_forward_equals_the_dense_factored_forward(monkeypatch):
    """SuccessorMLP acting: first layer from the bit-packed rasters (bridges_bits_linear) vs the torch-only factored
    forward on the f32 rasters vs the plain module forward, on the candidates of a running env."""
    from bridges_hip import ops
    from robotoddler.training.successor_dqn import build_parser, make_nets
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    dev = torch.device("cuda")
    env = make_env(256, seed=9, tower=4, max_steps=15)
    for _ in range(5):
        env.select_random()
        env.step()
    torch.manual_seed(3)
    net, _ = make_nets(args, dev)
    net.eval()
    E, px = env.E, 4096
    idx, row_env = env.valid_rows()
    binary = torch.zeros((E, 6), device=dev)
    binary[:, 0] = (torch.arange(E, device=dev) % 2).float()
    with torch.no_grad():
        W1 = net.first_layer().weight
        base = ops.bits_linear(env.state_bits, W1[:, :px].T, base=net.first_layer_env_terms(binary, env.reward_features, env.obstacle_raster),
                               base_row=torch.arange(E, device=dev))
        q_bits = net.q_from_first_layer(ops.bits_linear(env.cand_bits, W1[:, px:2 * px].T, bits_row=idx, base=base, base_row=row_env),
                                        env.reward_features)
        action = env.cand_raster.index_select(0, idx)
        q_fact = net.q_values_factored(env.state_raster, binary, action, row_env, env.reward_features, env.obstacle_raster)
        n = idx.numel()
        q_full = net(env.state_raster[row_env].unsqueeze(1), binary[row_env], action.unsqueeze(1),
                     env.reward_features.unsqueeze(0).expand(n, -1, -1, -1), env.obstacle_raster.unsqueeze(0).expand(n, -1, -1, -1))[0]
    assert n > 1000
    assert torch.allclose(q_bits, q_fact, rtol=1e-5, atol=1e-5), float((q_bits - q_fact).abs().max())
    assert torch.allclose(q_bits, q_full, rtol=1e-5, atol=1e-5), float((q_bits - q_full).abs().max())


@pytest.mark.parametrize("model", ["SuccessorMLP", "ConvNet"])
def test_rollout_td_error_follows_the_reference(model):
    """td_error of a transition (successor_dqn.py:413-426) = |q(s,a) - (reward + 0.95 * max_a' q(s',a'))|, next value 0
    when done, both q from the policy net; recomputed here with the plain module forward, env by env."""
    from robotoddler.training import records as R
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", model]))
    dev = torch.device("cuda")
    env = make_env(48, seed=13)
    torch.manual_seed(4)
    pol, tgt = make_nets(args, dev)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 4096, 8, 0.95, 0.01, "mse_q_values",
                   prioritized=True)
    agent.epsilon = 0.0                                              # greedy: q(s,a) is the maximum of the state's rows

    def rows_q():
        idx, row_env = env.valid_rows()
        stable = agent._stable_flags(env)
        with torch.no_grad():
            pol.eval()
            q = agent._forward_rows(pol, env, idx, row_env, stable)[0].float()
        return [q[row_env == e] for e in range(env.E)]

    checked = 0
    for it in range(6):
        q_before = rows_q()
        rec, valid = agent.act()
        td = agent.td_errors(rec)
        q_after = rows_q()
        for e in torch.nonzero(valid).squeeze(1).tolist():
            done = bool(rec[e, R.O_DONE] > 0.5)
            nxt = 0.0 if done or q_after[e].numel() == 0 else float(q_after[e].max())
            want = abs(float(q_before[e].max()) - (float(rec[e, R.O_REWARD]) + 0.95 * nxt))
            assert abs(float(td[e]) - want) <= 1e-5 + 1e-5 * abs(want), (it, e, float(td[e]), want)
            checked += 1
        agent.ring.push(rec[valid])
    assert checked > 100
    rec[:, R.O_TD] = td.to(rec.dtype)
    agent.ring.push(rec[valid])
    assert float(agent.ring.data[:len(agent.ring), R.O_TD].max()) > 0
    assert len(agent.train_steps(2)) == 2                            # prioritised sampling feeds the optimiser steps


def test_batched_targets_equal_per_batch_targets():
    """train_steps computes the TD targets of all its batches in one pass (the target net is constant meanwhile);
    the result must be what batch-by-batch evaluation gives."""
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    dev = torch.device("cuda")
    env = make_env(128, seed=5)
    torch.manual_seed(3)
    pol, tgt = make_nets(args, dev)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 10000, 16, 0.95, 0.01,
                   "mse_q_values+mse_block_features")
    for _ in range(8):
        rec, valid = agent.act()
        agent.ring.push(rec[valid])
    recs = [agent.ring.sample(16, agent.sample_gen) for _ in range(3)]
    whole = agent._targets(torch.cat(recs))
    for i, r in enumerate(recs):
        part = agent._targets(r)
        sl = slice(16 * i, 16 * (i + 1))
        for k in range(3):                                   # state raster, binary features, action raster: exact
            assert torch.equal(whole[k][sl], part[k])
        assert torch.allclose(whole[3][sl], part[3], rtol=1e-5, atol=1e-5)      # q target (GEMM batch shape differs)
        assert torch.allclose(whole[4][sl], part[4], rtol=1e-5, atol=1e-5)      # successor-feature target
    losses = agent.train_steps(3)
    assert len(losses) == 3 and all(np.isfinite(losses))


@pytest.mark.parametrize("model,loss,E,n_steps,locksteps", [("SuccessorMLP", "mse_q_values+mse_block_features", 64, 3, 6),
                                                            ("SuccessorMLP", "mse_block_features", 4096, 25, 14),
                                                            ("ConvNet", "mse_q_values", 64, 3, 6),
                                                            ("UNet", "mse_q_values+mse_block_features", 64, 3, 6),
                                                            ("UNet", "mse_q_values+mse_block_features", 256, 8, 8)])
def test_graph_captured_train_step_equals_eager(model, loss, E, n_steps, locksteps, monkeypatch):
    """The HIP-graph train step (third call onwards) performs the same optimiser steps and logs the same losses as
    eager PyTorch; the 4096-env case is the BASELINE.json configs[2] shape (25 steps of batch 32 per lock-step), the
    size at which a multi-workgroup reduction inside the graph used to return garbage (train_step.CapturedTrainStep)."""
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", model]))
    dev = torch.device("cuda")
    out = {}
    monkeypatch.setenv("BRIDGES_FUSED_MLP_STEP", "0")       # the autograd step in both modes (the hand-written one: below)
    for mode in ("1", "0"):
        monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", mode)
        env = make_env(E, seed=7, tower=4 if E > 64 else 2, max_steps=15 if E > 64 else 10)
        torch.manual_seed(11)
        pol, tgt = make_nets(args, dev)
        agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 100000, 32 if E > 64 else 16,
                       0.95, 0.01, loss, seed=2)
        losses = []
        for it in range(locksteps):
            l, _ = agent.lockstep(n_steps)
            losses += l
        assert (agent._graph_state is not None) == (mode == "1")
        out[mode] = (np.array(losses), torch.cat([p.detach().flatten() for p in pol.parameters()]).cpu())
    assert len(out["1"][0]) == len(out["0"][0]) == n_steps * locksteps
    assert (out["1"][0] >= 0).all()
    np.testing.assert_allclose(out["1"][0], out["0"][0], rtol=1e-4, atol=1e-6)
    # MIOpen's convolution backward is not bit-reproducible between runs and Adam turns a rounding-level gradient
    # difference of a near-zero gradient into a step of up to lr: the conv net gets 15 steps x lr of slack
    atol = 1e-6 if model == "SuccessorMLP" else 15 * 1e-4
    diff = float((out["1"][1] - out["0"][1]).abs().max())
    print(f"max |weight difference| graph vs eager after {n_steps * locksteps} steps: {diff:.3e}")
    assert torch.allclose(out["1"][1], out["0"][1], rtol=1e-4, atol=atol), diff


@pytest.mark.parametrize("loss,E,n_steps", [("mse_q_values+mse_block_features", 64, 3), ("mse_block_features", 4096, 25),
                                            ("mse_q_values", 64, 5)])
def test_hand_written_mlp_step_in_the_graph_follows_the_autograd_graph(loss, E, n_steps, monkeypatch):
    """The captured train step with the hand-written forward / loss / backward (bridges_hip/mlp_ops.py) against the
    captured autograd step.  Two identically seeded agents run two lock-steps eagerly (bit-identical), the third
    lock-step's optimiser steps go through the respective graph on the same ring, the same sampled batches and the
    same weights: the logged losses agree to 1e-4 relative.  The weights agree to Adam's sensitivity: a gradient entry
    that is rounding noise moves its weight by up to lr per step in either run."""
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    dev, lr = torch.device("cuda"), 1e-4
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("BRIDGES_FUSED_MLP_STEP", fused)
        env = make_env(E, seed=7, tower=4 if E > 64 else 2, max_steps=15 if E > 64 else 10)
        torch.manual_seed(11)
        pol, tgt = make_nets(args, dev)
        agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=lr, fused=True), env, 100000, 32 if E > 64 else 16,
                       0.95, 0.01, loss, seed=2)
        losses = [agent.lockstep(n_steps)[0] for _ in range(3)]
        assert agent._graph_state is not None and agent._graph_state["fused"] == (fused == "1")
        out[fused] = (losses, torch.cat([p.detach().flatten() for p in pol.parameters()]).cpu())
    for k in range(2):
        assert out["1"][0][k] == out["0"][0][k]                                    # eager lock-steps: the same bits
    a, b = np.array(out["1"][0][2]), np.array(out["0"][0][2])
    assert len(a) == n_steps and (a >= 0).all()
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-7)
    diff = (out["1"][1] - out["0"][1]).abs()
    print(f"weights after {n_steps} graph steps: max |diff| {float(diff.max()):.3e}, mean {float(diff.mean()):.3e}")
    assert float(diff.max()) <= 2 * n_steps * lr and float(diff.mean()) < 0.02 * lr


def test_graph_is_recaptured_when_a_call_brings_more_batches(monkeypatch):
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", "1")
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    dev = torch.device("cuda")
    env = make_env(64, seed=21)
    torch.manual_seed(1)
    pol, tgt = make_nets(args, dev)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 10000, 16, 0.95, 0.01, "mse_block_features")
    for _ in range(4):
        agent.lockstep(2)
    first = agent._graph_state
    assert first is not None and first["n_max"] == 2
    losses = agent.train_steps(5)                                    # more batches than the captured arrays hold
    assert agent._graph_state is not first and agent._graph_state["n_max"] == 5
    assert len(losses) == 5 and all(np.isfinite(losses)) and min(losses) >= 0
    assert len(agent.train_steps(1)) == 1                            # fewer batches re-use the graph


def test_vectorised_loop_writes_reference_layout_checkpoints(tmp_path):
    import json, os
    from robotoddler.training.successor_dqn import main
    main(["--model", "SuccessorMLP", "--loss_function", "mse_q_values", "--tower_height", "2", "--num_envs", "64",
          "--num_episodes", "120", "--num_training_steps", "1", "--batch_size", "8", "--seed", "0", "--learning_rate", "1e-4",
          "--save_checkpoint", str(tmp_path), "--checkpoint_every", "50"])
    latest = os.path.realpath(tmp_path / "latest")
    # the reference's five files (utils.py:54-89) + agent.pt: what the vectorised loop needs on top to resume exactly
    assert sorted(os.listdir(latest)) == ["agent.pt", "meta.json", "optimizer.pt", "policy_net.pt", "replay_buffer.pt", "target_net.pt"]
    assert json.load(open(os.path.join(latest, "meta.json")))["episode"] >= 50
    blob = torch.load(os.path.join(latest, "replay_buffer.pt"), weights_only=True)
    assert blob["records"].shape[0] > 0


@pytest.mark.parametrize("extra", [[], ["--prioritized_replay"], ["--image_size", "32x32"]])
def test_single_env_reference_loop_runs(extra):
    from robotoddler.training.successor_dqn import main
    hist = main(["--model", "SuccessorMLP", "--loss_function", "mse_q_values+mse_block_features", "--tower_height", "2",
                 "--num_episodes", "6", "--num_training_steps", "2", "--batch_size", "4", "--seed", "0",
                 "--learning_rate", "1e-4", *extra])
    assert len(hist) == 6 and all(h["num_steps"] >= 1 for h in hist)


def test_cpu_device_is_rejected():
    from robotoddler.training.successor_dqn import main
    with pytest.raises(SystemExit):
        main(["--device", "cpu"])


def test_vectorised_exploration_follows_the_batched_reading_of_the_reference_rule():
    """VecDQN.act with every env exploring (epsilon = 1): each env takes the valid candidate whose raster overlaps
    least with the count image of its episode step AS IT WAS AT THE START of the lock-step (first minimum, in candidate
    order), and the chosen rasters are added to the images afterwards -- successor_dqn.py:116-129 applied env by env
    (oracle.dqn.vectorised_explore).  With epsilon = 0 every env takes its arg-max q candidate and the images stay."""
    from oracle import dqn as O
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    dev = torch.device("cuda")
    for f32 in (False, True):                               # bit-packed acting path and the f32-raster path
        env = make_env(64, seed=21, tower=2, max_steps=10)
        if f32:
            VecDQN.FACTORED_ACTING = False
        try:
            torch.manual_seed(6)
            pol, tgt = make_nets(args, dev)
            opt = torch.optim.Adam(pol.parameters(), lr=1e-4)
            agent = VecDQN(pol, tgt, opt, env, 4096, 8, 0.9, 0.01, "mse_q_values", seed=2, eps_start=1.0, eps_end=1.0)
            n_checked = 0
            for it in range(6):
                E = env.E
                idx, row_env = env.valid_rows()
                off = env.cand_offset[:E].cpu().numpy()
                step_of_env = env.n_blocks.cpu().tolist()
                dense = ((env.cand_bits[idx].cpu().numpy().astype(np.uint64)[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1))
                dense = torch.tensor(dense.astype(np.float32))
                rows_of_env = [torch.nonzero(row_env.cpu() == e).squeeze(1) for e in range(E)]
                rasters = [dense[r] for r in rows_of_env]
                images_before = agent.step_images.cpu().clone()
                agent.epsilon = 1.0 if it < 4 else 0.0
                explore = [agent.epsilon == 1.0] * E
                sel, images_after = O.vectorised_explore(images_before, step_of_env, rasters, explore)
                q_all = agent._policy_q(env, idx, row_env, agent._stable_flags(env)).cpu() if it >= 4 else None
                agent.act()
                chosen = env.sel_index.cpu().numpy()
                for e in range(E):
                    if len(rows_of_env[e]) == 0:
                        continue
                    want_row = sel[e] if sel[e] is not None else int(torch.argmax(q_all[rows_of_env[e]]))
                    assert chosen[e] == int(idx[rows_of_env[e][want_row]]) - off[e], (f32, it, e)
                    n_checked += 1
                assert torch.equal(agent.step_images.cpu(), images_after), (f32, it)
            assert n_checked > 250
        finally:
            VecDQN.FACTORED_ACTING = True


def test_load_checkpoint_resumes_the_vectorised_loop(tmp_path):
    """--save_checkpoint / --load_checkpoint (utils.py:31-89, successor_dqn.py:654-665 of the reference): a run that is
    checkpointed after ~150 episodes and a second main() call that resumes from that directory produce the same losses
    for the lock-steps that follow (nets, optimiser, replay ring, epsilon, count images, RNG streams and counters are
    restored; a checkpoint is taken with all environments freshly reset)."""
    import os
    from robotoddler.training.successor_dqn import main
    common = ["--model", "SuccessorMLP", "--loss_function", "mse_q_values+mse_block_features", "--tower_height", "2", "--num_envs", "64",
              "--num_training_steps", "2", "--batch_size", "16", "--seed", "3", "--learning_rate", "1e-4", "--checkpoint_every", "150"]
    a = main([*common, "--num_episodes", "290", "--save_checkpoint", str(tmp_path)])
    ckpts = sorted(int(d) for d in os.listdir(tmp_path) if d.isdigit())
    assert ckpts and ckpts[0] < 290
    first = os.path.join(str(tmp_path), str(ckpts[0]))
    assert sorted(os.listdir(first)) == ["agent.pt", "meta.json", "optimizer.pt", "policy_net.pt", "replay_buffer.pt", "target_net.pt"]
    b = main([*common, "--num_episodes", "290", "--load_checkpoint", first])
    by_step = {h["lockstep"]: h for h in a}
    assert b[0]["lockstep"] == min(k for k, h in by_step.items() if h["episodes"] >= ckpts[0]) + 1
    n = 0
    for h in b[:20]:
        ref = by_step[h["lockstep"]]
        assert h["episodes"] == ref["episodes"] and h["env_steps"] == ref["env_steps"]
        assert h["epsilon"] == ref["epsilon"]
        assert h["avg_loss"] == pytest.approx(ref["avg_loss"], rel=1e-4), h["lockstep"]
        n += 1
    assert n >= 10


@pytest.mark.parametrize("E,amax,p_valid", [(1, 7, 0.5), (3, 70, 0.0), (1025, 130, 0.3), (5000, 9, 1.0)])
def test_valid_rows_operator_on_ragged_and_empty_inputs(E, amax, p_valid):
    """bridges_valid_rows straight through the C ABI on synthetic candidate sets: envs without candidates, without valid
    candidates, all valid, more envs than one scan pass (1024) and more candidates than one wave pass (64)."""
    import ctypes as C
    from bridges_hip import abi
    from bridges_hip.ops import _ptr, _stream
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(E + amax)
    n_cand = torch.randint(0, amax + 1, (E,), generator=g, dtype=torch.int32)
    n_cand[::7] = 0                                                          # envs with no candidate at all
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(n_cand, 0)
    total = int(off[E])
    mask = (torch.rand(max(total, 1), generator=g) < p_valid).to(torch.uint8)
    mask[total:] = 0
    env_of = torch.repeat_interleave(torch.arange(E), n_cand.long())
    n_valid = torch.zeros(E, dtype=torch.int32)
    n_valid.index_add_(0, env_of, mask[:total].to(torch.int32))
    d = lambda t: t.to(dev)
    off_d, nc_d, nv_d, mask_d = d(off), d(n_cand), d(n_valid), d(mask)
    seg = torch.full((E + 1,), -7, dtype=torch.int32, device=dev)
    idx = torch.full((max(total, 1),), -7, dtype=torch.int64, device=dev)
    renv = torch.full((max(total, 1),), -7, dtype=torch.int64, device=dev)
    host = torch.full((1,), -7, dtype=torch.int32).pin_memory()
    abi.check(abi.lib().bridges_valid_rows(E, _ptr(off_d), _ptr(nc_d), _ptr(nv_d), _ptr(mask_d), None, _ptr(seg), None, None, _ptr(idx),
                                           _ptr(renv), C.c_void_p(host.data_ptr()), _stream()), "bridges_valid_rows")
    torch.cuda.synchronize()
    want = torch.nonzero(mask[:total]).squeeze(1)
    n = int(host[0])
    assert n == want.numel() == int(n_valid.sum())
    assert torch.equal(idx[:n].cpu(), want) and torch.equal(renv[:n].cpu(), env_of[want])
    assert torch.equal(seg.cpu()[1:] - seg.cpu()[:-1], n_valid) and int(seg[0]) == 0
    assert bool((idx[n:] == -7).all()) and bool((renv[n:] == -7).all())      # nothing written past the rows


def test_record_kernels_at_the_last_block_slot_and_on_the_floor():
    """bridges_replay_unpack on hand-made records: a state that already holds K - 1 blocks (the action block takes the last
    slot), an action on the floor (target_block = -1: no occupancy update), one record for a scratch env of many."""
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    from robotoddler.training import records as R
    H = 0.8
    mk = lambda seed: VecAssemblyGym(6, [load_urdf("shapes/trapezoid.urdf")], [(0.5, 0., H / 2)], [(0.5, 0, H + H / 2)], max_steps=5, seed=seed)
    a, b = mk(1), mk(2)
    K = a.K
    g = torch.Generator().manual_seed(0)
    rec = torch.zeros((2, R.RECORD_WIDTH), dtype=torch.float64)
    for r, (nb, tb) in enumerate([(K - 1, 2), (0, -1)]):
        rec[r, R.O_NB] = nb
        rec[r, R.O_POSE:R.O_POSE + 4 * K] = torch.rand(4 * K, generator=g, dtype=torch.float64)
        rec[r, R.O_OCC:R.O_OCC + K] = torch.randint(0, 16, (K,), generator=g).double()
        rec[r, R.O_APOSE:R.O_APOSE + 4] = torch.tensor([0.3, 1.1, 1.0, 0.0], dtype=torch.float64)
        rec[r, R.O_ATB], rec[r, R.O_ATF], rec[r, R.O_AFACE] = tb, 1, 3
        rec[r, R.O_LIN], rec[r, R.O_DONE], rec[r, R.O_STABLE_S], rec[r, R.O_STABLE_N] = 0.25 * (r + 1), r, 1, 1 - r
    for n_rec in (2, 1):
        part = rec[:n_rec].cuda().contiguous()
        padded = torch.cat([part, part[:1].expand(6 - n_rec, -1)])
        (nb, sh, po, oc), (nnb, nsh, npo, noc) = R.unpack_states(padded, K)
        a.load_states(nnb, nsh, npo, noc)
        bits_s, lin, stable_s, done, stable_n = b.load_records(part)
        assert torch.equal(bits_s, a.prefix_state_bits(nb))
        for name in ("n_blocks", "blk_shape", "blk_pose", "blk_occ", "n_cand", "n_valid", "state_bits"):
            assert torch.equal(a.buf[name], b.buf[name]), name
        assert torch.equal(lin, padded[:, R.O_LIN].float()) and torch.equal(done.bool(), padded[:, R.O_DONE] > 0.5)


@pytest.mark.parametrize("model,loss", [("ConvNet", "mse_q_values"), ("UNet", "mse_q_values+mse_block_features")])
def test_distinct_row_forward_equals_the_forward_of_every_row(model, loss):
    """The conv Q-networks are fed every DISTINCT (state, candidate, stable flag) input once (VecDQN._distinct_rows: hash of the
    bit rasters, torch.unique, word-for-word verification against the group's representative) and the outputs are copied to
    the duplicates.  Against feeding every row: same q (1e-5: the batch composition of the convolutions differs), same TD /
    successor-feature targets, on the candidate sets of a running env set -- where many envs share early states."""
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", model, "--loss_function", loss]))
    dev = torch.device("cuda")
    env = make_env(256, seed=31, tower=2, max_steps=10)
    torch.manual_seed(8)
    pol, tgt = make_nets(args, dev)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 8192, 16, 0.95, 0.01, loss, seed=5)
    try:
        fed = []
        for it in range(5):
            idx, row_env = env.valid_rows()
            stable = agent._stable_flags(env)
            with torch.no_grad():
                pol.eval()
                VecDQN.DEDUP_ROWS = True
                agent.rows_fed = 0
                q_d, sf_d, sb_d, inv = agent._forward_rows(pol, env, idx, row_env, stable)
                fed.append((agent.rows_fed, idx.numel()))
                VecDQN.DEDUP_ROWS = False
                q_a, sf_a, sb_a, none = agent._forward_rows(pol, env, idx, row_env, stable)
            assert none is None and q_a.shape == q_d.shape == (idx.numel(),)
            assert torch.allclose(q_d, q_a, rtol=1e-5, atol=1e-5), float((q_d - q_a).abs().max())
            if inv is not None:
                assert inv.shape == (idx.numel(),) and int(inv.max()) + 1 == fed[-1][0] < idx.numel()
                if sf_a is not None:
                    assert torch.allclose(sf_d.index_select(0, inv), sf_a, rtol=1e-5, atol=1e-5)
                if sb_a is not None:
                    assert torch.allclose(sb_d.index_select(0, inv), sb_a, rtol=1e-5, atol=1e-5)
            VecDQN.DEDUP_ROWS = True
            rec, valid = agent.act()
            agent.ring.push(rec[valid])
        assert fed[0][0] * 20 < fed[0][1]              # lock-step 1: every env holds the reset state -- one env's rows are fed
        assert all(f < s for f, s in fed[:3])
        rec = agent.ring.sample(64, agent.sample_gen)
        VecDQN.DEDUP_ROWS = True
        with_d = agent._targets(rec)
        VecDQN.DEDUP_ROWS = False
        without = agent._targets(rec)
        for a, b in zip(with_d, without):
            if a is None:
                assert b is None
            else:
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), float((a - b).abs().max())
        # a hash that collides (all multipliers zero) must be caught by the word-for-word check: plain path, same result
        VecDQN.DEDUP_ROWS = True
        agent._hash_mult = torch.zeros((2, 64), dtype=torch.int64, device=dev)
        idx, row_env = env.valid_rows()
        stable = agent._stable_flags(env)
        assert agent._distinct_rows(env, idx, row_env, stable) is None
    finally:
        VecDQN.DEDUP_ROWS = True


def _state_keys(env, flag):
    nb = env.n_blocks.cpu().numpy()
    shape, pose, occ = env.blk_shape.cpu().numpy(), env.blk_pose.cpu().numpy().view(np.int64), env.blk_occ.cpu().numpy()
    fl = flag.cpu().numpy().astype(np.uint8)
    return [(int(nb[e]), shape[e, :nb[e]].tobytes(), pose[e, :nb[e]].tobytes(), occ[e, :nb[e]].tobytes(), int(fl[e])) for e in range(env.E)]


@pytest.mark.parametrize("shape,E", [("trapezoid", 256), ("hexagon", 100)])
def test_state_groups_and_shared_rows(shape, E):
    """bridges_env_groups: rep[e] = the first env whose state (block count, live shapes / pose bits / occupancy, flag byte)
    equals env e's, against a dictionary of the states built on the host; bridges_valid_rows with rep: only representatives
    get rows, and the range every env is given holds exactly its own valid candidates (same rasters, descriptors and poses in
    the same order)."""
    from bridges_hip.shapes import load_urdf
    from bridges_hip.vec_env import VecAssemblyGym
    H = 0.8
    env = VecAssemblyGym(E, [load_urdf(f"shapes/{shape}.urdf")], [(0.5, 0., i * H + H / 2) for i in range(2)],
                         [(0.5, 0, 2 * H + H / 2)], max_steps=12, seed=3)
    shared_some = False
    for it in range(6):
        flag = (env.step_flags[:, 1] != 0) | (env.n_blocks == 0)
        rep = env.state_groups(flag).cpu().numpy()
        first = {}
        want = np.array([first.setdefault(k, e) for e, k in enumerate(_state_keys(env, flag))])
        assert np.array_equal(rep, want), it
        if it == 0:
            assert (rep == 0).all()                                        # every env holds the reset state
        # stale data in dead block slots must not split a group: scribble over them
        dead = torch.arange(env.K, device=env.device)[None, :] >= env.n_blocks[:, None]
        env.blk_pose[dead] = float(it) + 0.5
        env.blk_shape[dead] = 7
        assert np.array_equal(env.state_groups(flag).cpu().numpy(), want)
        # the flag byte is part of the state
        odd = (torch.arange(E, device=env.device) % 2).bool()
        rep_f = env.state_groups(odd).cpu().numpy()
        first = {}
        assert np.array_equal(rep_f, np.array([first.setdefault(k, e) for e, k in enumerate(_state_keys(env, odd))]))
        idx_all, env_all = env.valid_rows()
        idx_all, env_all = idx_all.clone(), env_all.clone()
        lo_all, hi_all = (t.clone() for t in env.valid_segments())
        rep_d = env.state_groups(flag)
        idx, row_env = env.valid_rows(rep_d)
        lo, hi = env.valid_segments()
        is_rep = torch.tensor(want == np.arange(E), device=env.device)
        assert idx.numel() == int(env.n_valid[:E][is_rep].sum()) <= idx_all.numel()
        assert bool(is_rep[row_env].all())                                 # rows belong to representatives only
        shared_some |= idx.numel() < idx_all.numel()
        assert torch.equal(hi - lo, env.n_valid[:E])                       # every env: as many rows as it has valid candidates
        for e in range(E):
            mine, theirs = idx_all[lo_all[e]:hi_all[e]], idx[lo[e]:hi[e]]
            assert torch.equal(env.cand_bits[mine], env.cand_bits[theirs])
            assert torch.equal(env.cand_desc[mine], env.cand_desc[theirs]) and torch.equal(env.cand_pose[mine], env.cand_pose[theirs])
            assert torch.equal(mine - env.cand_offset[e], theirs - env.cand_offset[int(want[e])])       # same candidate numbers
        env.select_random()
        env.step()
    assert shared_some


def test_acting_on_shared_rows_selects_what_acting_on_every_row_selects():
    """VecDQN with DEDUP_STATES: q of the shared rows equals q of every env's own rows (1e-5; the head's column split
    depends on the row count), and with the same q values bridges_eps_greedy_select picks the same candidate NUMBER for every
    env, exploring or greedy, through (seg_lo, seg_hi, rep) as through the prefix sums of all rows."""
    from bridges_hip import ops
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    args = vars(build_parser().parse_args(["--model", "SuccessorMLP"]))
    dev = torch.device("cuda")
    env = make_env(256, seed=17, tower=2, max_steps=10)
    torch.manual_seed(12)
    pol, tgt = make_nets(args, dev)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), env, 4096, 8, 0.95, 0.01, "mse_q_values", seed=4)
    E = env.E
    try:
        for it in range(5):
            stable = agent._stable_flags(env)
            VecDQN.DEDUP_STATES = False
            env._dqn_rows = None
            idx_a, env_a, (lo_a, hi_a), rep_a = agent._rows(env, stable)
            assert rep_a is None
            idx_a, env_a, lo_a, hi_a = idx_a.clone(), env_a.clone(), lo_a.clone(), hi_a.clone()
            q_a = agent._policy_q(env, idx_a, env_a, stable).clone()
            VecDQN.DEDUP_STATES = True
            env._dqn_rows = None
            idx_s, env_s, (lo_s, hi_s), rep = agent._rows(env, stable)
            q_s = agent._policy_q(env, idx_s, env_s, stable)
            assert idx_s.numel() < idx_a.numel()
            # row of the shared set that serves every row of the full set
            src = torch.cat([torch.arange(int(lo_s[e]), int(hi_s[e]), device=dev) for e in range(E)])
            assert src.numel() == idx_a.numel()
            assert torch.allclose(q_s[src], q_a, rtol=1e-5, atol=1e-5), float((q_s[src] - q_a).abs().max())
            step_of = env.n_blocks.long()
            join_s = ops.bits_dot(env.cand_bits, agent.step_images + 0.25 * it, step_of[env_s], bits_row=idx_s)
            join_a = ops.bits_dot(env.cand_bits, agent.step_images + 0.25 * it, step_of[env_a], bits_row=idx_a)
            assert torch.equal(join_s[src], join_a)
            u = torch.rand(E, device=dev)
            for eps, greedy in ((0.5, False), (0.0, True)):
                got_s = ops.eps_greedy_select((lo_s, hi_s), q_s, join_s, u, eps, greedy, idx_s, env.cand_offset[:E], rep=rep)
                got_a = ops.eps_greedy_select((lo_a, hi_a), q_s[src].contiguous(), join_a, u, eps, greedy, idx_a, env.cand_offset[:E])
                assert torch.equal(got_s[1], got_a[1])                      # the same candidate number in every env
                assert torch.equal(got_s[2], got_a[2]) and torch.equal(got_s[3], got_a[3])
                assert torch.equal(env.cand_bits[got_s[0]], env.cand_bits[got_a[0]])
            rec, valid = agent.act()
            agent.ring.push(rec[valid])
    finally:
        VecDQN.DEDUP_STATES = True


def test_graph_guard_puts_weights_and_adam_state_back_on_the_device(monkeypatch):
    """The conv nets' replayed autograd step: parameters and Adam state are copied before the replays of a call and restored by a
    device-side torch.where when one of the call's losses is negative or not finite -- no host decision in between; good losses
    leave the updated weights alone."""
    from robotoddler.training.successor_dqn import build_parser, make_nets
    from robotoddler.training.vec_dqn import VecDQN
    monkeypatch.setenv("BRIDGES_TRAIN_GRAPH", "1")
    args = vars(build_parser().parse_args(["--model", "ConvNet", "--loss_function", "mse_q_values"]))
    dev = torch.device("cuda")
    env = make_env(64, seed=3, tower=2, max_steps=10)
    torch.manual_seed(2)
    pol, tgt = make_nets(args, dev)
    agent = VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4, fused=True), env, 10000, 16, 0.95, 0.01, "mse_q_values", seed=1)
    for _ in range(5):
        losses, _ = agent.lockstep(2)
    st = agent._graph_state
    assert st is not None and not st.get("fused") and "guard" in st          # the captured autograd step ran, with its snapshot
    tensors = agent._guard_tensors()
    assert len(tensors) > 10                                                  # flat parameters + every Adam moment / step count
    agent._guard_snapshot(st)
    before = [t.clone() for t in tensors]
    for t in tensors:
        t.add_(1)
    agent._guard_restore(st, torch.tensor([0.5, 0.25], device=dev))           # good losses: nothing is put back
    assert all(torch.equal(t, b + 1) for t, b in zip(tensors, before))
    for bad in ([0.5, -1e-3], [float("nan"), 0.1], [float("inf"), 0.1]):
        for t in tensors:
            t.fill_(float("nan")) if t.is_floating_point() else t.zero_()
        agent._guard_restore(st, torch.tensor(bad, device=dev))
        assert all(torch.equal(t, b) for t, b in zip(tensors, before)), bad
