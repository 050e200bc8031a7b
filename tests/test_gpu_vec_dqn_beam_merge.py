"""GPU: VecDQN.beam_search(merge=True) on the small SuccessorMLP setup of test_gpu_vec_dqn_beam.py (hidden [8], 8 or 16 held-out
tasks, max_steps 6, width 8).  Without merging the live beams of a group do hold duplicates (the keys are computed on the host from the
env's state after every depth, by tests/beam_merge_ref.py); with merging none survives a depth and merged_beams counts exactly the
beams a host-side statement closes; the returned structures replay to what the search reports; width 1 is untouched; no training
state changes; and merging adds no host wait."""
import pytest
import torch

import beam_merge_ref as MR
from test_gpu_vec_dqn_beam import GAMMA, M, _training_state, _waits, check_replay, make_agent, random_env

pytestmark = pytest.mark.gpu
WIDTH = 8
SEED = 77                                                    # the held-out tasks of test_gpu_vec_dqn_beam.py


def _keys(env, live):
    """The key (key_last = 1) of every live env, from the env's state arrays as they stand; None for a closed env."""
    case = dict(K=env.K, key_last=1, n_blocks=env.n_blocks.cpu().numpy(), blk_shape=env.blk_shape.cpu().numpy(),
                blk_pose=env.blk_pose.cpu().numpy(), blk_occ=env.blk_occ.cpu().numpy(), targets_left=env.targets_left.cpu().numpy())
    alive = live.cpu().numpy().astype(bool)
    return [MR.key(case, e) if alive[e] else None for e in range(env.E)]


def _duplicates(keys, B):
    """Per group: the live envs that share their key with an earlier live env of the group."""
    out = []
    for g in range(len(keys) // B):
        seen, n = set(), 0
        for k in keys[g * B:(g + 1) * B]:
            if k is not None:
                n += k in seen
                seen.add(k)
        out.append(n)
    return out


def _search(agent, beam_env, width, merge):
    """One search with the keys of the live beams recorded after every depth -> (result, per depth the per-group duplicates,
    per depth the live count)."""
    dups, lives = [], []

    def on_depth(d, live):
        assert d == len(dups) and live.dtype == torch.uint8 and live.numel() == beam_env.E
        dups.append(_duplicates(_keys(beam_env, live), width))
        lives.append(int(live.sum()))
    res = agent.beam_search(beam_env, width, merge=merge, on_depth=on_depth)
    return res, dups, lives


def _sharp_agent(scale):
    """make_agent() with the weights of its nets spread by ``scale`` rather than by 3: a sharper q concentrates the beam."""
    from robotoddler.models.cv import SuccessorMLP
    from robotoddler.training.vec_dqn import VecDQN
    from robotoddler.utils.utils import init_weights

    def mlp():
        torch.manual_seed(1)
        net = SuccessorMLP(img_size=(64, 64), hidden_dims=[8]).to("cuda")
        net.apply(init_weights)
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() > 1:
                    p.mul_(scale)
        return net
    pol, tgt = mlp(), mlp()
    return VecDQN(pol, tgt, torch.optim.Adam(pol.parameters(), lr=1e-4), random_env(32, seed=2), 4096, 16, GAMMA, 0.01,
                  "mse_q_values+mse_block_features", seed=3, per_env_tasks=True)


# Duplicates under key_last = 1 need two placements that commute AND a common last block, and the default ground positions leave
# room for one ground block: in this setup most seeds show none (40 task seeds x {8, 16} tasks were tried: one did).  The two
# configurations below are those found to hold some -- (agent, tasks, task seed); the first test asserts it for each.
CONFIGS = {"tasks_16_seed_75": (make_agent, 16, 75), "sharp_q_tasks_8_seed_79": (lambda: _sharp_agent(10.0), M, 79)}


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def setup(request):
    from robotoddler.training.vec_dqn import beam_env_like
    make, tasks, seed = CONFIGS[request.param]
    eval_env = random_env(tasks, seed=seed)
    return make(), eval_env, beam_env_like(eval_env, WIDTH)


@pytest.fixture(scope="module")
def fresh():
    """An agent and a beam env the duplicate tests do not share (one of them trains)."""
    from robotoddler.training.vec_dqn import beam_env_like
    return make_agent(), beam_env_like(random_env(M, seed=SEED), WIDTH)


def test_without_merging_live_beams_hold_duplicates(setup):
    agent, _eval_env, beam_env = setup
    res, dups, lives = _search(agent, beam_env, WIDTH, merge=False)
    total = [sum(d) for d in dups]
    print("duplicates among live beams per depth:", total, "live beams per depth:", lives)
    assert sum(total) > 0                                    # the search does spend width on permutations of one structure
    assert res["merged_beams"] == [0] * (beam_env.E // WIDTH)
    assert res == agent.beam_search(beam_env, WIDTH)         # on_depth and merge=False change nothing


def test_with_merging_no_duplicate_survives_a_depth_and_the_count_is_the_hosts(setup):
    agent, eval_env, beam_env = setup
    seen = []

    def on_depth(d, live):
        seen.append(_keys(beam_env, live))
    res = agent.beam_search(beam_env, WIDTH, merge=True, on_depth=on_depth)
    assert len(seen) == beam_env.K
    for d, keys in enumerate(seen):
        assert _duplicates(keys, WIDTH) == [0] * (beam_env.E // WIDTH), f"depth {d}: two live beams of a group share a key"
    assert sum(res["merged_beams"]) > 0 and len(res["merged_beams"]) == beam_env.E // WIDTH
    assert sum(res["merged_by_depth"]) == sum(res["merged_beams"])
    assert all(0 <= m <= n <= beam_env.E for m, n in zip(res["merged_by_depth"], res["live_by_depth"]))
    # the host's count: the same search again, holding the live flags BEFORE the merge (everything the merge closed was live and
    # shared its key with a survivor) against those after it
    res2, closed = _host_count(agent, beam_env)
    assert res2 == res
    assert res["merged_beams"] == closed
    check_replay(eval_env, res)
    assert agent.beam_search(beam_env, WIDTH, merge=True) == res             # again: the same search


def _host_count(agent, beam_env):
    """merge=True once more, with bridges_beam_merge's inputs captured at every call -> (result, per task the number of live envs
    whose key an env before them in (ret descending, env ascending) holds -- counted on the host with the numpy keys)."""
    from bridges_hip import ops
    closed = [0] * (beam_env.E // WIDTH)
    inner = ops.beam_merge

    def counting(n_blocks, blk_shape, blk_pose, blk_occ, targets_left, width, live, ret, key_last=True, out=None):
        assert width == WIDTH and key_last
        keys = _keys(beam_env, live)
        for g, n in enumerate(_duplicates(keys, WIDTH)):
            closed[g] += n
        out = inner(n_blocks, blk_shape, blk_pose, blk_occ, targets_left, width, live, ret, key_last=key_last, out=out)
        case = dict(B=WIDTH, K=beam_env.K, key_last=1, n_blocks=n_blocks.cpu().numpy(), blk_shape=blk_shape.cpu().numpy(),
                    blk_pose=blk_pose.cpu().numpy(), blk_occ=blk_occ.cpu().numpy(), targets_left=targets_left.cpu().numpy(),
                    live=live.cpu().numpy(), ret=ret.cpu().numpy())
        want = MR.reference(case)                            # and the launch inside the loop is the rule's, exactly
        for k in MR.OUTPUTS:
            assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        return out
    ops.beam_merge = counting
    try:
        res = agent.beam_search(beam_env, WIDTH, merge=True)
    finally:
        ops.beam_merge = inner
    return res, closed


def test_width_1_is_untouched_by_merging():
    from robotoddler.training.vec_dqn import beam_env_like
    agent = make_agent()
    beam_env = beam_env_like(random_env(M, seed=SEED), 1)
    plain, merged = agent.beam_search(beam_env, 1), agent.beam_search(beam_env, 1, merge=True)
    assert set(merged) - set(plain) == {"merged_by_depth", "live_by_depth"}
    for k in plain:
        assert plain[k] == merged[k], k
    assert merged["merged_beams"] == [0] * M and merged["merged_by_depth"] == [0] * beam_env.K
    assert all(0 <= n <= M for n in merged["live_by_depth"])


def test_merging_touches_no_training_state(fresh):
    agent, beam_env = fresh
    for _ in range(3):
        agent.lockstep(1)
    torch.cuda.synchronize()
    before = _training_state(agent)
    agent.beam_search(beam_env, WIDTH, merge=True)
    torch.cuda.synchronize()
    assert _training_state(agent) == before


def test_merging_adds_no_host_wait(fresh):
    agent, beam_env = fresh
    agent.beam_search(beam_env, WIDTH)
    agent.beam_search(beam_env, WIDTH, merge=True)           # (allocations and caches of the first calls are behind us)
    _waits(lambda: None)                                     # (switching the sync debug mode on warns once itself)
    plain = _waits(lambda: agent.beam_search(beam_env, WIDTH))
    merged = _waits(lambda: agent.beam_search(beam_env, WIDTH, merge=True))
    print("waits of beam_search():", plain, "with merging:", merged)
    assert sorted(merged) == sorted(plain), (merged, plain)
    assert merged.count("stream") == beam_env.K and merged.count("event") == merged.count("device") == 0
