"""Successor-feature DQN with the reference's CLI surface (robotoddler/training/successor_dqn.py of the reference).

Two ways to run:

* ``--num_envs 1`` (default): the reference's single-environment loop -- rollout_episode / train_policy_net /
  update_target_net with the same signatures and Transition layout -- on the assembly_gym drop-in (every
  placement, stability solve and raster is a HIP operator call).
* ``--num_envs N`` (N > 1): N environments in lock-step on the GPU (VecAssemblyGym) with a device replay buffer
  of compact transition records that are re-rasterised when sampled (robotoddler/training/vec_dqn.py).

Flags are the reference's (successor_dqn.py:573-596) plus ``--tower_height`` (README / BASELINE.json name for
``bridge_setup(num_stories=N)``; absent from the reference's argparse at HEAD), ``--num_envs``, ``--shapes``.
There is no CPU path: ``--device cpu`` is rejected.
"""
import argparse
import os
import random
import sys
from collections import namedtuple

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from assembly_gym.envs.assembly_env import AssemblyEnv, Block, Shape                      # noqa: E402
from assembly_gym.envs.gym_env import (AssemblyGym, bridge_setup, horizontal_bridge_setup,  # noqa: E402
                                       sparse_reward)
from assembly_gym.utils.rendering import render_blocks_2d_bits                            # noqa: E402
from bridges_hip import dqn_ops, ops                                                      # noqa: E402
from robotoddler.models.cv import ConvNet, Policy, SuccessorMLP                           # noqa: E402
from robotoddler.training import train_step as T                                         # noqa: E402
from robotoddler.utils.actions import filter_actions, filter_stable_actions, generate_actions  # noqa: E402
from robotoddler.utils.replay_memory import PrioritizedReplayBuffer, ReplayBuffer          # noqa: E402
from robotoddler.utils.utils import (convolve_with_gaussian, init_weights, parse_img_size,   # noqa: E402
                                     save_checkpoint)

Transition = namedtuple('Transition',
                        ('block_features', 'binary_features', 'action', 'action_features', 'reward', 'lin_reward',
                         'done', 'reward_features', 'obstacle_features', 'next_block_features',
                         'next_binary_features', 'next_available_actions', 'next_actions_features',
                         'next_reward_features', 'next_obstacle_features', 'td_error'))


def _image(bits, img_size):
    """bit raster(s) -> f32 [n, S, S] (contiguous)."""
    return ops.crop(ops.bits_to_f32(bits), img_size).contiguous()


# ---- feature extraction (successor_dqn.py:47-94) ---------------------------------------------------------------
def _state_features(observation, xlim, ylim, img_size, device):
    """get_state_features plus the state's bit raster (what the candidate filter tests overlaps against)."""
    binary = [observation['stable'], observation['collision'], observation['collision_block'],
              observation['collision_obstacle'], observation['collision_floor'], observation['collision_boundary']]
    bits = render_blocks_2d_bits(observation['blocks'], xlim, ylim, img_size)
    image = _image(bits, img_size)                                                                     # [1,S,S] f32
    binary_t, = ops.upload(image.device, np.asarray(binary, dtype=np.float32))                         # (no blocking copy)
    return image.to(device), binary_t.to(device), bits


def get_state_features(observation, xlim=(0, 1), ylim=(0, 1), img_size=(64, 64), device=None):
    image, binary, _bits = _state_features(observation, xlim, ylim, img_size, device)
    return image, binary


def get_task_features(obs, xlim=(0, 1), ylim=(0, 1), img_size=(64, 64), device=None):
    cube = Shape(urdf_file='shapes/cube06.urdf')
    target_blocks = [Block(shape=cube, position=target) for target in obs['targets']]
    reward = _image(render_blocks_2d_bits(target_blocks, xlim, ylim, img_size), img_size)[0]
    reward = convolve_with_gaussian(reward, 101, 16)                                      # successor_dqn.py:80-82
    obstacle = _image(render_blocks_2d_bits(obs['obstacle_blocks'], xlim, ylim, img_size), img_size)
    return reward.unsqueeze(0).to(device), obstacle.to(device)


def get_action_features(env, actions, xlim=(0, 1), ylim=(0, 1), img_size=(64, 64), device=None):
    # one batched bridges_create_block call for all candidates when the gym offers it (the reference: one call each)
    blocks = env.create_blocks(actions) if hasattr(env, "create_blocks") else [env.create_block(action) for action in actions]
    return _image(ops.raster_bits(blocks, xlim, ylim, img_size), img_size).unsqueeze(1).to(device)   # [A,1,S,S]


# ---- policies (successor_dqn.py:98-132) -------------------------------------------------------------------------
class EpsilonGreedy:
    """epsilon-greedy with count-based exploration: explore = the action whose raster overlaps least with the
    rasters already tried at this episode step."""

    def __init__(self, eps_start=0.5, eps_end=0.05, gamma=0.99, episode=0, max_steps=10, device=torch.device('cpu')):
        self.epsilon = (eps_start - eps_end) * (gamma ** episode) + eps_end
        self.eps_start, self.eps_end, self.gamma = eps_start, eps_end, gamma
        self.max_steps, self.device = max_steps, device
        self.step_images = [torch.zeros(64, 64, device=device) for _ in range(max_steps)]

    def step(self):
        self.epsilon = (self.epsilon - self.eps_end) * self.gamma + self.eps_end
        return self

    def __call__(self, q_values, step_index, action_features, *args, **kwargs):
        if random.random() > self.epsilon:
            return torch.argmax(q_values).item()
        if step_index >= len(self.step_images):            # the reference indexes past max_steps=10 (latent IndexError)
            self.step_images += [torch.zeros(64, 64, device=self.device) for _ in range(step_index + 1 - len(self.step_images))]
        feats = action_features.squeeze(1).to(self.device)
        if self.step_images[step_index].shape != feats.shape[-2:]:       # --image_size other than the 64x64 default
            self.step_images[step_index] = torch.zeros(feats.shape[-2:], device=self.device)
        join = torch.sum(self.step_images[step_index] * feats, dim=(-1, -2))
        sel = torch.argmin(join).item()
        self.step_images[step_index] += feats[sel]
        return sel


def check_temperature_schedule(temp_start, temp_end, decay, who="Softmax"):
    """0 < temp_end <= temp_start, 0 < decay <= 1, all three finite (a NaN fails every comparison)."""
    if not (0.0 < temp_end <= temp_start < float("inf")):
        raise ValueError(f"{who}: the temperature falls from temp_start to temp_end, 0 < temp_end <= temp_start < inf, "
                         f"not from {temp_start} to {temp_end}")
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"{who}: the decay of the temperature lies in (0, 1], not {decay}")


def boltzmann_row(q_values, u, temp):
    """The row a Boltzmann draw takes (the rule of bridges_boltzmann_select, include/bridges_hip.h, in float64 on the host):
    weights exp((q - m) / temp) with m the largest q that is neither NaN nor -inf (such rows weigh 0; m = +inf: the +inf rows weigh 1),
    prefix sums in row order, the first row whose prefix exceeds u * total -- none, by rounding: the last row that weighs anything;
    no eligible row: row 0."""
    q = np.asarray(q_values, dtype=np.float64).reshape(-1)
    elig = ~np.isnan(q) & (q != -np.inf)
    if not elig.any():
        return 0
    m = q[elig].max()
    w = np.zeros_like(q)
    if m == np.inf:
        w[q == np.inf] = 1.0
    else:
        with np.errstate(under="ignore"):
            w[elig] = np.exp((q[elig] - m) / float(temp))
    c = np.add.accumulate(w)
    hit = c > float(u) * c[-1]
    return int(np.argmax(hit)) if hit.any() else int(np.flatnonzero(w > 0)[-1])


class Softmax:
    """Boltzmann exploration with an annealed temperature (successor_dqn.py:138-154 of the reference, whose sketch cannot run: it
    never sets temp_end and draws a probability where it means an index).  Row j is taken with probability proportional to
    exp(q_j / temp); the uniform draw comes from ``random``, the stream EpsilonGreedy uses, so --seed covers it."""

    def __init__(self, temp_start=1, temp_end=0.1, decay=0.99, episode=0):
        check_temperature_schedule(temp_start, temp_end, decay)
        self.temp = (temp_start - temp_end) * (decay ** episode) + temp_end
        self.temp_start, self.temp_end, self.decay = temp_start, temp_end, decay

    def step(self):
        self.temp = (self.temp - self.temp_end) * self.decay + self.temp_end
        return self

    def __call__(self, q_values, *args, **kwargs):
        q = q_values.detach().float().cpu().numpy() if torch.is_tensor(q_values) else q_values
        return boltzmann_row(q, random.random(), self.temp)


# ---- training (successor_dqn.py:157-288) ------------------------------------------------------------------------
def _task_key(*tensors):
    """Fingerprint of an episode's task features (reward map, obstacle raster): transitions whose tensors carry the same key
    share them VALUE for value, which is what lets a batch go through the hand-written optimiser step (one reward / obstacle
    vector per batch).  One host read per episode."""
    import hashlib
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().float().cpu().numpy().tobytes())
    return h.hexdigest()


def _tagged(t, key):
    t._task_key = key
    return t


def _fused_applies(policy_net, optimizer, loss_parts, scheduler, transitions, batch=None, device=None):
    """train_policy_net's optimiser steps go through the hand-written SuccessorMLP step (train_step.CapturedTrainStep) when the
    transitions share one task fingerprint: one reward / obstacle vector per batch.  Same losses as the autograd form: the
    reference's q target is the [B, B] broadcast  lin_reward[j] + gamma q'[i]  (successor_dqn.py:222 with :435), whose
    mean-squared error against q[i] is  mean_i (q[i] - (mean(lin) + gamma q'[i]))^2 + var(lin)  -- the same gradient as the
    element-wise target mean(lin) + gamma q'[i]; the constant var(lin) is added to the logged loss."""
    if scheduler is not None or getattr(policy_net, "_flat_params", None) is None or type(optimizer) is not torch.optim.Adam:
        return False
    if not T.fused_step_enabled(policy_net, loss_parts) or not transitions:
        return False
    if batch is not None:
        if not batch.block_features.is_cuda or batch.block_features.dtype != torch.float32:
            return False
    elif torch.device(device).type != 'cuda' or any(t.block_features.dtype != torch.float32 for t in transitions):
        return False
    keys = {getattr(t.reward_features, "_task_key", None) for t in transitions}
    return len(keys) == 1 and None not in keys and all(getattr(t.obstacle_features, "_task_key", None) in keys for t in transitions)


def _fused_driver(policy_net, optimizer, batch_size, loss_parts, n):
    """The net's driver of the hand-written step, or None if the optimiser is not a plain Adam over the flattened parameters."""
    try:
        return T.CapturedTrainStep.of(policy_net, optimizer, batch_size, loss_parts, n, img=policy_net.img_size, fused=True)
    except ValueError:
        return None


def _run_fused(tr, drawn, target_net, gamma, device):
    """The optimiser steps on the batches ``drawn`` (lists of transitions of one task).  The target net does not change inside a
    train_policy_net call, so the TD targets of all steps come from ONE target forward and ONE segmented argmax over all
    next-action rows, and the steps are launch sequences that read their batch by a device-side counter: per step the host
    queues 11 launches and nothing else.  A transition drawn several times (the draws are with replacement across the steps;
    20 x 32 draws from a buffer of a few hundred) is stacked and evaluated once and its rows are gathered; the rows of a next
    state are gathered from one copy per transition; the task's reward / obstacle rasters are the same image for every row."""
    n, B, px = len(drawn), tr.B, tr.img[0] * tr.img[1]
    slot, uniq, which = {}, [], []
    for b in drawn:
        for t in b:
            k = slot.get(id(t))
            if k is None:
                k = slot[id(t)] = len(uniq)
                uniq.append(t)
            which.append(k)
    cat = lambda field: torch.cat([getattr(t, field) for t in uniq]).to(device=device)
    num_actions = [max(1, len(t.next_available_actions)) for t in uniq]
    assert [t.next_actions_features.shape[0] for t in uniq] == num_actions, "a next state's action rows and its action list differ"
    seg_np = np.zeros(len(uniq) + 1, dtype=np.int32)
    np.cumsum(num_actions, out=seg_np[1:])
    owner = np.repeat(np.arange(len(uniq), dtype=np.int64), num_actions)
    seg, done, owner, which = ops.upload(device, seg_np, np.asarray([t.done for t in uniq], dtype=np.bool_), owner,
                                         np.asarray(which, dtype=np.int64))
    rows = int(seg_np[-1])
    reward, obstacle = uniq[0].reward_features.to(device), uniq[0].obstacle_features.to(device)
    with torch.no_grad():
        action_u = cat('action_features')
        one_row = lambda x: x.shape[0] == 1 or x.stride(0) == 0              # rollout_episode stores expand()ed views
        if all(one_row(t.next_block_features) and one_row(t.next_binary_features) for t in uniq):
            nb = torch.cat([t.next_block_features[:1] for t in uniq]).to(device).index_select(0, owner)
            nbin = torch.cat([t.next_binary_features[:1] for t in uniq]).to(device).index_select(0, owner)
        else:
            nb, nbin = cat('next_block_features'), cat('next_binary_features')
        next_q, next_sf, _ = target_net(nb, nbin, cat('next_actions_features'), reward.expand(rows, -1, -1, -1),
                                        obstacle.expand(rows, -1, -1, -1))
        q_sel, sf_target = dqn_ops.next_targets(seg, next_q, done, gamma, next_sf=next_sf[:, 0] if tr.use_sf else None,
                                                action_raster=action_u.squeeze(1))
        if sf_target is not None:
            sf_target = sf_target.reshape(len(uniq), px).index_select(0, which)
        q_target = extra = None
        if tr.use_q:
            lin = cat('lin_reward').reshape(-1).float().index_select(0, which).view(n, B)
            m = lin.mean(dim=1, keepdim=True)
            q_target = (m + gamma * q_sel.index_select(0, which).view(n, B)).reshape(-1).contiguous()
            extra = ((lin - m) ** 2).mean(dim=1)
        losses = tr.run(n, cat('block_features').reshape(len(uniq), px).index_select(0, which),
                        action_u.reshape(len(uniq), px).index_select(0, which), cat('binary_features').index_select(0, which),
                        reward.reshape(px).contiguous(), obstacle.reshape(px).contiguous(), q_target, sf_target)
    return losses + extra if extra is not None else losses.clone()


sync_fused_optimizer = T.sync_optimizer      # (this module's name for it: call before optimizer.state_dict() / .step())


def train_policy_net(policy_net, target_net, optimizer, replay_buffer, gamma, loss_fct='mse_q_values', scheduler=None,
                     n_steps=10, batch_size=16, verbose=False, device='cuda'):
    if len(replay_buffer) < batch_size:
        return
    loss_fct = loss_fct.split('+')
    policy_net.train()
    target_net.eval()
    mse = torch.nn.MSELoss()
    losses = []
    # the draws of all steps first: they depend on the buffer and the random generators only, which the steps do not touch
    # (a buffer without draw(): one sample() per step, as the reference)
    draw = getattr(replay_buffer, "draw", None)
    if draw is not None:
        from robotoddler.utils.replay_memory import _stack
        drawn = [draw(batch_size) for _ in range(n_steps)]
        if batch_size is not None and _fused_applies(policy_net, optimizer, loss_fct, scheduler, [t for b in drawn for t in b], device=device):
            tr = _fused_driver(policy_net, optimizer, batch_size, loss_fct, min(n_steps, 64))
            if tr is not None:                            # (chunks of 64 bound the target pass: 64 steps x 32 transitions x their next actions)
                out = [_run_fused(tr, drawn[k:k + 64], target_net, gamma, device) for k in range(0, n_steps, 64)]
                return torch.cat(out).tolist()            # ONE host read for all steps
        steps = ((transitions, _stack(transitions, device)) for transitions in drawn)
    else:
        steps = (replay_buffer.sample(batch_size=batch_size, stack_tensors=True, device=device) for _ in range(n_steps))
    for transitions, batch in steps:
        tr = None
        if _fused_applies(policy_net, optimizer, loss_fct, scheduler, transitions, batch):
            tr = _fused_driver(policy_net, optimizer, batch.block_features.shape[0], loss_fct, 1)
        if tr is not None:                                # a batch of one task: the same step as a call of one batch
            losses.append(_run_fused(tr, [transitions], target_net, gamma, device))
            continue
        T.release(policy_net)                             # optimizer.step() takes over: it needs the true step count,
        #                                                   and a later hand-written step adopts the optimiser's state afresh
        q_values, succ_block_features, succ_binary_features = policy_net(
            batch.block_features, batch.binary_features, batch.action_features, batch.reward_features,
            batch.obstacle_features)
        with torch.no_grad():
            next_q, next_sf, _next_bin = target_net(
                batch.next_block_features, batch.next_binary_features, batch.next_actions_features,
                batch.next_reward_features, batch.next_obstacle_features)
            num_actions = [max(1, len(a)) for a in batch.next_available_actions]
            seg = torch.tensor(np.cumsum([0] + num_actions), dtype=torch.int32, device=next_q.device)
            done = torch.tensor(batch.done, dtype=torch.bool, device=next_q.device)
            use_sf = 'mse_block_features' in loss_fct
            if use_sf and succ_block_features is None:
                raise ValueError("No successor block features available from the chosen policy net.")
            # fused HIP op: segmented argmax over the ragged next-action rows, done masking, a + gamma psi'.  q_sel is the
            # done-masked next q of the selected action; the reward is added below with torch broadcasting, because the
            # reference adds a [B,1] lin_reward to a [B] vector (successor_dqn.py:222 with :435) and thereby trains on a
            # [B,B] target -- reproduced as is.
            q_sel, sf_target = dqn_ops.next_targets(seg, next_q, done, gamma, next_sf=next_sf[:, 0] if use_sf else None,
                                                    action_raster=batch.action_features.squeeze(1))
        loss = 0.
        if 'mse_q_values' in loss_fct:
            loss = loss + mse(q_values, batch.lin_reward + gamma * q_sel)
        if use_sf:
            loss = loss + mse(succ_block_features[:, 0], sf_target.view_as(succ_block_features[:, 0]))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        losses.append(loss.detach())
    return torch.stack([l.reshape(()) for l in losses]).tolist() if losses else []      # ONE host read for all steps


def update_target_net(policy_net, target_net, tau=0.01):
    """theta_target <- tau * theta + (1 - tau) * theta_target (successor_dqn.py:280-288) with the HIP soft-update
    kernel: one launch when both nets were flattened (dqn_ops.FlatParameters), else one per tensor."""
    fp, ft = getattr(policy_net, "_flat_params", None), getattr(target_net, "_flat_params", None)
    if fp is not None and ft is not None:
        dqn_ops.soft_update_(ft.flat, fp.flat, tau)
        return
    tsd, psd = target_net.state_dict(), policy_net.state_dict()
    for key, p in psd.items():
        t = tsd[key]
        if t.dtype == torch.float32 and t.is_contiguous() and p.is_contiguous() and t.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0:
            dqn_ops.soft_update_(t, p, tau)
        else:                                             # non-float / unaligned buffers: not on the hot path
            t.copy_(p * tau + t * (1 - tau))


def flatten_nets(*nets):
    for n in nets:
        n._flat_params = dqn_ops.FlatParameters(n)


# ---- rollout (successor_dqn.py:365-475) -------------------------------------------------------------------------
def rollout_episode(env, policy, policy_net, x_discr_ground, setup_fct, offset_values=[0.], img_size=(64, 64),
                    xlim=(0, 1), ylim=(0, 1), log_images=False, device=None, stable_actions_only=False):
    """stable_actions_only: the available actions of a state are filter_actions ∩ is_action_stable_rbe (one batched
    stability call per state, filter_stable_actions); everything downstream -- the policy's choice, the no-action
    termination, the next-state maximum and the transitions' next actions -- sees only those."""
    done, transitions = False, []
    images = [] if log_images else None
    policy_net.eval()
    obs, info = env.reset(**setup_fct())
    kw = dict(img_size=img_size, device=device, xlim=xlim, ylim=ylim)
    reward_features, obstacle_features = get_task_features(obs, **kw)
    task_key = _task_key(reward_features, obstacle_features)        # lets train_policy_net batch transitions of one task
    block_features, binary_features, state_bits = _state_features(obs, xlim, ylim, img_size, device)
    obstacle_bits = render_blocks_2d_bits(obs['obstacle_blocks'], xlim, ylim, img_size)
    batched = hasattr(env, "create_blocks") and tuple(img_size)[0] == tuple(img_size)[1] <= 64

    def candidates(block_f, bits_s):
        acts, feats = filtered_candidates(block_f, bits_s)
        return filter_stable_actions(env, acts, feats) if stable_actions_only else (acts, feats)

    def filtered_candidates(block_f, bits_s):
        """generate_actions -> get_action_features -> filter_actions (successor_dqn.py:375-377) of the current state.  With the
        drop-in gym the three are ONE operator call (bridges_action_features: rasters of every candidate, the bounds test of
        collision_on_action and the two overlap tests of filter_actions; tests/test_gpu_api_golden.py shows it equal to the
        composition) and one mask copied back, instead of a reduction pair and a host read per action."""
        acts = [*generate_actions(env, x_discr_ground=x_discr_ground, offset_values=offset_values)]
        if not batched or not acts:
            feats = get_action_features(env, acts, **kw)
            return filter_actions(env, acts, feats, block_features=block_f, obstacle_features=obstacle_features, xlim=xlim, ylim=ylim)
        _bits, img, mask, _lin = ops.action_features(env.create_blocks(acts), xlim, ylim, state_bits=bits_s, obstacle_bits=obstacle_bits,
                                                     img_size=img_size, want_f32=True)
        keep = np.flatnonzero(mask.cpu().numpy())                                          # the one host read of the filter
        rows, = ops.upload(img.device, keep.astype(np.int64))
        feats = ops.crop(img, img_size).index_select(0, rows).unsqueeze(1).contiguous().to(device)
        return [acts[i] for i in keep], feats

    available_actions, action_features = candidates(block_features, state_bits)
    num_actions = len(available_actions)
    step_index = 0

    def qnet(bf, binf, af, n):
        with torch.no_grad():
            return policy_net(bf.expand(n, -1, -1, -1), binf.expand(n, -1), af, reward_features.expand(n, -1, -1, -1),
                              obstacle_features.expand(n, -1, -1, -1))

    q_next = None
    while not done:
        # (the net's outputs for this state were computed as "next state" of the previous step: the same net in eval mode on
        # the same rows -- the reference runs the forward a second time, successor_dqn.py:383 after :420)
        q_values, succ_block_features, succ_binary_features = q_next if q_next is not None else qnet(
            block_features, binary_features, action_features, num_actions)
        sel = policy(q_values, step_index, action_features, succ_block_features, succ_binary_features)
        sel = int(sel)
        action = available_actions[sel]
        selected_action_features = action_features[sel]
        next_observation, reward, terminated, truncated, info = env.step(action)
        done = bool(terminated or truncated)
        frozen_stable, unfrozen_stable = env.stabilities_freezing()
        lin_reward = torch.zeros(1, device=device).view(-1)
        if frozen_stable:
            lin_reward = torch.sum(selected_action_features * reward_features).view(-1) / 100
        if unfrozen_stable:
            lin_reward = torch.sum(selected_action_features * reward_features).view(-1)
        next_block_features, next_binary_features, state_bits = _state_features(next_observation, xlim, ylim, img_size, device)
        next_available_actions, next_action_features = candidates(next_block_features, state_bits)
        num_actions = len(next_available_actions)
        if num_actions == 0:
            done = True
            next_action_features = torch.zeros([1, 1, *img_size], device=device)
        # q(s, a) and max_a' q(s', a') travel to the host together (one read instead of two)
        pair = [q_values[sel].reshape(1).float()]
        q_next = None
        if not done:
            q_next = qnet(next_block_features, next_binary_features, next_action_features, num_actions)
            pair.append(q_next[0].max().reshape(1).float())
        pair = torch.cat(pair).tolist()
        q_value, next_q_value = pair[0], (pair[1] if not done else 0)
        td_error = abs(q_value - (reward + 0.95 * next_q_value))          # successor_dqn.py:425 (hard-coded 0.95)
        n1 = max(1, num_actions)
        transitions.append(Transition(
            block_features=block_features.unsqueeze(0), binary_features=binary_features.unsqueeze(0),
            action_features=selected_action_features.unsqueeze(0), reward_features=_tagged(reward_features.unsqueeze(0), task_key),
            obstacle_features=_tagged(obstacle_features.unsqueeze(0), task_key), action=action, lin_reward=lin_reward.unsqueeze(0),
            reward=torch.Tensor([reward]), done=done,
            next_block_features=next_block_features.expand(n1, -1, -1, -1),
            next_binary_features=next_binary_features.expand(n1, -1), next_actions_features=next_action_features,
            next_reward_features=reward_features.expand(n1, -1, -1, -1),
            next_obstacle_features=obstacle_features.expand(n1, -1, -1, -1),
            next_available_actions=next_available_actions, td_error=td_error))
        block_features, binary_features = next_block_features, next_binary_features
        action_features, available_actions = next_action_features, next_available_actions
        if log_images:
            if succ_block_features is None:
                raise ValueError("No successor block features available from the chosen policy net. Disable image "
                                 "logging or use a different model.")
            images.append(dict(succ_block_features=succ_block_features[sel][0].cpu().numpy()))
        step_index += 1
    return transitions, images


def rollout_episode_scripted(env, predefined_actions, setup_fct, x_discr_ground, offset_values=[0.], img_size=(64, 64),
                             xlim=(-3, 7), ylim=(0., 10), log_images=False, device=None):
    """Roll out predefined actions (successor_dqn.py:290-362): lin_reward = sum(action raster * reward map) without
    the stability scaling, td_error = 0."""
    done, transitions, images = False, [], ([] if log_images else None)
    obs, info = env.reset(**setup_fct())
    kw = dict(img_size=img_size, device=device, xlim=xlim, ylim=ylim)
    reward_features, obstacle_features = get_task_features(obs, **kw)
    block_features, binary_features = get_state_features(obs, **kw)
    for action in predefined_actions:
        if done:
            break
        selected_action_features = get_action_features(env, [action], **kw)[0]
        next_observation, reward, terminated, truncated, info = env.step(action)
        done = bool(terminated or truncated)
        lin_reward = torch.sum(selected_action_features * reward_features)
        next_block_features, next_binary_features = get_state_features(next_observation, **kw)
        acts = [*generate_actions(env, x_discr_ground=x_discr_ground, offset_values=offset_values)]
        feats = get_action_features(env, acts, **kw)
        next_available_actions, next_action_features = filter_actions(env, acts, feats, next_block_features,
                                                                      obstacle_features=obstacle_features, xlim=xlim, ylim=ylim)
        n = len(next_available_actions)
        transitions.append(Transition(
            block_features=block_features.unsqueeze(0), binary_features=binary_features.unsqueeze(0),
            action_features=selected_action_features.unsqueeze(0), reward_features=reward_features.unsqueeze(0),
            obstacle_features=obstacle_features.unsqueeze(0), action=action, lin_reward=lin_reward.unsqueeze(0),
            reward=torch.Tensor([reward]), done=done, next_block_features=next_block_features.expand(n, -1, -1, -1),
            next_binary_features=next_binary_features.expand(n, -1), next_actions_features=next_action_features,
            next_reward_features=reward_features.expand(n, -1, -1, -1),
            next_obstacle_features=obstacle_features.expand(n, -1, -1, -1),
            next_available_actions=next_available_actions, td_error=0))
        block_features, binary_features = next_block_features, next_binary_features
        if log_images:
            images.append(dict(succ_block_features=next_block_features[0].cpu().numpy()))
    return transitions, images


def track_run_sinks(values, step, context, aim_run=None, wandb_run=None):
    """The two logging sinks of log_episode (successor_dqn.py:544-565 of the reference), shared by the single-env loop
    (step = episode) and the vectorised loop (step = finished episodes so far): aim gets one ``track(value, name=key,
    step=step, context={'context': context})`` per value that is not None; wandb one ``log`` of a dict with the
    reference's keys -- ``episode`` first, then the values as they are (``avg_loss`` may be None),
    ``episode_<step>_combined_image`` (None: this build draws no matplotlib figure) and ``eval_reward`` (the linear
    reward in an evaluation context, else None).  The reference calls the module-level ``wandb.log``; a run object's
    ``log`` is the same call."""
    if aim_run is not None:
        for k, v in values.items():
            if v is not None:
                aim_run.track(v, name=k, step=step, context=dict(context=context))
    if wandb_run is not None:
        payload = {"episode": step}
        payload.update({k: v for k, v in values.items() if k != 'epsilon'})
        payload[f"episode_{str(step).zfill(5)}_combined_image"] = None
        payload["eval_reward"] = values.get('lin_reward') if context == 'evaluation' else None
        wandb_run.log(payload)


def log_episode(episode, transitions, losses, gamma, context='training', policy=None, images=None, log_images=False,
                wandb_run=None, aim_run=None, verbose=False):
    """Episode summary (successor_dqn.py:479-567) without the matplotlib figure; aim / wandb sinks are used when the
    caller passes live run objects."""
    info = {
        'reward': sum(gamma ** i * t.reward for i, t in enumerate(transitions)).item(),
        'lin_reward': sum(gamma ** i * t.lin_reward for i, t in enumerate(transitions)).item(),
        'avg_loss': sum(losses) / len(losses) if losses else None,
        'num_steps': len(transitions),
        'stable': transitions[-1].next_binary_features[0, 0].item(),
        'collision': transitions[-1].next_binary_features[0, 1].item(),
    }
    if policy is not None and hasattr(policy, 'epsilon'):
        info['epsilon'] = policy.epsilon
    if policy is not None and hasattr(policy, 'temp'):       # a Softmax policy
        info['temperature'] = policy.temp
    track_run_sinks(info, episode, context, aim_run=aim_run, wandb_run=wandb_run)
    return info, None


# ---- CLI (successor_dqn.py:570-787) -----------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--num_episodes", type=int, default=1000, help="Number of episodes for training.")
    p.add_argument("--max_steps", type=int, default=10, help="Max steps per episode.")
    p.add_argument("--seed", type=int, default=None, help="Random seed.")
    p.add_argument("--num_training_steps", type=int, default=20, help="Number of training steps in each episode.")
    p.add_argument("--learning_rate", type=float, default=0.01, help="Adam learning rate.")
    p.add_argument("--loss_function", choices=['mse_q_values', 'mse_block_features', 'mse_q_values+mse_block_features'],
                   default='mse_q_values', help="Loss function for training")
    p.add_argument("--tau", type=float, default=0.01, help="Step size for updating target net.")
    p.add_argument("--batch_size", type=int, default=32, help="Batch size.")
    p.add_argument("--gamma", type=float, default=0.8, help="Discount factor.")
    p.add_argument("--model", choices=['SuccessorMLP', 'ConvNet', 'UNet'], default='UNet', help="Model type.")
    p.add_argument("--device", choices=['cpu', 'cuda'], default='cuda', help="Device to use (this build is GPU-only).")
    p.add_argument("--image_size", type=parse_img_size, default="64x64", help="Size of image features {width}x{height}.")
    p.add_argument("--load_checkpoint", type=str, default=None, help="Path to a checkpoint to load.")
    p.add_argument("--save_checkpoint", type=str, default=None, help="Path to save the checkpoint.")
    p.add_argument("--checkpoint_every", type=int, default=1000, help="")
    p.add_argument("--evaluate_every", type=int, default=100, help="")
    p.add_argument("--aim", action='store_true', help="Use aim logging.")
    p.add_argument("--aim_repo", type=str, default='aim-data/', help="Path to aim repository.")
    p.add_argument("--bridge_length", type=int, default=1, help="Length of the bridge in blocks")
    p.add_argument("--tower_height", type=int, default=None,
                   help="Height of the tower: bridge_setup(num_stories=N) (README / BASELINE.json flag).")
    p.add_argument("--verbose", action='store_true', help="Verbose output.")
    p.add_argument("--log_images", action='store_true', help="Log images.")
    p.add_argument("--replay_buffer_capacity", type=int, default=2000, help="Replay buffer capacity.")
    p.add_argument("--wandb", type=bool, default=False, help="Use wandb logging.")
    p.add_argument("--num_envs", type=int, default=1, help="Environments advanced in lock-step on the GPU.")
    p.add_argument("--prioritized_replay", action='store_true',
                   help="Sample transitions in proportion to |td_error| + 1e-5 (PrioritizedReplayBuffer, replay_memory.py:45-93).")
    p.add_argument("--shapes", choices=['trapezoid', 'hexagon', 'both'], default='trapezoid')
    p.add_argument("--stable_actions_only", action='store_true',
                   help="Restrict every action set to the stable placements (filter_actions ∩ is_action_stable_rbe), in both loops.")
    # the evaluation options of the vectorised loop enter the namespace only when given (argparse.SUPPRESS), so that a plain
    # parse keeps the keys it always had; their defaults (EVAL_DEFAULTS) apply where run_vectorised reads them
    p.add_argument("--eval_envs", type=int, default=argparse.SUPPRESS,
                   help="Vectorised loop: greedy evaluation of one episode in each of N envs every --evaluate_every episodes "
                        "(default 0: none). The single-env loop evaluates one episode anyway and ignores it.")
    p.add_argument("--eval_epsilon", type=float, default=argparse.SUPPRESS,
                   help="Vectorised loop: exploration rate of the evaluation episodes (default 0.0: greedy, as the reference).")
    p.add_argument("--random_targets", type=int, default=argparse.SUPPRESS, metavar="T",
                   help="Vectorised loop, SuccessorMLP: tower_setup(num_targets=T) per env and episode -- every env draws T "
                        "fresh targets whenever it starts an episode (trapezoid blocks, no obstacles); --eval_envs evaluates on a "
                        "fixed held-out set of tasks. Not with --tower_height / --bridge_length.")
    p.add_argument("--random_obstacles", type=int, default=argparse.SUPPRESS, metavar="O",
                   help="With --random_targets T only: every env also draws O obstacles (x in [-3, 3), z in [0.3, 2.5)) whenever it "
                        "starts an episode, as connecting_setup draws obstacles beside its targets; the evaluation env draws its own.")
    p.add_argument("--task_channels", action='store_true', default=argparse.SUPPRESS,
                   help="With --random_targets T [--random_obstacles O] and --model ConvNet or UNet at 64x64: train the conv "
                        "Q-network on the per-env tasks -- every row is fed the reward map and the obstacle raster of its env as "
                        "image channels, written with its block and action rasters by one kernel (bridges_conv_input_rows).")
    p.add_argument("--random_bridge_length", type=parse_size_range, default=argparse.SUPPRESS, metavar="LO:HI",
                   help="Vectorised loop: horizontal_bridge_setup(num_obstacles=n) per env and episode, n drawn from LO..HI "
                        "(0 <= LO <= HI <= 4) on the device whenever an env starts an episode; success is logged per n. "
                        "--model SuccessorMLP, or ConvNet / UNet with --task_channels; any --shapes.")
    p.add_argument("--random_tower_height", type=parse_size_range, default=argparse.SUPPRESS, metavar="LO:HI",
                   help="Vectorised loop: bridge_setup(num_stories=n) per env and episode, n drawn from LO..HI, as "
                        "--random_bridge_length draws the span.")
    add_training_arguments(p)
    add_eval_beam_argument(p)
    add_eval_particle_arguments(p)
    return p


def add_training_arguments(p, prioritized_flag=False):
    """Every option group of the vectorised loop's training, in the order --help lists them: the one list build_parser and the
    tools that train through VecDQN share (``prioritized_flag``: see add_priority_arguments)."""
    add_curriculum_arguments(p)
    add_n_step_argument(p)
    add_double_q_argument(p)
    add_target_temperature_argument(p)
    add_relative_temperature_arguments(p)
    add_munchausen_arguments(p)
    add_priority_arguments(p, prioritized_flag=prioritized_flag)
    add_exploration_arguments(p)
    add_hindsight_arguments(p)
    add_search_arguments(p)


def agent_options_from_args(args, num_envs=None):
    """VecDQN's keyword arguments for the groups of add_training_arguments, from parsed options (``num_envs``: for a parser whose
    flag has another name).  The groups are asked in the order main() checks them, so a line with two faults is refused in the
    words main() would use."""
    from robotoddler.training.vec_dqn import curriculum_from_args
    if num_envs is not None:
        args = dict(args, num_envs=num_envs)
    out = dict(curriculum=curriculum_from_args(args), n_step=args.get('n_step', 1), double_q=bool(args.get('double_q', False)))
    for group in (target_temperature_from_args, relative_temperature_from_args, munchausen_from_args, priority_from_args,
                  exploration_from_args, hindsight_from_args, search_from_args):
        out.update(group(args))
    return out


EXPLORATIONS = ("epsilon_greedy", "boltzmann")
# the schedules' defaults: the vectorised loop anneals per lock-step (as its epsilon), the single-env loop per episode
TEMP_DEFAULTS = dict(temp_start=1.0, temp_end=0.1, temp_decay=0.999)


def add_exploration_arguments(p):
    """--exploration / --temp_start / --temp_end / --temp_decay: shared with the tools that train through the vectorised loop."""
    p.add_argument("--exploration", choices=EXPLORATIONS, default=argparse.SUPPRESS,
                   help="How the agent explores, in both loops (default epsilon_greedy: the count-based rule of the reference). "
                        "boltzmann: every env draws its candidate with probability proportional to exp(q / temperature), on the "
                        "device in the vectorised loop (bridges_boltzmann_select), with the Softmax policy in the single-env loop; "
                        "the temperature falls as t <- (t - temp_end) * temp_decay + temp_end per lock-step (per episode in the "
                        "single-env loop). Evaluation stays greedy.")
    p.add_argument("--temp_start", type=float, default=argparse.SUPPRESS, help="With --exploration boltzmann: first temperature (1.0).")
    p.add_argument("--temp_end", type=float, default=argparse.SUPPRESS, help="With --exploration boltzmann: last temperature (0.1).")
    p.add_argument("--temp_decay", type=float, default=argparse.SUPPRESS,
                   help="With --exploration boltzmann: decay of the temperature per lock-step / episode (0.999).")


def check_exploration(args):
    """--exploration / --temp_*: refused in words (SystemExit) before anything touches the GPU."""
    given = [f"--{k}" for k in TEMP_DEFAULTS if k in args]
    boltzmann = args.get('exploration', EXPLORATIONS[0]) == "boltzmann"
    if given and not boltzmann:
        raise SystemExit(f"{' / '.join(given)} shape the temperature of Boltzmann exploration: they need --exploration boltzmann")
    if boltzmann:
        t = {k: args.get(k, v) for k, v in TEMP_DEFAULTS.items()}
        try:
            check_temperature_schedule(t['temp_start'], t['temp_end'], t['temp_decay'], who="--temp_start / --temp_end / --temp_decay")
        except ValueError as e:
            raise SystemExit(str(e)) from e
        if args.get('eval_epsilon', 0.0) > 0:
            raise SystemExit("--eval_epsilon > 0 explores with the epsilon-greedy rule: not with --exploration boltzmann, whose "
                             "evaluation is greedy")


def exploration_from_args(args):
    """The exploration arguments of VecDQN from parsed options (the temp_* keys only with --exploration boltzmann); refuses what
    check_exploration refuses."""
    check_exploration(args)
    if args.get('exploration', EXPLORATIONS[0]) != "boltzmann":
        return {}
    return dict(exploration="boltzmann", **{k: args.get(k, v) for k, v in TEMP_DEFAULTS.items()})


def add_priority_arguments(p, prioritized_flag=False):
    """--priority_alpha / --priority_refresh: shared with the tools that train through the vectorised loop
    (``prioritized_flag``: and --prioritized_replay itself, for a parser that has none)."""
    if prioritized_flag:
        p.add_argument("--prioritized_replay", action="store_true",
                       help="replay in proportion to td_error + 1e-5 (VecDQN(prioritized=True))")
    p.add_argument("--priority_alpha", type=float, default=argparse.SUPPRESS, metavar="A",
                   help="Vectorised loop with --prioritized_replay: replay a transition with probability proportional to "
                        "(td_error + 1e-5)^A, 0 <= A <= 1 (default 1: the reference's rule; 0: uniform), drawn by the sampler "
                        "kernel on the device.")
    p.add_argument("--priority_refresh", action="store_true", default=argparse.SUPPRESS,
                   help="Vectorised loop with --prioritized_replay, one rank: after every lock-step's target pass write "
                        "|q(s,a) - q_target| of the sampled transitions back as their priorities (rows keep the rollout's TD error "
                        "until they are first sampled). One more policy-net forward over the sampled rows per lock-step.")
    p.add_argument("--priority_beta", type=float, default=argparse.SUPPRESS, metavar="B",
                   help="Vectorised loop with --prioritized_replay: importance-sampling weights (N P(i))^(-B), 0 <= B <= 1, each batch "
                        "divided by its own maximum, computed on the device and multiplied into the loss of every sampled "
                        "transition (default: no weights).")
    p.add_argument("--priority_beta_anneal", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="With --priority_beta: raise the exponent linearly from B to 1 over the first N lock-steps that train "
                        "(default 0: constant).")


def check_priority(args):
    """--priority_alpha / --priority_refresh / --priority_beta / --priority_beta_anneal: refused in words (SystemExit) where the
    loop cannot run them, before anything touches the GPU."""
    given = [f"--{k}" for k in ('priority_alpha', 'priority_refresh', 'priority_beta', 'priority_beta_anneal') if k in args]
    if not given:
        return
    if args['num_envs'] <= 1:
        raise SystemExit(f"{' / '.join(given)} need the vectorised loop (--num_envs N, N > 1): the single-env loop samples through "
                         "the reference's PrioritizedReplayBuffer")
    if not args.get('prioritized_replay'):
        raise SystemExit(f"{' / '.join(given)} shape the prioritised draw: they need --prioritized_replay")
    a = args.get('priority_alpha', 1.0)
    if not 0.0 <= a <= 1.0:
        raise SystemExit(f"--priority_alpha must lie in [0, 1] (0: uniform, 1: proportional to td_error + 1e-5), not {a}")
    if 'priority_beta' in args and not 0.0 <= args['priority_beta'] <= 1.0:
        raise SystemExit(f"--priority_beta must lie in [0, 1] (0: all weights 1, 1: the full correction), not {args['priority_beta']}")
    if 'priority_beta_anneal' in args and ('priority_beta' not in args or args['priority_beta_anneal'] < 0):
        raise SystemExit("--priority_beta_anneal N (N >= 0) anneals --priority_beta: give --priority_beta as well")


def priority_from_args(args):
    """The prioritised-replay arguments of VecDQN from parsed options (a tool's: every lock-step there is vectorised);
    --priority_alpha / --priority_refresh / --priority_beta without --prioritized_replay is refused as check_priority refuses
    it.  The keys of the weights are there only when --priority_beta was given."""
    check_priority(dict(args, num_envs=2))
    out = dict(prioritized=bool(args.get('prioritized_replay', False)), priority_alpha=args.get('priority_alpha', 1.0),
               priority_refresh=bool(args.get('priority_refresh', False)))
    if 'priority_beta' in args:
        out.update(priority_beta=args['priority_beta'], priority_beta_anneal=args.get('priority_beta_anneal', 0))
    return out


def add_n_step_argument(p):
    """--n_step: shared with the tools that train through the vectorised loop."""
    p.add_argument("--n_step", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="Vectorised loop: train on N-step returns, 1 <= N <= 8 and N <= --max_steps (default 1: the one-step target). "
                        "Every env folds its last N transitions on the device; the replay ring then holds h-step records (h = N, "
                        "shorter at the end of an episode) and the mean_lin_reward / lin_reward of the log is the mean h-step "
                        "return G = sum_k gamma^k lin_reward_k of the rows pushed in the lock-step, not the mean one-step reward.")


def check_n_step(args):
    """--n_step N: refused in words (SystemExit) where the loop cannot run it, before anything touches the GPU."""
    n = args.get('n_step')
    if n is None:
        return
    from bridges_hip import abi
    if not 1 <= n <= abi.NSTEP_MAX:
        raise SystemExit(f"--n_step must be 1..{abi.NSTEP_MAX} (the window of an env holds at most {abi.NSTEP_MAX} transitions)")
    if n > 1 and args['num_envs'] <= 1:
        raise SystemExit("--n_step N > 1 needs the vectorised loop (--num_envs N, N > 1): the single-env loop trains on the "
                         "reference's one-step target")
    if n > args['max_steps']:
        raise SystemExit(f"--n_step {n} is above --max_steps {args['max_steps']}: no episode has that many transitions")


def add_double_q_argument(p):
    """--double_q: shared with the tools that train through the vectorised loop."""
    p.add_argument("--double_q", action="store_true", default=argparse.SUPPRESS,
                   help="Vectorised loop: double Q-learning targets -- the policy net chooses the next action, the target net "
                        "values it: q = G + gamma^h q_target(s', argmax_a' q_policy(s', a')), and the successor-feature target "
                        "takes the target net's features of that action. One more forward over the next-state rows per "
                        "lock-step. Composes with --n_step and --prioritized_replay.")


def check_double_q(args):
    """--double_q: refused in words (SystemExit) where the loop cannot run it, before anything touches the GPU."""
    if args.get('double_q') and args['num_envs'] <= 1:
        raise SystemExit("--double_q needs the vectorised loop (--num_envs N, N > 1): the single-env loop trains on the "
                         "reference's target, where the target net both chooses and values the next action")


def add_target_temperature_argument(p):
    """--target_temperature: shared with the tools that train through the vectorised loop."""
    p.add_argument("--target_temperature", type=float, default=argparse.SUPPRESS, metavar="T",
                   help="Vectorised loop: expected-value targets under the Boltzmann policy at temperature T (finite, > 0) -- the "
                        "bootstrap is sum_a' pi(a'|s') q'(s', a') with pi ~ exp(q' / T) instead of max_a' q'(s', a'), and the "
                        "successor-feature target takes the same expectation of the features (with --double_q the policy net's "
                        "q weighs the actions). T is constant; it is not the exploration temperature. Logs target_entropy and "
                        "soft_value_gap. Composes with --n_step, --double_q and --prioritized_replay.")


def check_target_temperature(args):
    """--target_temperature T: refused in words (SystemExit) where the loop cannot run it, before anything touches the GPU."""
    T = args.get('target_temperature')
    if T is None:
        return
    if not (0.0 < T < float("inf")):                         # (a NaN fails the comparison)
        raise SystemExit(f"--target_temperature must be a finite number > 0, got {T}")
    if args['num_envs'] <= 1:
        raise SystemExit("--target_temperature needs the vectorised loop (--num_envs N, N > 1): the single-env loop trains on the "
                         "reference's target, the maximum over the next actions")


def target_temperature_from_args(args):
    """--target_temperature T -> VecDQN's keyword, nothing without the flag."""
    return dict(target_temperature=args['target_temperature']) if args.get('target_temperature') is not None else {}


def add_relative_temperature_arguments(p):
    """--temp_relative / --target_temp_relative / --spread_floor: shared with the tools that train through the vectorised loop."""
    p.add_argument("--temp_relative", action="store_true", default=argparse.SUPPRESS,
                   help="Vectorised loop with --exploration boltzmann: the temperature is a multiple of each state's own spread of q -- "
                        "an env draws at temperature * max(s, F), s the standard deviation of q among its candidates, formed on the "
                        "device in the draw's own launch (bridges_boltzmann_select_rel). Logs temperature_effective.")
    p.add_argument("--target_temp_relative", action="store_true", default=argparse.SUPPRESS,
                   help="Vectorised loop with --target_temperature T: every transition is backed up at T * max(s, F), s the standard "
                        "deviation of q' among its next state's candidates (bridges_soft_expect_rel; with --double_q the policy "
                        "net's values). Logs target_temperature_effective.")
    p.add_argument("--spread_floor", type=float, default=argparse.SUPPRESS, metavar="F",
                   help="With --temp_relative / --target_temp_relative: the least spread a temperature multiplies (finite, > 0; 1e-3), "
                        "which keeps the temperature positive where a state's candidates tie.")


def relative_temperature_from_args(args):
    """--temp_relative / --target_temp_relative / --spread_floor F -> VecDQN's keywords, nothing without the flags; refused in
    words (SystemExit) without the option whose temperature they make relative."""
    rel, trel = bool(args.get('temp_relative')), bool(args.get('target_temp_relative'))
    if rel and args.get('exploration', EXPLORATIONS[0]) != "boltzmann":
        raise SystemExit("--temp_relative makes the temperature of Boltzmann exploration relative to each state's spread of q: it "
                         "needs --exploration boltzmann")
    if trel and args.get('target_temperature') is None:
        raise SystemExit("--target_temp_relative makes the temperature of the soft targets relative to each state's spread of q: it "
                         "needs --target_temperature T")
    out = {}
    if 'spread_floor' in args:
        if not (rel or trel):
            raise SystemExit("--spread_floor is the floor of the spread a relative temperature multiplies: it needs --temp_relative "
                             "or --target_temp_relative")
        if not (0.0 < args['spread_floor'] < float("inf")):  # (a NaN fails the comparison)
            raise SystemExit(f"--spread_floor must be a finite number > 0, got {args['spread_floor']}")
        out['spread_floor'] = args['spread_floor']
    if rel:
        out['temp_relative'] = True
    if trel:
        out['target_temp_relative'] = True
    return out


def check_relative_temperature(args):
    """The three flags: refused in words (SystemExit) where the loop cannot run them, before anything touches the GPU."""
    given = [f"--{k}" for k in ('temp_relative', 'target_temp_relative', 'spread_floor') if k in args]
    if given and args['num_envs'] <= 1:
        raise SystemExit(f"{' / '.join(given)} need the vectorised loop (--num_envs N, N > 1): the single-env loop draws and backs "
                         "up at one temperature for every state")
    relative_temperature_from_args(args)


def add_munchausen_arguments(p):
    """--munchausen_alpha / --munchausen_clip: shared with the tools that train through the vectorised loop."""
    p.add_argument("--munchausen_alpha", type=float, default=argparse.SUPPRESS, metavar="A",
                   help="Vectorised loop with --target_temperature T: Munchausen targets -- q = r + A * max(T ln pi(a|s), L0) + gamma * "
                        "V_T(s'), pi = softmax(q' / T) of the target net and V_T the log-sum-exp value (bridges_soft_value; the taken "
                        "action is found among the rebuilt candidates of s by bridges_action_row). A in [0, 1]. Logs "
                        "munchausen_bonus, munchausen_clipped and munchausen_missed. Not with --double_q or --n_step N > 1.")
    p.add_argument("--munchausen_clip", type=float, default=argparse.SUPPRESS, metavar="L0",
                   help="With --munchausen_alpha: the lower clip of T ln pi(a|s) (finite, <= 0; -1.0).")


def munchausen_from_args(args):
    """--munchausen_alpha A [--munchausen_clip L0] -> VecDQN's keywords, nothing without the flags; refused in words (SystemExit)
    where the loop cannot run them."""
    given = [f"--{k}" for k in ('munchausen_alpha', 'munchausen_clip') if k in args]
    if not given:
        return {}
    who = ' / '.join(given)
    if 'munchausen_alpha' not in args:
        raise SystemExit("--munchausen_clip clips the Munchausen bonus: it needs --munchausen_alpha A")
    A, L0 = args['munchausen_alpha'], args.get('munchausen_clip', -1.0)
    if not (0.0 <= A <= 1.0):                                # (a NaN fails both comparisons)
        raise SystemExit(f"--munchausen_alpha must lie in [0, 1], got {A}")
    if not (float("-inf") < L0 <= 0.0):
        raise SystemExit(f"--munchausen_clip must be a finite number <= 0, got {L0}")
    if args.get('target_temperature') is None:
        raise SystemExit(f"{who}: the bonus and the bootstrap are formed under the Boltzmann policy of the target net: it needs "
                         "--target_temperature T")
    if args.get('double_q'):
        raise SystemExit(f"{who} does not run with --double_q: the bonus and the bootstrap are one estimator's, the target net's")
    if args.get('n_step', 1) > 1:
        raise SystemExit(f"{who} needs --n_step 1: an h-step row does not hold the descriptors of its intermediate actions, and "
                         "their bonuses would take h forwards")
    return dict(munchausen_alpha=A, munchausen_clip=L0)


def check_munchausen(args):
    """The two flags: refused in words (SystemExit) where the loop cannot run them, before anything touches the GPU."""
    given = [f"--{k}" for k in ('munchausen_alpha', 'munchausen_clip') if k in args]
    if given and args['num_envs'] <= 1:
        raise SystemExit(f"{' / '.join(given)} need the vectorised loop (--num_envs N, N > 1): the single-env loop trains on the "
                         "reference's target, the maximum over the next actions")
    munchausen_from_args(args)


def add_eval_beam_argument(p):
    """--eval_beam: shared with the tools that evaluate through the vectorised loop."""
    p.add_argument("--eval_beam", type=int, default=argparse.SUPPRESS, metavar="B",
                   help="Vectorised loop with --eval_envs M: every evaluation also runs a beam search of width B (1..16) on the same "
                        "M tasks, with the policy net's q as the heuristic (VecDQN.beam_search: B envs per task, forked on the "
                        "device), and logs beam_success_rate / beam_reward / beam_lin_reward / beam_width beside the greedy keys.")
    p.add_argument("--eval_beam_merge", action="store_true", default=argparse.SUPPRESS,
                   help="With --eval_beam B: after every depth the search closes the beams that hold the same structure as another "
                        "beam of their task -- the same blocks placed in another order, the same last block -- and keeps the one with "
                        "the best return (bridges_beam_merge), so the width is not spent on permutations; logs eval_merged_beams, "
                        "the beams closed that way.")


def check_eval_beam(args, flag="--eval_beam", operator="the widest beam bridges_beam_select orders"):
    """--eval_beam B / --eval_beam_merge: refused in words (SystemExit) where the loop cannot run it, before anything touches the
    GPU."""
    B = args.get('eval_beam')
    if B is None:
        if args.get('eval_beam_merge'):
            raise SystemExit("--eval_beam_merge merges the beams of the search --eval_beam B runs: it needs --eval_beam B")
        return
    from bridges_hip import abi
    if not 1 <= B <= abi.BEAM_MAX_WIDTH:
        raise SystemExit(f"{flag} must be 1..{abi.BEAM_MAX_WIDTH} ({operator})")
    if args.get('num_envs', 1) <= 1:
        raise SystemExit(f"{flag} needs the vectorised loop (--num_envs N, N > 1): the search forks lock-step envs on the device")
    if args.get('eval_envs', EVAL_DEFAULTS['eval_envs']) <= 0:
        raise SystemExit(f"{flag} searches the tasks of the evaluation env: it needs --eval_envs M, M > 0")


def add_eval_particle_arguments(p):
    """--eval_particles and its companions: shared with the tools that evaluate through the vectorised loop."""
    p.add_argument("--eval_particles", type=int, default=argparse.SUPPRESS, metavar="B",
                   help="Vectorised loop with --eval_envs M: every evaluation also runs a particle search of B particles (1..16) on "
                        "the same M tasks (VecDQN.particle_search: rollouts sampled from the Boltzmann policy at "
                        "--eval_particle_temperature, resampled every depth by their value), and logs particle_success_rate / "
                        "particle_reward / particle_lin_reward / particles / particle_ess / particle_p_sel beside the greedy keys.")
    p.add_argument("--eval_particle_temperature", type=float, default=argparse.SUPPRESS, metavar="T",
                   help="With --eval_particles B: temperature of the action draws, finite and > 0 (required).")
    p.add_argument("--eval_particle_resample_temperature", type=float, default=argparse.SUPPRESS, metavar="TR",
                   help="With --eval_particles B: temperature of the resampling weights, > 0 (the action temperature); inf: no "
                        "resampling -- with --eval_particle_no_elite plain best-of-B rollouts.")
    p.add_argument("--eval_particle_no_elite", action="store_true", default=argparse.SUPPRESS,
                   help="With --eval_particles B: no particle is reserved for the best parent's best candidate.")
    p.add_argument("--eval_particle_merge", action="store_true", default=argparse.SUPPRESS,
                   help="With --eval_particles B: merge particles that hold the same structure (as --eval_beam_merge).")


def check_eval_particles(args):
    """--eval_particles B and its companions: refused in words (SystemExit) where the loop cannot run them, before anything touches
    the GPU."""
    import math
    B = args.get('eval_particles')
    if B is None:
        for k in ('eval_particle_temperature', 'eval_particle_resample_temperature', 'eval_particle_no_elite', 'eval_particle_merge'):
            if k in args:
                raise SystemExit(f"--{k} shapes the search --eval_particles B runs: it needs --eval_particles B")
        return
    if 'eval_beam' in args:
        raise SystemExit("--eval_particles and --eval_beam are two searches of the same tasks: an evaluation runs one of them")
    if 'eval_particle_temperature' not in args:
        raise SystemExit("--eval_particles needs --eval_particle_temperature T: the temperature its actions are drawn at")
    T = args['eval_particle_temperature']
    if not (math.isfinite(T) and T > 0.0):
        raise SystemExit("--eval_particle_temperature must be finite and > 0")
    if not args.get('eval_particle_resample_temperature', T) > 0.0:          # (a NaN fails the comparison)
        raise SystemExit("--eval_particle_resample_temperature must be > 0 (inf: no resampling)")
    check_eval_beam(dict(args, eval_beam=B, eval_beam_merge=False), flag="--eval_particles",
                    operator="the most particles bridges_particle_select resamples")


def eval_particles_from_args(args):
    """The arguments of VecDQN.particle_search from parsed options (None without --eval_particles); refuses what
    check_eval_particles refuses."""
    check_eval_particles(args)
    if 'eval_particles' not in args:
        return None
    return dict(width=args['eval_particles'], temperature=args['eval_particle_temperature'],
                resample_temperature=args.get('eval_particle_resample_temperature'), elite=not args.get('eval_particle_no_elite'),
                merge=bool(args.get('eval_particle_merge')))


def add_hindsight_arguments(p):
    """--hindsight / --hindsight_goals / --hindsight_fold: shared with the tools that train through the vectorised loop."""
    p.add_argument("--hindsight", choices=("final", "per_step"), default=argparse.SUPPRESS,
                   help="With --random_targets T only: hindsight goal relabelling -- every episode that ends is stored a second "
                        "time under T targets its own final structure reached (the centres of the bounding boxes of blocks drawn "
                        "from it), with the rewards the env would have given under them. per_step (hindsight experience replay's 'future' "
                        "strategy): every transition gets goals of its own instead -- a block the episode places at that step or "
                        "later, and others from the structure as it then stands. The log gains hindsight_rows.")
    p.add_argument("--hindsight_goals", type=int, default=argparse.SUPPRESS, metavar="G",
                   help="With --hindsight final: relabelled copies of every finished episode, 1..4 (1); with --hindsight per_step: "
                        "relabelled rows per transition.")
    p.add_argument("--hindsight_fold", action="store_true", default=argparse.SUPPRESS,
                   help="With --hindsight final or per_step: run it beside --n_step n > 1 -- the relabelled episode is folded on the device into "
                        "h-step rows, the return taken over the relabelled linear rewards; an episode whose last relabelled step is "
                        "not terminal still stores its last n - 1 starts, which bootstrap from the final state.")


def check_hindsight(args):
    """--hindsight / --hindsight_goals: refused in words (SystemExit) where the loop cannot run them, before anything touches the GPU."""
    if 'hindsight' not in args:
        if 'hindsight_goals' in args:
            raise SystemExit("--hindsight_goals counts the relabelled copies of an episode: it needs --hindsight final or per_step")
        if args.get('hindsight_fold'):
            raise SystemExit("--hindsight_fold folds the relabelled rows into n-step returns: it needs --hindsight final or per_step")
        return
    if not 1 <= args.get('hindsight_goals', 1) <= 4:
        raise SystemExit("--hindsight_goals must be 1..4")
    opt = f"--hindsight {args['hindsight']}"
    if not args.get('random_targets'):
        raise SystemExit(f"{opt} needs --random_targets T (and with it --num_envs N, N > 1): only a record that ends "
                         "in its own targets can be given others")
    if args.get('random_bridge_length') is not None or args.get('random_tower_height') is not None or args.get('curriculum'):
        raise SystemExit(f"{opt} does not run on a task family (--random_bridge_length / --random_tower_height) or "
                         "with --curriculum: a family's task is its class, and a box centre names none")
    if args.get('n_step', 1) > 1 and not args.get('hindsight_fold'):
        raise SystemExit(f"{opt} needs --n_step 1 or --hindsight_fold: an h-step row's return has to be folded again under "
                         "the new targets")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{opt} runs on one rank only: the relabelled rows are not part of the all-gather")


def hindsight_from_args(args):
    """The hindsight arguments of VecDQN from parsed options; refuses what check_hindsight refuses."""
    check_hindsight(args)
    if 'hindsight' not in args:
        return {}
    return dict(hindsight=args['hindsight'], hindsight_goals=args.get('hindsight_goals', 1),
                **(dict(hindsight_fold=True) if args.get('hindsight_fold') else {}))


def add_search_arguments(p):
    """--search_every / --search_tasks / --search_width / --search_merge: shared with the tools that train through the vectorised
    loop."""
    p.add_argument("--search_every", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="With --num_envs N > 1: search in training -- every N-th lock-step a beam search with the policy net's q as "
                        "the heuristic runs on the tasks the first --search_tasks rollout envs are playing, and the transitions of "
                        "every task's best finished beam are pushed into the replay buffer behind the lock-step's own (as h-step "
                        "rows with --n_step). The log gains search_rows, search_success_rate and search_lin_reward.")
    p.add_argument("--search_tasks", type=int, default=argparse.SUPPRESS, metavar="M",
                   help="With --search_every: tasks searched, those of rollout envs 0..M-1 (min(num_envs, 64); a fixed task: 1).")
    p.add_argument("--search_width", type=int, default=argparse.SUPPRESS, metavar="B",
                   help="With --search_every: width of the beam, 1..16 (8).")
    p.add_argument("--search_merge", action="store_true", default=argparse.SUPPRESS,
                   help="With --search_every: the search merges beams that hold the same structure (as --eval_beam_merge).")
    p.add_argument("--search_particles", action="store_true", default=argparse.SUPPRESS,
                   help="With --search_every: the search is a particle search (VecDQN.particle_search: --search_width rollouts per "
                        "task sampled from the Boltzmann policy and resampled every depth by their value) instead of the beam search.")
    p.add_argument("--search_temperature", type=float, default=argparse.SUPPRESS, metavar="T",
                   help="With --search_particles: temperature of the action draws, finite and > 0 (required).")
    p.add_argument("--search_resample_temperature", type=float, default=argparse.SUPPRESS, metavar="TR",
                   help="With --search_particles: temperature of the resampling weights, > 0 or inf (the action temperature).")


def check_search(args):
    """--search_every and its companions: refused in words (SystemExit) where the loop cannot run them, before anything touches
    the GPU."""
    if 'search_every' not in args:
        for k in ('search_tasks', 'search_width', 'search_merge', 'search_particles', 'search_temperature', 'search_resample_temperature'):
            if k in args:
                raise SystemExit(f"--{k} shapes the search in training: it needs --search_every N")
        return
    from bridges_hip import abi
    if args['search_every'] < 1:
        raise SystemExit("--search_every must be >= 1 (lock-steps between two searches)")
    if args.get('num_envs', 1) <= 1:
        raise SystemExit("--search_every needs the vectorised loop (--num_envs N, N > 1): the search forks lock-step envs on the device")
    if not 1 <= args.get('search_width', 8) <= abi.BEAM_MAX_WIDTH:
        raise SystemExit(f"--search_width must be 1..{abi.BEAM_MAX_WIDTH} (the widest beam bridges_beam_select orders)")
    if 'search_tasks' in args and not 1 <= args['search_tasks'] <= args['num_envs']:
        raise SystemExit(f"--search_tasks must be 1..--num_envs ({args['num_envs']}): the tasks are those of the first rollout envs")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--search_every runs on one rank only: the rows a search finds are not part of the all-gather")
    if 'search_particles' not in args:
        for k in ('search_temperature', 'search_resample_temperature'):
            if k in args:
                raise SystemExit(f"--{k} is a temperature of the particle search: it needs --search_particles")
        return
    import math
    if 'search_temperature' not in args:
        raise SystemExit("--search_particles needs --search_temperature T: the temperature its actions are drawn at")
    if not (math.isfinite(args['search_temperature']) and args['search_temperature'] > 0.0):
        raise SystemExit("--search_temperature must be finite and > 0")
    if not args.get('search_resample_temperature', 1.0) > 0.0:               # (a NaN fails the comparison)
        raise SystemExit("--search_resample_temperature must be > 0 (inf: no resampling)")


def search_from_args(args):
    """The search arguments of VecDQN from parsed options; refuses what check_search refuses."""
    check_search(args)
    if 'search_every' not in args:
        return {}
    out = dict(search_every=args['search_every'], search_width=args.get('search_width', 8), search_merge=bool(args.get('search_merge')))
    if 'search_tasks' in args:
        out['search_tasks'] = args['search_tasks']
    if 'search_particles' in args:
        out.update(search_sampler="particles", search_temperature=args['search_temperature'])
        if 'search_resample_temperature' in args:
            out['search_resample_temperature'] = args['search_resample_temperature']
    return out


def add_curriculum_arguments(p):
    """--family_weights and --curriculum*: how a task family (--random_bridge_length / --random_tower_height) draws its classes;
    shared with the tools that take the family options."""
    p.add_argument("--family_weights", type=parse_family_weights, default=argparse.SUPPRESS, metavar="W,W,...",
                   help="With --random_bridge_length / --random_tower_height LO:HI: HI - LO + 1 non-negative integer weights "
                        "(each <= 2^20, not all zero); n = LO + k is drawn with probability W[k] / sum(W) instead of uniformly. "
                        "The evaluation envs stay uniform.")
    p.add_argument("--curriculum", action="store_true", default=argparse.SUPPRESS,
                   help="With --random_bridge_length / --random_tower_height: adapt the weights on the device -- every "
                        "--curriculum_every lock-steps the weight of n becomes floor + the failure rate of the training episodes "
                        "played on n (an exponential moving average), so episodes move to the spans / heights the policy fails on.")
    p.add_argument("--curriculum_every", type=int, default=argparse.SUPPRESS, help="Lock-steps between curriculum updates (10).")
    p.add_argument("--curriculum_beta", type=float, default=argparse.SUPPRESS,
                   help="Weight of the newest success rate in the moving average, 0..1 (0.25).")
    p.add_argument("--curriculum_floor", type=float, default=argparse.SUPPRESS,
                   help="Share of the weight scale every n keeps whatever its success, 0..1 (0.1): no n is starved.")


def parse_family_weights(text):
    """'W,W,...' -> (W, W, ...), integers."""
    try:
        return tuple(int(w) for w in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected W,W,... (integers), got {text!r}")


def parse_size_range(text):
    """'LO:HI' -> (LO, HI), two integers."""
    try:
        lo, hi = text.split(":")
        return int(lo), int(hi)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected LO:HI (two integers), got {text!r}")


EVAL_DEFAULTS = dict(eval_envs=0, eval_epsilon=0.0)


def check_random_targets(args):
    """--random_targets T is the vectorised SuccessorMLP loop on per-env random tasks, --random_obstacles O adds O random
    obstacles per env to it, --task_channels runs ConvNet / UNet on them instead; every other combination is refused in words (SystemExit), before anything touches the GPU."""
    T, O = args.get('random_targets'), args.get('random_obstacles')
    conv = bool(args.get('task_channels', False))
    if args.get('random_bridge_length') is not None or args.get('random_tower_height') is not None:
        return check_random_bridges(args)
    check_curriculum(args, None)
    if conv and T is None:
        raise SystemExit("--task_channels is valid only together with --random_targets T: it feeds the conv Q-networks the task "
                         "of every env, and without --random_targets all envs share one task")
    if O is not None and T is None:
        raise SystemExit("--random_obstacles O is valid only together with --random_targets T: per-env obstacles ride on the "
                         "per-env task buffers and records of the loop on per-env tasks")
    if T is None:
        return
    from bridges_hip import abi
    if O is not None and not 1 <= O <= abi.MAX_OBSTACLES:
        raise SystemExit(f"--random_obstacles must be 1..{abi.MAX_OBSTACLES} obstacles per env")
    if not 1 <= T <= abi.MAX_TARGETS:
        raise SystemExit(f"--random_targets must be 1..{abi.MAX_TARGETS} targets per env")
    if args.get('tower_height') or args['bridge_length'] != 1:
        raise SystemExit("--random_targets draws every env's task (tower_setup: random targets, no obstacles): it cannot be "
                         "combined with --tower_height or --bridge_length, which name one fixed task")
    if args['num_envs'] <= 1:
        raise SystemExit(f"--random_targets{' / --task_channels' if conv else ''} needs the vectorised loop (--num_envs N, N > 1): "
                         "the single-env loop trains on the fixed tasks of --tower_height / --bridge_length only")
    if conv and args['model'] == 'SuccessorMLP':
        raise SystemExit("--task_channels is for the conv Q-networks (--model ConvNet or UNet): --model SuccessorMLP trains on "
                         "--random_targets without it")
    if not conv and args['model'] != 'SuccessorMLP':
        raise SystemExit(f"--random_targets{' / --random_obstacles' if O is not None else ''} trains --model SuccessorMLP only: "
                         f"{args['model']} takes the reward map as an image "
                         "channel and its rows are shared by state alone (add --task_channels to train ConvNet or UNet on per-env "
                         "tasks)")
    if tuple(args['image_size']) != (64, 64):
        raise SystemExit("--random_targets needs --image_size 64x64 (the stacked conv input of --task_channels is built for 64x64)"
                         if conv else "--random_targets needs --image_size 64x64 (the factored acting path of SuccessorMLP; "
                                      "--task_channels is built for 64x64 as well)")
    if args['shapes'] != 'trapezoid':
        raise SystemExit("--random_targets is tower_setup: --shapes trapezoid")


def check_random_bridges(args):
    """--random_bridge_length LO:HI / --random_tower_height LO:HI: the vectorised loop on a task family (one integer n per env
    and episode names the bridge span / tower height); what it cannot run is refused in words (SystemExit), before anything
    touches the GPU."""
    span, tower = args.get('random_bridge_length'), args.get('random_tower_height')
    if span is not None and tower is not None:
        raise SystemExit("--random_bridge_length and --random_tower_height name two task families: give one of them")
    flag = "--random_bridge_length" if span is not None else "--random_tower_height"
    lo, hi = span if span is not None else tower
    if args.get('random_targets') is not None or args.get('random_obstacles') is not None:
        raise SystemExit(f"{flag} draws the target and the obstacles of every env from one integer: it cannot be combined with "
                         "--random_targets / --random_obstacles, which draw them independently")
    if args.get('tower_height') or args['bridge_length'] != 1:
        raise SystemExit(f"{flag} draws every env's task: it cannot be combined with --tower_height or --bridge_length, which name "
                         "one fixed task")
    if args['num_envs'] <= 1:
        raise SystemExit(f"{flag} needs the vectorised loop (--num_envs N, N > 1): the single-env loop trains on the fixed tasks "
                         "of --tower_height / --bridge_length only")
    if tuple(args['image_size']) != (64, 64):
        raise SystemExit(f"{flag} needs --image_size 64x64 (the acting paths on per-env tasks are built for 64x64)")
    from bridges_hip import abi
    if hi > abi.MAX_OBSTACLES or lo < 0 or lo > hi or hi < 1:
        raise SystemExit(f"{flag} LO:HI must satisfy 0 <= LO <= HI and 1 <= HI <= {abi.MAX_OBSTACLES} (an env holds at most "
                         f"{abi.MAX_OBSTACLES} obstacles), got {lo}:{hi}")
    conv = bool(args.get('task_channels', False))
    if conv and args['model'] == 'SuccessorMLP':
        raise SystemExit(f"--task_channels is for the conv Q-networks (--model ConvNet or UNet): --model SuccessorMLP trains on "
                         f"{flag} without it")
    if not conv and args['model'] != 'SuccessorMLP':
        raise SystemExit(f"{flag} with --model {args['model']} needs --task_channels: the conv Q-networks take the task of every "
                         "env as image channels")
    check_curriculum(args, (lo, hi))


CURRICULUM_OPTIONS = ("curriculum_every", "curriculum_beta", "curriculum_floor")


def check_curriculum(args, sizes):
    """--family_weights / --curriculum*: ``sizes`` is the (LO, HI) of an accepted --random_bridge_length / --random_tower_height
    (which has checked --num_envs > 1 already), None without one; refusals in words (SystemExit) as everywhere here."""
    weights, on = args.get('family_weights'), bool(args.get('curriculum'))
    given = [f"--{k}" for k in CURRICULUM_OPTIONS if args.get(k) is not None]
    if sizes is None:
        asked = (["--family_weights"] if weights is not None else []) + (["--curriculum"] if on else []) + given
        if asked:
            raise SystemExit(f"{asked[0]} weighs the classes of a task family: it needs --random_bridge_length LO:HI or "
                             "--random_tower_height LO:HI (and the vectorised loop, --num_envs N, N > 1)")
        return
    if given and not on:
        raise SystemExit(f"{given[0]} is a setting of --curriculum: give --curriculum as well")
    if on and weights is not None:
        raise SystemExit("--curriculum adapts the weights itself: it cannot be combined with the fixed --family_weights")
    if weights is not None:
        from bridges_hip.vec_env import check_family_weights
        try:
            check_family_weights(weights, sizes[1] - sizes[0] + 1)
        except ValueError as e:
            raise SystemExit(f"--family_weights: {e}")
    if on:
        from robotoddler.training.vec_dqn import curriculum_from_args
        try:
            curriculum_from_args(args)
        except ValueError as e:
            raise SystemExit(f"--{e}".replace("--curriculum: ", "--curriculum_"))


def make_setup_fct(args):
    trap, hexa = args['shapes'] in ('trapezoid', 'both'), args['shapes'] in ('hexagon', 'both')
    if args.get('tower_height'):
        return lambda: bridge_setup(num_stories=args['tower_height'], trapezoid=trap, hexagon=hexa)
    return lambda: horizontal_bridge_setup(num_obstacles=args['bridge_length'], trapezoid=trap, hexagon=hexa)


def make_nets(args, device):
    if args['model'] == 'SuccessorMLP':
        mk = lambda: SuccessorMLP(img_size=args['image_size'], hidden_dims=[256, 128, 64, 128, 256])
    elif args['model'] == 'ConvNet':
        mk = lambda: ConvNet(img_size=args['image_size'])
    elif args['model'] == 'UNet':
        mk = Policy
    else:
        raise ValueError(f"Unknown model type {args['model']}.")
    policy_net, target_net = mk().to(device), mk().to(device)
    policy_net.apply(init_weights)
    target_net.load_state_dict(policy_net.state_dict())
    flatten_nets(policy_net, target_net)
    return policy_net, target_net


def main(argv=None):
    args = vars(build_parser().parse_args(argv))
    if args['device'] == 'cpu':
        raise SystemExit("this build has no CPU path: the simulator and the DQN ops are HIP kernels (use --device cuda)")
    check_random_targets(args)
    check_n_step(args)
    check_double_q(args)
    check_target_temperature(args)
    check_relative_temperature(args)
    check_munchausen(args)
    check_priority(args)
    check_exploration(args)
    check_hindsight(args)
    check_search(args)
    check_eval_beam(args)
    check_eval_particles(args)
    from bridges_hip import abi
    abi.require_gpu()
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    if args['seed'] is not None:
        random.seed(args['seed'])
        np.random.seed(args['seed'])
        torch.manual_seed(args['seed'])
    aim_run = wandb_run = None
    if args['aim']:                                                         # successor_dqn.py:671-674
        try:
            import aim
        except ImportError as e:
            raise SystemExit("--aim was given but the 'aim' package is not installed") from e
        aim_run = aim.Run(experiment="SuccessorQLearning", repo=args['aim_repo'])
    if args['wandb']:
        try:
            import wandb
        except ImportError as e:
            raise SystemExit("--wandb was given but the 'wandb' package is not installed") from e
        wandb_run = wandb.init(project="dual_arm", config=args)
    if args['num_envs'] > 1:
        from robotoddler.training.vec_dqn import run_vectorised
        return run_vectorised(args, device, aim_run=aim_run, wandb_run=wandb_run)

    x_discr_ground = np.linspace(-2, 0, 10)
    offset_values = [0]
    xlim, ylim = (-3, 7), (0., 10)
    gamma = args['gamma']
    policy_net, target_net = make_nets(args, device)
    if args['prioritized_replay']:
        replay_buffer = PrioritizedReplayBuffer(capacity=args['replay_buffer_capacity'], gamma=gamma, policy_net=policy_net,
                                                target_net=target_net, device=device)
    else:
        replay_buffer = ReplayBuffer(capacity=args['replay_buffer_capacity'])
    temps = exploration_from_args(args)                   # --exploration boltzmann: the Softmax policy in EpsilonGreedy's place

    def make_policy(episode):
        if temps:
            return Softmax(temp_start=temps['temp_start'], temp_end=temps['temp_end'], decay=temps['temp_decay'], episode=episode)
        return EpsilonGreedy(eps_start=0.5, gamma=0.999, eps_end=0.05, episode=episode, max_steps=args['max_steps'], device=device)
    eps_greedy = make_policy(0)
    greedy = lambda q, *a, **k: torch.argmax(q)
    setup_fct = make_setup_fct(args)
    env = AssemblyGym(reward_fct=sparse_reward, max_steps=args['max_steps'], restrict_2d=True,
                      assembly_env=AssemblyEnv(render=False))
    optimizer = torch.optim.Adam(policy_net.parameters(), lr=args['learning_rate'])
    first_episode = 1
    if args['load_checkpoint']:                          # successor_dqn.py:654-665 (disabled there: "not tested")
        from robotoddler.utils.utils import load_checkpoint, optimizer_to
        meta = load_checkpoint(args['load_checkpoint'], policy_net, target_net, replay_buffer, optimizer,
                               devices=dict(policy_net=device, target_net=device, optimizer=device))
        optimizer_to(optimizer, device)
        first_episode = int(meta['episode']) + 1
        eps_greedy = make_policy(int(meta['episode']))
    history = []
    roll = dict(env=env, policy_net=policy_net, setup_fct=setup_fct, x_discr_ground=x_discr_ground, xlim=xlim, ylim=ylim,
                offset_values=offset_values, img_size=args['image_size'], device=device, log_images=False,
                stable_actions_only=args['stable_actions_only'])
    for i in range(first_episode, args['num_episodes'] + 1):
        transitions, images = rollout_episode(policy=eps_greedy.step(), **roll)
        replay_buffer.push(transitions)
        losses = train_policy_net(policy_net=policy_net, target_net=target_net, optimizer=optimizer,
                                  loss_fct=args['loss_function'], replay_buffer=replay_buffer, gamma=gamma,
                                  batch_size=args['batch_size'], n_steps=args['num_training_steps'], device=device)
        update_target_net(policy_net=policy_net, target_net=target_net, tau=args['tau'])
        log_info, _ = log_episode(episode=i, transitions=transitions, policy=eps_greedy, losses=losses, gamma=gamma,
                                  aim_run=aim_run, wandb_run=wandb_run)
        history.append(log_info)
        if args['verbose']:
            print(f"episode {i}: {log_info}")
        if args['save_checkpoint'] and i % args['checkpoint_every'] == 0:     # utils.py:54-89 layout
            T.sync_optimizer(policy_net)
            save_checkpoint(args['save_checkpoint'], policy_net, target_net, replay_buffer, optimizer, i,
                            {k: (str(v) if not isinstance(v, (int, float, str, bool, type(None))) else v) for k, v in args.items()})
        if i % args['evaluate_every'] == 0:
            transitions, _ = rollout_episode(policy=greedy, **roll)
            ev, _ = log_episode(episode=i, transitions=transitions, losses=None, context='evaluation', gamma=gamma,
                                aim_run=aim_run, wandb_run=wandb_run)
            if args['verbose']:
                print(f"evaluation {i}: {ev}")
    return history


if __name__ == '__main__':
    main()
