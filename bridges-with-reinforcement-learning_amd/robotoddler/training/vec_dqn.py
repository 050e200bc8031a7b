"""Vectorised successor-feature DQN: E environments per GPU in lock-step (VecAssemblyGym), device replay ring of
compact records re-rasterised on sample, fused HIP target / soft-update ops, one all-gather of records per
lock-step across ranks.

Semantics follow rollout_episode / train_policy_net / update_target_net of the reference
(robotoddler/training/successor_dqn.py:157-288, 365-475) with these batched readings:
* epsilon-greedy draws one uniform per env; exploring envs take the candidate whose raster overlaps least with the
  per-episode-step count images (successor_dqn.py:112-132), all envs scored against the images of the lock-step
  start and the chosen rasters added afterwards;
* exploration="boltzmann" (an extension: the reference's Softmax policy, successor_dqn.py:138-154, cannot run) draws every env's
  candidate from softmax(q / temperature) on the device instead, the temperature annealed per lock-step (DESIGN.md section 7,
  "Boltzmann exploration");
* the TD target is the elementwise  lin_reward + gamma * q'  (the single-env reference path trains on a [B,B]
  broadcast of it because its lin_reward is [B,1]; that quirk is reproduced only in the single-env loop);
  with n_step = n > 1 (an extension: the reference has no multi-step target) it is  G + gamma^h * q',  G the h-step return of
  the transition's window, h = n or what the end of the episode leaves ("n-step returns");
* "done" of a transition = terminated | truncated | no next action (successor_dqn.py:393, 409-411);
* epsilon decays once per LOCK-STEP (the reference: once per episode, successor_dqn.py:702 -- with thousands of envs
  hundreds of episodes end per lock-step and a per-episode decay would reach the floor within a dozen lock-steps);
* uniform replay draws WITH replacement (torch.randint on the device ring; the reference's random.sample draws without:
  a duplicate inside a batch of 32 out of >= 10^4 records has probability ~5e-2 and only repeats a sample);
* prioritised replay draws in proportion to td_error + 1e-5, the rollout's TD error (PrioritizedReplayBuffer); priority_alpha /
  priority_refresh (extensions: the reference has neither) add Schaul et al.'s exponent and write |q(s,a) - q_target| of the
  sampled transitions back as their priorities, both on the device ("Prioritised replay on the device");
  priority_beta (an extension likewise) multiplies the loss terms of every sampled transition with its importance-sampling weight;
* with several ranks every rank trains an identical replica on the identical gathered ring (same sampling seed); extra
  GPUs add rollout throughput, not optimiser throughput; parameters are re-broadcast every 100 lock-steps;
* log_episode's numbers (successor_dqn.py:479-499) are logged per lock-step as means over the episodes that ended in it on all
  ranks (EpisodeStats; the reference logs every episode);
* the evaluation (successor_dqn.py:749-781) runs one greedy episode in each of --eval_envs envs at once and logs their means;
  --eval_epsilon > 0 (an extension: the reference evaluates greedily only) explores with the training rule on the evaluation's
  own count images.

How a lock-step is spent: acting through the factored SuccessorMLP forward whose first layer reads
the bit-packed rasters (bridges_bits_linear); the TD / successor-feature targets of ALL optimiser steps of the lock-step
in one pass (the target net is constant meanwhile); the optimiser steps themselves as replays of one HIP graph.
"""
import os
import time
from typing import NamedTuple, Optional

import numpy as np
import torch

from bridges_hip import abi, dqn_ops, ops
from bridges_hip.shapes import load_urdf
from bridges_hip.vec_env import RandomBridges, RandomObstacles, RandomTargets, VecAssemblyGym
from robotoddler.training import distributed as D
from robotoddler.training import records as R
from robotoddler.training.curriculum import Curriculum, CurriculumRun
from robotoddler.training.episode_stats import EpisodeStats
from robotoddler.training import train_step as T


# --random_obstacles: every obstacle of every env is drawn from x in [-3, 3), z in [0.3, 2.5) at the start of an episode
OBSTACLE_RANGE = ((-3.0, 3.0), (0.3, 2.5))
SEARCH_SEED = 24681357                                   # particle_search: its stream is seeded with SEARCH_SEED + the agent's seed
# the means that ride to the host behind a train_steps call's losses, under their log keys (and attribute names) in the order
# _targets stacks them: soft targets, a relative target temperature, Munchausen targets
SOFT_TARGET_KEYS = ("target_entropy", "soft_value_gap")
RELATIVE_TARGET_KEYS = ("target_temperature_effective",)
MUNCHAUSEN_KEYS = ("munchausen_bonus", "munchausen_clipped", "munchausen_missed")


class TargetBatch(NamedTuple):
    """What VecDQN._targets hands to train_steps for n transitions: the five fields of a plain agent's batch in the order they
    always had, then what only some modes fill or read.  Every tensor is the first n rows of one of the scratch env's."""
    block_f: Optional[torch.Tensor]                          # [n, 1, S, S] f32 raster of s; None with task_channels
    binary: torch.Tensor                                     # [n, 6] f32 binary features
    action_f: Optional[torch.Tensor]                         # [n, 1, S, S] f32 raster of the action block; None with task_channels
    q_target: torch.Tensor                                   # [n] f32 TD targets
    sf_target: Optional[torch.Tensor]                        # [n, px] f32 successor-feature targets; None without mse_block_features
    reward_maps: Optional[torch.Tensor] = None               # [n, px] f32 map of every transition (per_env_tasks, else None)
    obstacle_bits: Optional[torch.Tensor] = None             # [n, 64] int64 obstacle bit raster of every transition (per_env_obstacles)
    state_bits: Optional[torch.Tensor] = None                # [n, 64] int64 bit rasters of s and of the action block, filled in every
    action_bits: Optional[torch.Tensor] = None               # mode: with task_channels the train step builds its rows from them


class VecDQN:
    # an instance that __init__ has not filled (tests build such stand-ins with __new__) reads the loop as it was
    exploration, n_step, rows_fed, search_every = "epsilon_greedy", 1, 0, 0
    hindsight = hindsight_buffer = curriculum = priority_beta = _rows_seen_dev = _hash_mult = _task_mult = last_search = None
    target_temperature = _soft_stats = target_entropy = soft_value_gap = None
    temp_relative = target_temp_relative = hindsight_fold = False
    spread_floor, temperature_effective, target_temperature_effective, _temp_out, _soft_names = 1e-3, None, None, None, ()
    munchausen = replay_env_s = munchausen_bonus = munchausen_clipped = munchausen_missed = None
    search_sampler = search_gen = search_temperature = search_resample_temperature = None

    def __init__(self, policy_net, target_net, optimizer, env, replay_capacity, batch_size, gamma, tau, loss_function,
                 seed=0, rank=0, eps_start=0.5, eps_end=0.05, eps_decay=0.999, prioritized=False, stable_actions_only=False,
                 episode_stats=False, per_env_tasks=False, per_env_obstacles=False, task_channels=False, curriculum=None,
                 n_step=1, double_q=False, priority_alpha=1.0, priority_refresh=False, priority_beta=None, priority_beta_anneal=0,
                 exploration="epsilon_greedy", temp_start=1.0, temp_end=0.1, temp_decay=0.999, hindsight=None, hindsight_goals=1,
                 search_every=0, search_tasks=None, search_width=None, search_merge=False, search_priority=None,
                 target_temperature=None, temp_relative=False, target_temp_relative=False, spread_floor=1e-3,
                 munchausen_alpha=None, munchausen_clip=None, search_sampler=None, search_temperature=None,
                 search_resample_temperature=None, hindsight_fold=False):
        """``per_env_tasks=True``: train on a rollout env whose envs own their tasks (VecAssemblyGym(targets=RandomTargets())
        or set_targets).  Rows are then shared by (state, task), acting and the target forward weigh every row with the reward
        map of its env, a record ends in the targets its transition was taken under and replay rebuilds the map from them,
        and the optimiser step reads a map per transition.  Only the path that is hand-written from acting to Adam takes it:
        a SuccessorMLP on 64x64 images with the fused optimiser step.
        ``per_env_obstacles=True`` (with per_env_tasks=True only): the envs own their obstacles as well
        (VecAssemblyGym(obstacles=RandomObstacles()) or set_obstacles).  Acting and the target forward add every env's obstacle
        raster to the first layer as a second bit-packed operand (bridges_bits_linear2), a record ends in the targets AND the
        obstacles of its transition, replay filters the next states' candidates against them, and the optimiser step reads a
        bit-packed obstacle raster per transition.
        ``task_channels=True`` (with per_env_tasks=True only): the conv Q-networks on per-env tasks -- a ConvNet(in_channels=4,
        img_size=(64, 64)) or the U-Net Policy, which take the task as two image channels.  Every row a net is fed gets the
        reward map and the obstacle raster of its env (of its transition, in replay) beside its block and action rasters, all
        four channels written by one launch from the bit-packed rasters and a map index (ops.conv_input); rows are shared by
        (state, candidate, stable flag, task); the optimiser step is the autograd body on per-transition rows.  Neither the
        rollout env nor the replay scratch env needs f32 rasters in this mode.
        ``curriculum=Curriculum(...)`` (a rollout env on a task family only): the weights of the family's classes follow the
        failure rate per class on the device (robotoddler.training.curriculum); evaluation envs are not touched.
        ``n_step=n`` (1..8, at most the env's max_steps): train on n-step returns.  Every env keeps a window of its last n
        transitions on the device (bridges_nstep_fold); a lock-step pushes, per env, the h-step record of the oldest start once
        the window is full (h = n) and of every pending start when the episode ends (h = n .. 1).  A ring row is the record of
        the window's LAST step with the h-step return in O_LIN, the start's stable flag and priority in O_STABLE_S / O_TD and h
        in a new last column; _targets rebuilds the start state as a prefix of the row's block list and discounts the
        bootstrap by gamma^h ("n-step returns").  n_step=1 is the one-step loop: no column, no launch of this.
        ``double_q=True``: double Q-learning targets (an extension: the reference keeps the form as a commented alternative).
        _targets runs the POLICY net over the candidate rows of the sampled next states as well, and the row of a transition is
        the first maximum of the policy net's q while its value and successor features stay the target net's
        (bridges_td_target_select): q = G + gamma^h q_target_net(s', argmax_a' q_policy_net(s', a')).  The selection uses the
        policy net as it stands when _targets runs, once per lock-step for all n_steps batches -- the approximation the loop
        already makes by sharing one target pass between them.  It composes with n_step, prioritized, stable_actions_only, the
        curriculum, per-env tasks / obstacles, task_channels and several ranks (the targets are computed after the gather);
        td_errors stays the reference's formula.  The ring stores transitions, not targets, so a checkpoint can be resumed with
        the option switched ("Double Q-learning").  False is the loop as it was: no launch of this.
        ``priority_alpha=a`` (0..1, with prioritized=True only): a transition is replayed with probability proportional to
        (td_error + 1e-5)^a -- Schaul et al.'s exponent; 1 is the reference's rule, 0 the uniform draw -- through the sampler
        kernel (ReplayRing.sample_prioritized).  ``priority_refresh=True`` (with prioritized=True only, one rank): after _targets
        the policy net as it stands then values (s_t, a_t) of all n_steps * B sampled transitions, and |q(s_t, a_t) - q_target| is
        written back to the sampled rows (ReplayRing.update_priorities); rows keep the rollout's td_errors until they are first
        sampled.  Neither option changes the record, the ring or a checkpoint, so a run may be resumed with other settings; with
        priority_alpha=1.0 and priority_refresh=False the loop samples through ReplayRing.sample as it always did (DESIGN.md,
        "Prioritised replay on the device").
        ``priority_beta=b`` (0..1, with prioritized=True only; None, the default: no weights anywhere): Schaul et al.'s
        importance-sampling correction.  Every sampled transition gets the weight (N P(i))^(-b), each batch divided by its own
        maximum (ReplayRing.sample_weights, computed on the device from the masses the draw was made from), and the optimiser step
        multiplies the transition's loss terms by it.  The loop then always samples through the sampler kernel, at
        priority_alpha=1 without refresh too.  ``priority_beta_anneal=n`` (> 0): the exponent rises linearly from b to 1 over the
        first n train_steps calls that trained (0: constant); the count is checkpointed.  Several ranks are allowed: the weights
        are a deterministic function of identical rings.
        ``exploration="boltzmann"`` (an extension: the reference sketches a Softmax policy that cannot run): every env draws its
        candidate with probability proportional to exp(q / temperature) in one launch on the device (bridges_boltzmann_select, the
        rule in include/bridges_hip.h) with the uniform draw epsilon-greedy would have compared with epsilon.  The overlap with the
        count images is not computed and the images stay as they are (two launches fewer per acting lock-step).  The temperature
        starts at ``temp_start`` (1.0) and follows t <- (t - temp_end) * temp_decay + temp_end per lock-step (``temp_end`` 0.1,
        ``temp_decay`` 0.999: the reference's form, per lock-step as epsilon's); epsilon is left alone.  It is a function of the
        lock-step count alone, so ranks agree; it is checkpointed.  act(greedy=True) and evaluate() stay greedy.  The temp_*
        arguments are refused without the option.  "epsilon_greedy" is the loop as it was: no launch of this.
        ``hindsight="final"`` (with per_env_tasks=True only, one rank, one-step returns unless hindsight_fold=True; an extension: hindsight experience replay,
        Andrychowicz et al., strategy "final"): every episode that ends is pushed a second time, ``hindsight_goals`` = G times
        (1..4), under T targets its own final structure reached -- the centres of the bounding boxes of blocks drawn from it on a
        stream of its own -- with the reward, linear reward and done flag the env would have recorded under those targets
        (bridges_hindsight_relabel, the rule in include/bridges_hip.h; DESIGN.md, "Hindsight relabelling").  The loop keeps every
        env's running episode on the device (records.HindsightBuffer); the relabelled rows follow the lock-step's own records
        into the ring, their number rides to the host with the lock-step's counts: no wait of its own.  The training step does
        not change.  It composes with per-env obstacles, task_channels, double_q, prioritised replay (a relabelled row carries
        the priority of the transition it restates) and Boltzmann exploration.  None is the loop as it was: no launch of this.
        ``hindsight_fold=True`` (with hindsight="final" only): the relabelling under n-step returns.  The buffer keeps the one-step
        records, and the relabelled walk of a finished episode is folded on the device into the ring's h-step rows
        (bridges_hindsight_relabel_nstep: the return over the RELABELLED linear rewards, O_STABLE_S and O_TD of the start, h in the
        last column; the end of a walk flushes its pending starts whether or not its last step is done -- under hindsight targets
        a final step that is not terminal bootstraps like any other).  With n_step = 1 it is hindsight="final" bit for bit.
        Without it hindsight="final" with n_step > 1 stays refused.
        ``hindsight="per_step"`` (every condition and refusal of "final", hindsight_fold included): hindsight experience replay's
        strategy "future".  It is not called "future" here because that value was refused by name before the strategy existed and
        stays refused: the option names what the loop does -- goals per step.  Every transition t of an episode that ends gets,
        per slot g < ``hindsight_goals``, T goals of its own: the box centre of a block f >= t of the episode, drawn per (g, t),
        and T - 1 more from the structure as it stands after step f; the transition is pushed once per slot under them, unless
        the episode would have been over before step t (bridges_hindsight_per_step / _nstep, the rule in include/bridges_hip.h).
        So early transitions no longer see goals that only blocks placed much later reach by chance, and G counts relabelled rows
        per transition.  Buffer, counts, host waits, checkpoint keys and the training step are those of "final"; a checkpoint of
        one strategy is refused by the other ((hindsight, hindsight_goals) is recorded).
        ``search_every=N`` (N >= 1; one rank; an extension: search in training): every N-th lockstep(), after
        the lock-step's own rows are pushed and before train_steps, a beam search of width ``search_width`` = B (1..16, default
        8) with the policy net's q as the heuristic runs on the tasks the rollout envs 0 .. ``search_tasks`` - 1 (M, at most the
        env's E; default min(E, 64)) are playing at that moment, in a search env of M * B envs the agent owns
        (search_env_like), and the records of every task's best finished beam follow into the ring: one-step rows, or
        n_step-step rows as the fold would have emitted them (beam_search(trace=True), bridges_beam_trace).  A row nobody has
        scored carries ``search_priority`` in O_TD under prioritized=True (default 1.0; priority_refresh corrects it once the row
        is drawn) and 0.0 otherwise, as the loop's own rows do.  ``search_merge=True`` merges equal structures in the search.  On
        a fixed task (per_env_tasks=False) every group would find the same episode: M is forced to 1.  The search reads the nets
        and the rollout env's tasks and writes the ring; the rollout env, the count images, the exploration stream, epsilon and
        the temperature, the n-step windows, the hindsight buffer, the episode statistics, the curriculum, env_steps and
        episodes_done stay as they are.  search_env_steps, search_rows and search_success_rate count what it did; last_search
        holds the numbers of the lock-step that searched (None for one that did not).  0 is the loop as it was: no launch of
        this.
        ``target_temperature=T`` (a finite number > 0; an extension: the Boltzmann softmax backup, Expected SARSA for the policy
        Boltzmann exploration draws from; DESIGN.md section 7, "Soft targets"): the bootstrap of every target is the expectation
        under pi(a'|s') ~ exp(q'(s', a') / T) over the next state's candidates instead of the maximum -- q = G + gamma^h sum_a'
        pi(a') q'(s', a'), and the successor-feature target takes sum_a' pi(a') psi'(s', a') (bridges_soft_expect, then the
        existing target kernel on one-row segments).  The factored SuccessorMLP runs its middle layers over ALL next-state rows
        and applies the linear psi' head to the pi-weighted mean of the last hidden rows; the other nets average channel 0 of
        their distinct rows' outputs.  double_q=True: the policy net's q weighs the rows, values and features stay the target
        net's.  It composes with n_step, prioritised replay (refresh, weights), per-env tasks and obstacles, task_channels,
        stable_actions_only and several ranks (every rank forms its own targets, as ever).  The rollout's td_errors stay the
        max-operator error, evaluation and beam search stay greedy, T is constant.  target_entropy and soft_value_gap hold the
        last train_steps call's means over the transitions that are not done (they ride to the host with the losses).  None is
        the loop as it was: no launch of this.
        ``temp_relative=True`` (with exploration="boltzmann" only) / ``target_temp_relative=True`` (with target_temperature
        only): the temperature is a MULTIPLE of each state's own spread of q -- env e draws at temperature * max(s_e,
        ``spread_floor``), transition i is backed up at target_temperature * max(s_i, spread_floor), s the population standard
        deviation of the finite q among the state's candidate rows (double_q: of the policy net's q, the values that weigh the
        rows), formed on the device inside the operator's own launch (bridges_boltzmann_select_rel / bridges_soft_expect_rel,
        the rule in include/bridges_hip.h; DESIGN.md section 7, "Relative temperatures").  ``temperature`` keeps its schedule
        and target_temperature its value; each is now the multiple.  temperature_effective holds the mean effective temperature
        over the last lock-step's valid envs (it rides with the counts), target_temperature_effective the mean over the last
        train_steps call's transitions that are not done (it rides with the losses): no host wait of their own.  Both compose
        with whatever their parent option composes with; evaluation and beam search stay greedy.  ``spread_floor`` (finite,
        > 0; default 1e-3) is refused unless one of the two is set.  False is the loop as it was: no launch of this.
        ``munchausen_alpha=A`` (in [0, 1]; with target_temperature only; DESIGN.md section 7, "Munchausen targets"): Munchausen
        DQN.  With pi = softmax(q' / T) of the target net, q = r + A * max(T ln pi(a|s), ``munchausen_clip``) + gamma * V_T(s'),
        V_T = T ln sum exp(q' / T) the log-sum-exp value in place of the expectation (bridges_soft_value over the next rows, and
        over the rows of the state the transition was taken IN with the taken action's row, bridges_action_row).  A second
        scratch env, replay_env_s, rebuilds the candidates of s (load_records(prev=True)) and the target net runs over them:
        one more host wait per train_steps call (its valid_rows).  The successor-feature target stays the soft target's.
        ``munchausen_clip`` (finite, <= 0; default -1.0) is refused without munchausen_alpha.  target_temp_relative gives each
        of s and s' its own spread.  Refused with double_q (the bonus and the bootstrap are one estimator's) and with n_step > 1
        (an h-step row does not hold its intermediate actions).  munchausen_bonus (the mean bonus), munchausen_clipped (the
        share at or below the clip) and munchausen_missed (taken actions not found among the rebuilt candidates; 0) ride with
        the losses.  None is the loop as it was: no launch of this, no second env."""
        self.munchausen = None
        if munchausen_clip is not None and munchausen_alpha is None:
            raise ValueError("VecDQN(munchausen_clip=...) clips the Munchausen bonus: it needs munchausen_alpha")
        if munchausen_alpha is not None:
            clip = -1.0 if munchausen_clip is None else munchausen_clip
            for name, v in (("munchausen_alpha", munchausen_alpha), ("munchausen_clip", clip)):
                if not isinstance(v, (int, float)) or isinstance(v, bool):
                    raise ValueError(f"VecDQN({name}={v!r}): a number")
            if not 0.0 <= float(munchausen_alpha) <= 1.0:                            # (a NaN fails both comparisons)
                raise ValueError(f"VecDQN(munchausen_alpha={munchausen_alpha!r}): the weight of the log-policy bonus lies in [0, 1]")
            if not float("-inf") < float(clip) <= 0.0:
                raise ValueError(f"VecDQN(munchausen_clip={clip!r}): the lower clip of T ln pi is finite and <= 0")
            if target_temperature is None:
                raise ValueError("VecDQN(munchausen_alpha=...) forms its bonus and its bootstrap under the Boltzmann policy of the "
                                 "target net: it needs target_temperature")
            if double_q:
                raise ValueError("VecDQN(munchausen_alpha=...) does not run with double_q=True: the bonus and the bootstrap are one "
                                 "estimator's, the target net's")
            if int(n_step) > 1:
                raise ValueError("VecDQN(munchausen_alpha=...) needs n_step=1: an h-step row does not hold the descriptors of its "
                                 "intermediate actions, and their bonuses would take h forwards")
            self.munchausen = (float(munchausen_alpha), float(clip))
        self.munchausen_bonus = self.munchausen_clipped = self.munchausen_missed = None
        self.temp_relative, self.target_temp_relative = bool(temp_relative), bool(target_temp_relative)
        if self.temp_relative and str(exploration) != "boltzmann":
            raise ValueError("VecDQN(temp_relative=True) makes the temperature of Boltzmann exploration relative to each state's "
                             "spread of q: it needs exploration='boltzmann'")
        if self.target_temp_relative and target_temperature is None:
            raise ValueError("VecDQN(target_temp_relative=True) makes the temperature of the soft targets relative to each state's "
                             "spread of q: it needs target_temperature")
        ok = isinstance(spread_floor, (int, float)) and not isinstance(spread_floor, bool)
        if not ok or not (0.0 < float(spread_floor) < float("inf")):                 # (a NaN fails the comparison)
            raise ValueError(f"VecDQN(spread_floor={spread_floor!r}): a finite number > 0")
        if float(spread_floor) != 1e-3 and not (self.temp_relative or self.target_temp_relative):
            raise ValueError("VecDQN(spread_floor=...) is the floor of the spread a relative temperature multiplies: it needs "
                             "temp_relative=True or target_temp_relative=True")
        self.spread_floor = float(spread_floor)
        self.temperature_effective = self.target_temperature_effective = self._temp_out = None
        if target_temperature is not None:
            ok = isinstance(target_temperature, (int, float)) and not isinstance(target_temperature, bool)
            if not ok or not (0.0 < float(target_temperature) < float("inf")):       # (a NaN fails the comparison)
                raise ValueError(f"VecDQN(target_temperature={target_temperature!r}): a finite number > 0 (None: the max-operator target)")
            target_temperature = float(target_temperature)
        self.target_temperature = target_temperature
        self._soft_stats, self._soft_names = None, ()        # on the device: what the last _targets call left for the log, and its keys
        self.target_entropy = self.soft_value_gap = None
        self._init_search(env, search_every, search_tasks, search_width, search_merge, search_priority, per_env_tasks, prioritized,
                          sampler=search_sampler, temperature=search_temperature, resample_temperature=search_resample_temperature)
        self.exploration = str(exploration)
        if self.exploration not in ("epsilon_greedy", "boltzmann"):
            raise ValueError(f"VecDQN(exploration={exploration!r}): one of 'epsilon_greedy', 'boltzmann'")
        if self.exploration != "boltzmann" and (temp_start, temp_end, temp_decay) != (1.0, 0.1, 0.999):
            raise ValueError("VecDQN(temp_start=..., temp_end=..., temp_decay=...) shape the temperature of Boltzmann exploration: "
                             "they need exploration='boltzmann' (epsilon-greedy has no temperature)")
        self.temp_start, self.temp_end, self.temp_decay = float(temp_start), float(temp_end), float(temp_decay)
        if self.exploration == "boltzmann":
            from robotoddler.training.successor_dqn import check_temperature_schedule
            check_temperature_schedule(self.temp_start, self.temp_end, self.temp_decay, who="VecDQN(exploration='boltzmann')")
        self.temperature = self.temp_start
        self.explored_fraction = None                        # Boltzmann: the share of the last lock-step's valid envs off the arg-max
        self._ex_w = None
        self.priority_alpha, self.priority_refresh = float(priority_alpha), bool(priority_refresh)
        self.priority_beta = None if priority_beta is None else float(priority_beta)
        self.priority_beta_anneal = int(priority_beta_anneal)
        self.priority_beta_calls = 0                         # train_steps calls that trained so far: the annealing clock
        if self.priority_beta is not None and not 0.0 <= self.priority_beta <= 1.0:      # (a NaN fails both comparisons)
            raise ValueError(f"VecDQN(priority_beta={priority_beta}): the exponent of the importance-sampling weights lies in "
                             "[0, 1] (0: all weights 1, 1: the full correction)")
        if self.priority_beta_anneal < 0:
            raise ValueError(f"VecDQN(priority_beta_anneal={priority_beta_anneal}): a number of train_steps calls, >= 0")
        if not prioritized and (self.priority_beta is not None or self.priority_beta_anneal):
            raise ValueError("VecDQN(priority_beta=..., priority_beta_anneal=...) correct the prioritised draw: they need "
                             "prioritized=True (a uniform draw has nothing to correct)")
        if self.priority_beta is None and self.priority_beta_anneal:
            raise ValueError("VecDQN(priority_beta_anneal=...) anneals priority_beta: give priority_beta as well")
        if not 0.0 <= self.priority_alpha <= 1.0:            # (a NaN fails both comparisons)
            raise ValueError(f"VecDQN(priority_alpha={priority_alpha}): the exponent of the priorities lies in [0, 1] "
                             "(0: uniform, 1: proportional to td_error + 1e-5)")
        if not prioritized and (self.priority_refresh or self.priority_alpha != 1.0):
            raise ValueError("VecDQN(priority_alpha=..., priority_refresh=...) shape the prioritised draw: they need prioritized=True "
                             "(a uniform loop stores no priorities: O_TD of its records is 0)")
        if self.priority_refresh and D.active():
            raise ValueError("VecDQN(priority_refresh=True) runs on one rank only: the replica nets drift between the parameter "
                             "broadcasts, so every rank would write other priorities and the rings would stop being replicas "
                             "(priority_alpha alone is allowed: the sampler is deterministic on identical rings)")
        self._transitions = None                             # priority_refresh: what _targets leaves for _transition_q
        self.double_q = bool(double_q)
        self.n_step = int(n_step)
        if not 1 <= self.n_step <= abi.NSTEP_MAX:
            raise ValueError(f"VecDQN(n_step={n_step}): the window holds 1..{abi.NSTEP_MAX} transitions per env (BRIDGES_NSTEP_MAX)")
        if self.n_step > 1 and self.n_step > int(env.max_steps):
            raise ValueError(f"VecDQN(n_step={n_step}): an episode of this env has at most max_steps = {env.max_steps} transitions, "
                             "no window would ever fill")
        self.per_env_tasks, self.per_env_obstacles = bool(per_env_tasks), bool(per_env_obstacles)
        self.task_channels = bool(task_channels)
        self.hindsight, self.hindsight_goals, self.hindsight_fold = hindsight, int(hindsight_goals), bool(hindsight_fold)
        if self.hindsight not in (None, "final", "per_step"):
            raise ValueError(f"VecDQN(hindsight={hindsight!r}): None, 'final' or 'per_step'")
        if self.hindsight is None and self.hindsight_goals != 1:
            raise ValueError("VecDQN(hindsight_goals=...) counts the relabelled copies of an episode: it needs hindsight='final' or 'per_step'")
        if self.hindsight is None and self.hindsight_fold:
            raise ValueError("VecDQN(hindsight_fold=True) folds the relabelled rows into n-step returns: it needs hindsight='final' or 'per_step'")
        if self.hindsight is not None:
            opt = f"VecDQN(hindsight={self.hindsight!r})"
            if not 1 <= self.hindsight_goals <= 4:
                raise ValueError(f"VecDQN(hindsight_goals={hindsight_goals}): an episode is relabelled 1..4 times")
            if not self.per_env_tasks:
                raise ValueError(f"{opt} needs per_env_tasks=True: only a record that ends in its own targets can be given others")
            if getattr(env, "task_family", None) is not None or curriculum is not None:
                raise ValueError(f"{opt} does not run on a task family (RandomBridges) or under a curriculum: a family's task is its class, and a box centre names none")
            if self.n_step > 1 and not self.hindsight_fold:
                raise ValueError(f"{opt} needs n_step=1 or hindsight_fold=True: an h-step row's return has to be "
                                 "folded again under the new targets")
            if D.active():
                raise ValueError(f"{opt} runs on one rank only: the relabelled rows are not part of the all-gather")
        if self.task_channels:
            self._check_task_channels(policy_net, target_net, env)
        if getattr(env, "per_env_obstacles", False) and not self.per_env_obstacles:
            raise ValueError("VecDQN cannot train on a rollout env with per-env obstacles (RandomObstacles / set_obstacles) unless it "
                             "is built with per_env_tasks=True AND per_env_obstacles=True: by default the first layer's "
                             "image-independent part, the replay record and the captured train steps hold ONE obstacle raster")
        if self.per_env_obstacles:
            if not self.per_env_tasks:
                raise ValueError("VecDQN(per_env_obstacles=True) needs per_env_tasks=True: per-env obstacles ride on the per-env task "
                                 "buffers, the per-env tables and the per-transition records")
            if not getattr(env, "per_env_obstacles", False):
                raise ValueError("VecDQN(per_env_obstacles=True) needs a rollout env with per-env obstacles "
                                 "(VecAssemblyGym(obstacles=RandomObstacles()) or set_obstacles); this env has one shared obstacle list")
        if getattr(env, "per_env_tasks", False) and not self.per_env_tasks:
            raise ValueError("VecDQN cannot train on a rollout env with per-env tasks (RandomTargets / set_targets) unless it is "
                             "built with per_env_tasks=True: by default envs in the same state share candidate rows whatever "
                             "their task (bridges_env_groups keys rows by state alone), the factored SuccessorMLP acting path "
                             "and the captured train steps hold ONE reward map, and a replay record does not store its task")
        if self.per_env_tasks and not self.task_channels:
            loss_parts = loss_function.split('+')
            if not getattr(env, "per_env_tasks", False):
                raise ValueError("VecDQN(per_env_tasks=True) needs a rollout env with per-env tasks "
                                 "(VecAssemblyGym(targets=RandomTargets()) or set_targets); this env has one fixed task")
            for name, net in (("policy", policy_net), ("target", target_net)):
                if not hasattr(net, "q_from_first_layer"):
                    raise ValueError(f"VecDQN(per_env_tasks=True): the {name} net is a {type(net).__name__}; only SuccessorMLP "
                                     "weighs its output with a per-row reward map (the conv nets take the map as an image channel: "
                                     "build the agent with task_channels=True for them)")
                if tuple(getattr(net, "img_size", (64, 64))) != (64, 64) or env.img != 64:
                    raise ValueError(f"VecDQN(per_env_tasks=True): the factored acting path is built for 64x64 images, the {name} "
                                     f"net has {tuple(getattr(net, 'img_size', ()))} and the env {env.img}x{env.img}")
                if not self._factored(net):
                    raise ValueError("VecDQN(per_env_tasks=True) needs the factored acting path (VecDQN.FACTORED_ACTING)")
            if not T.fused_step_enabled(policy_net, loss_parts):
                raise ValueError("VecDQN(per_env_tasks=True) needs the fused optimiser step (train_step.fused_step_enabled): a "
                                 "float32 SuccessorMLP, the MSE losses of the CLI and BRIDGES_FUSED_MLP_STEP != 0 -- the "
                                 "autograd body of the captured step holds one reward map")
        self.policy_net, self.target_net, self.opt, self.env = policy_net, target_net, optimizer, env
        # stable actions only: the rollout env and the replay scratch env narrow every candidate set to the stable placements,
        # so acting, exploring, the TD target's max over next actions and the done flags all see the same smaller set
        self.stable_actions_only = bool(stable_actions_only)
        if self.stable_actions_only != bool(getattr(env, "stable_actions_only", False)):
            raise ValueError("VecDQN(stable_actions_only=...) must match the rollout env's stable_actions_only")
        self.device = env.device
        self.B, self.gamma, self.tau = batch_size, gamma, tau
        self.loss_parts = loss_function.split('+')
        self.prioritized = bool(prioritized)      # PrioritizedReplayBuffer semantics (replay_memory.py:45-93)
        # per-env tasks: a record ends in the T targets (x, y, z) its transition was taken under, per-env obstacles: followed by
        # its O obstacles (x, y, z)
        self.n_task_targets = env.n_targets if self.per_env_tasks else 0
        self.n_task_obstacles = env.n_obstacles if self.per_env_obstacles else 0
        self.task_width = 3 * self.n_task_targets + 3 * self.n_task_obstacles
        # n-step returns: one more column, the horizon h of the row
        self.ring = R.ReplayRing(replay_capacity, self.device, width=R.RECORD_WIDTH + self.task_width + (self.n_step > 1))
        self._window = None                                  # the n-step windows of the envs of all ranks, made by the first fold
        # hindsight relabelling: the running episode of every env, in the ring's width (n-step returns: one-step records, one
        # column narrower, folded as they are relabelled)
        self.hindsight_buffer = (R.HindsightBuffer(env.E, self.ring.width, self.device, goals=self.hindsight_goals, n_blocks=env.K,
                                                   strategy=self.hindsight or "final",
                                                   **(dict(n_step=self.n_step, gamma=self.gamma) if self.n_step > 1 else {}))
                                 if self.hindsight is not None else None)
        self.hindsight_rows = 0                              # relabelled rows the last lock-step pushed
        # replay sampling must be identical on every rank (replicated rings) -> shared seed; exploration differs
        self.sample_gen = torch.Generator(device=self.device).manual_seed(1234567 + seed)
        self.explore_gen = torch.Generator(device=self.device).manual_seed(7654321 + seed * 1000 + rank)
        self.seed, self.rank = int(seed), int(rank)
        self.epsilon, self.eps_end, self.eps_decay = eps_start, eps_end, eps_decay
        self.step_images = torch.zeros((env.K + 1, env.img, env.img), dtype=torch.float32, device=self.device)
        # scratch env used to rebuild the candidate sets of sampled next states (see _replay_env)
        self.replay_env = self._make_replay_env(batch_size)
        # Munchausen targets: a second one for the states the transitions were taken in
        self.replay_env_s = self._make_replay_env(batch_size) if self.munchausen is not None else None
        self.mse = torch.nn.MSELoss()
        for g in optimizer.param_groups:                # step counter on the device: the train step is graph-captured
            if 'capturable' in g:
                g['capturable'] = True
        self._eager_reduce = None                            # dqn_ops.ReduceTables of the eager optimiser steps
        self.episodes_done = 0
        self.env_steps = 0
        # the counts of a lock-step (_count): env-steps and finished episodes; n-step returns: the emitted rows (one rank);
        # Boltzmann exploration: the envs whose draw left the first maximum; hindsight relabelling: the relabelled rows
        self._count_names = (("valid", "done") + (("emitted",) if self.n_step > 1 else ())
                             + (("explored",) if self.exploration == "boltzmann" else ()) + (("hindsight",) if self.hindsight is not None else ())
                             + (("temp_sum",) if self.temp_relative else ()))
        self._counts_host = torch.zeros(len(self._count_names), dtype=torch.int64).pin_memory()
        # per-episode statistics of the rollout envs (log_episode's numbers), folded on the device after every act()
        # (a task family -- RandomBridges -- keeps them per class as well: one row per span / height n = 0..hi)
        self.episode_stats = (EpisodeStats(env.E, env.K, gamma, env.n_targets, self.device, n_classes=self._n_classes(env))
                              if episode_stats else None)
        self._eval_state = {}                                # evaluate(): (random stream, EpisodeStats, count images) per env shape
        self._trace_state = {}                               # beam_search(trace=True): the per-depth buffers per (E, K)
        # the curriculum keeps an accumulator of its own: whether and when the logging statistics above are taken is not its business
        self.curriculum = CurriculumRun(curriculum, env, gamma) if curriculum is not None else None
        self.curriculum_weights_host = None                  # pinned copy of the weights as of the last lock-step

    def _init_search(self, env, every, tasks, width, merge, priority, per_env_tasks, prioritized, sampler=None, temperature=None,
                     resample_temperature=None):
        """The conditions of search_every=N, decided from the arguments alone; the search env is built by the first search."""
        self.search_every = int(every)
        self.search_env = self.last_search = None
        self.search_calls = 0                                # lockstep() calls since the last search: the phase, checkpointed
        self.search_env_steps = self.search_rows = 0
        self.search_success_rate = None
        if self.search_every < 0:
            raise ValueError(f"VecDQN(search_every={every!r}): a number of lock-steps, >= 0 (0: no search)")
        if not self.search_every:
            if tasks is not None or width is not None or merge or priority is not None:
                raise ValueError("VecDQN(search_tasks=..., search_width=..., search_merge=..., search_priority=...) shape the search in "
                                 "training: they need search_every=N")
            if sampler is not None or temperature is not None or resample_temperature is not None:
                raise ValueError("VecDQN(search_sampler=..., search_temperature=..., search_resample_temperature=...) shape the search "
                                 "in training: they need search_every=N")
            return
        self._init_search_sampler(sampler, temperature, resample_temperature)
        if D.active():
            raise ValueError("VecDQN(search_every=N) runs on one rank only: the rows a search finds are not part of the all-gather")
        if not isinstance(env, VecAssemblyGym):
            raise ValueError(f"VecDQN(search_every=N) needs a VecAssemblyGym rollout env; a {type(env).__name__} (env groups on streams "
                             "of their own) is not what the fork of the search env serves")
        self.search_width = 8 if width is None else int(width)
        if not 1 <= self.search_width <= abi.BEAM_MAX_WIDTH:
            raise ValueError(f"VecDQN(search_width={width!r}): 1..{abi.BEAM_MAX_WIDTH}")
        self.search_tasks = min(env.E, 64) if tasks is None else int(tasks)
        if not 1 <= self.search_tasks <= env.E:
            raise ValueError(f"VecDQN(search_tasks={tasks!r}): the tasks are those of the rollout envs 0 .. M - 1, 1 <= M <= {env.E}")
        if not per_env_tasks:
            self.search_tasks = 1                            # one task: every group would find the same episode
        self.search_merge = bool(merge)
        if self.search_merge and env.K > abi.BEAM_MAX_SLOTS:
            raise ValueError(f"VecDQN(search_merge=True): bridges_beam_merge orders at most {abi.BEAM_MAX_SLOTS} block slots per env, "
                             f"the env has {env.K}")
        if priority is not None and not prioritized:
            raise ValueError("VecDQN(search_priority=...) is the priority of a row nobody has scored: it needs prioritized=True")
        self.search_priority = (1.0 if priority is None else float(priority)) if prioritized else 0.0
        if not self.search_priority >= 0.0:                  # (a NaN fails the comparison)
            raise ValueError(f"VecDQN(search_priority={priority!r}): a priority, >= 0")

    def _init_search_sampler(self, sampler, temperature, resample_temperature):
        """search_sampler="particles": the search in training is particle_search at ``search_temperature`` (finite, > 0) and
        ``search_resample_temperature`` (> 0, inf allowed; None: the temperature).  None: beam_search, as ever."""
        import math
        if sampler is None:
            if temperature is not None or resample_temperature is not None:
                raise ValueError("VecDQN(search_temperature=..., search_resample_temperature=...) are the temperatures of "
                                 "search_sampler='particles': they need it")
            return
        if sampler != "particles":
            raise ValueError(f"VecDQN(search_sampler={sampler!r}): 'particles' or None (the beam search)")
        if temperature is None or not (math.isfinite(float(temperature)) and float(temperature) > 0.0):
            raise ValueError(f"VecDQN(search_sampler='particles') needs search_temperature, finite and > 0; got {temperature!r}")
        if resample_temperature is not None and not float(resample_temperature) > 0.0:        # (a NaN fails the comparison)
            raise ValueError(f"VecDQN(search_resample_temperature={resample_temperature!r}): > 0 (inf: no resampling)")
        self.search_sampler, self.search_temperature = "particles", float(temperature)
        self.search_resample_temperature = self.search_temperature if resample_temperature is None else float(resample_temperature)

    def _search(self):
        """One search in training: the tasks of rollout envs 0 .. M - 1 as they stand, repeated B times, into the search env; a
        traced beam search on it; the rows into the ring.  No host wait but the search's own."""
        env, M, B = self.env, self.search_tasks, self.search_width
        if self.search_env is None:
            self.search_env = search_env_like(env, M, B)
        senv = self.search_env
        if self.per_env_tasks:
            targets = env.env_targets[:M].repeat_interleave(B, dim=0)
            if self.per_env_obstacles:
                senv.load_task(targets, env.env_obstacles[:M].repeat_interleave(B, dim=0))
            else:
                senv.load_targets(targets)
        traced = dict(merge=self.search_merge, trace=True, trace_n_step=self.n_step, trace_priority=self.search_priority)
        if self.search_sampler == "particles":
            res = self.particle_search(senv, B, self.search_temperature, self.search_resample_temperature, **traced)
        else:
            res = self.beam_search(senv, B, **traced)
        self.ring.push(res["trace_rows"])
        self.search_env_steps += senv.E * senv.K
        self.search_rows += res["trace_count"]
        self.search_success_rate = res["success_rate"]
        self.last_search = dict(search_rows=res["trace_count"], search_success_rate=res["success_rate"], search_lin_reward=res["lin_reward"])

    @staticmethod
    def _n_classes(env):
        """Rows of the per-class episode statistics: hi + 1 on a task-family env (class = the drawn n), else 1."""
        family = getattr(env, "task_family", None)
        return family.n_classes if family is not None else 1

    def _check_task_channels(self, policy_net, target_net, env):
        """The conditions of task_channels=True, decided from the arguments alone."""
        if not self.per_env_tasks:
            raise ValueError("VecDQN(task_channels=True) needs per_env_tasks=True: the option feeds the conv Q-networks the task of "
                             "every row, which only an agent on per-env tasks has")
        if not getattr(env, "per_env_tasks", False):
            raise ValueError("VecDQN(task_channels=True) needs a rollout env with per-env tasks "
                             "(VecAssemblyGym(targets=RandomTargets()) or set_targets); this env has one fixed task")
        for name, net in (("policy", policy_net), ("target", target_net)):
            if not T.conv_task_net(net):
                raise ValueError(f"VecDQN(task_channels=True): the {name} net is a {type(net).__name__}; the option is for the conv "
                                 "Q-networks, ConvNet(in_channels=4, img_size=(64, 64)) or Policy (a SuccessorMLP trains on "
                                 "per-env tasks without it)")
        if env.img != 64:
            raise ValueError(f"VecDQN(task_channels=True): the stacked input is built for 64x64 images (bridges_conv_input_rows), "
                             f"the env has {env.img}x{env.img}")

    ROW_CHUNK = 2048       # rows per forward call: ONE input shape for the whole run (MIOpen tunes per shape)
    DEDUP_STATES = True    # envs in the same state share one set of candidate rows (tests compare with False)
    DEDUP_ROWS = True      # conv nets: feed every distinct (state, candidate, stable flag) input once (tests compare with False)
    TRACK_ROWS = False     # tools: count the valid rows of every Q pass (rows_seen) beside the rows actually fed (rows_fed)
    #                        (double_q=True: rows_fed counts BOTH passes over the next-state rows, the target net's and the policy net's)
    _COMPUTE = object()    # _forward_rows(groups=...): "find the distinct rows yourself"

    def _rows(self, env, stable):
        """The candidate rows a Q pass over ``env`` is fed: (idx, row_env, (seg_lo, seg_hi), rep).  Thousands of envs of one task
        pass through the same states -- every freshly reset env holds the empty assembly, and the reference's policy is a
        near-deterministic function of the state (greedy arg-max, or the least-tried candidate of the episode step) -- and
        the rows of a state and their values depend on the state alone: envs whose block lists and stable flag are equal
        word for word (VecAssemblyGym.state_groups) share the rows of the first of them; rows seg_lo[e] .. seg_hi[e] are env
        e's.  Exact (the same kernels on the same inputs), two extra launches, no extra wait."""
        cache = getattr(env, "_dqn_rows", None)
        if cache is not None and cache[0] == env._cand_version:
            return cache[1]
        # (per-env tasks: the env's own targets are part of the key -- same state, other task, other values)
        rep = env.state_groups(stable, task=bool(getattr(env, "per_env_tasks", False))) if self.DEDUP_STATES else None
        idx, row_env = env.valid_rows(rep)
        out = (idx, row_env, env.valid_segments(), rep)
        env._dqn_rows = (env._cand_version, out)
        if self.TRACK_ROWS:
            seen = env.n_valid[:env.E].sum()
            self._rows_seen_dev = seen if self._rows_seen_dev is None else self._rows_seen_dev + seen
        return out

    @property
    def rows_seen(self):
        return int(self._rows_seen_dev) if self._rows_seen_dev is not None else 0

    def _distinct_rows(self, env, idx, row_env, stable_flag):
        """Candidate rows whose network input is the same tensor, bit for bit: the input of a row is (state raster of its env,
        its candidate raster, the env's stable flag, the task's reward map and obstacle raster), and thousands of environments
        of one task pass through the same early states -- every freshly reset env holds the same state and the same
        candidates.  Rows are keyed by a 64-bit hash of their bit rasters, grouped with torch.unique, and every row is then
        compared WORD FOR WORD with the representative of its group (a hash collision -- probability ~ n^2 / 2^64 -- sends the
        call down the plain path), so feeding only the representatives and copying their outputs is exact.
        An env with per-env tasks: the map and the obstacle raster of a row are its env's, so the words that determine them --
        the int64 bit patterns of env_targets[e], and of env_obstacles[e] on per-env obstacles, the words
        state_groups(task=True) keys on -- are folded into the key and compared as well.
        -> (rep [m]: positions into idx of one row per distinct input, inverse [n]: group of every row) or None."""
        n = idx.numel()
        if not self.DEDUP_ROWS or n < 2:
            return None
        m = self._hash_mult
        if m is None:
            g = torch.Generator().manual_seed(0x5eed5)
            m = self._hash_mult = (torch.randint(-2 ** 62, 2 ** 62, (2, 64), generator=g, dtype=torch.int64) | 1).to(self.device)
        cb = env.cand_bits.index_select(0, idx)                                    # [n, 64] int64
        flag = stable_flag.to(torch.int64)
        hs = (env.state_bits * m[0]).sum(dim=1) + flag * 0x51ED270B27B4F3D           # [E]  (int64 arithmetic wraps)
        task = self._task_words(env)                                                 # [E, w] int64 or None
        if task is not None:
            hs = hs * 0x1E3779B97F4A7C15 + (task * self._task_hash_mult(task.shape[1])).sum(dim=1)
        key = hs.index_select(0, row_env) * 0x2545F4914F6CDD1D + (cb * m[1]).sum(dim=1)
        key = key ^ (key >> 29)
        uniq, inverse = torch.unique(key, return_inverse=True)                      # (one wait: the number of groups)
        n_groups = uniq.numel()
        if n_groups == n:
            return None
        pos = torch.arange(n, device=self.device)
        rep = torch.full((n_groups,), n, dtype=torch.int64, device=self.device).scatter_reduce_(0, inverse, pos, reduce="amin")
        r = rep.index_select(0, inverse)                                             # representative of every row
        renv = row_env.index_select(0, r)
        same = ((cb == cb.index_select(0, r)).all(dim=1)
                & (env.state_bits.index_select(0, row_env) == env.state_bits.index_select(0, renv)).all(dim=1)
                & (flag.index_select(0, row_env) == flag.index_select(0, renv)))
        if task is not None:
            same = same & (task.index_select(0, row_env) == task.index_select(0, renv)).all(dim=1)
        if not bool(same.all()):
            return None
        return rep, inverse

    @staticmethod
    def _task_words(env):
        """[E, 3 T (+ 3 O)] int64: the bit patterns of every env's own targets (and obstacles), None without per-env tasks."""
        if not getattr(env, "per_env_tasks", False):
            return None
        E = env.env_targets.shape[0]
        words = env.env_targets.reshape(E, -1)
        if getattr(env, "per_env_obstacles", False):
            words = torch.cat([words, env.env_obstacles.reshape(E, -1)], dim=1)
        return words.contiguous().view(torch.int64)

    def _task_hash_mult(self, w):
        m = self._task_mult
        if m is None or m.numel() != w:
            g = torch.Generator().manual_seed(0x7a5c)
            m = self._task_mult = (torch.randint(-2 ** 62, 2 ** 62, (w,), generator=g, dtype=torch.int64) | 1).to(self.device)
        return m

    def _forward_rows(self, net, env, idx, row_env, stable_flag, groups=_COMPUTE):
        """net(...) over the candidate rows in chunks of ROW_CHUNK rows; the last chunk is padded with copies of row 0
        (sliced off again), so the convolution / GEMM shapes never change from lock-step to lock-step.  Rows with identical
        inputs are fed once (_distinct_rows).  -> (q [n], successor block features of the DISTINCT rows or None, successor
        binary features of the distinct rows or None, inverse [n] = the distinct row of every row (None: every row is fed)).
        ``groups``: what _distinct_rows returned for these very rows, for a caller that feeds them to two nets (the hashing and
        torch.unique then run once)."""
        if groups is VecDQN._COMPUTE:
            groups = self._distinct_rows(env, idx, row_env, stable_flag)
        inverse = None
        if groups is not None:
            rep, inverse = groups
            idx, row_env = idx.index_select(0, rep), row_env.index_select(0, rep)
        n, C = idx.numel(), self.ROW_CHUNK
        self.rows_fed += n
        pad = (-n) % C
        if pad:
            idx = torch.cat([idx, idx[:1].expand(pad)])
            row_env = torch.cat([row_env, row_env[:1].expand(pad)])
        outs = [net(*self._row_features(env, idx[o:o + C], row_env[o:o + C], stable_flag)) for o in range(0, n + pad, C)]
        q = torch.cat([o[0] for o in outs])[:n]
        sf = torch.cat([o[1] for o in outs])[:n] if outs[0][1] is not None else None
        sb = torch.cat([o[2] for o in outs])[:n] if outs[0][2] is not None else None
        if inverse is not None:
            q = q.index_select(0, inverse)
        return q, sf, sb, inverse

    # ------------------------------------------------------------------ features of the rows a net is fed
    def _row_features(self, env, idx, row_env, stable_flag):
        n = idx.numel()
        if self.task_channels:
            # the conv nets on per-env tasks: all four channels of every row in ONE launch, straight from the bit-packed rasters
            # and the env's maps (bridges_conv_input_rows); the nets get the channel views and stack them back without a copy
            if getattr(env, "per_env_obstacles", False):
                x = ops.conv_input(env.state_bits, env.cand_bits, env.reward_maps, env.env_obstacle_bits, block_row=row_env,
                                   action_row=idx, reward_row=row_env, obstacle_row=row_env)
            else:
                x = ops.conv_input(env.state_bits, env.cand_bits, env.reward_maps, env.obstacle_bits.reshape(1, 64),
                                   block_row=row_env, action_row=idx, reward_row=row_env)
            binary = torch.zeros((n, 6), dtype=torch.float32, device=self.device)
            binary[:, 0] = stable_flag[row_env].float()
            return x[:, 0:1], binary, x[:, 1:2], x[:, 2:3], x[:, 3:4]
        if env.cand_raster is not None:
            block = env.crop(env.state_raster[row_env]).unsqueeze(1)     # crop: no-op for the 64x64 default
            action = env.crop(env.cand_raster[idx]).unsqueeze(1)
        else:                                                            # env without f32 rasters: expand the rows asked for
            block = env.crop(ops.bits_to_f32(env.state_bits[row_env])).unsqueeze(1)
            action = env.crop(ops.bits_to_f32(env.cand_bits[idx])).unsqueeze(1)
        binary = torch.zeros((n, 6), dtype=torch.float32, device=self.device)
        binary[:, 0] = stable_flag[row_env].float()
        reward = env.reward_features.unsqueeze(0).expand(n, -1, -1, -1)
        obstacle = env.obstacle_raster.unsqueeze(0).expand(n, -1, -1, -1)
        return block, binary, action, reward, obstacle

    FACTORED_ACTING = True      # tests set it to False to run the same lock-steps through the plain module forward

    @classmethod
    def _factored(cls, net):
        """Acting through the factored SuccessorMLP forward on bit-packed rasters.  The bit-packed first layer is built for
        64x64 images; other --image_size values (and every other net) act through the module forward on f32 rasters."""
        return (cls.FACTORED_ACTING and hasattr(net, "q_from_first_layer")
                and tuple(getattr(net, "img_size", (64, 64))) == (64, 64))

    @classmethod
    def acting_needs_f32_rasters(cls, net):
        """False when acting reads only the bit-packed rasters of the rollout env: it can then be created with
        f32_rasters=False and its rasteriser skips the 16 KiB-per-candidate expansion."""
        return not cls._factored(net)


    @staticmethod
    def _stable_flags(env):
        """'stable' binary feature of the current state of every env (a freshly reset env is stable)."""
        fresh = env.n_blocks == 0
        return torch.where(fresh, torch.ones_like(fresh), env.step_flags[:, 1].bool())

    @torch.no_grad()
    def _policy_q(self, env, idx, row_env, stable):
        """q of the policy net for the candidate rows ``idx`` of ``env``."""
        return self._net_q(self.policy_net, env, idx, row_env, stable)

    @torch.no_grad()
    def _net_q(self, net, env, idx, row_env, stable, return_h=False, groups=_COMPUTE):
        """q of ``net`` for the candidate rows; with return_h (factored nets only) also the first layer's pre-activation
        of every row, from which the successor features of selected rows follow without a second first-layer pass.
        ``groups`` (nets fed through _forward_rows only): the distinct rows, found by the caller."""
        net.eval()
        if not self._factored(net):
            if env.cand_raster is None and not self.task_channels:
                raise ValueError("this Q-network acts on f32 rasters: create the rollout env with f32_rasters=True")
            return self._forward_rows(net, env, idx, row_env, stable, groups=groups)[0]
        # the first layer consumes the BIT-PACKED rasters (bridges_bits_linear): a raster times a weight slice is the
        # sum of the ~35 weight rows of its set pixels, so neither f32 images nor a [n, 4096] GEMM
        px = 64 * 64
        self.rows_fed += idx.numel()
        W1 = net.first_layer().weight
        if getattr(env, "per_env_tasks", False):
            # every env owns its reward map: the image-independent part of the first layer is a [E, 2, hidden] table (one
            # [E, px] x [px, hidden] product per net and call) indexed by 2 * env + stable, and the head weighs row r with the
            # map of its env (bridges_head_sigmoid_dot_rows / bridges_sigmoid_dot_rows)
            if not self.per_env_tasks:
                raise ValueError("an env with per-env tasks needs VecDQN(per_env_tasks=True)")
            E = env.E
            maps = env.reward_maps.reshape(E, px)
            base_row = 2 * torch.arange(E, device=self.device) + stable.long()
            if getattr(env, "per_env_obstacles", False):
                # every env owns its obstacle raster too: the table leaves the obstacle term out and the env's bit-packed raster
                # selects its rows of W_obst as the second operand of the same launch (bridges_bits_linear2)
                if not self.per_env_obstacles:
                    raise ValueError("an env with per-env obstacles needs VecDQN(per_env_obstacles=True)")
                table = net.first_layer_stable_tables(maps, None).reshape(2 * E, -1)
                base = ops.bits_linear2(env.state_bits, W1[:, :px].T, env.env_obstacle_bits, W1[:, 3 * px:4 * px].T, base=table,
                                        base_row=base_row)
            else:
                table = net.first_layer_stable_tables(maps, env.obstacle_raster.reshape(-1)).reshape(2 * E, -1)
                base = ops.bits_linear(env.state_bits, W1[:, :px].T, base=table, base_row=base_row)
            h_pre = ops.bits_linear(env.cand_bits, W1[:, px:2 * px].T, bits_row=idx, base=base, base_row=row_env)
            q = net.q_from_first_layer(h_pre, maps, head=ops.sigmoid_dot, fused_head=ops.head_sigmoid_dot,
                                       reward_rows=row_env.to(torch.int32))
            return (q, h_pre) if return_h else q
        # the part of the first layer that does not depend on the images: a two-row table indexed by the env's stable flag
        # (the other binary features are 0, as in the reference without pybullet)
        ro = getattr(env, "_reward_obstacle_flat", None)
        if ro is None:
            ro = env._reward_obstacle_flat = torch.cat([env.reward_features.reshape(-1), env.obstacle_raster.reshape(-1)]).contiguous()
        base = ops.bits_linear(env.state_bits, W1[:, :px].T, base=net.first_layer_stable_table(ro), base_row=stable.long())
        h_pre = ops.bits_linear(env.cand_bits, W1[:, px:2 * px].T, bits_row=idx, base=base, base_row=row_env)
        q = net.q_from_first_layer(h_pre, env.reward_features, head=ops.sigmoid_dot, fused_head=ops.head_sigmoid_dot)
        return (q, h_pre) if return_h else q

    @torch.no_grad()
    def td_errors(self, rec):
        """td_error of the transitions just recorded (successor_dqn.py:413-426): |q(s,a) - (reward + 0.95 max_a' q(s',a'))|
        with the policy net as it is now, next value 0 when done; the env holds s' (or a fresh state when done)."""
        env, E = self.env, self.env.E
        done = rec[:, R.O_DONE] > 0.5
        stable = self._stable_flags(env)
        idx, row_env, seg, _rep = self._rows(env, stable)
        next_q = torch.zeros(E, dtype=torch.float32, device=self.device)
        if idx.numel():
            q = self._policy_q(env, idx, row_env, stable)
            zeros = torch.zeros(E, dtype=torch.float32, device=self.device)
            next_q, _, _ = dqn_ops.td_target(seg, q.contiguous().float(), zeros, done | (env.n_valid[:E] == 0), 1.0)   # segmented max
        expected = rec[:, R.O_REWARD].float() + 0.95 * next_q                      # hard-coded 0.95 (successor_dqn.py:425)
        return (self._q_sel - expected).abs()

    # ------------------------------------------------------------------ one lock-step of acting
    @torch.no_grad()
    def act(self, greedy=False):
        rec, valid, self._q_sel = self._act_on(self.env, self.step_images, self.explore_gen, self.epsilon, greedy)
        return rec, valid

    @torch.no_grad()
    def _act_on(self, env, step_images, explore_gen, epsilon, greedy):
        """One lock-step of acting on ``env``: epsilon-greedy choice (exploring envs draw from ``explore_gen`` and take the
        candidate that overlaps least with the count images ``step_images`` [K + 1, S, S], which get the explored rasters
        added; exploration="boltzmann": a draw from softmax(q / temperature) per env, ``epsilon`` and the count images unused),
        records, env.step.  -> (rec [E, W], valid [E], q of the chosen rows [E])."""
        E = env.E
        stable = self._stable_flags(env)
        idx, row_env, seg, rep = self._rows(env, stable)
        q_sel = torch.zeros(E, dtype=torch.float32, device=self.device)
        if idx.numel() and self.exploration == "boltzmann":
            # every env draws its row from softmax(q / temperature) with its own uniform, in ONE launch (bridges_boltzmann_select;
            # greedy: the first maximum, as below); no overlap with the count images is computed and none is added to them.  Envs
            # in the same state still share their representative's rows, but stop acting alike sooner than under a greedy choice
            q = self._policy_q(env, idx, row_env, stable)
            u = torch.rand(E, generator=explore_gen, device=self.device)
            if self.temp_relative:                      # (the same launch grid; the effective temperatures are one more result)
                sel_compact, sel_index, q_sel, self._ex_w, _p, self._temp_out = ops.boltzmann_select(
                    seg, q, u, self.temperature, greedy, idx, env.cand_offset[:E], rep=rep, relative=True, spread_floor=self.spread_floor)
            else:
                sel_compact, sel_index, q_sel, self._ex_w, _p = ops.boltzmann_select(seg, q, u, self.temperature, greedy, idx,
                                                                                     env.cand_offset[:E], rep=rep)
        elif idx.numel():
            step_of_row = env.n_blocks[row_env].long()
            q = self._policy_q(env, idx, row_env, stable)
            if self._factored(self.policy_net) or self.task_channels:
                # overlap of every candidate with the count image of its episode step, straight from the bit-packed
                # rasters (exact: integer-valued sums)
                join = ops.bits_dot(env.cand_bits, step_images, step_of_row, bits_row=idx)
            else:
                join = (step_images[step_of_row] * env.crop(env.cand_raster[idx])).sum(dim=(1, 2))
            # greedy row = first maximum of q, exploring row = first minimum of the overlap, per env, in ONE launch
            # (bridges_eps_greedy_select; an `if explore.any()` here would make the host wait for the Q pass it has just queued)
            u = torch.rand(E, generator=explore_gen, device=self.device)
            sel_compact, sel_index, q_sel, ex_w = ops.eps_greedy_select(seg, q, join, u, epsilon, greedy, idx, env.cand_offset[:E],
                                                                        rep=rep)
            # count images of the explored choices; every env takes part with weight 0 or 1, so no host decision
            step_of_env = env.n_blocks.long()
            if env.img == 64:                                     # the set pixels of the chosen rasters, by float atomics
                ops.bits_accumulate_(step_images, env.cand_bits, step_of_env, weight=ex_w, bits_row=sel_compact)
            else:
                picked = env.crop(ops.bits_to_f32(env.cand_bits[sel_compact])) * ex_w[:, None, None]
                step_images.index_add_(0, step_of_env, picked)
        else:
            sel_compact = torch.zeros(E, dtype=torch.long, device=self.device)
            sel_index = (sel_compact - env.cand_offset[:E].long()).clamp(min=0).to(torch.int32)
            self._ex_w = None                                     # (Boltzmann: no env drew anything)
        # the record of the lock-step in two launches around the step (bridges_record_state / _result); the torch formulation
        # R.snapshot + R.make_records (~35 launches) is what tests/test_gpu_vec_dqn.py compares them with
        rec = R.pack_state(env, sel_compact)
        if getattr(env, "per_env_tasks", False):
            # the task the transition is taken under: the step that ends an episode redraws the env's targets (task_tail)
            env._task_tail = (torch.cat([env.env_targets.reshape(E, -1), env.env_obstacles.reshape(E, -1)], dim=1)
                              if self.per_env_obstacles else env.env_targets.reshape(E, -1).clone())
        if getattr(env, "task_family", None) is not None:
            env._task_class = env.task_class.clone()            # likewise the class: the step that ends an episode redraws it
        if self.hindsight is not None and env is self.env:
            env._task_episode = env.task_episode.clone()        # and the episode counter, which keys the hindsight draw
        env.step(sel_index)
        valid = R.pack_result(env, rec)
        return rec, valid, q_sel

    def with_task(self, rec, env=None):
        """The records of the last act() on ``env`` (default: the rollout env) in the width the ring stores: on per-env tasks
        the RECORD_WIDTH columns followed by the env's targets as they were BEFORE the step (one device copy; the record
        kernels, the episode statistics and td_errors address rows of RECORD_WIDTH doubles and see ``rec`` as it is).  Per-env
        obstacles: the targets are followed by the env's obstacles, as they were before the step as well."""
        if not self.per_env_tasks:
            return rec
        return torch.cat([rec, (env or self.env)._task_tail], dim=1)

    # ------------------------------------------------------------------ greedy evaluation (successor_dqn.py:749-781)
    @torch.no_grad()
    def evaluate(self, eval_env, epsilon=0.0):
        """One episode in every env of ``eval_env`` (a VecAssemblyGym of the training task) under the current policy net: greedy
        (the first maximum of q) for epsilon == 0, else the training rule with the evaluation's own count images and random
        stream.  Runs exactly eval_env.K lock-steps -- every episode ends by truncation at K at the latest -- and reads the
        statistics back once.  Touches no training state (rollout env, count images, ring, random streams, epsilon, counters).
        -> log_episode's keys as means over the N = eval_env.E episodes, plus success_rate and episodes; on a task-family env
        (RandomBridges) also success_by_class and episodes_by_class, lists indexed by the drawn n = 0..hi.
        Per-env tasks: reset() sets task_episode to 0, so every evaluation runs on the SAME eval_env.E tasks -- the draws of
        (the eval env's seed, env, episode 0): a fixed held-out task set, not fresh tasks per evaluation."""
        if eval_env is self.env:
            raise ValueError("evaluate() needs an env of its own: the training env's episodes would be cut short")
        if float(epsilon) > 0.0 and self.exploration == "boltzmann":
            raise ValueError("evaluate(epsilon > 0) explores with the epsilon-greedy rule on count images; an agent built with "
                             "exploration='boltzmann' evaluates greedily only (epsilon=0)")
        if bool(getattr(eval_env, "stable_actions_only", False)) != self.stable_actions_only:
            raise ValueError("the evaluation env's stable_actions_only must match the training env's")
        if bool(getattr(eval_env, "per_env_tasks", False)) != self.per_env_tasks:
            raise ValueError("the evaluation env must have per-env tasks exactly when the agent was built with per_env_tasks=True")
        if bool(getattr(eval_env, "per_env_obstacles", False)) != self.per_env_obstacles:
            raise ValueError("the evaluation env must have per-env obstacles exactly when the agent was built with "
                             "per_env_obstacles=True")
        n_classes = self._n_classes(eval_env)
        key = (eval_env.E, eval_env.K, eval_env.n_targets, n_classes)
        st = self._eval_state.get(key)
        if st is None:
            gen = torch.Generator(device=self.device).manual_seed(0xE7A1 + self.seed * 1000 + self.rank)
            stats = EpisodeStats(eval_env.E, eval_env.K, self.gamma, eval_env.n_targets, self.device, count_first_only=True,
                                 across_ranks=False, n_classes=n_classes)
            images = torch.zeros((eval_env.K + 1, eval_env.img, eval_env.img), dtype=torch.float32, device=self.device)
            st = self._eval_state[key] = (gen, stats, images)
        gen, stats, images = st
        stats.reset()
        images.zero_()
        eval_env.reset()
        epsilon = float(epsilon)
        for _ in range(eval_env.K):
            rec, valid, _q = self._act_on(eval_env, images, gen, epsilon, epsilon <= 0.0)
            stats.fold(rec, valid, cls=eval_env._task_class if n_classes > 1 else None)
        vals = stats.take().get()                                  # the one wait of the evaluation
        if vals["episodes"] != eval_env.E:
            raise RuntimeError(f"evaluation: {vals['episodes']} of {eval_env.E} episodes ended within {eval_env.K} lock-steps "
                               "(an env whose fresh state has no valid candidate never starts one)")
        out = dict(reward=vals["reward"], lin_reward=vals["lin_reward"], avg_loss=None, num_steps=vals["num_steps"],
                   stable=vals["stable"], collision=0.0, success_rate=vals["success_rate"], episodes=vals["episodes"])
        if n_classes > 1:                                          # a task family: per span / height n = 0..hi
            out["success_by_class"] = [c["success_rate"] for c in vals["by_class"]]
            out["episodes_by_class"] = [c["episodes"] for c in vals["by_class"]]
        return out

    # ------------------------------------------------------------------ beam-search evaluation
    @torch.no_grad()
    def beam_search(self, beam_env, width, merge=False, on_depth=None, trace=False, trace_n_step=1, trace_priority=0.0):
        """Beam search of width B = ``width`` over every task of ``beam_env`` (beam_env_like(eval_env, B): M * B envs, the B envs
        of a group share one task), the policy net's q as the heuristic: how much the learned Q is worth when the simulator is
        allowed to look ahead.  Per depth, for all groups at once and without a host decision: the candidate rows and their q
        through the paths acting uses (_rows, _policy_q); bridges_beam_select keeps the B candidates of every group with the
        best  return so far + discount * q  ("Beam search"); beam_env.fork(src) makes slot i continue from
        the env that owns its candidate; beam_env.step places it; the returns are advanced in float64 on the device
        (ret += disc * lin_reward, disc *= gamma).  A live beam whose step ends its episode (done, or no next action) is held
        against its group's best finished beam -- success (reward == n_targets, evaluate()'s statistic) first, then the higher
        return, then the earlier depth, then the lower slot -- and dies; a dead slot spends its lock-steps resetting.  Runs
        beam_env.K depths and reads the results back once; per depth the host waits only where acting waits (the row count of
        valid_rows).  Touches no training state.  width = 1 is the greedy episode of evaluate().
        merge: after a depth's finished beams are recorded and closed, one bridges_beam_merge launch closes every live beam that
        holds the same structure as another live beam of its group with a return at least as high -- the same multiset of blocks,
        the same targets_left and the same last block (key_last = 1: the frozen block, on which the candidate set can depend), so
        "same key, same future" holds and the next depth's select refills the group from the survivors' candidates.  merge=False
        launches nothing of it.  on_depth(d, live): called after depth d's bookkeeping with the live flags (uint8 [E], on the
        device) -- for tests and tools, which read the env's state then; None costs nothing.
        -> evaluate()'s keys as means over the M tasks (success_rate, reward, lin_reward, num_steps, episodes; reward and
        lin_reward are the best beam's discounted sums, in float64), beam_width, and structures: per task a dict of the best
        beam's placed blocks (shape ids, poses (x, z, cos, sin)), its actions (the candidate index placed at every depth),
        success, reward, lin_reward, num_steps and final_reward, and merged_beams: per task the beams that merging closed over the
        search (zeros without merge); with merge also merged_by_depth and live_by_depth: per depth, over all tasks, the beams
        closed and the live beams the merge looked at.  On a beam env of a task family also success_by_class and episodes_by_class, indexed by the
        class n = 0..hi of every task.
        trace: the transition records of every task's best beam as rows a replay ring stores ("Search in
        training").  Per depth the record of the step is taken with the two launches acting uses (R.pack_state after the fork
        and before the step, R.pack_result after it) into slice d of a [K, E, RECORD_WIDTH] buffer kept per (E, K), beside the
        depth's src and live & step_flags[0]; where ``best`` is updated, so are the env and depth its episode ended in; after the
        last depth ONE bridges_beam_trace call walks every best beam back through the slots it occupied and writes its episode
        as ``trace_n_step``-step rows (the record of the horizon's last step, the start's stable flag, the h-step return, the
        task tail with_task joins on, and h when trace_n_step > 1) with ``trace_priority`` in O_TD.  The result gains trace_rows
        (device, [trace_count, W_out]), trace_count (host: the sum of num_steps, from the read-back the search makes anyway),
        trace_offset, trace_status and trace_end_env (device: row offsets per task, 1 where a chain was broken -- never, by
        construction --, the env every task's best episode ended in).
        Tracing adds no host wait.  trace=False launches nothing of it and returns what the search always returned."""
        def select(d, seg, q, live, ret, disc, idx, cand_offset, rep):
            return ops.beam_select(seg, q, int(width), live, ret, disc, idx, cand_offset, rep=rep)
        return self._depth_search("beam_search", beam_env, width, select, merge, on_depth, trace, trace_n_step, trace_priority)

    @torch.no_grad()
    def particle_search(self, beam_env, width, temperature, resample_temperature=None, elite=True, merge=False, on_depth=None,
                        trace=False, trace_n_step=1, trace_priority=0.0, generator=None):
        """Best-of-N rollouts with resampling over every task of ``beam_env``: beam_search's depth loop with the select swapped for
        bridges_particle_select ("Particle search").  Per depth every slot of a group takes a parent among
        the group's live envs by systematic resampling over exp((ret + disc * max q) / ``resample_temperature``) (None: the
        ``temperature``; inf: no particle moves -- B independent rollouts, the best-of-N control) and places one of the parent's
        candidates drawn from the Boltzmann policy at ``temperature``; ``elite``: slot 0 follows the best parent's best
        candidate instead.  The uniforms come per depth from ``generator`` (None: self.search_gen, a stream of the search's own
        seeded from the agent's seed, so neither the replay draw nor exploration moves).  Everything else -- fork, step, the
        float64 returns, the best finished beam, merge, trace -- is beam_search's, and so are the arguments and the result, which
        gains particles (= width), ess_by_depth (per depth the mean effective sample size over the groups that had parents) and
        p_sel_mean_by_depth (the mean probability of the drawn candidates over the filled slots), read back with the rest.
        No host wait is added per depth."""
        import math
        T = float(temperature)
        Tr = T if resample_temperature is None else float(resample_temperature)
        if not (math.isfinite(T) and T > 0.0):
            raise ValueError(f"particle_search(temperature={temperature!r}): finite and > 0")
        if not Tr > 0.0:                                     # (a NaN fails the comparison; inf passes)
            raise ValueError(f"particle_search(resample_temperature={resample_temperature!r}): > 0 (inf: no resampling)")
        gen = self._search_generator() if generator is None else generator
        K, dev = beam_env.K, self.device
        stats = torch.zeros(2 * K, dtype=torch.float64, device=dev)      # per depth: mean ess, mean p_sel

        def select(d, seg, q, live, ret, disc, idx, cand_offset, rep):
            E = live.numel()
            u_act = torch.rand(E, generator=gen, device=dev)
            u_res = torch.rand(E // int(width), generator=gen, device=dev)
            sel = ops.particle_select(seg, q.float().contiguous(), int(width), live, ret, disc, idx.contiguous(), cand_offset.contiguous(),
                                      u_act, u_res, T, Tr, elite=elite, rep=rep)
            ess, filled = sel["ess"], sel["live"].double()
            stats[d] = ess.sum() / (ess > 0).sum().clamp(min=1)
            stats[K + d] = (sel["p_sel"].double() * filled).sum() / filled.sum().clamp(min=1)
            return sel
        out = self._depth_search("particle_search", beam_env, width, select, merge, on_depth, trace, trace_n_step, trace_priority,
                                 stats=stats)
        st, n = out.pop("depth_stats"), out.pop("depths")
        out.update(particles=int(width), ess_by_depth=st[:n], p_sel_mean_by_depth=st[K:K + n])
        return out

    def _search_generator(self):
        """The random stream of particle_search: made by the first search that needs it, seeded from the agent's seed."""
        if self.search_gen is None:
            self.search_gen = torch.Generator(device=self.device).manual_seed(SEARCH_SEED + int(self.seed))
        return self.search_gen

    def _depth_search(self, what, beam_env, width, select, merge, on_depth, trace, trace_n_step, trace_priority, stats=None):
        """The depth loop of beam_search and particle_search (``what`` names the caller in messages): select(d, seg, q, live, ret,
        disc, idx, cand_offset, rep) -> the dict of ops.beam_select chooses every slot's parent and candidate; ``stats``: a
        float64 vector on the device that rides with the one read-back (-> depth_stats, beside depths: the depths that ran)."""
        B, env = int(width), beam_env
        if env is self.env:
            raise ValueError(f"{what}() needs an env of its own: the training env's episodes would be cut short")
        if not 1 <= B <= abi.BEAM_MAX_WIDTH:
            raise ValueError(f"{what}(width={width!r}): 1..{abi.BEAM_MAX_WIDTH}")
        if not isinstance(env, VecAssemblyGym) or env.E % B != 0:
            raise ValueError(f"{what}(width={B}) needs a VecAssemblyGym of M * {B} envs (beam_env_like(eval_env, {B}))")
        if env.random_targets is not None or env.random_obstacles is not None or env.task_family is not None:
            raise ValueError(f"{what}(): the beam env draws tasks per episode, so the envs of a group would not share one; build "
                             "it with beam_env_like(eval_env, width)")
        if bool(env.stable_actions_only) != self.stable_actions_only:
            raise ValueError("the beam env's stable_actions_only must match the training env's")
        if bool(env.per_env_tasks) != self.per_env_tasks or bool(env.per_env_obstacles) != self.per_env_obstacles:
            raise ValueError("the beam env must have per-env tasks / obstacles exactly when the agent was built with them")
        E, K, dev = env.E, env.K, self.device
        M = E // B
        if merge and K > abi.BEAM_MAX_SLOTS:
            raise ValueError(f"{what}(merge=True): bridges_beam_merge orders at most {abi.BEAM_MAX_SLOTS} block slots per env, "
                             f"the beam env has {K}")
        if trace:
            if K > R.K:
                raise ValueError(f"{what}(trace=True): a record holds {R.K} block slots, the beam env has {K}")
            if not 1 <= int(trace_n_step) <= abi.NSTEP_MAX:
                raise ValueError(f"{what}(trace_n_step={trace_n_step!r}): 1..{abi.NSTEP_MAX}")
            tr_rec, tr_valid, tr_parent = self._trace_buffers(E, K)
            # the task every record of a group is taken under: explicit arrays that no episode of a beam env redraws
            tr_tail = None
            if self.per_env_tasks:
                tr_tail = (torch.cat([env.env_targets.reshape(E, -1), env.env_obstacles.reshape(E, -1)], dim=1)
                           if self.per_env_obstacles else env.env_targets.reshape(E, -1))
        # per task and depth: the beams merging closed, then the live beams it looked at
        merged = torch.zeros((M, 2 * K), dtype=torch.int32, device=dev) if merge else None
        slots = torch.arange(E, device=dev) % B
        first = torch.arange(M, device=dev) * B
        live = (slots == 0).to(torch.uint8)                  # only slot 0 of every group is open
        ret = torch.zeros(E, dtype=torch.float64, device=dev)       # discounted lin_reward so far: what the search scores
        ret_r = torch.zeros(E, dtype=torch.float64, device=dev)     # discounted reward so far: what evaluate() reports
        disc = torch.ones(E, dtype=torch.float64, device=dev)
        hist = torch.zeros((E, K, 6), dtype=torch.float64, device=dev)    # per depth: shape id, pose[4], candidate index
        # per group: has, success, lin return, reward return, steps, final reward, then the beam's history
        best = torch.zeros((M, 6 + 6 * K), dtype=torch.float64, device=dev)
        one, ninf = torch.ones(M, dtype=torch.float64, device=dev), torch.full((), -float("inf"), dtype=torch.float64, device=dev)
        if trace:                                            # per task: where the episode of ``best`` ended
            end_env, end_depth = first.to(torch.int32), torch.full((M,), -1, dtype=torch.int32, device=dev)
        env.reset()
        depths = 0
        for d in range(K):
            stable = self._stable_flags(env)
            idx, row_env, seg, rep = self._rows(env, stable)
            if not idx.numel():                              # no env holds a valid candidate: every beam is closed
                break
            q = self._policy_q(env, idx, row_env, stable)
            sel = select(d, seg, q, live, ret, disc, idx, env.cand_offset[:E], rep)
            src, sc = sel["src"].long(), sel["sel_compact"]
            placed = torch.cat([env.cand_desc[sc, 2:3].double(), env.cand_pose[sc], sel["sel_index"].double().unsqueeze(1)], dim=1)
            ret, ret_r, disc, hist = ret[src], ret_r[src], disc[src], hist[src]
            hist[:, d] = placed
            live = sel["live"].bool()
            env.fork(sel["src"])
            env.needs_reset.masked_fill_(~live, 1)           # a closed slot places nothing: its lock-step is a reset
            if trace:
                # (sel_compact indexes the candidate arrays of BEFORE the fork; the fork's refresh has laid them out anew)
                R.pack_state(env, env.cand_offset[:E].long() + sel["sel_index"].long(), out=tr_rec[d])
            env.step(sel["sel_index"])
            f = env.step_flags
            live &= f[:, 0].bool()
            if trace:
                R.pack_result(env, tr_rec[d])
                tr_parent[d].copy_(sel["src"])
                tr_valid[d].copy_(live)
            lin, rew = env.lin_reward.double(), env.reward.double()
            ret = torch.where(live, ret + disc * lin, ret)   # two roundings each, as the score of bridges_beam_select
            ret_r = torch.where(live, ret_r + disc * rew, ret_r)
            disc = disc * self.gamma
            fin = live & (f[:, 5].bool() | f[:, 6].bool())   # done | no next action: the episode's last record (REC_DONE)
            succ = fin & (env.reward == float(env.n_targets))
            fin_g, succ_g, ret_g = fin.view(M, B), succ.view(M, B), ret.view(M, B)
            elig = fin_g & (succ_g | ~succ_g.any(dim=1, keepdim=True))
            top = torch.where(elig, ret_g, ninf).max(dim=1, keepdim=True).values
            pick_slot = torch.where(elig & (ret_g == top), slots.view(M, B), B).min(dim=1).values      # B: nothing finished
            has_new = pick_slot < B
            pick = first + pick_slot.clamp(max=B - 1)
            new = torch.cat([torch.stack([one, succ[pick].double(), ret[pick], ret_r[pick], one * (d + 1), rew[pick]], dim=1),
                             hist[pick].reshape(M, -1)], dim=1)
            better = has_new & ((best[:, 0] == 0) | (new[:, 1] > best[:, 1]) | ((new[:, 1] == best[:, 1]) & (new[:, 2] > best[:, 2])))
            best = torch.where(better.unsqueeze(1), new, best)
            if trace:
                end_env = torch.where(better, pick.to(torch.int32), end_env)
                end_depth = torch.where(better, d, end_depth)
            live = (live & ~fin).to(torch.uint8)
            if merge:                                        # beams that hold the same structure: the best return stays open
                mg = ops.beam_merge(env.n_blocks, env.blk_shape, env.blk_pose, env.blk_occ, env.targets_left, B, live, ret, key_last=True)
                merged[:, d], merged[:, K + d] = mg["n_merged"], live.view(M, B).sum(dim=1)
                live = mg["live"]
            if on_depth is not None:
                on_depth(d, live)
            depths = d + 1
        if trace:                                            # (depths a search that broke off early left unwritten lie beyond every end)
            tr = ops.beam_trace(tr_rec, tr_valid, tr_parent, end_env, end_depth, B, self.gamma, n_step=int(trace_n_step), tail=tr_tail,
                                priority=float(trace_priority))
        # the one wait of the search (with merge: the merged counts ride along as further columns)
        cols = [best] + ([merged.double()] if merge else []) + ([stats.unsqueeze(0).expand(M, -1)] if stats is not None else [])
        host = (torch.cat(cols, dim=1) if len(cols) > 1 else best).cpu()
        if int(host[:, 0].sum()) != M:
            raise RuntimeError(f"{what.replace('_', ' ')}: {int(host[:, 0].sum())} of {M} tasks ended an episode within {K} depths "
                               "(a task whose fresh state has no valid candidate never starts one)")
        succ_h, steps_h = host[:, 1].tolist(), [int(v) for v in host[:, 4].tolist()]
        hist_h = host[:, 6:6 + 6 * K].reshape(M, K, 6)
        structures = []
        for m in range(M):
            n = steps_h[m]
            structures.append(dict(shape=[int(v) for v in hist_h[m, :n, 0].tolist()], pose=hist_h[m, :n, 1:5].tolist(),
                                   actions=[int(v) for v in hist_h[m, :n, 5].tolist()], success=bool(succ_h[m]),
                                   lin_reward=float(host[m, 2]), reward=float(host[m, 3]), num_steps=n, final_reward=float(host[m, 5])))
        out = dict(reward=float(host[:, 3].mean()), lin_reward=float(host[:, 2].mean()), avg_loss=None,
                   num_steps=float(host[:, 4].mean()), success_rate=float(host[:, 1].mean()), episodes=M, beam_width=B,
                   structures=structures, merged_beams=[0] * M)
        if merge:
            counts = host[:, 6 + 6 * K:6 + 8 * K].long()
            out.update(merged_beams=counts[:, :K].sum(dim=1).tolist(), merged_by_depth=counts[:, :K].sum(dim=0).tolist(),
                       live_by_depth=counts[:, K:].sum(dim=0).tolist())
        if trace:
            n_rows = sum(steps_h)
            out.update(trace_rows=tr["rows"][:n_rows], trace_count=n_rows, trace_offset=tr["offset"], trace_status=tr["status"],
                       trace_end_env=end_env)
        if stats is not None:
            out.update(depth_stats=host[0, host.shape[1] - stats.numel():].tolist(), depths=depths)
        classes = getattr(env, "beam_task_class", None)
        if classes is not None:                              # the tasks of a family: per span / height n = 0..hi
            n_classes = env.beam_n_classes
            per = [[s for s, c in zip(succ_h, classes) if c == n] for n in range(n_classes)]
            out["success_by_class"] = [sum(p) / len(p) if p else None for p in per]
            out["episodes_by_class"] = [len(p) for p in per]
        return out

    def _trace_buffers(self, E, K):
        """beam_search(trace=True): what a search keeps per depth -- records [K, E, RECORD_WIDTH], valid uint8 [K, E], parent
        int32 [K, E] -- made once per (E, K) and kept, like _eval_state."""
        kept = self.__dict__.setdefault("_trace_state", {})
        st = kept.get((E, K))
        if st is None:
            st = kept[(E, K)] = (torch.zeros((K, E, R.RECORD_WIDTH), dtype=torch.float64, device=self.device),
                                              torch.zeros((K, E), dtype=torch.uint8, device=self.device),
                                              torch.zeros((K, E), dtype=torch.int32, device=self.device))
        return st

    # ------------------------------------------------------------------ gradient steps on sampled batches
    def _make_replay_env(self, n_states):
        """A scratch env of n_states envs of the rollout env's task; on per-env tasks with per-env targets of its own (zeros
        until _targets writes the sampled records' tasks into them); on per-env obstacles with explicit per-env obstacles too."""
        env = self.env
        targets = (torch.zeros((n_states, env.n_targets, 3), dtype=torch.float64) if self.per_env_tasks else env.targets)
        obstacles = (torch.zeros((n_states, env.n_obstacles, 3), dtype=torch.float64) if self.per_env_obstacles else env.obstacles)
        return VecAssemblyGym(n_states, env.shapes, obstacles, targets, max_steps=env.max_steps,
                              mu=env.mu, density=env.density, bounds=env.bounds, xlim=env.xlim,
                              ylim=env.ylim, x_discr_ground=env.x_discr_ground,
                              offset_values=env.offset_values, device=self.device, a_max=env.a_max,
                              img_size=(env.img, env.img), f32_rasters=self._replay_f32(),
                              stable_actions_only=self.stable_actions_only)

    def _replay_env(self, n_states):
        """Scratch env that rebuilds the states / candidate sets of sampled transitions (grown on demand)."""
        if self.replay_env.E < n_states:
            self.replay_env = self._make_replay_env(n_states)
        return self.replay_env

    def _replay_env_s(self, n_states):
        """The scratch env of the states s (Munchausen targets), grown as _replay_env grows its own."""
        if self.replay_env_s.E < n_states:
            self.replay_env_s = self._make_replay_env(n_states)
        return self.replay_env_s

    def _replay_f32(self):
        """The scratch env writes f32 rasters of every raw candidate only for nets that consume them row by row; the
        factored MLP reads the bit rasters and expands the few rows it needs (the arg-max row of each transition)."""
        return not (self._factored(self.target_net) or self.task_channels)

    @torch.no_grad()
    def _targets(self, rec):
        """Inputs and TD targets of the transitions in ``rec`` (train_policy_net, successor_dqn.py:178-213).  The
        target net is constant during one train_policy_net call (it is only updated afterwards, :704-708), so the
        targets of all its n_steps batches can be computed in one pass: one state rebuild, one candidate refresh,
        one target-net forward and one k_td_target launch for n_steps * batch_size transitions.
        double_q: a second forward, the policy net's as it stands now, over the same rows behind the first, and the target launch
        selects every transition's row by its q (k_td_target_select); the conv nets' distinct rows are found once for both.
        Per-env tasks: the records' tails (their targets) go to the scratch env first, which rebuilds every transition's reward
        map from them (bridges_env_load_targets; envs beyond n repeat record 0's task, as their states do).
        Per-env obstacles: the tails' obstacles go in beside the targets (load_task: one bridges_env_load_targets), so the
        rasteriser filters every next state's candidates against its transition's own obstacles.
        task_channels: the target net's rows come from _row_features on the scratch env (one ops.conv_input per chunk) and no
        f32 image of a transition is built.
        target_temperature: the bootstrap is the expectation under the Boltzmann policy of the rows' q (double_q: of the policy
        net's q) instead of the arg-max row's -- bridges_soft_expect over the segments, then the target kernel on one-row
        segments; the factored net's middle layers then run over ALL next-state rows and its psi' head over their weighted mean.
        -> a TargetBatch (the fields are listed there) of views: valid until the next call."""
        n = rec.shape[0]
        renv = self._replay_env(n)
        E = renv.E
        munch = self.munchausen
        renv_s = self._replay_env_s(n) if munch is not None else None
        assert renv_s is None or renv_s.E == E
        horizon = None
        if self.n_step > 1:                                  # an h-step row: the record of the window's last step, then its tail, then h
            if rec.shape[1] != self.ring.width:
                raise ValueError(f"n-step returns: records of {self.ring.width} columns expected, got {rec.shape[1]}")
            horizon, rec = rec[:, -1], rec[:, :-1]
        if self.per_env_tasks:
            if rec.shape[1] != R.RECORD_WIDTH + self.task_width:
                raise ValueError(f"per-env tasks: records of {R.RECORD_WIDTH + self.task_width} columns expected, got {rec.shape[1]}")
            tail = rec[:, R.RECORD_WIDTH:]
            tail = tail if n == E else torch.cat([tail, tail[:1].expand(E - n, -1)])
            for task_env in (renv,) if renv_s is None else (renv, renv_s):
                if self.per_env_obstacles:
                    nt = 3 * self.n_task_targets
                    task_env.load_task(tail[:, :nt].contiguous(), tail[:, nt:].contiguous())
                else:
                    task_env.load_targets(tail)
            rec = rec[:, :R.RECORD_WIDTH]
        # state s' (= s + action block): candidates, masks, rasters by the same kernels as the rollout; s is the
        # prefix of its block list, so its raster comes out of the same per-block bit rasters.  One launch unpacks the
        # records into the scratch env (envs beyond n repeat record 0 and are sliced off below); R.unpack_states +
        # load_states + prefix_state_bits is the torch formulation the tests compare it with.
        bits_s, lin, stable_s, done_rec, stable_n = renv.load_records(rec.contiguous())
        use_sf = 'mse_block_features' in self.loss_parts
        discount = sf_action = None
        if horizon is None:
            action_bits = renv.state_bits & ~bits_s                                           # s' minus s = the new block
        else:
            # the scratch env holds s_{t+h} and G came out as lin, the start's stable flag as stable_s; the start state s_t is the
            # first O_NB - (h - 1) blocks of the row's block list, a_t the block after them, and the successor-feature target
            # takes the discounted sum of the h blocks placed since (bridges_bits_discounted_sum) in place of a_t's raster
            h = horizon.to(torch.int32)
            nb_t = rec[:, R.O_NB].to(torch.int32) - (h - 1)
            if n < E:                                        # envs beyond n repeat record 0, as load_records loads them
                h, nb_t = torch.cat([h, h[:1].expand(E - n)]), torch.cat([nb_t, nb_t[:1].expand(E - n)])
            bits_s = renv.prefix_state_bits(nb_t)
            action_bits = renv.prefix_state_bits(nb_t + 1) & ~bits_s
            first = torch.arange(E, dtype=torch.int64, device=self.device) * renv.K + nb_t
            asum, discount = ops.bits_discounted_sum(renv._keep[0], first, h, self.gamma, want_sum=use_sf)
            sf_action = renv.crop(asum).unsqueeze(1) if use_sf else None
        block_f = None if self.task_channels else renv.crop(ops.bits_to_f32(bits_s)).unsqueeze(1)
        # (task_channels: the action raster as f32 only where the successor-feature target adds it)
        action_f = (renv.crop(ops.bits_to_f32(action_bits)).unsqueeze(1)
                    if ((use_sf and horizon is None) or not self.task_channels) else None)
        if horizon is None:
            sf_action = action_f
        stable_n = stable_n.bool()
        idx, row_env, seg, _rep = self._rows(renv, stable_n)      # transitions with the same next state share its rows
        done = done_rec.bool() | (renv.n_valid[:E] == 0)
        select_q, double_q = None, self.double_q
        soft = self.target_temperature is not None
        soft_feat = soft_row = soft_head = None
        self._soft_stats, self._soft_names = None, ()
        if idx.numel() and self._factored(self.target_net):
            # q of every next candidate through the factored forward on the bit-packed rasters; the 8204-wide output
            # (successor features) is only needed for the arg-max row of each transition: its channel 0 from the first-layer
            # pre-activations already at hand
            nq, h_pre = self._net_q(self.target_net, renv, idx, row_env, stable_n, return_h=True)
            nsf0 = lambda best: self.target_net.sf0_from_first_layer(h_pre.index_select(0, best)).contiguous()
            if double_q:                                # (h_pre stays the target net's: the selected row's psi' is its)
                select_q = self._net_q(self.policy_net, renv, idx, row_env, stable_n)
            if soft and use_sf:
                # the psi' head is linear in the last hidden activation, so its expectation is the head of the expected hidden
                # row: the middle layers over ALL next-state rows, the head GEMM over E rows as ever
                lin_layers = [m for m in self.target_net.mlp.layers if isinstance(m, torch.nn.Linear)]
                px = self.target_net.img_size[0] * self.target_net.img_size[1]
                soft_feat = self.target_net._middle_layers(h_pre, lin_layers)
                soft_head = lambda mean: torch.addmm(lin_layers[-1].bias[:px], mean, lin_layers[-1].weight[:px].T)
        elif idx.numel():
            groups = self._distinct_rows(renv, idx, row_env, stable_n)
            nq, nsf, _, inverse = self._forward_rows(self.target_net, renv, idx, row_env, stable_n, groups=groups)
            if double_q:
                select_q = self._net_q(self.policy_net, renv, idx, row_env, stable_n, groups=groups)
            if use_sf and nsf is None:
                raise ValueError("No successor block features available from the chosen policy net.")
            # (nsf holds the DISTINCT rows' outputs)
            nsf0 = lambda best: nsf[:, 0].index_select(0, best if inverse is None else inverse.index_select(0, best)).reshape(E, -1).contiguous()
            if soft and use_sf:                         # channel 0 of the distinct rows' outputs; row j stands at inverse[j]
                soft_feat, soft_row = nsf[:, 0].reshape(nsf.shape[0], -1), inverse
        relative = dict(relative=True, spread_floor=self.spread_floor) if self.target_temp_relative else {}
        cur = {}
        if munch is not None:
            # Munchausen targets: the states s in the second scratch env, the target net's q over their candidates, and the row
            # of each that holds the action its record took
            rec_s = rec.contiguous()
            rec_s = rec_s if n == E else torch.cat([rec_s, rec_s[:1].expand(E - n, -1)])     # envs beyond n repeat record 0
            renv_s.load_records(rec_s, prev=True)
            flag_s = stable_s.bool()
            idx_s, row_env_s, seg_s, _ = self._rows(renv_s, flag_s)                  # transitions taken in the same state share rows
            cur_q = (self._net_q(self.target_net, renv_s, idx_s, row_env_s, flag_s).contiguous().float() if idx_s.numel()
                     else torch.zeros(1, dtype=torch.float32, device=self.device))
            taken = (dqn_ops.action_row(renv_s, seg_s, idx_s, rec_s) if idx_s.numel()
                     else torch.full((E,), 0x7fffffff, dtype=torch.int32, device=self.device))
            cur = dict(munchausen=munch, cur_seg=seg_s, cur_q=cur_q, taken_row=taken)
        if idx.numel() and soft:
            stats = {}
            q_target, sf_target = dqn_ops.next_targets(seg, nq, done, self.gamma, action_raster=sf_action.squeeze(1) if use_sf else None,
                                                       lin=lin, discount=discount, select_q=select_q, temperature=self.target_temperature,
                                                       next_feat=soft_feat, feat_row=soft_row, feat_head=soft_head, stats=stats, **relative,
                                                       **cur)
            # the log's two means over the transitions that are not done; they wait on the device for the losses' copy
            # (of the n sampled ones: the scratch env's envs beyond n repeat record 0)
            at_max = nq.contiguous().float().index_select(0, stats["argmax_row"].long().clamp_(0, nq.numel() - 1))
            both = torch.stack([stats["entropy"], at_max - stats["value"]]
                               + ([stats["temp_out"].float()] if self.target_temp_relative else []))[:, :n]
            self._soft_stats = torch.where(done[:n], torch.zeros_like(both), both).sum(dim=1) / (~done[:n]).sum().clamp_(min=1)
            self._soft_names = SOFT_TARGET_KEYS + (RELATIVE_TARGET_KEYS if self.target_temp_relative else ())
            if munch is not None:
                # the log's three: the mean bonus, the share at or below the clip, the taken actions not found (over the n sampled)
                found = stats["miss"][:n] == 0
                extra = torch.stack([stats["bonus"][:n].mean(), ((stats["tlogp"][:n] <= munch[1]) & found).float().mean(),
                                     stats["miss"][:n].sum().float()])
                self._soft_stats, self._soft_names = torch.cat([self._soft_stats, extra]), self._soft_names + MUNCHAUSEN_KEYS
        elif idx.numel():
            q_target, sf_target = dqn_ops.next_targets(seg, nq, done, self.gamma, next_sf=nsf0 if use_sf else None,
                                                       action_raster=sf_action.squeeze(1) if use_sf else None, lin=lin,
                                                       discount=discount, select_q=select_q)
        else:
            q_target = lin
            if munch is not None:                            # no next candidate anywhere: the bonus is all the target adds
                q_target = lin + dqn_ops.soft_value(seg_s, cur_q, self.target_temperature, taken_row=taken, alpha=munch[0],
                                                    clip_lo=munch[1], **relative)[2]
            sf_target = sf_action.reshape(E, -1) if use_sf else None
        binary = torch.zeros((E, 6), dtype=torch.float32, device=self.device)
        binary[:, 0] = stable_s
        if self.priority_refresh:                            # (s_t, a_t) of every transition, for _transition_q
            self._transitions = (renv, bits_s, action_bits, stable_s, block_f, action_f)
        return TargetBatch(None if self.task_channels else block_f[:n], binary[:n], None if self.task_channels else action_f[:n],
                           q_target[:n], sf_target[:n] if use_sf else None, state_bits=bits_s[:n], action_bits=action_bits[:n],
                           reward_maps=renv.reward_maps_img[:n].reshape(n, -1) if self.per_env_tasks else None,
                           obstacle_bits=renv.env_obstacle_bits[:n] if self.per_env_obstacles else None)

    @torch.no_grad()
    def _transition_q(self, n):
        """q(s_t, a_t) of the POLICY net as it stands now for the n transitions the last _targets call was given (priority_refresh),
        through the forwards acting uses (_net_q): the transitions stand in for an env whose state e is s_t of transition e and
        whose only candidate row is a_t (_TransitionRows over the scratch env, which still holds their tasks).  The factored
        SuccessorMLP reads the bit rasters (bridges_bits_linear; per-env tasks: the scratch env's reward maps and the
        [E, 2, hidden] tables, per-env obstacles: bridges_bits_linear2), the conv nets run the module forward in eval() over the
        f32 images _targets built, in ROW_CHUNK chunks padded as _forward_rows pads, or with task_channels over one
        ops.conv_input per chunk.  Every row is fed: looking for equal rows would cost a host wait.  -> q [n] float32."""
        renv, bits_s, action_bits, stable_s, block_f, action_f = self._transitions
        view = getattr(renv, "_transition_rows", None)
        if view is None:
            view = renv._transition_rows = _TransitionRows(renv)
        view.state_bits, view.cand_bits = bits_s, action_bits
        factored = self._factored(self.policy_net)
        view.state_raster = block_f.squeeze(1) if (block_f is not None and not factored) else None
        view.cand_raster = action_f.squeeze(1) if (action_f is not None and not factored and not self.task_channels) else None
        rows = torch.arange(renv.E, dtype=torch.int64, device=self.device)
        q = self._net_q(self.policy_net, view, rows, rows, stable_s.bool(), groups=None)
        return q[:n].contiguous().float()

    def beta_now(self):
        """The exponent of the importance-sampling weights of the next train_steps call that trains:
        min(1, beta0 + (1 - beta0) * k / anneal), k = the calls that trained so far (anneal == 0: beta0).  Host arithmetic on a
        scalar launch argument: the weights launch lies outside the captured graph."""
        b0, n = self.priority_beta, self.priority_beta_anneal
        return b0 if n == 0 else min(1.0, b0 + (1.0 - b0) * self.priority_beta_calls / n)

    def _loss(self, q, sf, q_target, sf_target, w=None):
        """``w`` [B] (importance-sampling weights): every row's term times its weight before the mean over the rows -- the
        formulas of the captured autograd body (train_step.CapturedTrainStep._autograd_body)."""
        if w is not None:
            loss = 0.
            if 'mse_q_values' in self.loss_parts:
                loss = loss + (w * (q - q_target) ** 2).mean()
            if sf_target is not None:
                loss = loss + (w * ((sf[:, 0] - sf_target.view_as(sf[:, 0])) ** 2).reshape(w.shape[0], -1).mean(dim=1)).mean()
            return loss
        loss = 0.
        if 'mse_q_values' in self.loss_parts:
            loss = loss + self.mse(q, q_target)
        if sf_target is not None:
            loss = loss + self.mse(sf[:, 0], sf_target.view_as(sf[:, 0]))
        return loss

    def _train_step(self, n_steps):
        """The policy net's captured-step driver as this loop uses it: two eager calls before the first capture (they
        initialise the optimiser state and the library workspaces a capture needs), the hand-written step for SuccessorMLP
        with its first-layer rows built per call, the task maps of the rollout env (task_channels: the conv nets' autograd step
        on per-transition rows, the shared obstacle raster bit-packed)."""
        from robotoddler.models.cv import ConvNet, Policy, SuccessorMLP
        env = self.env
        return T.CapturedTrainStep.of(self.policy_net, self.opt, self.B, self.loss_parts, n_steps, owner=self, img=(env.img, env.img),
                                      fused=T.fused_step_enabled(self.policy_net, self.loss_parts),
                                      graph_default=isinstance(self.policy_net, (SuccessorMLP, ConvNet, Policy)), warmup=2,
                                      eager_body=False, prepared=True, task_rows=self.per_env_tasks,
                                      obstacle_rows=self.per_env_obstacles, weights=self.priority_beta is not None,
                                      task=((None if self.per_env_tasks else env.reward_features),
                                            (None if self.per_env_obstacles else
                                             (env.obstacle_bits if self.task_channels else env.obstacle_raster))))

    @property
    def _graph_state(self):
        """This loop's capture on the policy net's driver (n_max, fused, the guard's snapshot), None while it steps eagerly."""
        drv = getattr(self.policy_net, "_fused_trainer", None)
        return drv.state if drv is not None and drv.key[3] is self and drv._graphs else None

    # the on-device restore guard of the captured autograd step (train_step.CapturedTrainStep) on this loop's capture
    def _guard_tensors(self):
        return self.policy_net._fused_trainer._guard_tensors()

    def _guard_snapshot(self, st):
        self.policy_net._fused_trainer._guard_snapshot(st)

    def _guard_restore(self, st, losses):
        self.policy_net._fused_trainer._guard_restore(st, losses)

    def train_steps(self, n_steps, defer=False):
        """n_steps optimiser steps on n_steps independently sampled batches; returns the losses (one host sync).
        defer=True: returns a ``DeferredLosses`` -- the losses travel to pinned host memory behind the optimiser steps and
        ``.get()`` waits for that copy only, so the host can queue the next lock-step's acting while the GPU still
        trains (the list form makes the host wait for the last optimiser step before it queues anything)."""
        if len(self.ring) < self.B or n_steps <= 0:
            return DeferredLosses(None, None, None) if defer else []
        B = self.B
        # n_steps independent batches = ONE draw of n_steps * B records: both sampling rules draw with replacement, so
        # the batches are i.i.d. either way (25 separate draws cost ~100 launches of host time per lock-step)
        drawn = weights = None
        if self.priority_beta is not None or self.priority_refresh or self.priority_alpha != 1.0:
            # the sampler kernel: the exponent, and the ring rows of the draws for the refresh and the weights
            rec, drawn = self.ring.sample_prioritized(n_steps * B, self.sample_gen, self.priority_alpha)
            if self.priority_beta is not None:
                # importance-sampling weights (they need the draws' rows and the masses) directly behind the draw: they describe
                # the distribution it was made from, before any refresh
                weights = self.ring.sample_weights(drawn, B, self.beta_now())
                self.priority_beta_calls += 1
        else:
            rec = self.ring.sample(n_steps * B, self.sample_gen, self.prioritized)
        batch = self._targets(rec)
        binary, q_target, sf_target, maps, obst_bits = batch.binary, batch.q_target, batch.sf_target, batch.reward_maps, batch.obstacle_bits
        if self.priority_refresh:
            # |q(s_t, a_t) - q_target| of the policy net as it stands now, back to the sampled rows in one launch (once per
            # lock-step for all n_steps batches, the approximation double_q makes); q_target is what _targets returned, whatever
            # the loss parts are
            self.ring.update_priorities(drawn, self._transition_q(n_steps * B), q_target)
        # task_channels: the transitions' bit rasters stand in for their f32 images
        block, action = (batch.state_bits, batch.action_bits) if self.task_channels else (batch.block_f, batch.action_f)
        drv = self._train_step(n_steps)
        out = drv.run(n_steps, block, action, binary, maps, obst_bits, q_target, sf_target, weights=weights)
        if out is None:
            drv = None
            S = self.env.img
            if self.task_channels:
                # the rows of all n_steps * B transitions as the captured step builds them: one launch from bits and maps
                x = ops.conv_input(block, action, maps, obst_bits if obst_bits is not None else self.env.obstacle_bits.reshape(1, 64))
            else:
                reward = self.env.reward_features.unsqueeze(0).expand(B, -1, -1, -1) if maps is None else None
                obstacle = self.env.obstacle_raster.unsqueeze(0).expand(B, -1, -1, -1) if obst_bits is None else None
            self.policy_net.train()
            losses = []
            for i in range(n_steps):
                sl = slice(i * B, (i + 1) * B)
                if self.task_channels:
                    xb = x[sl]
                    q, sf, _ = self.policy_net(xb[:, 0:1], binary[sl], xb[:, 1:2], xb[:, 2:3], xb[:, 3:4])
                else:
                    if maps is not None:
                        reward = maps[sl].reshape(B, 1, S, S)
                    if obst_bits is not None:
                        obstacle = ops.bits_to_f32(obst_bits[sl]).reshape(B, 1, S, S)
                    q, sf, _ = self.policy_net(block[sl], binary[sl], action[sl], reward, obstacle)
                loss = self._loss(q, sf, q_target[sl], sf_target[sl] if sf_target is not None else None, weights[sl] if weights is not None else None)
                self.opt.zero_grad()
                if self._eager_reduce is None:
                    self._eager_reduce = dqn_ops.ReduceTables(self.device)
                with dqn_ops.deferred_wgrad_reduce(self._eager_reduce):
                    loss.backward()
                self.opt.step()
                losses.append(loss.detach())
            out = torch.stack(losses)
        if self._soft_stats is not None:                     # soft targets: the means named in _soft_names ride behind the losses
            out = torch.cat([out.to(torch.float32).reshape(-1), self._soft_stats.to(torch.float32)])
        if defer:
            host = torch.empty(out.numel(), dtype=torch.float32, pin_memory=True)
            host.copy_(out, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            return DeferredLosses(host, done, drv, names=self._soft_names, owner=self)
        return DeferredLosses(out, None, drv, names=self._soft_names, owner=self).get()     # the one host sync of the call

    def train_step(self):
        out = self.train_steps(1)
        return out[0] if out else None

    def update_target(self):
        from robotoddler.training.successor_dqn import update_target_net
        update_target_net(self.policy_net, self.target_net, self.tau)

    # ------------------------------------------------------------------ checkpoint of what the nets / ring do not hold
    def _recorded_options(self):
        """What a checkpoint records about the options, one row each: the key in the file; what its value names, for a refusal;
        this agent's value (None without the option: save_extra then writes no key); what a file without the key means; and why
        a run under another value cannot go on from the file (None: recorded only, load_extra does not compare it)."""
        T, O = int(self.n_task_targets), int(self.n_task_obstacles)
        backup, rows = "the nets were trained towards another backup operator", "the ring does not hold the "
        return (
            # (T, O) of the records' tails: the width alone cannot tell T = 3, O = 0 from T = 2, O = 1 (a file written before the
            # tails held obstacles holds targets only, whose number the ring's width check has pinned)
            ("task_shape", "(targets, obstacles)", (T, O), (T, 0), "the tails do not mean the same task"),
            ("n_step", "n_step", int(self.n_step), 1, "the rows of the ring do not mean the same returns"),
            ("target_temperature", "target_temperature", None if self.target_temperature is None else float(self.target_temperature),
             None, backup),
            ("target_temp_relative", "target_temp_relative, spread_floor", float(self.spread_floor) if self.target_temp_relative else None,
             None, backup),
            ("munchausen", "(munchausen_alpha, munchausen_clip)", None if self.munchausen is None else tuple(map(float, self.munchausen)),
             None, backup),
            ("search_sampler", "(search_sampler, search_temperature, search_resample_temperature)",
             (str(self.search_sampler), float(self.search_temperature), float(self.search_resample_temperature))
             if self.search_sampler is not None else None, None, rows + "rows of the same search"),
            ("hindsight", "(hindsight, hindsight_goals)", (str(self.hindsight), int(self.hindsight_goals)) if self.hindsight is not None else None,
             None, rows + "same mix of rolled-out and relabelled rows"),
            ("hindsight_fold", "hindsight_fold", True if self.hindsight_fold else None, False, "the two runs do not agree on the option"),
            # what the schedule's temperature multiplies goes the way of the exploration setting itself
            ("temp_relative", "temp_relative, spread_floor", float(self.spread_floor) if self.temp_relative else None, None, None),
        )

    def save_extra(self, path, **counters):
        blob = dict(epsilon=float(self.epsilon), episodes_done=int(self.episodes_done), env_steps=int(self.env_steps),
                    step_images=self.step_images.cpu(), sample_gen=self.sample_gen.get_state().cpu(),
                    explore_gen=self.explore_gen.get_state().cpu(), counters={k: int(v) for k, v in counters.items()})
        blob.update({key: value for key, _, value, _, _ in self._recorded_options() if value is not None})
        if self.curriculum is not None:                      # one more key: (ema, seen), weights, sums and accumulator
            blob["curriculum"] = self.curriculum.state_dict()
        if self.priority_beta is not None:                   # one more key: the annealing clock of the weights' exponent
            blob["priority_beta_calls"] = int(self.priority_beta_calls)
        if self.exploration == "boltzmann":                  # one more key: where the schedule stands
            blob["temperature"] = float(self.temperature)
        if self.search_every:                                # one more key: the lock-steps since the last search
            blob["search_phase"] = int(self.search_calls)
        if self.search_sampler is not None:                  # one more key: where the particle search's stream stands
            blob["search_gen"] = self._search_generator().get_state().cpu()
        if self.hindsight is not None:                       # one more key: the running episodes
            blob["hindsight_buffer"] = self.hindsight_buffer.state_dict()
        torch.save(blob, path)

    def load_extra(self, path):
        """Restores what save_extra wrote.  The file is rank 0's: exact continuation (same exploration draws, same
        env-step count) holds for a single-rank run.  With several ranks the shared items (epsilon, count images, replay
        sampling stream, episode counter) are restored everywhere, while a rank > 0 -- whose exploration stream and
        env-step count were never saved -- re-seeds its exploration stream from (seed, rank, lock-step) so that the
        ranks keep drawing different uniforms, and starts its local env-step count from rank 0's."""
        blob = torch.load(path, weights_only=True)
        for key, what, want, absent, why in self._recorded_options():
            got = blob.get(key, absent)
            got = tuple(got) if isinstance(got, (tuple, list)) else got
            want = absent if want is None else want
            if why is None or got == want:
                continue
            if key == "task_shape":
                raise ValueError(f"{path} was written by a run whose records end in {got[0]} targets and {got[1]} obstacles, this "
                                 f"agent's end in {want[0]} targets and {want[1]} obstacles: {why}")
            raise ValueError(f"{path} was written by a run with {what} = {got}, this agent has {what} = {want}: {why}")
        if self.hindsight is not None:
            self.hindsight_buffer.load_state_dict(blob["hindsight_buffer"])
        self.epsilon, self.episodes_done, self.env_steps = blob["epsilon"], blob["episodes_done"], blob["env_steps"]
        self.step_images.copy_(blob["step_images"])
        self.sample_gen.set_state(blob["sample_gen"])
        if self.rank == 0:
            self.explore_gen.set_state(blob["explore_gen"])
        else:
            self.explore_gen.manual_seed(7654321 + self.seed * 1000 + self.rank + 7919 * (int(blob["counters"].get("lockstep", 0)) + 1))
        if self.curriculum is not None and "curriculum" in blob:     # continue with the same table
            self.curriculum.load_state_dict(blob["curriculum"])
        if self.priority_beta is not None:                   # (a file of a run without the option carries no entry: 0)
            self.priority_beta_calls = int(blob.get("priority_beta_calls", 0))
        if self.exploration == "boltzmann":                  # (a file of a run without the option: temp_start)
            self.temperature = float(blob.get("temperature", self.temp_start))
        if self.search_every:                                # (a file of a run without the option: phase 0)
            self.search_calls = int(blob.get("search_phase", 0)) % self.search_every
        if self.search_sampler is not None:
            self._search_generator().set_state(blob["search_gen"])
        return blob["counters"]

    # ------------------------------------------------------------------ driver
    def reset_window(self):
        """Empty the n-step window of every env (n_step > 1; a no-op otherwise).  Called wherever env.reset() abandons the
        running episodes -- after a checkpoint is written and on resume -- so that no start of an abandoned episode is folded
        into the next one; the pending starts (up to n - 1 transitions per env) are dropped, they never reach the ring."""
        if self._window is not None:
            self._window[0].zero_()
        if self.hindsight_buffer is not None:                # hindsight relabelling: the running episodes go with them
            self.hindsight_buffer.clear()

    def _fold(self, rec, valid):
        """One lock-step's one-step rows (of all ranks) through the n-step windows -> (out [rows * n, W + 1], out_valid)."""
        if self._window is None:
            rows, n = rec.shape[0], self.n_step
            self._window = (torch.zeros(rows, dtype=torch.int32, device=self.device),
                            *(torch.zeros((rows, n), dtype=torch.float64, device=self.device) for _ in range(4)))
        return dqn_ops.nstep_fold(rec.contiguous(), valid, self.gamma, self.n_step, *self._window)

    def _count(self, name, float64=False):
        """One of the last lock-step's counts, as it arrived in pinned memory (float64: the slot holds a float64's bits)."""
        at = self._count_names.index(name)
        return float(self._counts_host[at:at + 1].view(torch.float64)) if float64 else int(self._counts_host[at])

    def lockstep(self, n_train_steps, defer_losses=False):
        """act -> all-gather -> replay push -> n optimiser steps -> soft update.  defer_losses=True returns the losses as
        a DeferredLosses (see train_steps): nothing after the replay push waits for the GPU, so the optimiser steps run
        under the host's queueing of the next lock-step.
        n_step > 1: act -> gather -> fold -> push; the statistics, the curriculum and td_errors see the one-step records (a start's
        priority is its one-step TD error), the ring and the caller get the emitted h-step rows."""
        rec, valid = self.act()
        if self.episode_stats is not None:
            # before the all-gather: env identity still holds (a task family: under the class of before the step)
            self.episode_stats.fold(rec, valid, cls=self.env._task_class if self.episode_stats.n_classes > 1 else None)
        if self.curriculum is not None:
            # every `every` lock-steps this launches the update as well: the draws of the next lock-step's step read its table
            self.curriculum.fold(rec, valid, self.env._task_class)
            self.curriculum_weights_host = self.curriculum.weights_to_host()
        if self.prioritized:
            rec[:, R.O_TD] = self.td_errors(rec).to(rec.dtype)
        # ONE wait per lock-step on this side: the two counts ride to pinned memory in front of the next act's candidate rows,
        # whose row count the host has to wait for anyway (bridges_valid_rows)
        done_rec = valid & (rec[:, R.O_DONE] > 0.5)
        counts = dict(valid=valid.sum(), done=done_rec.sum())
        if self.n_step > 1:
            # one rank: the fold runs here, and the number of emitted rows rides with the two counts -- no wait of its own
            folded = self._fold(self.with_task(rec), valid) if not D.active() else None
            counts["emitted"] = folded[1].sum() if folded is not None else torch.zeros_like(counts["valid"])
        boltzmann = self.exploration == "boltzmann"
        if boltzmann:                                   # the envs that left the arg-max ride with the counts: no wait of their own
            counts["explored"] = (self._ex_w * valid).sum().to(torch.int64) if self._ex_w is not None else torch.zeros_like(counts["valid"])
        if self.temp_relative:                          # the sum of the valid envs' effective temperatures: a float64's bits among the counts
            counts["temp_sum"] = ((self._temp_out * valid).sum().view(torch.int64) if self._temp_out is not None
                                  else torch.zeros_like(counts["valid"]))
        hind = None
        if self.hindsight is not None:
            # the lock-step joins every env's running episode; the episodes that end are relabelled at once (three launches) and
            # the number of rows that came out rides with the counts: no wait of its own
            self.hindsight_buffer.write(self.with_task(rec), self.env.step_flags, valid, self.env._task_episode)
            hind = self.hindsight_buffer.relabel(self.env, done_rec)
            counts["hindsight"] = hind[1][0].to(torch.int64)
        self._counts_host.copy_(torch.stack([counts[k] for k in self._count_names]), non_blocking=True)
        arrived = torch.cuda.Event()
        arrived.record()
        self._rows(self.env, self._stable_flags(self.env))
        arrived.synchronize()                           # passed already unless the rows came out of the env's cache
        n_valid, n_done = self._count("valid"), self._count("done")
        self.env_steps += n_valid
        if boltzmann:
            self.explored_fraction = self._count("explored") / n_valid if n_valid else None
        if self.temp_relative:
            self.temperature_effective = self._count("temp_sum", float64=True) / n_valid if n_valid else None
        if self.n_step > 1 and folded is None:
            # several ranks: the fold runs AFTER the gather, on the uncompacted rows of all ranks, so every rank holds the same
            # windows and pushes the same rows; the collective carries what it carries for n_step = 1
            out, out_valid = self._fold(*D.all_gather_rows(self.with_task(rec), valid))
            allrec = out[out_valid]
        elif self.n_step > 1:
            out, out_valid = folded
            allrec = out.index_select(0, torch.nonzero_static(out_valid, size=self._count("emitted")).squeeze(1))
        else:
            allrec = D.all_gather_records(self.with_task(rec), valid, n_valid=n_valid)
        self.ring.push(allrec)
        if hind is not None:                            # behind the lock-step's own records
            self.hindsight_rows = self._count("hindsight")
            self.ring.push(hind[0][:self.hindsight_rows])
        if not D.active():
            self.episodes_done += n_done
        elif self.n_step > 1:
            # a finished episode emits up to n done rows: the one of its last transition has h = 1
            self.episodes_done += int(((allrec[:, R.O_DONE] > 0.5) & (allrec[:, -1] == 1.0)).sum().item())
        else:
            self.episodes_done += int((allrec[:, R.O_DONE] > 0.5).sum().item())
        if self.search_every:                           # search in training: every N-th lock-step, behind the rows pushed above
            self.search_calls += 1
            self.last_search = None
            if self.search_calls >= self.search_every:
                self.search_calls = 0
                self._search()
        losses = self.train_steps(n_train_steps, defer=defer_losses)
        self.update_target()
        if boltzmann:                                   # (epsilon is left alone: nothing reads it in this mode)
            self.temperature = (self.temperature - self.temp_end) * self.temp_decay + self.temp_end
        else:
            self.epsilon = (self.epsilon - self.eps_end) * self.eps_decay + self.eps_end
        return losses, allrec


class _TransitionRows:
    """The transitions of a _targets call as the env a Q pass reads (VecDQN._transition_q): state e = s_t of transition e
    (state_bits / state_raster), its one candidate row e = a_t (cand_bits / cand_raster); the images are cropped already.  The
    task -- reward maps, obstacle rasters, the flags -- is the scratch env's, which every other attribute is read from."""

    def __init__(self, env):
        self._env = env
        self.state_bits = self.cand_bits = self.state_raster = self.cand_raster = None

    def __getattr__(self, name):                             # (only what the instance itself does not hold)
        return getattr(self._env, name)

    @staticmethod
    def crop(x):
        return x


class DeferredLosses:
    """Losses of one train_steps call on their way to the host (pinned buffer + event; no event: a tensor read where it lies).
    ``names``: the log keys of the means that follow the losses in the buffer, one value each (VecDQN._soft_names)."""

    def __init__(self, host, done, driver, names=(), owner=None):
        self._host, self._done, self._driver, self._list = host, done, driver, None
        self._names, self._owner = tuple(names), owner       # the agent that keeps the means as attributes of the same names
        self.soft = None                                     # after get(): the means under their log keys (None: there are none)

    def get(self):
        if self._list is None:
            if self._host is None:
                self._list = []
            else:
                if self._done is not None:
                    self._done.synchronize()
                self._list = self._host.tolist()
                if self._names:
                    k = len(self._names)
                    self._list, tail = self._list[:-k], self._list[-k:]
                    self.soft = dict(zip(self._names, tail))
                    for key, v in self.soft.items():
                        setattr(self._owner, key, v)
                if self._driver is not None:
                    self._driver.check_losses(self._list)
        return self._list


def lockstep_log_values(info):
    """What one lock-step hands to the aim / wandb sinks, under the reference's names (successor_dqn.py:489-499) where the
    quantity exists per lock-step: reward / lin_reward = mean over the lock-step's transitions (the reference: discounted
    sum over one episode), avg_loss, num_steps = env-steps of the lock-step on this rank, epsilon; plus the run counters.
    Then the per-episode statistics (EpisodeStats): the episodes that ended in the lock-step on all ranks and the means over
    them of log_episode's discounted reward / lin_reward, episode length and final stability, and the fraction that reached
    the targets (None when no episode ended).  A run on a task family (info['success_by_class']: a list indexed by the drawn
    n) appends success_rate_n{k}, the success rate of the episodes played on n = k, for the family's n_lo..n_hi; a run with a
    curriculum (info['curriculum_weights']: the weights of n_lo..n_hi) appends curriculum_weight_n{n}."""
    vals = dict(reward=info['mean_reward'], lin_reward=info['mean_lin_reward'], avg_loss=info['avg_loss'],
                num_steps=info['lockstep_env_steps'], epsilon=info['epsilon'], env_steps=info['env_steps'],
                steps_per_s=info['steps_per_s'], **{k: info.get(k) for k in EPISODE_KEYS})
    if 'temperature' in info:                                # Boltzmann exploration only
        vals.update(temperature=info['temperature'], explored_fraction=info.get('explored_fraction'))
    # what rode behind the losses, each only with its option; between them the relative exploration temperature's mean
    for key in SOFT_TARGET_KEYS + ('temperature_effective',) + RELATIVE_TARGET_KEYS + MUNCHAUSEN_KEYS:
        if key in info:
            vals[key] = info[key]
    if 'hindsight_rows' in info:                             # hindsight relabelling only
        vals.update(hindsight_rows=info['hindsight_rows'])
    if 'search_rows' in info:                                # search in training: the lock-steps that searched
        vals.update({k: info[k] for k in ('search_rows', 'search_success_rate', 'search_lin_reward')})
    by_class = info.get('success_by_class')
    if by_class is not None:
        lo = info.get('class_lo', 0)
        vals.update({f"success_rate_n{k}": v for k, v in enumerate(by_class) if k >= lo})
    weights = info.get('curriculum_weights')
    if weights is not None:                                  # the curriculum's weight of every class n = class_lo + k
        vals.update({f"curriculum_weight_n{info.get('class_lo', 0) + k}": w for k, w in enumerate(weights)})
    return vals


# per-lock-step keys of the episode statistics in run_vectorised's info (and lockstep_log_values), in log order
EPISODE_KEYS = ("episodes_finished", "episode_reward", "episode_lin_reward", "episode_num_steps", "episode_stable", "success_rate")


def curriculum_from_args(args):
    """--curriculum [--curriculum_every N --curriculum_beta B --curriculum_floor F] -> Curriculum, or None without --curriculum."""
    if not args.get('curriculum'):
        return None
    defaults = Curriculum()
    return Curriculum(beta=args.get('curriculum_beta', defaults.beta), floor=args.get('curriculum_floor', defaults.floor),
                      every=args.get('curriculum_every', defaults.every),
                      min_episodes=args.get('curriculum_min_episodes', defaults.min_episodes))


class _ShapeOf:
    """A shape as VecAssemblyGym's constructor takes it: the geometry and the faces blocks may be placed on."""

    def __init__(self, geometry, target_faces_2d):
        self.geometry, self.target_faces_2d = geometry, list(target_faces_2d)


def _env_like(ev, n_envs, targets, obstacles):
    """A VecAssemblyGym of ``n_envs`` envs on the given task with the shapes, limits, options and seed of ``ev``."""
    shapes = [_ShapeOf(g, faces) for g, faces in zip(ev.shapes, ev.shape_target_faces)]
    return VecAssemblyGym(n_envs, shapes, obstacles, targets, max_steps=ev.max_steps or None, mu=ev.mu, density=ev.density,
                          bounds=ev.bounds, xlim=ev.xlim, ylim=ev.ylim, x_discr_ground=ev.x_discr_ground, offset_values=ev.offset_values,
                          seed=ev.seed, device=ev.device, f32_rasters=ev.f32_rasters, a_max=ev.a_max, img_size=(ev.img, ev.img),
                          sparse_raster_update=ev.sparse_raster_update, candidate_snapshots=ev.candidate_snapshots,
                          stable_actions_only=ev.stable_actions_only)


def search_env_like(env, tasks, width):
    """The env VecDQN's search in training runs on: tasks * width envs with the shapes, limits and options of the rollout env
    ``env``, whose tasks are loaded before every search (load_targets / load_task: explicit per-env arrays that no episode
    redraws, zeros until then; a task family goes in the same way, as the coordinates of the rollout envs' drawn classes).  A
    fixed task is passed through."""
    M, B = int(tasks), int(width)
    if not 1 <= B <= abi.BEAM_MAX_WIDTH:
        raise ValueError(f"search_env_like(width={width!r}): 1..{abi.BEAM_MAX_WIDTH}")
    if not isinstance(env, VecAssemblyGym):
        raise ValueError(f"search_env_like() takes a VecAssemblyGym; a {type(env).__name__} (env groups on streams of their own) "
                         "cannot be forked across its groups")
    if not 1 <= M <= env.E:
        raise ValueError(f"search_env_like(tasks={tasks!r}): 1..{env.E}")
    if env.per_env_tasks:
        targets = torch.zeros((M * B, env.n_targets, 3), dtype=torch.float64)
        obstacles = torch.zeros((M * B, env.n_obstacles, 3), dtype=torch.float64) if env.per_env_obstacles else list(env.obstacles)
    else:
        targets, obstacles = list(env.targets), list(env.obstacles)
    return _env_like(env, M * B, targets, obstacles)


def beam_env_like(eval_env, width):
    """The env VecDQN.beam_search runs on: M * width envs, M = eval_env.E, in which envs m * width .. (m + 1) * width - 1 hold the
    task evaluate() plays in env m of ``eval_env`` -- same shapes, limits, options and seed.  A fixed task is passed through.
    Per-env tasks: eval_env is reset, the targets (and obstacles) of its episode 0 are taken once and repeated ``width`` times as
    explicit [E, T, 3] / [E, O, 3] arrays, which no episode redraws: a finished beam's auto-reset changes no task.  A task family
    goes in the same way, as the coordinates of every env's drawn class (parked obstacle slots included); the classes are kept
    on the env (beam_task_class, a host list) for the statistics by class."""
    B = int(width)
    if not 1 <= B <= abi.BEAM_MAX_WIDTH:
        raise ValueError(f"beam_env_like(width={width!r}): 1..{abi.BEAM_MAX_WIDTH}")
    if not isinstance(eval_env, VecAssemblyGym):
        raise ValueError(f"beam_env_like() takes a VecAssemblyGym; a {type(eval_env).__name__} (env groups on streams of their own) "
                         "cannot be forked across its groups")
    ev = eval_env
    if ev.per_env_tasks:
        ev.reset()                                           # task_episode 0: the tasks every evaluate() plays
        targets = ev.env_targets.repeat_interleave(B, dim=0)
        obstacles = ev.env_obstacles.repeat_interleave(B, dim=0) if ev.per_env_obstacles else list(ev.obstacles)
    else:
        targets, obstacles = list(ev.targets), list(ev.obstacles)
    env = _env_like(ev, ev.E * B, targets, obstacles)
    if ev.task_family is not None:
        env.beam_task_class, env.beam_n_classes = ev.task_class.tolist(), ev.task_family.n_classes
    return env


def next_multiple(n, every):
    """The first multiple of ``every`` above ``n`` finished episodes: the next checkpoint / evaluation threshold of the vectorised
    loop, from 0 at the start and from the restored episode count on resume."""
    return (n // every + 1) * every


def run_vectorised(args, device, aim_run=None, wandb_run=None, return_agent=False):
    from robotoddler.training.successor_dqn import (EVAL_DEFAULTS, agent_options_from_args, make_nets, track_run_sinks,
                                                    eval_particles_from_args)
    backend = os.environ.get("BRIDGES_DIST_BACKEND")          # 'gloo' = rehearsal with several ranks on one card
    rank, world = D.init(backend=backend, device=device)
    names = dict(trapezoid=["trapezoid"], hexagon=["hexagon"], both=["trapezoid", "hexagon"])[args['shapes']]
    geoms = [load_urdf(f"shapes/{n}.urdf") for n in names]
    random_targets = args.get('random_targets')
    random_obstacles = args.get('random_obstacles')
    task_channels = bool(args.get('task_channels', False))
    family = None                                              # --random_bridge_length / --random_tower_height: (kind, lo, hi)
    if args.get('random_bridge_length') is not None:
        family = ("span", *args['random_bridge_length'])
    elif args.get('random_tower_height') is not None:
        family = ("tower", *args['random_tower_height'])
    if family:
        # horizontal_bridge_setup(num_obstacles=n) / bridge_setup(num_stories=n) per env and episode, n drawn from LO..HI on the
        # device: one target, up to HI obstacles, both per env
        # --family_weights: fixed weights of the classes LO..HI (the evaluation env below stays uniform)
        targets, obstacles = RandomBridges(family[0], sizes=family[1:], weights=args.get('family_weights')), []
    elif random_targets:
        # tower_setup(num_targets=T) per env and episode (gym_env.py:64-79 of the reference): no obstacles, every env draws
        # its own targets whenever it starts an episode; --random_obstacles O: and O obstacles beside them, as connecting_setup
        # draws both at every reset (gym_env.py:91-99)
        targets = RandomTargets(random_targets)
        obstacles = RandomObstacles([OBSTACLE_RANGE] * random_obstacles) if random_obstacles else []
    elif args.get('tower_height'):
        H, N = 0.8, args['tower_height']
        targets = [(0.5, 0, N * H + H / 2)]
        obstacles = [(0.5, 0., i * H + H / 2) for i in range(N)]
    else:
        sq, n = 0.6, args['bridge_length']
        targets = [(n * sq + 2.5 * sq, 0, sq / 2)]
        obstacles = [(i * sq, 0, sq / 2) for i in range(1, n + 1)]
    seed = args['seed'] or 0
    torch.manual_seed(seed)                                    # identical initial weights on every rank
    policy_net, target_net = make_nets(args, device)
    env = VecAssemblyGym(args['num_envs'], geoms, obstacles, targets, max_steps=args['max_steps'],
                         seed=seed * 1000003 + rank, device=device, env_id_base=rank * args['num_envs'],
                         f32_rasters=VecDQN.acting_needs_f32_rasters(policy_net) and not task_channels,
                         img_size=args.get('image_size') or (64, 64), stable_actions_only=args.get('stable_actions_only', False))
    opt = torch.optim.Adam(policy_net.parameters(), lr=args['learning_rate'], fused=True)    # one launch for all tensors
    capacity = max(args['replay_buffer_capacity'], 4 * args['num_envs'] * world)
    agent = VecDQN(policy_net, target_net, opt, env, capacity, args['batch_size'], args['gamma'], args['tau'],
                   args['loss_function'], seed=seed, rank=rank, stable_actions_only=args.get('stable_actions_only', False),
                   episode_stats=True, per_env_tasks=bool(random_targets or family),
                   per_env_obstacles=bool(random_obstacles or family), task_channels=task_channels, **agent_options_from_args(args))
    # greedy evaluation (successor_dqn.py:749-781 of the reference): rank 0 runs one episode in each of --eval_envs envs of the
    # training task every --evaluate_every finished episodes (--random_targets: a sampler of its own for the evaluation env,
    # whose seed gives it other tasks than any rollout env's; evaluate() resets it, so every evaluation sees the same tasks)
    eval_envs = args.get('eval_envs', EVAL_DEFAULTS['eval_envs'])
    eval_epsilon = args.get('eval_epsilon', EVAL_DEFAULTS['eval_epsilon'])
    eval_env = None
    if eval_envs > 0 and rank == 0:
        eval_targets = (RandomBridges(family[0], sizes=family[1:]) if family else
                        RandomTargets(random_targets) if random_targets else targets)
        eval_obstacles = RandomObstacles([OBSTACLE_RANGE] * random_obstacles) if random_obstacles else obstacles
        eval_env = VecAssemblyGym(eval_envs, geoms, eval_obstacles, eval_targets, max_steps=args['max_steps'], seed=seed * 1000003 + 999983,
                                  device=device, f32_rasters=VecDQN.acting_needs_f32_rasters(policy_net) and not task_channels,
                                  img_size=args.get('image_size') or (64, 64), stable_actions_only=args.get('stable_actions_only', False))
    # --eval_beam B: every evaluation also searches the same tasks with a beam of width B (B envs per task, forked on the device)
    eval_beam = args.get('eval_beam')
    beam_env = beam_env_like(eval_env, eval_beam) if eval_beam and eval_env is not None else None
    eval_beam_merge = bool(args.get('eval_beam_merge'))      # --eval_beam_merge: that search merges beams of the same structure
    # --eval_particles B: ... or with B particles per task (particle_search: sampled rollouts, resampled by their value)
    eval_particles = eval_particles_from_args(args)
    if eval_particles is not None and eval_env is not None:
        beam_env = beam_env_like(eval_env, eval_particles['width'])
    history, t0, it = [], time.time(), 0
    next_ckpt = next_multiple(0, args['checkpoint_every'])
    next_eval = next_multiple(0, args['evaluate_every'])
    if args.get('load_checkpoint'):                      # successor_dqn.py:654-665 + utils.py:31-50 of the reference
        from robotoddler.utils.utils import load_checkpoint
        path = args['load_checkpoint']
        load_checkpoint(path, policy_net, target_net, agent.ring, opt,
                        devices=dict(policy_net=device, target_net=device, optimizer=device))
        it = agent.load_extra(os.path.join(path, 'agent.pt'))['lockstep']
        next_ckpt = next_multiple(agent.episodes_done, args['checkpoint_every'])
        next_eval = next_multiple(agent.episodes_done, args['evaluate_every'])
        env.reset()                                      # a checkpoint is taken with all environments freshly reset
        agent.reset_window()
    steps_at_start, t0 = agent.env_steps, time.time()    # throughput counts what THIS run (resumed or not) has stepped

    def finish(entry):
        """Fill in the numbers of a lock-step that were still on their way to the host when its entry was made."""
        info, deferred, stats_host, done, episodes, weights_host = entry
        ls = deferred.get()
        info['avg_loss'] = float(np.mean(ls)) if ls else None
        if deferred.soft is not None:                        # soft targets: the two means that rode with the losses
            info.update(deferred.soft)
        if stats_host is not None:
            done.synchronize()
            info['mean_reward'], info['mean_lin_reward'] = float(stats_host[0]), float(stats_host[1])
        ep = episodes.get()
        info.update(episodes_finished=ep['episodes'], episode_reward=ep['reward'], episode_lin_reward=ep['lin_reward'],
                    episode_num_steps=ep['num_steps'], episode_stable=ep['stable'], success_rate=ep['success_rate'])
        if 'by_class' in ep:
            info.update(success_by_class=[c['success_rate'] for c in ep['by_class']],
                        episodes_by_class=[c['episodes'] for c in ep['by_class']], class_lo=family[1])
        if weights_host is not None:                         # copied in front of the losses and the statistics waited for above
            info.update(curriculum_weights=weights_host.tolist(), class_lo=family[1])
        if rank == 0 and (aim_run is not None or wandb_run is not None):
            # one call per lock-step, step = episodes finished so far (the reference's x axis is the episode number)
            track_run_sinks(lockstep_log_values(info), info['episodes'], 'training', aim_run=aim_run, wandb_run=wandb_run)
        if args['verbose'] and rank == 0:
            print(info)

    pending = None
    while agent.episodes_done < args['num_episodes']:
        # losses and record statistics are read one lock-step late: nothing here waits for the optimiser steps, so they
        # run while the host queues the next lock-step's acting
        steps_before = agent.env_steps
        losses, rec = agent.lockstep(args['num_training_steps'], defer_losses=True)
        it += 1
        if args.get('save_checkpoint') and agent.episodes_done >= next_ckpt:                  # utils.py:54-89 layout
            T.sync_optimizer(policy_net)
            if rank == 0:
                from robotoddler.utils.utils import save_checkpoint
                save_checkpoint(args['save_checkpoint'], policy_net, target_net, agent.ring, opt, agent.episodes_done,
                                {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v)) for k, v in args.items()})
                agent.save_extra(os.path.join(args['save_checkpoint'], str(agent.episodes_done), 'agent.pt'), lockstep=it)
            next_ckpt = next_multiple(agent.episodes_done, args['checkpoint_every'])
            # the single-env reference checkpoints between episodes; the lock-step analogue: every rank starts all its
            # environments afresh, so that a resumed run (fresh environments) continues exactly like this one (n-step returns:
            # the pending starts of the abandoned episodes are dropped with them)
            env.reset()
            agent.reset_window()
        if it % 100 == 0:
            D.broadcast_module(policy_net)
            D.broadcast_module(target_net)
        stats_host, done = None, None
        if rec.numel():
            stats_host = torch.empty(2, dtype=torch.float64, pin_memory=True)
            stats_host.copy_(torch.stack([rec[:, R.O_REWARD].mean(), rec[:, R.O_LIN].mean()]).double(), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        episodes = agent.episode_stats.take()             # the episodes that ended in this lock-step, on every rank
        info = dict(lockstep=it, episodes=agent.episodes_done, env_steps=agent.env_steps, avg_loss=None, mean_reward=None,
                    mean_lin_reward=None, epsilon=agent.epsilon, lockstep_env_steps=agent.env_steps - steps_before,
                    steps_per_s=(agent.env_steps - steps_at_start) * world / max(time.time() - t0, 1e-9),
                    **{k: None for k in EPISODE_KEYS})
        if agent.exploration == "boltzmann":                 # (the temperature the NEXT lock-step draws at, as epsilon above)
            info.update(temperature=agent.temperature, explored_fraction=agent.explored_fraction)
        if agent.temp_relative:                              # the mean effective temperature THIS lock-step's envs drew at
            info.update(temperature_effective=agent.temperature_effective)
        if agent.hindsight is not None:                      # the relabelled rows this lock-step pushed behind its own records
            info.update(hindsight_rows=agent.hindsight_rows)
        if agent.last_search is not None:                    # search in training: a lock-step that searched
            info.update(agent.last_search)
        if eval_envs > 0 and agent.episodes_done >= next_eval:
            if rank == 0:
                ev = info['evaluation'] = agent.evaluate(eval_env, eval_epsilon)
                if beam_env is not None and eval_particles is not None:      # the same tasks under the particle search
                    ps = agent.particle_search(beam_env, **eval_particles)
                    ev.update(particle_success_rate=ps['success_rate'], particle_reward=ps['reward'], particle_lin_reward=ps['lin_reward'],
                              particles=ps['particles'])
                    # means over the depths at which a task was still open (ess 0: every task had ended before that depth)
                    opened = [d for d, e in enumerate(ps['ess_by_depth']) if e > 0.0]
                    ev.update(particle_ess=float(np.mean([ps['ess_by_depth'][d] for d in opened])) if opened else None,
                              particle_p_sel=float(np.mean([ps['p_sel_mean_by_depth'][d] for d in opened])) if opened else None)
                    if eval_particles['merge']:
                        ev.update(eval_merged_particles=sum(ps['merged_beams']))
                elif beam_env is not None:                   # the same tasks under the beam search, beside the greedy keys
                    bs = agent.beam_search(beam_env, eval_beam, merge=eval_beam_merge)
                    ev.update(beam_success_rate=bs['success_rate'], beam_reward=bs['reward'], beam_lin_reward=bs['lin_reward'],
                              beam_width=eval_beam)
                    if eval_beam_merge:                      # the beams closed as duplicates, over all tasks and depths
                        ev.update(eval_merged_beams=sum(bs['merged_beams']))
                if aim_run is not None or wandb_run is not None:
                    if family:                               # the sinks take scalars: success_rate_n{k} for the lists by class
                        by_class = ev['success_by_class']
                        ev = {k: v for k, v in ev.items() if not k.endswith('_by_class')}
                        ev.update({f"success_rate_n{k}": v for k, v in enumerate(by_class) if k >= family[1]})
                    track_run_sinks(ev, agent.episodes_done, 'evaluation', aim_run=aim_run, wandb_run=wandb_run)
                if args['verbose']:
                    print(f"evaluation {agent.episodes_done}: {info['evaluation']}")
            next_eval = next_multiple(agent.episodes_done, args['evaluate_every'])
        history.append(info)
        if pending is not None:
            finish(pending)
        pending = (info, losses, stats_host, done, episodes, agent.curriculum_weights_host)
    if pending is not None:
        finish(pending)
    T.sync_optimizer(policy_net)       # the captured step counts Adam's steps itself: hand the count back before anyone reads opt.state
    return (history, agent) if return_agent else history
