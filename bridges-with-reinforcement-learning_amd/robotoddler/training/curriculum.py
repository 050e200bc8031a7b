"""Task-family curriculum of the vectorised loop: the weights of the family's classes (the spans / heights n a RandomBridges env
draws) follow the policy's failure rate per class, on the device.  Every lock-step the finished training episodes are folded by
class (bridges_episode_stats_by_class); every ``every`` lock-steps one small kernel (bridges_family_curriculum) turns the sums
into an exponential moving average of the success rate per class, into integer weights w = w_min + round(fail * 65536) and into the
threshold table the env's class draw reads (bridges_env_set_family_thresholds).  Nothing here waits on the host."""
from dataclasses import dataclass

import torch

from bridges_hip import abi, ops
from robotoddler.training import distributed as D
from robotoddler.training.episode_stats import EpisodeStats


@dataclass(frozen=True)
class Curriculum:
    """Settings (not measurements): ``beta`` the weight of a new success rate in the moving average, ``floor`` the share of the
    weight scale every class keeps whatever its success (w_min = max(1, round(floor * 65536)): no class is starved), ``every``
    lock-steps between updates, ``min_episodes`` finished episodes a class needs before its rate is taken."""
    beta: float = 0.25
    floor: float = 0.1
    every: int = 10
    min_episodes: int = 16

    def __post_init__(self):
        if not 0.0 <= self.beta <= 1.0:
            raise ValueError(f"curriculum: beta must be in [0, 1], got {self.beta!r}")
        if not 0.0 <= self.floor <= 1.0:
            raise ValueError(f"curriculum: floor must be in [0, 1], got {self.floor!r}")
        if int(self.every) != self.every or self.every < 1:
            raise ValueError(f"curriculum: every must be an integer >= 1, got {self.every!r}")
        if int(self.min_episodes) != self.min_episodes or self.min_episodes < 1:
            raise ValueError(f"curriculum: min_episodes must be an integer >= 1, got {self.min_episodes!r}")

    @property
    def w_min(self):
        return max(1, round(self.floor * abi.FAMILY_FAIL_SCALE))


class CurriculumRun:
    """The curriculum of one rollout env (a VecAssemblyGym on a task family).  ``fold(rec, valid, cls)`` after every act() with
    the class snapshot of before the step: a finished training episode is counted exactly once, here, whatever the logging
    statistics of the loop do with theirs.  Every ``every``-th fold: the ranks' new sums are added up (all-reduce with a process
    group active, so every rank ends with the same table), added to ``sums``, and the update kernel runs on the caller's stream.
    ``w`` / ``thr`` are the env's own family_weights / family_thresholds: the next lock-step's draws read the new table."""

    def __init__(self, settings, env, gamma):
        family = getattr(env, "task_family", None)
        if family is None or not hasattr(env, "set_family_weights") or not hasattr(env, "task_class"):
            raise ValueError("VecDQN(curriculum=...) needs a rollout env on a task family (VecAssemblyGym(targets=RandomBridges(...)))")
        self.settings, self.env = settings, env
        self.lo, self.hi, self.n_classes = family.lo, family.hi, family.n_classes
        if env.family_weights is None:                       # every class unseen: equal weights, the uniform draw's classes
            env.set_family_weights([settings.w_min + abi.FAMILY_FAIL_SCALE] * (self.hi - self.lo + 1))
        self.w, self.thr = env.family_weights, env.family_thresholds
        # the accumulator of this rank since the last update; n_classes >= 2 as hi >= 1
        self.acc = EpisodeStats(env.E, env.K, gamma, env.n_targets, env.device, across_ranks=False, n_classes=self.n_classes)
        self.sums = torch.zeros((self.n_classes, 8), dtype=torch.float64, device=env.device)       # all ranks, not yet consumed
        self.state = torch.zeros((self.n_classes, 2), dtype=torch.float64, device=env.device)      # (ema, seen) per class
        self.folds = 0

    def fold(self, rec, valid, cls):
        self.acc.fold(rec, valid, cls=cls)
        self.folds += 1
        if self.folds % self.settings.every == 0:
            self.update()

    def update(self):
        new = self.acc.out_by_class
        if D.active():
            new = D.all_reduce_sum_(new.clone())
        self.sums += new
        self.acc.out_by_class.zero_()
        s = self.settings
        ops.family_curriculum_(self.sums, self.state, self.lo, self.hi, s.beta, s.w_min, s.min_episodes, self.w, self.thr)

    def weights_to_host(self):
        """-> a pinned int32 [C] the current weights are on their way to (no wait: read it behind a later event of the stream)."""
        host = torch.empty(self.w.numel(), dtype=torch.int32, pin_memory=True)
        host.copy_(self.w, non_blocking=True)
        return host

    def state_dict(self):
        return dict(state=self.state.cpu(), w=self.w.cpu(), sums=self.sums.cpu(), acc=self.acc.out_by_class.cpu(),
                    folds=int(self.folds), classes=(int(self.lo), int(self.hi)))

    def load_state_dict(self, blob):
        if tuple(int(v) for v in blob["classes"]) != (self.lo, self.hi):
            raise ValueError(f"the checkpoint's curriculum is over the classes {tuple(blob['classes'])}, this run's over "
                             f"{(self.lo, self.hi)}")
        self.state.copy_(blob["state"])
        self.sums.copy_(blob["sums"])
        self.acc.reset()
        self.acc.out_by_class.copy_(blob["acc"])
        self.folds = int(blob["folds"])
        self.w.copy_(blob["w"])
        ops.family_thresholds_(self.thr, self.w)             # the table follows from the weights
