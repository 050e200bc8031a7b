"""Per-episode statistics of the vectorised loop: what log_episode of the reference reports per episode (successor_dqn.py:479-499
-- the discounted reward and linear reward, the episode length, the final stability) plus whether the episode reached its targets,
folded on the device from every lock-step's records by bridges_episode_stats and read back one lock-step late."""
import torch

from bridges_hip import ops
from robotoddler.training import distributed as D


class EpisodeStats:
    """Running sums of the episodes of E envs.  ``fold(rec, valid)`` after every lock-step's act() (records of this rank, before
    the all-gather); ``take()`` hands the sums collected so far to the host -- summed over the ranks when ``across_ranks`` and a
    process group is active -- and starts afresh.  With ``count_first_only`` only the first episode of every env counts (an
    evaluation of E envs: E episodes).  ``n_classes`` > 1 (a task family: one class per span / height): ``fold`` takes the class
    of every env's episode as well and the sums are kept per class beside the totals (bridges_episode_stats_by_class)."""

    def __init__(self, E, K, gamma, n_targets, device, count_first_only=False, across_ranks=True, n_classes=1):
        self.E, self.K, self.n_targets = int(E), int(K), int(n_targets)
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= 8:
            raise ValueError("n_classes must be 1..8")
        self.count_first_only, self.across_ranks = bool(count_first_only), bool(across_ranks)
        self.device = torch.device(device)
        # float32(gamma ** i) with Python's **, as log_episode's  gamma ** i * t.reward  evaluates it on float32 tensors
        self.gpow = torch.tensor([gamma ** i for i in range(self.K)], dtype=torch.float32).to(self.device)
        self.run = torch.zeros((self.E, 2), dtype=torch.float32, device=self.device)
        self.counted = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        self.out = torch.zeros(8, dtype=torch.float64, device=self.device)
        # per class: rows of the same eight sums; `out` is then their sum, taken in take()
        self.out_by_class = (torch.zeros((self.n_classes, 8), dtype=torch.float64, device=self.device)
                             if self.n_classes > 1 else None)

    def reset(self):
        """Forget every episode in progress and every sum (the next record of an env must start an episode)."""
        self.run.zero_()
        self.counted.zero_()
        self.out.zero_()
        if self.out_by_class is not None:
            self.out_by_class.zero_()

    def fold(self, rec, valid, cls=None):
        """``cls`` int32 [E] (n_classes > 1 only, then required): the class every env's episode is played under."""
        if self.out_by_class is None:
            if cls is not None:
                raise ValueError("fold(cls=...) needs EpisodeStats(n_classes > 1)")
            ops.episode_stats_(self.out, rec, valid, self.gpow, self.n_targets, self.run, self.counted, self.count_first_only)
            return
        if cls is None:
            raise ValueError("EpisodeStats(n_classes > 1): fold() needs the class of every env (cls)")
        ops.episode_stats_by_class_(self.out_by_class, rec, valid, self.gpow, self.n_targets, self.run, self.counted, cls,
                                    self.count_first_only)

    def take(self):
        """-> DeferredStats of the sums since the last take(); ``out`` is zeroed behind the copy.  No host wait on a single rank."""
        if self.out_by_class is not None:
            # the totals of a run by class: every in-range class summed (an out-of-range class is in no row)
            self.out.copy_(self.out_by_class.sum(dim=0))
            both = torch.cat([self.out.unsqueeze(0), self.out_by_class], dim=0)
            if self.across_ranks:
                D.all_reduce_sum_(both)
            host = torch.empty((1 + self.n_classes, 8), dtype=torch.float64, pin_memory=True)
            host.copy_(both, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            self.out.zero_()
            self.out_by_class.zero_()
            return DeferredStats(host, done, n_classes=self.n_classes)
        if self.across_ranks:
            D.all_reduce_sum_(self.out)
        host = torch.empty(8, dtype=torch.float64, pin_memory=True)
        host.copy_(self.out, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.out.zero_()
        return DeferredStats(host, done)


class DeferredStats:
    """Sums of one take() on their way to the host (pinned buffer + event, as DeferredLosses)."""

    def __init__(self, host, done, n_classes=1):
        self._host, self._done, self._vals, self._n_classes = host, done, None, int(n_classes)

    def sums(self):
        if self._vals is None:
            self._done.synchronize()
            self._vals = self._host.tolist()
        return self._vals

    def get(self):
        """-> dict(episodes, reward, lin_reward, num_steps, stable, success_rate): the last five are means over the episodes,
        None when no episode ended.  With n_classes > 1 also by_class: a list of the same dict per class."""
        s = self.sums()
        if self._n_classes > 1:
            out = self._means(s[0])
            out["by_class"] = [self._means(row) for row in s[1:]]
            return out
        return self._means(s)

    @staticmethod
    def _means(s):
        n = int(s[0])
        means = [v / n if n else None for v in s[1:6]]
        return dict(episodes=n, reward=means[0], lin_reward=means[1], num_steps=means[2], stable=means[3], success_rate=means[4])
