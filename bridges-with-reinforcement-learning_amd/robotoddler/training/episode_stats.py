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
    evaluation of E envs: E episodes)."""

    def __init__(self, E, K, gamma, n_targets, device, count_first_only=False, across_ranks=True):
        self.E, self.K, self.n_targets = int(E), int(K), int(n_targets)
        self.count_first_only, self.across_ranks = bool(count_first_only), bool(across_ranks)
        self.device = torch.device(device)
        # float32(gamma ** i) with Python's **, as log_episode's  gamma ** i * t.reward  evaluates it on float32 tensors
        self.gpow = torch.tensor([gamma ** i for i in range(self.K)], dtype=torch.float32).to(self.device)
        self.run = torch.zeros((self.E, 2), dtype=torch.float32, device=self.device)
        self.counted = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        self.out = torch.zeros(8, dtype=torch.float64, device=self.device)

    def reset(self):
        """Forget every episode in progress and every sum (the next record of an env must start an episode)."""
        self.run.zero_()
        self.counted.zero_()
        self.out.zero_()

    def fold(self, rec, valid):
        ops.episode_stats_(self.out, rec, valid, self.gpow, self.n_targets, self.run, self.counted, self.count_first_only)

    def take(self):
        """-> DeferredStats of the sums since the last take(); ``out`` is zeroed behind the copy.  No host wait on a single rank."""
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

    def __init__(self, host, done):
        self._host, self._done, self._vals = host, done, None

    def sums(self):
        if self._vals is None:
            self._done.synchronize()
            self._vals = self._host.tolist()
        return self._vals

    def get(self):
        """-> dict(episodes, reward, lin_reward, num_steps, stable, success_rate): the last five are means over the episodes,
        None when no episode ended."""
        s = self.sums()
        n = int(s[0])
        means = [v / n if n else None for v in s[1:6]]
        return dict(episodes=n, reward=means[0], lin_reward=means[1], num_steps=means[2], stable=means[3], success_rate=means[4])
