"""Python / float64 restatement of the per-class episode statistics (bridges_episode_stats_by_class): log_episode's fold of
tests/test_gpu_episode_stats.py::Restated with an ended episode of env e filed under cls[e].  Test infrastructure."""
import numpy as np


class RestatedByClass:
    """Per env a running float32 discounted sum restarted at step index 0; at done one episode (float32 sums, i + 1 steps,
    stable(s'), reward == n_targets) appended to the list of class cls[e] -- to no list when cls[e] is outside [0, n_classes);
    run and counted advance either way."""

    def __init__(self, E, K, gamma, n_targets, n_classes, count_first_only=False):
        self.gpow = np.array([gamma ** i for i in range(K)], dtype=np.float32)
        self.run = np.zeros((E, 2), dtype=np.float32)
        self.counted = np.zeros(E, dtype=np.int64)
        self.n_targets, self.count_first_only, self.n_classes = n_targets, count_first_only, n_classes
        self.episodes = [[] for _ in range(n_classes)]

    def fold(self, rec, valid, cls):
        from robotoddler.training import records as R
        for e in np.flatnonzero(valid):
            i = int(rec[e, R.O_NB])
            if i == 0:
                self.run[e] = 0
            g = self.gpow[i]
            rw, lin = np.float32(rec[e, R.O_REWARD]), np.float32(rec[e, R.O_LIN])
            self.run[e, 0] = np.float32(self.run[e, 0] + np.float32(g * rw))
            self.run[e, 1] = np.float32(self.run[e, 1] + np.float32(g * lin))
            if rec[e, R.O_DONE] > 0.5:
                if not (self.count_first_only and self.counted[e] > 0) and 0 <= int(cls[e]) < self.n_classes:
                    self.episodes[int(cls[e])].append((float(self.run[e, 0]), float(self.run[e, 1]), i + 1,
                                                       1.0 if rec[e, R.O_STABLE_N] > 0.5 else 0.0,
                                                       1.0 if rw == self.n_targets else 0.0))
                self.counted[e] += 1

    def sums(self):
        """float64 [n_classes, 8]: the sums the kernel keeps (slots 6 and 7 spare)."""
        out = np.zeros((self.n_classes, 8), dtype=np.float64)
        for c, eps in enumerate(self.episodes):
            ep = np.array(eps, dtype=np.float64).reshape(-1, 5)
            out[c, 0] = len(eps)
            out[c, 1:6] = ep.sum(axis=0)
        return out

    def check(self, out):
        """The comparison of test_gpu_episode_stats.Restated.check, row by row: counts exact, the two float sums to 1e-12 of
        the sum of magnitudes (the kernel adds in another order)."""
        out = np.asarray(out).reshape(self.n_classes, 8)
        for c, eps in enumerate(self.episodes):
            ep = np.array(eps, dtype=np.float64).reshape(-1, 5)
            assert out[c, 0] == len(eps), (c, out[c, 0], len(eps))
            assert out[c, 3] == ep[:, 2].sum() and out[c, 4] == ep[:, 3].sum() and out[c, 5] == ep[:, 4].sum(), c
            for k in (1, 2):
                want = ep[:, k - 1].sum()
                assert abs(out[c, k] - want) <= 1e-12 * (1 + np.abs(ep[:, k - 1]).sum()), (c, k, out[c, k], want)
            assert out[c, 6] == 0 and out[c, 7] == 0
