"""NumPy float64 restatement of gaussreg_amd.scene_optim: the Adam step with optional per-Gaussian visibility, and the
densification statistics.  The yardstick of tests/test_gpu_scene_optim.py; pinned on the CPU by
tests/test_scene_optim_f64_reference.py (torch.optim.Adam in float64, a plain loop for the statistics).

Step t (the optimiser's global count, 1-based), per element of a visible Gaussian:
    m = beta1 m + (1 - beta1) g
    v = beta2 v + (1 - beta2) g g
    p = p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
An invisible Gaussian keeps p, m and v: nothing decays, but t advances for everybody.
"""
import numpy as np


class AdamF64:
    """State of one scene: lists of float64 arrays of shape (P, ...), one per group."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-15):
        self.p = [np.array(p, dtype=np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)  # per group, as torch counts: a step without a gradient does not count
        self.betas, self.eps = betas, eps

    def step(self, grads, lrs, visible=None):
        """grads[i]: array like p[i] or None (group skipped); lrs[i]: this step's lr; visible: (P,) bool or None."""
        beta1, beta2 = self.betas
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.t[i] += 1
            t = self.t[i]
            g = np.asarray(g, dtype=np.float64)
            m = beta1 * self.m[i] + (1.0 - beta1) * g
            v = beta2 * self.v[i] + (1.0 - beta2) * g * g
            bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
            p = self.p[i] - (lrs[i] / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + self.eps)
            if visible is None:
                self.p[i], self.m[i], self.v[i] = p, m, v
            else:
                rows = np.asarray(visible, dtype=bool)
                self.p[i][rows], self.m[i][rows], self.v[i][rows] = p[rows], m[rows], v[rows]


def visible_from_radii(radii):
    """(V, P) or (P,) int radii -> (P,) bool: seen by any view."""
    r = np.asarray(radii)
    return (r.reshape(-1, r.shape[-1]) > 0).any(axis=0)


def densify_stats(grad_accum, denom, max_radii, means2D_grad, radii):
    """Returns the updated (grad_accum f64, denom i64, max_radii i64); means2D_grad (V, P, 3), radii (V, P)."""
    g = np.asarray(means2D_grad, dtype=np.float64)
    r = np.asarray(radii, dtype=np.int64)
    seen = r > 0
    norm = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2)
    return (np.asarray(grad_accum, np.float64) + np.where(seen, norm, 0.0).sum(axis=0),
            np.asarray(denom, np.int64) + seen.sum(axis=0),
            np.maximum(np.asarray(max_radii, np.int64), np.where(seen, r, 0).max(axis=0)))


def seeded_grad(shape, seed):
    """fp32 gradient for the accuracy tests: magnitudes 10^U(-12, -1), random signs, about one in eight exactly zero.
    Every non-zero |g| is >= 1e-12 > 1e-15, so g^2 is a normal fp32 number."""
    rng = np.random.default_rng(seed)
    g = 10.0 ** rng.uniform(-12.0, -1.0, shape) * rng.choice([-1.0, 1.0], shape)
    g[rng.random(shape) < 0.125] = 0.0
    return g.astype(np.float32)
