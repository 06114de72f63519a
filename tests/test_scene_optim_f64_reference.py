"""CPU: tests/scene_optim_f64.py (the float64 yardstick of the scene optimiser) against torch.optim.Adam on float64
tensors, the definition of the masked step, and a plain loop over views for the densification statistics."""
import numpy as np
import pytest
import torch

import scene_optim_f64 as R
from gaussreg_amd import scene_optim

P = 37
SHAPES = [(P, 3), (P, 1), (P, 15, 3), (P, 4)]
BASE_LR = [1.6e-4, 5e-2, 1.25e-4, 1e-3]


def _params(seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(0.0, 1.0, s) for s in SHAPES]


def _grads(step):
    return [R.seeded_grad(s, 100 * step + i).astype(np.float64) for i, s in enumerate(SHAPES)]


def _lrs(step):
    return [lr * (0.9 ** step) for lr in BASE_LR]  # a schedule: the lr changes every step, per group


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("steps", [1, 2, 25])
def test_dense_step_is_torch_adam(steps):
    init = _params(0)
    ref = R.AdamF64(init)
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in init]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(tp, BASE_LR)], betas=(0.9, 0.999), eps=1e-15,
                           foreach=False)
    for s in range(steps):
        grads, lrs = _grads(s), _lrs(s)
        if s % 3 == 1:
            grads[2] = None  # a parameter without .grad is skipped and its step count does not advance
        for group, lr in zip(opt.param_groups, lrs):
            group["lr"] = lr
        for p, g in zip(tp, grads):
            p.grad = None if g is None else torch.tensor(g)
        opt.step()
        ref.step(grads, lrs)
    for i, p in enumerate(tp):
        st = opt.state[p]
        assert int(st["step"].item()) == ref.t[i]
        for name, got, want in (("p", ref.p[i], p.detach().numpy()), ("exp_avg", ref.m[i], st["exp_avg"].numpy()),
                                ("exp_avg_sq", ref.v[i], st["exp_avg_sq"].numpy())):
            assert _rel(got, want) <= 1e-12, (i, name, _rel(got, want))


def test_masked_step_definition():
    init = _params(1)
    rng = np.random.default_rng(5)
    dense, sparse = R.AdamF64(init), R.AdamF64(init)
    for s in range(4):
        grads, lrs = _grads(s), _lrs(s)
        visible = rng.random(P) < 0.5
        visible[0], visible[1] = True, False
        before = [(p.copy(), m.copy(), v.copy()) for p, m, v in zip(sparse.p, sparse.m, sparse.v)]
        # the dense step from the sparse run's own state: visible rows must equal it, invisible rows must not move
        dense.p, dense.m, dense.v = ([a.copy() for a in x] for x in (sparse.p, sparse.m, sparse.v))
        dense.t = list(sparse.t)
        dense.step(grads, lrs)
        sparse.step(grads, lrs, visible)
        assert sparse.t == dense.t == [s + 1] * len(SHAPES)  # the count is global: it advances for invisible rows too
        for i in range(len(SHAPES)):
            for got, was, full in zip((sparse.p[i], sparse.m[i], sparse.v[i]), before[i], (dense.p[i], dense.m[i], dense.v[i])):
                assert np.array_equal(got[~visible], was[~visible])
                assert np.array_equal(got[visible], full[visible])
                assert not np.array_equal(got[visible], was[visible])


def test_visible_from_radii():
    radii = np.array([[0, 3, 0, -1], [0, 0, 2, 0]], np.int32)
    assert R.visible_from_radii(radii).tolist() == [False, True, True, False]
    assert R.visible_from_radii(radii[0]).tolist() == [False, True, False, False]


def test_statistics_against_a_loop():
    rng = np.random.default_rng(2)
    V = 3
    grad = rng.normal(0.0, 1e-3, (V, P, 3))
    radii = rng.integers(-2, 9, (V, P)).astype(np.int32)
    acc0, den0, rad0 = rng.random(P), rng.integers(0, 5, P), rng.integers(0, 6, P)
    acc, den, rad = R.densify_stats(acc0, den0, rad0, grad, radii)
    for i in range(P):
        a, d, r = float(acc0[i]), int(den0[i]), int(rad0[i])
        for v in range(V):
            if radii[v, i] > 0:
                a += float(np.sqrt(grad[v, i, 0] ** 2 + grad[v, i, 1] ** 2))
                d += 1
                r = max(r, int(radii[v, i]))
        assert abs(acc[i] - a) <= 1e-15 * max(1.0, abs(a)) and den[i] == d and rad[i] == r
    # a batch equals its views one at a time
    one = (acc0, den0, rad0)
    for v in range(V):
        one = R.densify_stats(*one, grad[v:v + 1], radii[v:v + 1])
    assert np.allclose(one[0], acc, rtol=1e-15, atol=0) and np.array_equal(one[1], den) and np.array_equal(one[2], rad)


def test_seeded_grad_range():
    g = R.seeded_grad((4099, 3), 7)
    nz = np.abs(g[g != 0])
    assert g.dtype == np.float32 and (g == 0).any() and nz.min() >= 1e-15 and nz.max() <= 1e-1
    assert nz.min() < 1e-10 and nz.max() > 1e-3


def test_cpu_tensors_are_refused():
    p = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(ValueError, match="no CPU fallback"):
        scene_optim.GaussianAdam([{"params": [p], "lr": 1e-3, "name": "xyz"}])
