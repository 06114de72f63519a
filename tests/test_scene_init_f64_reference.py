"""CPU: tests/scene_init_f64.py against a per-point Python loop; the fp32 brute force against float64 on uniform clouds (the
same neighbours on every row, so the GPU test can demand bit-equality with it and equality of indices with float64);
expon_lr at hand-computed steps; gaussians_from_points' formulas on the CPU path; the simple_knn alias."""
import math

import numpy as np
import pytest
import torch

import scene_init_f64 as R
from gaussreg_amd import scene_init


def test_brute_force_matches_the_loop():
    rng = np.random.default_rng(0)
    p = rng.random((40, 3)).astype(np.float32)
    p[7] = p[3]      # a duplicate: a neighbour at distance 0, the lower index first for everyone else
    p[11] = p[3]
    for k in (1, 3, 8):
        d_loop, j_loop = R.knn_loop(p, k)
        d64, j64 = R.knn_f64(p, k, chunk=16)
        assert np.array_equal(j64, j_loop)
        assert np.allclose(d64, d_loop, rtol=1e-15, atol=0)
        d32, j32, m32 = R.knn_f32(p, k, chunk=16)
        assert np.array_equal(j32, j_loop)
        dt, jt, mt = R.knn_f32_torch(torch.from_numpy(p), k, chunk=16)
        assert np.array_equal(jt.numpy(), j32) and np.array_equal(dt.numpy().view(np.uint32), d32.view(np.uint32))
        assert np.array_equal(mt.numpy().view(np.uint32), m32.view(np.uint32))
    assert list(j_loop[3][:2]) == [7, 11] and list(j_loop[7][:2]) == [3, 11] and d_loop[3][0] == 0.0


def test_mean_is_a_left_to_right_sum_and_a_division():
    d = np.array([[0.1, 0.2, 0.7]], np.float32)
    want = np.float32(np.float32(np.float32(d[0, 0] + d[0, 1]) + d[0, 2]) / np.float32(3.0))
    assert R.mean_f32(d)[0] == want


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fp32_brute_force_agrees_with_float64_on_uniform_clouds(seed):
    p = np.random.default_rng(seed).random((4096, 3)).astype(np.float32)
    d64, j64 = R.knn_f64(p, 9)
    d32, j32, _ = R.knn_f32(p, 8)
    gap = (d64[:, 1:] - d64[:, :-1]) / d64[:, 1:]
    close = int((gap.min(axis=1) < 2.0 ** -20).sum())
    rel = float((np.abs(d32.astype(np.float64) - d64[:, :8]) / d64[:, :8]).max())
    print(f"seed {seed}: rows with a relative gap below 2^-20: {close}, largest relative distance error {rel:.3e}")
    # (seeds 0 and 1 have no such row, seed 2 has one, between its 8th and 9th neighbour; the neighbours still agree)
    # u = 2^-24 per rounding: the difference (doubled by the square), the square, the two sums -> at most 5 u
    assert rel < 5 * 2.0 ** -24
    for k in (1, 3, 8):  # the first k of the 8 are the k nearest
        assert np.array_equal(j32[:, :k], j64[:, :k])


def test_expon_lr():
    # hand-computed: log-linear between 1.6e-4 and 1.6e-6 over 30 000 steps, sine ramp from 0.01 over 1 000 steps
    kw = dict(lr_init=1.6e-4, lr_final=1.6e-6, lr_delay_steps=1000, lr_delay_mult=0.01, max_steps=30_000)
    assert scene_init.expon_lr(0, **kw) == pytest.approx(1.6e-6, rel=1e-12)                       # 0.01 * lr_init
    assert scene_init.expon_lr(1000, **kw) == pytest.approx(1.6e-4 * 10.0 ** (-2.0 / 30.0), rel=1e-12)  # ramp done
    assert scene_init.expon_lr(500, **kw) == pytest.approx((0.01 + 0.99 * math.sin(math.pi / 4)) * 1.6e-4 * 10.0 ** (-1.0 / 30.0),
                                                          rel=1e-12)
    assert scene_init.expon_lr(30_000, **kw) == pytest.approx(1.6e-6, rel=1e-12)
    assert scene_init.expon_lr(45_000, **kw) == pytest.approx(1.6e-6, rel=1e-12)                  # clamped
    assert scene_init.expon_lr(15_000, 1.6e-4, 1.6e-6) == pytest.approx(1.6e-5, rel=1e-12)        # no delay: geometric mean
    assert scene_init.expon_lr(0, 1.6e-4, 1.6e-6) == pytest.approx(1.6e-4, rel=1e-12)
    assert scene_init.expon_lr(-1, 1.6e-4, 1.6e-6) == 0.0 and scene_init.expon_lr(5, 0.0, 0.0) == 0.0
    for step in (0, 1, 250, 999, 1000, 1001, 29_999, 30_000):
        assert scene_init.expon_lr(step, **kw) == pytest.approx(R.expon_lr_f64(step, **kw), rel=1e-12)


@pytest.mark.parametrize("sh_degree", [0, 3])
def test_scene_formulas_on_the_cpu_path(sh_degree):
    rng = np.random.default_rng(5)
    N = 300
    p = rng.random((N, 3)).astype(np.float32)
    p[10] = p[11] = p[12] = p[13]  # four identical points: mean distance 0, the 1e-7 floor
    colors = rng.random((N, 3)).astype(np.float32)
    _, _, mean = R.knn_f32(p, 3)
    assert mean[10] == 0.0
    got = scene_init.scene_from_dist2(torch.from_numpy(p), torch.from_numpy(colors), torch.from_numpy(mean), sh_degree, 0.1)
    want = R.scene_f64(p, colors, mean, sh_degree, 0.1)
    assert list(got) == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    for name, t in got.items():
        assert t.requires_grad and t.is_leaf and t.dtype == torch.float32 and t.is_contiguous(), name
        assert tuple(t.shape) == want[name].shape, name
        assert np.allclose(t.detach().numpy().astype(np.float64), want[name], rtol=1e-6, atol=1e-7), name
    assert got["f_rest"].shape[1] == (sh_degree + 1) ** 2 - 1
    assert got["scaling"][10, 0].item() == pytest.approx(math.log(math.sqrt(1e-7)), rel=1e-6)
    assert got["opacity"][0, 0].item() == pytest.approx(math.log(0.1 / 0.9), rel=1e-6)


def test_simple_knn_alias():
    from simple_knn._C import distCUDA2
    assert distCUDA2.__module__ == "simple_knn._C"
    import inspect
    source = inspect.getsource(distCUDA2)
    assert "mean_knn_dist2(points, 3)" in source and len(source.strip().splitlines()) <= 3


def test_argument_errors_need_no_gpu():
    p = torch.rand(10, 3)
    for bad in (torch.rand(10, 2), torch.rand(10), torch.rand(10, 3, dtype=torch.float64), torch.rand(3, 10).t()):
        with pytest.raises(ValueError):
            scene_init.knn(bad, 3)
    for k in (0, 9, 10, 2.0):
        with pytest.raises(ValueError):
            scene_init.knn(p, k)
    with pytest.raises(ValueError, match="no CPU fallback"):
        scene_init.mean_knn_dist2(p, 3)
