"""CPU: the brute-force restatements of tests/cloud_nn_f64.py agree with the per-query loop that states the definition, with
each other where fp32 and float64 must agree, with the figures the GPU checks are stated for, and -- where scipy is
installed -- with the k-d tree the reference uses."""
import numpy as np
import pytest
import torch

import cloud_nn_cases as C
import cloud_nn_f64 as R

SMALL = ("tiny_1_1", "tiny_5_1", "tiny_5_3")


def small_pairs():
    rng = np.random.default_rng(11)
    out = [C.pair(n) for n in SMALL]
    out.append((rng.random((40, 3)).astype(np.float32), rng.random((60, 3)).astype(np.float32)))
    lattice = lambda n: (rng.integers(0, 4, (n, 3)) / 4.0).astype(np.float32)      # ties and duplicates
    out.append((lattice(30), lattice(50)))
    return out


@pytest.mark.parametrize("cap", (np.inf, 0.0625, 0.25))
@pytest.mark.parametrize("k", (1, 3, 8))
def test_brute_forces_agree_with_the_loop(k, cap):
    for q, s in small_pairs():
        for dtype, fn in ((np.float64, R.knn_f64), (np.float32, R.knn_f32)):
            want_d, want_i = R.knn_loop(q, s, k, cap, dtype)
            got_d, got_i = fn(q, s, k, cap)
            assert got_d.dtype == dtype and got_i.dtype == np.int64 and got_d.shape == (q.shape[0], k)
            assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)
        t_d, t_i = R.knn_f32_torch(torch.from_numpy(q), torch.from_numpy(s), k, float(cap))
        got_d, got_i = R.knn_f32(q, s, k, cap)
        assert np.array_equal(t_i.numpy(), got_i) and np.array_equal(t_d.numpy().view(np.int32), got_d.view(np.int32))
        if cap != np.inf:
            for dtype, fn in ((np.float64, R.pairs_f64), (np.float32, R.pairs_f32)):
                assert np.array_equal(fn(q, s, cap), R.pairs_loop(q, s, cap, dtype))
            assert np.array_equal(R.pairs_f32_torch(torch.from_numpy(q), torch.from_numpy(s), cap).numpy(), R.pairs_f32(q, s, cap))


def test_padding_and_ties():
    q, s = C.pair("tiny_5_3")
    d, i = R.knn_f32(q, s, 8)
    assert (i[:, :3] >= 0).all() and (i[:, 3:] == -1).all() and np.isinf(d[:, 3:]).all() and np.isfinite(d[:, :3]).all()
    s = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1]], np.float32)          # four points at distance 1 of the origin
    d, i = R.knn_f32(np.zeros((1, 3), np.float32), s, 3)
    assert i.tolist() == [[0, 1, 2]] and d.tolist() == [[1.0, 1.0, 1.0]]
    assert R.pairs_f32(np.zeros((1, 3), np.float32), s, 1.0).tolist() == [[0, 0], [0, 1], [0, 2], [0, 3]]
    assert R.pairs_f32(np.zeros((1, 3), np.float32), s, np.nextafter(np.float32(1), np.float32(0))).shape == (0, 2)


def test_the_stated_pair():
    """What the GPU checks of the half-offset pair rest on: fp32 picks float64's neighbours, its distances are within
    2.5e-7, the overlap at 0.05 is 0.5175 and no query lies within 1e-5 r of the threshold."""
    q, s = C.half_pair()
    d64, i64 = R.knn_f64(q, s, 8)
    d32, i32 = R.knn_f32(q, s, 8)
    assert np.array_equal(i32, i64)
    assert (np.abs(d32.astype(np.float64) - d64) / d64).max() <= 2.5e-7
    near = np.sqrt(d64[:, 0])
    assert float(np.mean(near < 0.05)) == 4239 / 8192 == R.overlap_f64(q, s, None, 0.05)      # 0.5175 to four places
    assert np.abs(near - 0.05).min() > 1e-5 * 0.05


@pytest.mark.parametrize("name", ("uniform_257_4097", "uniform_4097_257", "c2_support", "blobs", "outliers_both", "plane"))
def test_against_the_kd_tree(name):
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    q, s = C.pair(name)
    tree = cKDTree(s.astype(np.float64))
    k = min(8, s.shape[0])
    tree_d, tree_i = tree.query(q.astype(np.float64), k=k)
    d64, i64 = R.knn_f64(q, s, k)
    # the tree breaks ties in its own way: compare distances everywhere, indices where a row has no tie
    assert np.allclose(np.sqrt(d64), tree_d.reshape(d64.shape), rtol=1e-12, atol=0)
    untied = (np.diff(d64, axis=1) > 0).all(axis=1) if k > 1 else np.ones(len(q), bool)
    assert np.array_equal(i64[untied], tree_i.reshape(i64.shape)[untied])
    for radius in C.RADII[name]:
        rows = tree.query_ball_point(q.astype(np.float64), radius)
        want = np.array([(i, j) for i, row in enumerate(rows) for j in sorted(row)], dtype=np.int64).reshape(-1, 2)
        # float64 squares the distance, the tree compares the distance itself: pairs on the threshold may differ
        d = ((q.astype(np.float64)[want[:, 0]] - s.astype(np.float64)[want[:, 1]]) ** 2).sum(1) if len(want) else np.zeros(0)
        got = R.pairs_f64(q, s, radius * radius)
        if np.all(np.abs(d - radius * radius) > 1e-12):
            assert np.array_equal(got, want)
        else:
            assert abs(len(got) - len(want)) <= np.sum(np.abs(d - radius * radius) <= 1e-12)
