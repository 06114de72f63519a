"""GPU: gr_feature_nn (csrc/feature_nn.hip) and the functions on it.

1. bits: every output equals ops.pairwise_distance -- the unchanged operator, not the code under test -- reduced with
   "minimum value, then smallest index holding it", NaN as +inf, on every case of feature_nn_cases, normalized 0 and 1;
2. exact arithmetic and ties: integer-valued features, planted duplicates next to each other, 128 apart and a strip
   (STRIP columns) apart, for rows and for columns; constant features;
3. float64: clear decisions exactly, unclear ones within their threshold, every distance within PD_BOUND * s;
4. edges: empty sides, overflowing and NaN rows, nothing requested, CPU tensors;
5. invariants: repeatability, streams, rows-only / columns-only / both, the swapped call when normalized, permutations;
6. the reference's extract_corr_indices_from_feats / extract_correspondences_from_feats, direct and through the alias;
7. registration_with_ransac_from_feats on planted descriptors.
The worst figures of 3 are printed and kept in docs/feature_nn_f64_errors.md."""
import os

import numpy as np
import pytest
import torch

import feature_nn_cases as C
import feature_nn_f64 as F64

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STRIP = C.TILE * C.strip_tiles(*C.STRIP_SHAPE[:2])      # 256 columns: where a row's running minimum leaves the registers


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _gpu(a, misaligned=False):
    a = np.ascontiguousarray(a)
    if not misaligned:
        return torch.from_numpy(a.copy()).to(_dev())
    store = torch.empty(a.size + 1, dtype=torch.float32, device=_dev())    # the rows start one float into the storage
    t = store[1:].view(a.shape)
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _np(outs):
    return tuple(None if t is None else t.cpu().numpy() for t in outs)


def _oracle(xt, yt, normalized):
    from gaussreg_amd import ops
    return C.reduce_matrix(ops.pairwise_distance(xt, yt, normalized))


def _assert_equal(got, want, what):
    for k, name in enumerate(("row_index", "row_dist2", "col_index", "col_dist2")):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, name)


# ---- 1. bits
@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_bits_equal_pairwise_distance(name, normalized):
    from gaussreg_amd import feature_nn as fnn
    case = C.BY_NAME[name]
    x, y = C.build(name)
    xt, yt = _gpu(x, case.misaligned), _gpu(y, case.misaligned)
    _assert_equal(_np(fnn.feature_nn(xt, yt, normalized)), _oracle(xt, yt, normalized), (name, normalized))


# ---- 2. ties and exact arithmetic
def _planted(n, m, c, seed):
    """Integer features; rows of y copied so that a row of x has two exact nearest neighbours (distance 0) at j and j + 1,
    at j and j + 128, and at j and j + STRIP; the same for columns with copies among the rows of x."""
    x, y = C.integer_features(n, m, c, seed)
    for i, j, step in ((3, 5, 1), (70, 40, C.TILE), (200, 100, STRIP), (129, 127, 1), (300, STRIP - 1, 1),
                       (301, STRIP - 1 - C.TILE, STRIP), (310, m - 1 - STRIP, STRIP)):
        y[j] = x[i]
        y[j + step] = x[i]
    for j, i, step in ((9, 11, 1), (77, 300 + 17, C.TILE), (250, 400, STRIP), (131, 127 + 512, 1), (260, n - 1 - C.TILE, C.TILE)):
        x[i] = y[j]
        x[i + step] = y[j]
    return x, y


def _exact_reference(x, y):
    d = F64.F.pairwise_distance(x, y, False)
    ri, ci = d.argmin(1), d.argmin(0)       # (first of equal minima)
    return (ri.astype(np.int64), d[np.arange(d.shape[0]), ri].astype(np.float32), ci.astype(np.int64),
            d[ci, np.arange(d.shape[1])].astype(np.float32))


@pytest.mark.parametrize("n,m,c", [(900, 1000, 64), (1100, 900, 13)])
def test_exact_integer_features_and_planted_ties(n, m, c):
    from gaussreg_amd import feature_nn as fnn
    x, y = _planted(n, m, c, seed=n + c)
    want = _exact_reference(x, y)
    # the planted pairs are exact ties and the lower index wins
    d = F64.F.pairwise_distance(x, y, False)
    assert (d[3, 5], d[3, 6], want[0][3]) == (0, 0, 5) and (d[70, 40], d[70, 40 + C.TILE], want[0][70]) == (0, 0, 40)
    assert (d[200, 100], d[200, 100 + STRIP]) == (0, 0) and want[0][200] <= 100
    assert (d[11, 9], d[12, 9]) == (0, 0) and want[2][9] <= 11
    _assert_equal(_np(fnn.feature_nn(_gpu(x), _gpu(y))), want, (n, m, c))


def test_planted_ties_across_strips():
    """The strip case's shape (strips of STRIP = 256 columns, several row tiles): duplicates a strip apart, in both
    directions, with integer features."""
    from gaussreg_amd import feature_nn as fnn
    n, m, _ = C.STRIP_SHAPE
    assert C.strip_tiles(n, m) * C.TILE == STRIP
    x, y = _planted(n, m, 8, seed=5)
    for i, j in ((2000, 255), (2001, 256), (4099, 4199 - STRIP)):     # the last column of a strip, the first of the next
        y[j] = x[i]
        y[j + STRIP] = x[i]
    want = _exact_reference(x, y)
    _assert_equal(_np(fnn.feature_nn(_gpu(x), _gpu(y))), want, "strip")


@pytest.mark.parametrize("n,m,c", [(300, 520, 5), (1, 1, 3), (130, 129, 64)])
def test_constant_features_pick_index_zero(n, m, c):
    from gaussreg_amd import feature_nn as fnn
    x, y = np.full((n, c), 2.0, np.float32), np.full((m, c), 2.0, np.float32)
    ri, rd, ci, cd = _np(fnn.feature_nn(_gpu(x), _gpu(y)))
    assert not ri.any() and not ci.any() and not rd.any() and not cd.any()
    y = y + 1.0                                   # every distance c, still all equal
    ri, rd, ci, cd = _np(fnn.feature_nn(_gpu(x), _gpu(y)))
    assert not ri.any() and not ci.any() and (rd == c).all() and (cd == c).all()


# ---- 3. float64
NORMALIZED_F64 = ("1300x1200x36_unit", "65x63x33_gauss", "2000x1500x32_gauss")


@pytest.mark.parametrize("name,normalized", [(n, False) for n in C.F64_CASES] + [(n, True) for n in NORMALIZED_F64])
def test_float64(name, normalized):
    from gaussreg_amd import feature_nn as fnn
    x, y, ref = F64.reference(name, normalized)
    fig = F64.compare(ref, _np(fnn.feature_nn(_gpu(x), _gpu(y), normalized)))
    print(f"feature_nn f64 {name} normalized={int(normalized)}: " + " ".join(f"{k}={v:.4g}" for k, v in fig.items()))
    assert fig["row_unclear"] <= C.UNCLEAR_CAP and fig["col_unclear"] <= C.UNCLEAR_CAP


# ---- 4. edges
def test_empty_sides():
    from gaussreg_amd import feature_nn as fnn
    x, e = _gpu(np.ones((5, 7), np.float32)), torch.empty((0, 7), dtype=torch.float32, device=_dev())
    ri, rd, ci, cd = _np(fnn.feature_nn(x, e))
    assert ri.tolist() == [-1] * 5 and np.isposinf(rd).all() and rd.dtype == np.float32 and ci.shape == cd.shape == (0,)
    ri, rd, ci, cd = _np(fnn.feature_nn(e, x))
    assert ci.tolist() == [-1] * 5 and np.isposinf(cd).all() and ri.shape == rd.shape == (0,)
    ri, rd, ci, cd = _np(fnn.feature_nn(e, e))
    assert ri.shape == rd.shape == ci.shape == cd.shape == (0,)
    dist2, index = fnn.nearest(x, e)
    assert index.tolist() == [-1] * 5 and torch.isposinf(dist2).all()


def test_overflowing_and_nan_rows_are_ordered_last():
    from gaussreg_amd import feature_nn as fnn
    x, y = (a.copy() for a in C.build("200x130x256_gauss"))
    base = _np(fnn.feature_nn(_gpu(x), _gpu(y)))
    y[17] = 1e30          # the norm overflows: d = +inf, or NaN (inf - inf) against ...
    x[40] = 1e30          # ... a row whose norm overflows too
    y[90] = np.nan
    x[7, 3] = np.nan
    xt, yt = _gpu(x), _gpu(y)
    got = _np(fnn.feature_nn(xt, yt))
    _assert_equal(got, _oracle(xt, yt, False), "overflow")
    ri, rd, ci, cd = got
    assert np.isposinf(rd[[40, 7]]).all() and ri[40] == ri[7] == 0          # all equal (+inf): index 0
    assert np.isposinf(cd[[17, 90]]).all() and ci[17] == ci[90] == 0
    assert not np.isin(ri, (17, 90))[np.isfinite(rd)].any() and not np.isin(ci, (40, 7))[np.isfinite(cd)].any()
    keep_r = ~np.isin(np.arange(200), (40, 7)) & ~np.isin(base[0], (17, 90))   # rows whose answer was not one of the spoilt
    keep_c = ~np.isin(np.arange(130), (17, 90)) & ~np.isin(base[2], (40, 7))
    assert np.array_equal(ri[keep_r], base[0][keep_r]) and np.array_equal(rd[keep_r], base[1][keep_r])
    assert np.array_equal(ci[keep_c], base[2][keep_c]) and np.array_equal(cd[keep_c], base[3][keep_c])


def test_nothing_requested_and_cpu_tensors_raise():
    from gaussreg_amd import _lib
    from gaussreg_amd import feature_nn as fnn
    x = _gpu(np.ones((5, 7), np.float32))
    with pytest.raises(ValueError, match="neither"):
        fnn.feature_nn(x, x, rows=False, cols=False)
    ws = torch.empty(4096, dtype=torch.uint8, device=_dev())
    L = _lib.lib()
    rc = L.gr_feature_nn(x.data_ptr(), 5, x.data_ptr(), 5, 7, 0, None, None, None, None, ws.data_ptr(), 4096, None)
    assert rc != 0 and b"neither" in L.gr_last_error()
    idx = torch.empty(5, dtype=torch.int64, device=_dev())
    rc = L.gr_feature_nn(x.data_ptr(), 5, x.data_ptr(), 5, 7, 0, idx.data_ptr(), None, None, None, ws.data_ptr(), 4096, None)
    assert rc != 0 and b"together" in L.gr_last_error()
    for call in (lambda: fnn.nearest(x.cpu(), x), lambda: fnn.mutual_nearest(x, x.cpu()),
                 lambda: fnn.extract_corr_indices_from_feats(x.cpu(), x.cpu())):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="channels"):
        fnn.nearest(x, x[:, :3].contiguous())
    with pytest.raises(ValueError, match="float32"):
        fnn.nearest(x.double(), x.double())


# ---- 5. invariants
def test_repeatable_streams_and_directions():
    from gaussreg_amd import feature_nn as fnn
    for name, normalized in (("1700x1700x16_gauss", False), ("4100x4200x8_gauss_strip", False), ("129x257x17_gauss", True)):
        x, y = C.build(name)
        xt, yt = _gpu(x), _gpu(y)
        first = _np(fnn.feature_nn(xt, yt, normalized))
        _assert_equal(_np(fnn.feature_nn(xt, yt, normalized)), first, (name, "again"))
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            other = fnn.feature_nn(xt, yt, normalized)
        stream.synchronize()
        _assert_equal(_np(other), first, (name, "stream"))
        ri, rd, none_i, none_d = fnn.feature_nn(xt, yt, normalized, cols=False)
        assert none_i is None and none_d is None
        _, _, ci, cd = fnn.feature_nn(xt, yt, normalized, rows=False)
        _assert_equal(_np((ri, rd, ci, cd)), first, (name, "one direction"))
        dist2, index = fnn.nearest(xt, yt, normalized)
        assert np.array_equal(index.cpu().numpy(), first[0]) and np.array_equal(dist2.cpu().numpy(), first[1])
        assert torch.equal(fnn.nearest(xt, yt, normalized, return_index=False), dist2)


@pytest.mark.parametrize("name", ["1300x1200x36_unit", "129x257x17_gauss"])
def test_normalized_columns_are_the_rows_of_the_swapped_call(name):
    from gaussreg_amd import feature_nn as fnn
    x, y = C.build(name)
    xt, yt = _gpu(x), _gpu(y)
    ri, rd, ci, cd = _np(fnn.feature_nn(xt, yt, True))
    si, sd, ti, td = _np(fnn.feature_nn(yt, xt, True))
    assert np.array_equal(ci, si) and np.array_equal(cd, sd) and np.array_equal(ri, ti) and np.array_equal(rd, td)


def test_permuting_y_permutes_the_row_index():
    from gaussreg_amd import feature_nn as fnn
    x, y = C.build("2000x1500x32_gauss")          # N(0,1) rows: no two distances of a row are equal
    perm = np.random.default_rng(3).permutation(y.shape[0])
    ri, rd, _, _ = _np(fnn.feature_nn(_gpu(x), _gpu(y)))
    pi, pd, _, _ = _np(fnn.feature_nn(_gpu(x), _gpu(y[perm])))
    assert np.array_equal(perm[pi], ri) and np.array_equal(pd, rd)


# ---- 6. the reference's functions
@pytest.fixture(scope="module")
def corr_case():
    x, y = C.build("1300x1200x36_unit")           # every 7th row of y is a copy of a row of x: mutual pairs exist
    xt, yt = _gpu(x), _gpu(y)
    ri, _, ci, _ = _oracle(xt, yt, False)
    rng = np.random.default_rng(11)
    return {"x": x, "y": y, "xt": xt, "yt": yt, "ri": ri, "ci": ci,
            "px": rng.random((x.shape[0], 3)).astype(np.float32), "py": rng.random((y.shape[0], 3)).astype(np.float32)}


@pytest.mark.parametrize("mutual,bilateral", [(False, False), (True, False), (False, True), (True, True)])
def test_extract_corr_indices(corr_case, mutual, bilateral):
    from gaussreg_amd import feature_nn as fnn
    from geotransformer.utils import registration as alias
    k = corr_case
    want = C.reference_corr_indices(k["ri"], k["ci"], k["x"].shape[0], k["y"].shape[0], mutual, bilateral)
    assert not mutual or 100 < want[0].shape[0] < k["x"].shape[0]
    got = fnn.extract_corr_indices_from_feats(k["xt"], k["yt"], mutual=mutual, bilateral=bilateral)
    assert all(g.is_cuda and g.dtype == torch.int64 for g in got)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    from_np = alias.extract_corr_indices_from_feats(np.array(k["x"]), np.array(k["y"]), mutual, bilateral)
    from_t = alias.extract_corr_indices_from_feats(k["xt"], k["yt"], mutual=mutual, bilateral=bilateral)
    for a, t, w in zip(from_np, from_t, want):
        assert isinstance(a, np.ndarray) and a.dtype == np.int64 and np.array_equal(a, w)
        assert isinstance(t, torch.Tensor) and np.array_equal(t.cpu().numpy(), w)


@pytest.mark.parametrize("mutual", [False, True])
def test_extract_correspondences(corr_case, mutual):
    import gaussreg_amd
    from geotransformer.utils import registration as alias
    k = corr_case
    ref_c, src_c = C.reference_corr_indices(k["ri"], k["ci"], k["x"].shape[0], k["y"].shape[0], mutual, False)
    want = [k["px"][ref_c], k["py"][src_c], np.linalg.norm(k["x"][ref_c] - k["y"][src_c], axis=1)]
    got = gaussreg_amd.extract_correspondences_from_feats(_gpu(k["px"]), _gpu(k["py"]), k["xt"], k["yt"], mutual=mutual,
                                                          return_feat_dist=True)
    assert isinstance(got, list) and len(got) == 3
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    np.testing.assert_allclose(got[2].cpu().numpy(), want[2], rtol=1e-5, atol=1e-6)   # fp32 norm of a gathered difference
    two = gaussreg_amd.extract_correspondences_from_feats(_gpu(k["px"]), _gpu(k["py"]), k["xt"], k["yt"], mutual=mutual)
    assert len(two) == 2 and torch.equal(two[0], got[0]) and torch.equal(two[1], got[1])
    from_np = alias.extract_correspondences_from_feats(k["px"], k["py"], np.array(k["x"]), np.array(k["y"]), mutual, True)
    assert len(from_np) == 3 and all(isinstance(a, np.ndarray) for a in from_np)
    assert np.array_equal(from_np[0], want[0]) and np.array_equal(from_np[1], want[1])
    np.testing.assert_allclose(from_np[2], want[2], rtol=1e-5, atol=1e-6)


def test_golden_reference_outputs(golden_dir):
    """tests/golden/feature_corr.npz: planted, well-separated descriptors and what the reference's own functions (scipy's
    cKDTree on the host) return for them; no decision in it is unclear, so the index arrays are equal exactly."""
    from gaussreg_amd import feature_nn as fnn
    g = np.load(os.path.join(golden_dir, "feature_corr.npz"))
    ref_f, src_f = _gpu(g["ref_feats"]), _gpu(g["src_feats"])
    for tag, kw in (("plain", {}), ("mutual", {"mutual": True}), ("bilateral", {"bilateral": True})):
        got = fnn.extract_corr_indices_from_feats(ref_f, src_f, **kw)
        assert np.array_equal(got[0].cpu().numpy(), g[tag + "_ref"]) and np.array_equal(got[1].cpu().numpy(), g[tag + "_src"]), tag
    for tag, mutual in (("corr", False), ("corr_mutual", True)):
        got = fnn.extract_correspondences_from_feats(_gpu(g["ref_points"]), _gpu(g["src_points"]), ref_f, src_f, mutual=mutual,
                                                     return_feat_dist=True)
        assert np.array_equal(got[0].cpu().numpy(), g[tag + "_ref_points"])
        assert np.array_equal(got[1].cpu().numpy(), g[tag + "_src_points"])
        np.testing.assert_allclose(got[2].cpu().numpy(), g[tag + "_feat_dists"], rtol=1e-5, atol=1e-6)


# ---- 7. RANSAC from descriptors
def _rotation_translation_ok(est, T):
    # the bars of tests/test_gpu_next.py::test_ransac_similarity_recovers_planted_transform
    np.testing.assert_allclose(est[:3, :3], T[:3, :3], atol=5e-3)
    np.testing.assert_allclose(est[:3, 3], T[:3, 3], atol=2e-2)
    assert est[3].tolist() == [0, 0, 0, 1]


def test_ransac_from_descriptors_recovers_the_motion():
    from gaussreg_amd import feature_nn as fnn
    from gaussreg_amd.registration import registration_with_ransac_from_feats
    from gaussreg_amd.synthetic import descriptor_pair
    p = descriptor_pair(n=2000, c=32, outlier_frac=0.3, seed=1)
    src, ref, sf, rf = (_gpu(p[k]) for k in ("src_points", "ref_points", "src_feats", "ref_feats"))
    shares = {}
    for mutual in (False, True):
        est = registration_with_ransac_from_feats(src, ref, sf, rf, distance_threshold=0.05, num_iterations=5000, mutual=mutual)
        assert est.shape == (4, 4) and est.dtype == torch.float32 and est.is_cuda
        _rotation_translation_ok(est.cpu().numpy().astype(np.float64), p["transform"])
        si, ri = (t.cpu().numpy() for t in fnn.extract_corr_indices_from_feats(sf, rf, mutual=mutual))
        shares[mutual] = float((p["perm"][si] == ri).mean())
        assert si.shape[0] >= 1000
    assert 0.6 < shares[False] < 0.8 and shares[True] >= shares[False]
