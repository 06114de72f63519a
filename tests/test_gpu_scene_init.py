"""GPU: gaussreg_amd.scene_init against the brute-force restatements of tests/scene_init_f64.py.

The kernel's result is defined bit for bit (the k smallest j != i under (d, j), d in fp32 in a fixed association), so the
expected values are those of the fp32 brute force, compared with torch.equal on the raw bits; the float64 restatement
bounds the error of `mean` and confirms the neighbours wherever float64 separates them by more than 2^-20 relative.
Expected values never come from the code under test."""
import functools
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import scene_init_f64 as R
from gaussreg_amd import _lib, scene_init, synthetic
from gaussreg_amd.scene_optim import GaussianAdam

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KS = (1, 3, 8)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def cloud(name):
    """-> (N, 3) fp32 numpy."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("uniform"):
        return rng.random((int(name[7:]), 3)).astype(np.float32)
    if name.startswith("c2_"):
        return synthetic.gaussians_c2(int(name[3:]), seed=4)["means3D"]
    if name == "dyadic2048":
        return (rng.integers(0, 32, (2048, 3)) / 8.0).astype(np.float32)
    if name == "identical1000":
        return np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (1000, 1))
    if name == "line1000":
        t = rng.random((1000, 1)).astype(np.float32)
        return (np.array([[1.0, 2.0, -0.5]], np.float32) + t * np.array([[0.0, 3.0, 0.0]], np.float32)).astype(np.float32)
    if name == "diagonal1000":
        t = rng.random((1000, 1)).astype(np.float32)
        return (t * np.array([[1.0, -2.0, 0.5]], np.float32)).astype(np.float32)
    if name == "plane1000":
        p = rng.random((1000, 3)).astype(np.float32)
        p[:, 2] = 0.75
        return p
    if name == "outliers4096":
        p = rng.random((4096, 3)).astype(np.float32)
        far = rng.choice(4096, 41, replace=False)
        p[far[:40]] *= np.float32(100.0)
        p[far[40]] = np.float32(1e6)
        return p
    if name == "translated2000":
        return (rng.random((2000, 3)).astype(np.float32) + np.float32(1e4)).astype(np.float32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The fp32 brute force with as many neighbours as any test asks for, once per cloud; a test takes the first k columns."""
    p = torch.from_numpy(cloud(name)).cuda()
    k = min(8, p.shape[0] - 1)
    dist, index, _ = R.knn_f32_torch(p, k)
    return p, dist, index


def expected_mean(dist, k):
    s = dist[:, 0].clone()
    for t in range(1, k):
        s = s + dist[:, t]
    return s / torch.full_like(s, float(k))


def check_bits(name, k):
    p, dist, index = expected(name)
    got_d, got_i = scene_init.knn(p, k)
    got_m = scene_init.mean_knn_dist2(p, k)
    assert got_d.dtype == torch.float32 and got_i.dtype == torch.int64 and got_m.dtype == torch.float32
    assert got_d.shape == (p.shape[0], k) and got_i.shape == (p.shape[0], k) and got_m.shape == (p.shape[0],)
    bad = (got_i != index[:, :k]).any(dim=1).sum().item()
    assert bad == 0, f"{name} k={k}: {bad} rows with other neighbours"
    assert same_bits(got_d, dist[:, :k])
    assert same_bits(got_m, expected_mean(dist, k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["uniform8192", "c2_8192", "uniform257", "uniform4097"])
def test_general_clouds_are_bit_equal(name, k):
    check_bits(name, k)


@pytest.mark.parametrize("N,k", [(2, 1), (4, 3), (9, 8), (5, 1), (5, 3)])
def test_tiny_clouds_are_bit_equal(N, k):
    check_bits(f"uniform{N}", k)


@pytest.mark.parametrize("k", KS)
def test_ties_and_duplicates(k):
    """Dyadic coordinates: every fp32 distance is exact, so the float64 restatement is the expected value, bit for bit."""
    p = cloud("dyadic2048")
    d64, j64 = R.knn_f64(p, 4)
    assert int((d64[:, 1:] == d64[:, :-1]).any(axis=1).sum()) > 1000 and int((d64[:, 0] == 0).sum()) > 100
    d64, j64 = R.knn_f64(p, k)
    got_d, got_i = scene_init.knn(torch.from_numpy(p).cuda(), k)
    assert np.array_equal(got_i.cpu().numpy(), j64)
    assert np.array_equal(got_d.cpu().numpy().astype(np.float64), d64)
    check_bits("dyadic2048", k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["identical1000", "line1000", "diagonal1000", "plane1000", "outliers4096", "translated2000"])
def test_degenerate_geometry(name, k):
    check_bits(name, k)


@pytest.mark.parametrize("name", ["uniform8192", "c2_8192"])
def test_against_float64(name):
    p, dist, index = expected(name)
    d64, j64 = R.knn_f64(cloud(name), 9)
    gap = (d64[:, 1:] - d64[:, :-1]) / d64[:, 1:]
    for k in KS:
        got_d, got_i = scene_init.knn(p, k)
        got_m = scene_init.mean_knn_dist2(p, k).cpu().numpy().astype(np.float64)
        want_m = d64[:, :k].sum(axis=1) / k
        err = np.abs(got_m - want_m).max()
        err_brute = np.abs(expected_mean(dist, k).cpu().numpy().astype(np.float64) - want_m).max()
        clear = gap[:, :k].min(axis=1) > 2.0 ** -20
        print(f"{name} k={k}: mean error {err:.3e}, brute force {err_brute:.3e}, ratio {err / err_brute:.3f}; "
              f"rows excused {int((~clear).sum())} of {len(clear)}")
        assert err <= 4 * err_brute
        assert (~clear).mean() <= 0.005
        assert np.array_equal(got_i.cpu().numpy()[clear], j64[clear, :k])


def test_relabelling_permutes_the_result():
    p, dist, index = expected("uniform8192")
    d64, _ = R.knn_f64(cloud("uniform8192"), 4)
    assert bool((d64[:, 1:] > d64[:, :-1]).all())  # tie-free
    perm = torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(p.shape[0], device="cuda")
    d, i = scene_init.knn(p, 3)
    dp, ip = scene_init.knn(p[perm].contiguous(), 3)
    assert same_bits(dp, d[perm])
    assert torch.equal(ip, inverse[i[perm]])


def test_two_calls_and_another_stream_give_the_same_bits():
    p = expected("c2_8192")[0]
    d0, i0 = scene_init.knn(p, 8)
    m0 = scene_init.mean_knn_dist2(p, 8)
    d1, i1 = scene_init.knn(p, 8)
    assert same_bits(d0, d1) and torch.equal(i0, i1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d2, i2 = scene_init.knn(p, 8)
        m2 = scene_init.mean_knn_dist2(p, 8)
    side.synchronize()
    assert same_bits(d0, d2) and torch.equal(i0, i2) and same_bits(m0, m2)


def test_every_combination_of_outputs_through_the_c_abi():
    L = _lib.lib()
    p, dist, index = expected("uniform4097")
    N, k, dev = p.shape[0], 3, p.device
    nbytes = L.gr_gs_knn_workspace_bytes(N, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    want = (dist[:, :k].contiguous(), index[:, :k].contiguous(), expected_mean(dist, k))
    for mask in itertools.product((False, True), repeat=3):
        outs = [torch.full_like(w, 77) if on else None for w, on in zip(want, mask)]
        rc = L.gr_gs_knn(_lib.ptr(p), N, k, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(ws), nbytes,
                         _lib.stream_ptr(dev))
        assert rc == 0, L.gr_last_error()
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            if o is not None:
                assert torch.equal(o, w) if o.dtype == torch.int64 else same_bits(o, w), mask


def test_c_abi_refuses_bad_arguments():
    L = _lib.lib()
    p = expected("uniform257")[0]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((257,), 5.0, device="cuda")
    stream = _lib.stream_ptr(p.device)
    assert L.gr_gs_knn_workspace_bytes(257, 0) == 0 and L.gr_gs_knn_workspace_bytes(257, 9) == 0
    assert L.gr_gs_knn_workspace_bytes(3, 3) == 0 and L.gr_gs_knn_workspace_bytes(1 << 31, 3) == 0
    assert L.gr_gs_knn_workspace_bytes((1 << 31) - 1, 3) > 0
    call = lambda pts, n, k, nbytes: L.gr_gs_knn(pts, n, k, None, None, _lib.ptr(out), _lib.ptr(ws), nbytes, stream)
    assert call(_lib.ptr(p), 257, 0, 1 << 20) == -1 and call(_lib.ptr(p), 257, 9, 1 << 20) == -1
    assert call(_lib.ptr(p), 3, 3, 1 << 20) == -1 and call(_lib.ptr(None), 257, 3, 1 << 20) == -1
    assert call(_lib.ptr(p), 257, 3, 64) == -3
    bad = p.clone()
    bad[100, 1] = float("nan")
    assert call(_lib.ptr(bad), 257, 3, 1 << 20) == -1 and b"points must be finite" in L.gr_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())  # no refused call wrote anything


def test_errors():
    p = expected("uniform257")[0]
    for bad in (p[:, :2].contiguous(), p[:, 0].contiguous(), p.double(), p.t().contiguous().t(), p.cpu().numpy()):
        with pytest.raises(ValueError):
            scene_init.knn(bad, 3)
    for k in (0, 9):
        with pytest.raises(ValueError, match="outside 1..8"):
            scene_init.knn(p, k)
        with pytest.raises(ValueError, match="outside 1..8"):
            scene_init.mean_knn_dist2(p, k)
    with pytest.raises(ValueError, match="need more than"):
        scene_init.knn(p[:3].contiguous(), 3)
    for value in (float("nan"), float("inf"), float("-inf")):
        bad = p.clone()
        bad[200, 2] = value
        with pytest.raises(ValueError, match="points must be finite"):
            scene_init.knn(bad, 3)
        with pytest.raises(ValueError, match="points must be finite"):
            scene_init.gaussians_from_points(bad, torch.rand_like(bad))
    with pytest.raises(ValueError, match="no CPU fallback"):
        scene_init.knn(p.cpu(), 3)
    with pytest.raises(ValueError, match="colors"):
        scene_init.gaussians_from_points(p, torch.rand(5, 3, device="cuda"))
    check_bits("uniform257", 3)  # and the next good call is unaffected


def test_simple_knn_alias_runs():
    from simple_knn._C import distCUDA2
    p, dist, _ = expected("uniform4097")
    assert same_bits(distCUDA2(p), expected_mean(dist, 3))


def load_example():
    spec = importlib.util.spec_from_file_location("finetune_scene", os.path.join(ROOT, "examples", "finetune_scene.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_scene_construction_and_one_training_step():
    example = load_example()
    N = 2000
    g = synthetic.gaussians_c2(N, seed=6)
    pts = torch.from_numpy(g["means3D"]).cuda()
    colors = torch.from_numpy(np.random.default_rng(6).random((N, 3)).astype(np.float32)).cuda()
    raw = scene_init.gaussians_from_points(pts, colors, sh_degree=3, initial_opacity=0.1)
    d64, _ = R.knn_f64(g["means3D"], 3)
    want = R.scene_f64(g["means3D"], colors.cpu().numpy(), d64.sum(axis=1) / 3.0, 3, 0.1)
    assert list(raw) == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    for name, t in raw.items():
        assert t.requires_grad and t.is_leaf and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), name
        assert tuple(t.shape) == want[name].shape, name
    assert torch.equal(raw["xyz"], pts) and raw["xyz"].data_ptr() != pts.data_ptr()
    # scaling = log(sqrt(mean)): the mean carries 5 u of its distances and 3 u of its sum and division, halved by the
    # square root; sqrt and log add an ulp each of their results -> well inside 4 ulps of |scaling| >= 1
    s = raw["scaling"].detach().cpu().numpy()
    ulp = np.spacing(np.abs(want["scaling"]).astype(np.float32)).astype(np.float64)
    worst = (np.abs(s.astype(np.float64) - want["scaling"]) / ulp).max()
    print(f"scaling: largest error {worst:.2f} ulps")
    assert worst <= 4.0
    for name in ("f_dc", "f_rest", "opacity", "rotation"):
        assert np.allclose(raw[name].detach().cpu().numpy().astype(np.float64), want[name], rtol=3e-7, atol=1e-7), name
    # straight into GaussianAdam; one rasterize_views + backward + step
    opt = GaussianAdam([{"params": [raw[name]], "lr": lr, "name": name} for name, lr in example.LEARNING_RATES.items()], eps=1e-15)
    cam = synthetic.camera_ring(1, 64, 48, seed=3)[0]
    settings = example.GaussianRasterizationSettings(48, 64, cam["tanfovx"], cam["tanfovy"], torch.zeros(3, device="cuda"), 1.0,
                                                     torch.from_numpy(cam["viewmatrix"]).cuda(),
                                                     torch.from_numpy(cam["projmatrix"]).cuda(), 3,
                                                     torch.from_numpy(cam["campos"]).cuda(), False, False)
    means2D = torch.zeros((1, N, 3), device="cuda", requires_grad=True)
    image, radii = example.render(raw, example.ViewBatch([settings]), means2D)
    assert bool(torch.isfinite(image).all()) and image.sum().item() > 0
    image.sum().backward()
    before = {name: t.detach().clone() for name, t in raw.items()}
    opt.step(visibility=radii)
    torch.cuda.synchronize()
    assert not same_bits(before["opacity"], raw["opacity"]) and not same_bits(before["xyz"], raw["xyz"])
    assert all(bool(torch.isfinite(t).all()) for t in raw.values())


def test_training_from_points():
    example = load_example()
    lines = []
    r = example.finetune(points=20_000, views=4, steps=40, width=64, height=48, optimizer="hip", densify_every=10,
                         from_points=2000, log=lines.append)
    print(f"from points: PSNR {r['before'][1]:.2f} -> {r['after'][1]:.2f} dB, loss {r['before'][0]:.6f} -> {r['after'][0]:.6f}, "
          f"counts {r['counts']}")
    assert r["start"]["xyz"].shape == (2000, 3) and r["start"]["f_rest"].shape == (2000, 15, 3)
    assert r["after"][1] > r["before"][1]
    assert [e["step"] for e in r["densifications"]] == [10, 20, 30]
    assert r["optimizer"].param_groups[0]["name"] == "xyz"
    extent = (r["start"]["xyz"] - r["start"]["xyz"].mean(0)).norm(dim=1).max().item() * 1.1
    assert r["optimizer"].param_groups[0]["lr"] == pytest.approx(extent * scene_init.expon_lr(39, **example.POSITION_LR), rel=1e-6)
