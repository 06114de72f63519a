"""The three evaluations of GeometricStructureEmbedding (function tables, split-bf16 MFMA, fp32 MFMA; gaussreg_amd/csrc/
geo_embedding.hip) against the float64 restatement of tests/geo_embedding_f64.py, on the cases of tests/geo_embedding_cases.py.

Dyadic cases are held to helpers.assert_as_exact_as_reference over the WHOLE output tensor, diagonal included:
|hip - f64| <= 1e-5 scale, |hip - ref32| <= 1e-5 scale and |hip - f64| <= 8 |ref32 - f64| + 1e-7 scale.  A marked case
(largest index above 100: no fp32 sine can meet 1e-5 of the scale against float64 there, see the case table) keeps the
last two.  Generic clouds carry index noise by design: they are held to the fp32 restatement off the diagonal at rtol =
atol = 5e-5 and their float64 figures are printed only.  Each case prints a "GSEF64" row; docs/geo_embedding_f64_errors.md
holds the rows of an MI355X run.
"""
import functools

import numpy as np
import pytest
import torch

import geo_embedding_cases as GC
import geo_embedding_f64 as F
from helpers import assert_as_exact_as_reference

pytestmark = pytest.mark.gpu

GR_OK, GR_ERR_INVALID, GR_ERR_WORKSPACE = 0, -1, -3


def _c(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _state(params):
    return {"embedding.div_term": torch.from_numpy(params["div"]), "proj_d.weight": torch.from_numpy(params["w_d"]),
            "proj_d.bias": torch.from_numpy(params["b_d"]), "proj_a.weight": torch.from_numpy(params["w_a"]),
            "proj_a.bias": torch.from_numpy(params["b_a"])}


def _module(cfg, params, mode, device="cuda"):
    from gaussreg_amd.embedding import GeometricStructureEmbedding
    m = GeometricStructureEmbedding(cfg.C, cfg.sigma_d, cfg.sigma_a, cfg.k, reduction_a=cfg.red, fp32_mfma=mode == "fp32",
                                    mode="table" if mode == "table" else "gemm")
    m.load_state_dict(_state(params))
    return m.to(device)


def _params_of(m):
    g = lambda t: t.detach().cpu().numpy().copy()
    return {"w_d": g(m.proj_d.weight), "b_d": g(m.proj_d.bias), "w_a": g(m.proj_a.weight), "b_a": g(m.proj_a.bias),
            "div": g(m.embedding.div_term)}


def _refs(pts, params, cfg):
    return tuple(F.embedding(pts, params, cfg.sigma_d, cfg.sigma_a, cfg.k, cfg.red, dt) for dt in (np.float32, np.float64))


@functools.lru_cache(maxsize=None)
def _built(name):
    cfg = GC.BY_NAME[name]
    pts, params = GC.build(cfg)
    return (pts, params) + _refs(pts, params, cfg)


def _hold(what, got, r32, r64, marked=False, kernel=""):
    """Print the figures, then assert the bar over the whole tensor."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == r64.shape and np.isfinite(got).all(), what
    e_hip = np.abs(got.astype(np.float64) - r64).max()
    e_ref = np.abs(r32.astype(np.float64) - r64).max()
    e_32 = np.abs(got.astype(np.float64) - r32).max()
    scale = np.abs(r64).max()
    print(f"GSEF64 | {what} | {kernel} | {scale:.3e} | {e_hip:.3e} | {e_ref:.3e} | {e_hip / scale:.2e} | "
          f"{e_hip / max(e_ref, 1e-300):.2f} | {e_32 / scale:.2e} |")
    if marked:
        assert e_32 <= 1e-5 * scale, f"{what}: max |hip - ref32| = {e_32:.3e}, scale {scale:.3g}"
        assert e_hip <= 8.0 * e_ref + 1e-7 * scale, f"{what}: |hip - f64| = {e_hip:.3e} vs |ref32 - f64| = {e_ref:.3e}"
    else:
        assert_as_exact_as_reference(got, r32, r64, what=what)


def _run(cfg, params, mode, pts):
    return _module(cfg, params, mode)(_c(pts)[None])[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", [c for c in GC.CASES if c.cfg.dyadic], ids=lambda c: c.name)
def test_embedding_matches_float64(case):
    cfg = case.cfg
    pts, params, r32, r64 = _built(cfg.name)
    got = _run(cfg, params, case.mode, pts)
    _hold(case.name, got, r32, r64, cfg.marked, GC.kernel_of(cfg.C, case.mode))


@pytest.mark.parametrize("case", [c for c in GC.CASES if not c.cfg.dyadic], ids=lambda c: c.name)
def test_embedding_on_generic_clouds(case):
    cfg = case.cfg
    pts, params, r32, r64 = _built(cfg.name)
    got = _run(cfg, params, case.mode, pts)
    off = ~np.eye(len(pts), dtype=bool)
    e_hip, e_ref, scale = np.abs(got - r64)[off].max(), np.abs(r32 - r64)[off].max(), np.abs(r64).max()
    print(f"GSEF64-GENERIC | {case.name} | {GC.kernel_of(cfg.C, case.mode)} | {scale:.3e} | {e_hip:.3e} | {e_ref:.3e} | "
          f"{e_hip / scale:.2e} | {e_hip / e_ref:.2f} | diagonal {np.abs(got - r64)[~off].max() / scale:.2e} |")
    np.testing.assert_allclose(got[off], r32[off], rtol=5e-5, atol=5e-5)


@pytest.mark.parametrize("cfg", [c for c in GC.CONFIGS if c.dyadic and len(c.modes) > 1], ids=lambda c: c.name)
def test_evaluations_agree_with_each_other(cfg):
    pts, params, _, r64 = _built(cfg.name)
    outs = {mode: _run(cfg, params, mode, pts).astype(np.float64) for mode in cfg.modes}
    scale = np.abs(r64).max()
    modes = list(cfg.modes)
    for i, a in enumerate(modes):
        for b in modes[i + 1:]:
            d = np.abs(outs[a] - outs[b]).max()
            assert d <= 2e-5 * scale, f"{cfg.name}: {a} and {b} differ by {d / scale:.2e} of the scale"


@pytest.mark.parametrize("name,rows_d", [("w64", 4), ("w64", 32 * 20 + 4), ("w20", 32 * 9 + 4), ("weights-x4", 32 * 12 + 3)])
def test_truncated_distance_table_switches_to_direct_evaluation(name, rows_d):
    """gr_geo_embedding_table with only the first rows of the distance table: indices the short table cannot serve
    (m + 3 > rows - 1) are evaluated from the weights.  On an unmarked cloud both evaluations meet the full float64 bar on
    either side of the switch, and pairs on both sides exist."""
    from gaussreg_amd import _lib
    cfg = GC.BY_NAME[name]
    pts, params, r32, r64 = _built(name)
    idx = F.embedding_indices(pts, cfg.sigma_d, cfg.sigma_a, cfg.k, np.float32)[0]
    served = np.floor(idx.astype(np.float64) * 32) + 3 <= rows_d - 1
    assert served.any() and (~served).sum() > served.sum() // 4
    m = _module(cfg, params, "table")
    dev = torch.device("cuda", torch.cuda.current_device())
    td, ta = m._function_tables(dev)
    full = td
    td = torch.full((rows_d + 4, cfg.C), 1e30, device=dev)             # rows past rows_d exist and are poisoned: a read
    td[:rows_d] = full[:rows_d]                                         # beyond the stated table shows in the output
    L = _lib.lib()
    n = len(pts)
    p, out = _c(pts), torch.full((n, n, cfg.C), 7.0, device=dev)
    t = {k: _c(v) for k, v in params.items()}
    ws = _lib.workspace(dev, L.gr_geo_embedding_workspace_bytes(n, cfg.k))
    rc = L.gr_geo_embedding_table(_lib.ptr(p), n, _lib.ptr(td), rows_d, _lib.ptr(ta), ta.shape[0], 32.0, _lib.ptr(t["w_d"]),
                                  _lib.ptr(t["b_d"]), _lib.ptr(t["w_a"]), _lib.ptr(t["b_a"]), _lib.ptr(t["div"]), cfg.C,
                                  cfg.sigma_d, 180.0 / (cfg.sigma_a * np.pi), cfg.k, int(cfg.red == "mean"), _lib.ptr(out),
                                  _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    assert rc == GR_OK
    _hold(f"{name}-table-rows{rows_d}", out.cpu().numpy(), r32, r64, cfg.marked, "table+direct")


# ------------------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("mode", ["table", "gemm", "fp32"])
def test_batch_of_three_equals_three_single_calls(mode):
    cfg = GC.Config("batch3", None, 64, 3, "max", 0.2, 15, 1.0, (mode,), "", True, False)
    params = GC.build_params(64, 1.0, 99)
    clouds = np.stack([GC.build_cloud(s) for s in GC.BATCH])
    m = _module(cfg, params, mode)
    both = m(_c(clouds)).cpu().numpy()
    assert both.shape == (3, 29, 29, 64)
    for b in range(3):
        single = m(_c(clouds[b])[None]).cpu().numpy()[0]
        assert np.array_equal(both[b].view(np.uint32), single.view(np.uint32)), f"element {b} is not bit-equal to its single call"
        r32, r64 = _refs(clouds[b], params, cfg)
        _hold(f"batch3-{mode}[{b}]", both[b], r32, r64, kernel=GC.kernel_of(64, mode))


# ------------------------------------------------------------------------------------------------------------ the cache
@pytest.mark.parametrize("mode", ["table", "gemm", "fp32"])
def test_weights_changed_in_place_and_reloaded_are_followed(mode):
    cfg = GC.BY_NAME["w64"]
    pts, params, r32, r64 = _built("w64")
    m = _module(cfg, params, mode)
    x = _c(pts)[None]
    _hold(f"cache-{mode}-first", m(x)[0].cpu().numpy(), r32, r64)
    with torch.no_grad():
        m.proj_d.weight.mul_(1.5)
        m.proj_a.bias.add_(0.25)
    changed = _params_of(m)
    assert not np.array_equal(changed["w_d"], params["w_d"])
    r32b, r64b = _refs(pts, changed, cfg)
    assert np.abs(r64b - r64).max() > 1e-2 * np.abs(r64).max()          # the stale table would be far outside the bar
    _hold(f"cache-{mode}-in-place", m(x)[0].cpu().numpy(), r32b, r64b)
    with torch.no_grad():
        m.proj_a.weight[3, 5] += 0.5                                    # one element, through a view
    r32c, r64c = _refs(pts, _params_of(m), cfg)
    _hold(f"cache-{mode}-one-element", m(x)[0].cpu().numpy(), r32c, r64c)
    other = GC.build_params(cfg.C, 2.0, 1234)
    m.load_state_dict(_state(other))
    r32d, r64d = _refs(pts, other, cfg)
    _hold(f"cache-{mode}-state-dict", m(x)[0].cpu().numpy(), r32d, r64d)
    m.load_state_dict(_state(params))                                   # and back: the first answer again
    _hold(f"cache-{mode}-restored", m(x)[0].cpu().numpy(), r32, r64)


@pytest.mark.parametrize("mode", ["table", "gemm"])
def test_module_moved_between_devices(mode):
    cfg = GC.BY_NAME["k2-mean"]
    pts, params, r32, r64 = _built("k2-mean")
    m = _module(cfg, params, mode, device="cpu")
    out = m(_c(pts)[None])                                              # weights on the host, points on the GPU
    assert out.is_cuda
    _hold(f"device-{mode}-host-weights", out[0].cpu().numpy(), r32, r64)
    m = m.cuda()
    _hold(f"device-{mode}-moved", m(_c(pts)[None])[0].cpu().numpy(), r32, r64)
    with torch.no_grad():
        m.proj_d.bias.add_(0.125)
    m = m.cpu()
    out = m(torch.from_numpy(pts.astype(np.float32))[None])             # host points: the answer comes back to the host
    assert not out.is_cuda
    r32b, r64b = _refs(pts, _params_of(m), cfg)
    _hold(f"device-{mode}-back-on-host", out[0].numpy(), r32b, r64b)


@pytest.mark.parametrize("mode", ["table", "gemm"])
def test_inference_mode_tensors(mode):
    cfg = GC.BY_NAME["k3-mean"]
    pts, params, r32, r64 = _built("k3-mean")
    with torch.inference_mode():
        m = _module(cfg, params, mode)                                  # parameters without version counters
        assert m.proj_d.weight.is_inference()
        _hold(f"inference-{mode}", m(_c(pts)[None])[0].cpu().numpy(), r32, r64)
        m.proj_d.weight.mul_(0.5)
        r32b, r64b = _refs(pts, _params_of(m), cfg)
        _hold(f"inference-{mode}-changed", m(_c(pts)[None])[0].cpu().numpy(), r32b, r64b)
    m = _module(cfg, params, mode)                                      # ordinary parameters, inference-mode points
    with torch.inference_mode():
        _hold(f"inference-{mode}-points", m(_c(pts)[None])[0].cpu().numpy(), r32, r64)


# ------------------------------------------------------------------------------------------------------------ arguments
def _abi(entry, n, C, k, flags=0, ws_short=0, n_alloc=None):
    """One call of the C entry point on well-formed buffers; returns (status, out) -- out was filled with 7."""
    from gaussreg_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    na = max(n if n_alloc is None else n_alloc, 1)
    pts = torch.rand((na, 3), device=dev)
    w, b, div = torch.rand((C, C), device=dev), torch.rand((C,), device=dev), torch.rand((max(C // 2, 1),), device=dev)
    out = torch.full((na, na, C), 7.0, device=dev)
    need = L.gr_geo_embedding_workspace_bytes(max(n, 0), min(max(k, 0), 8))
    ws = torch.empty(need + 4096, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    if entry == "table":
        tab = torch.rand((64, C), device=dev)
        rc = L.gr_geo_embedding_table(_lib.ptr(pts), n, _lib.ptr(tab), 64, _lib.ptr(tab), 64, 32.0, _lib.ptr(w), _lib.ptr(b),
                                      _lib.ptr(w), _lib.ptr(b), _lib.ptr(div), C, 0.2, 3.8, k, flags, _lib.ptr(out), _lib.ptr(ws),
                                      need - ws_short, st)
    else:
        rc = L.gr_geo_embedding(_lib.ptr(pts), n, _lib.ptr(w), _lib.ptr(b), _lib.ptr(w), _lib.ptr(b), _lib.ptr(div), C, 0.2, 3.8, k,
                                flags, _lib.ptr(out), _lib.ptr(ws), need - ws_short, st)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("entry,n,C,k,flags,what", [
    ("gemm", 20, 64, 9, 0, "angle_k = 9"), ("table", 20, 64, 9, 0, "angle_k = 9"),
    ("gemm", 3, 64, 3, 0, "angle_k = N"), ("table", 3, 64, 3, 0, "angle_k = N"), ("gemm", 2, 64, 8, 1, "angle_k > N"),
    ("gemm", 20, 24, 2, 0, "C % 16"), ("gemm", 20, 40, 2, 1, "C % 16"), ("gemm", 20, 48, 2, 2, "C % 32 with fp32_mfma"),
    ("gemm", 20, 16, 0, 3, "C % 32 with fp32_mfma"), ("table", 20, 6, 2, 0, "C % 4"), ("gemm", 20, 64, -1, 0, "angle_k < 0")])
def test_bad_arguments_are_refused_on_the_host(entry, n, C, k, flags, what):
    rc, out = _abi(entry, n, C, k, flags)
    assert rc == GR_ERR_INVALID, what
    assert (out == 7.0).all(), f"{what}: the output was written"


@pytest.mark.parametrize("entry,flags", [("gemm", 0), ("gemm", 2), ("table", 0)])
def test_short_workspace_is_refused(entry, flags):
    rc, out = _abi(entry, 20, 64, 3, flags, ws_short=1)
    assert rc == GR_ERR_WORKSPACE and (out == 7.0).all()
    rc, out = _abi(entry, 20, 64, 3, flags, ws_short=0)                 # exactly the stated size is enough
    assert rc == GR_OK and not (out == 7.0).any()


@pytest.mark.parametrize("entry", ["gemm", "table"])
def test_empty_cloud_returns_ok_and_touches_nothing(entry):
    rc, out = _abi(entry, 0, 64, 3, n_alloc=4)
    assert rc == GR_OK and (out == 7.0).all()
    rc, out = _abi(entry, 0, 64, 0, n_alloc=4)
    assert rc == GR_OK and (out == 7.0).all()


def test_module_refuses_what_the_library_refuses():
    from gaussreg_amd.embedding import GeometricStructureEmbedding
    x = torch.rand(1, 12, 3).cuda()
    for C, k, kw in [(64, 9, {}), (64, 12, {}), (48, 2, {"fp32_mfma": True}), (24, 2, {"mode": "gemm"}), (64, 9, {"mode": "gemm"})]:
        with pytest.raises(RuntimeError):
            GeometricStructureEmbedding(C, 0.2, 15, k, **kw).cuda()(x)
    out = GeometricStructureEmbedding(64, 0.2, 15, 3).cuda()(torch.zeros(2, 0, 3).cuda())
    assert out.shape == (2, 0, 0, 64)
