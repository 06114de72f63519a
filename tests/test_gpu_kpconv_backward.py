"""GPU: the HIP backward of KPConv / maxpool / nearest_upsample inside gaussreg_amd.kpconv.differentiable() against torch
autograd of the float64 restatement (tests/kpconv_grad_f64.py).

Bars, per gradient tensor (those of the forward path tests, docs/kpconv_rpe_path_errors.md): with e_hip = max|HIP - f64|,
e_ref = max|fp32 restatement autograd - f64| and scale = max|f64|,  e_hip <= 1e-5 scale  and  e_hip <= 8 e_ref + 1e-7 scale.
The measured figures are in docs/kpconv_backward_f64_errors.md.  The cases are chosen so that every bit
gr_kpconv_backward_plan can return occurs, and each case asserts the bits it expects.
"""
import numpy as np
import pytest
import torch

import kpconv_cases
from kpconv_cases import case
from kpconv_grad_f64 import kpconv_grads, maxpool_ref, nearest_upsample_ref

pytestmark = pytest.mark.gpu

# plan bits of include/gaussreg_hip.h
G16, G32, G64, SUM_MASK, MULTIPASS, FEATS, WEIGHTS, SLABS, BIAS, CHUNKED, EMPTY = 0, 1, 2, 3, 4, 8, 16, 32, 64, 128, 256

# (case, stress, chunk_rows): stress edits the neighbour table (see _build)
CASES = [
    (case("cin1-cout16-h37", 1, 16, 37), None, 0),
    (case("cin4-cout3-h3", 4, 3, 3, feats="mixed", bias=True), None, 0),
    (case("cin16-cout130-h1-k7", 16, 130, 1, k=7), None, 0),
    (case("cin32-cout16-h4", 32, 16, 4, feats="mixed", bias=True), None, 0),
    (case("cin64-cout130-h64", 64, 130, 64, feats="mixed"), None, 0),
    (case("cin128-cout3-h65", 128, 3, 65, bias=True), None, 0),
    (case("cin256-cout16-h37", 256, 16, 37, feats="mixed"), None, 0),
    (case("cin300-cout130-h300", 300, 130, 300, m=260, n=640, bias=True), None, 0),
    (case("k1-cin4-cout16", 4, 16, 20, k=1, feats="mixed"), None, 0),
    (case("k16-cin32-cout3", 32, 3, 20, k=16, bias=True), None, 0),
    (case("ragged-m255", 20, 16, 20, m=255, n=400, feats="mixed", bias=True), None, 0),
    (case("ragged-m257", 16, 130, 20, m=257, n=400), None, 0),
    (case("one-slab-m50", 32, 16, 12, m=50, n=120, bias=True), None, 0),
    (case("m0", 32, 16, 5, m=0, n=300, bias=True, special="m0"), None, 0),
    (case("h0", 32, 16, 0, m=300, n=300, bias=True, special="h0"), None, 0),
    (case("n0", 4, 16, 5, m=300, n=0, bias=True, special="n0"), None, 0),
    (case("shadow-rows", 64, 16, 30, feats="mixed", bias=True, special="shadow_rows"), None, 0),
    (case("zero-feature-rows", 32, 16, 30, bias=True, special="zero_rows"), None, 0),
    (case("small-sigma", 64, 16, 30, sigma=0.008, feats="mixed", bias=True), None, 0),
    (case("unreferenced-rows", 32, 16, 20, feats="mixed"), "unreferenced", 0),
    (case("hub-row", 16, 16, 20, feats="mixed", bias=True), "hub", 0),
    (case("repeated-index", 48, 16, 20, feats="mixed"), "repeat", 0),
    (case("three-chunks", 32, 16, 20, feats="mixed", bias=True), None, 256),
    (case("three-chunks-cin100", 100, 130, 20, bias=True), "hub", 256),
]
IDS = [c.name for c, _, _ in CASES]


def _build(c, stress):
    x = kpconv_cases.build(c)
    idx = x["idx"]
    if stress == "unreferenced":          # the last 50 support rows are named by no query
        idx[idx >= c.n - 50] = c.n
    if stress == "hub":                   # every query names support row 5: the longest inverted list
        idx[:, 0] = 5
    if stress == "repeat":                # an index twice in one query's row
        idx[::3, 1] = idx[::3, 0]
    kpconv_cases.assert_flag_margin(x["f"])
    return x


def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _conv(c, x):
    from gaussreg_amd.kpconv import KPConv
    conv = KPConv(c.cin, c.cout, c.k, 0.0625, c.sigma, bias=c.bias, kernel_points=x["kp"]).cuda()
    with torch.no_grad():
        conv.weights.copy_(_c(x["w"]))
        if c.bias:
            conv.bias.copy_(_c(x["b"]))
    return conv


def _hip_grads(c, x, go, chunk_rows, f_grad=True):
    from gaussreg_amd.kpconv import differentiable
    conv = _conv(c, x)
    f = _c(x["f"]).requires_grad_(f_grad)
    with differentiable(chunk_rows=chunk_rows):
        out = conv(f, _c(x["qp"]), _c(x["sp"]), _c(x["idx"]))
    assert out.grad_fn is not None
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), f.grad, conv.weights.grad, (conv.bias.grad if c.bias else None), conv


def _grad_out(c, kind):
    g = torch.Generator().manual_seed(1234 + c.cin + c.cout)
    if kind == "dense":
        return torch.randn(c.m, c.cout, generator=g).cuda()
    return torch.randn(1, c.cout, generator=g).cuda().expand(c.m, c.cout)   # zero stride over the rows, as .sum().backward() hands over


def _expected_plan(c, chunk_rows):
    plan = BIAS if c.bias else 0
    if c.m == 0 or c.n == 0 or c.h == 0:
        return plan | EMPTY, 0
    plan |= FEATS | WEIGHTS | (G16 if c.cin <= 16 else G32 if c.cin <= 32 else G64) | (MULTIPASS if c.cin > 64 else 0)
    if chunk_rows and c.m > chunk_rows:
        plan |= CHUNKED
    return plan, SLABS     # SLABS depends on the workspace budget: reported, and covered by test_every_plan_bit_occurs


@pytest.mark.parametrize("kind", ["dense", "expanded"])
@pytest.mark.parametrize("c,stress,chunk_rows", CASES, ids=IDS)
def test_kpconv_backward_vs_float64(c, stress, chunk_rows, kind):
    from gaussreg_amd import _lib
    x = _build(c, stress)
    go = _grad_out(c, kind)
    plan = _lib.lib().gr_kpconv_backward_plan(c.n, c.m, c.h, c.cin, c.cout, c.k, 3 | (4 if c.bias else 0), chunk_rows)
    want_plan, free = _expected_plan(c, chunk_rows)
    assert plan >= 0 and plan & ~free == want_plan, (plan, want_plan)
    out, gf, gw, gb, conv = _hip_grads(c, x, go, chunk_rows)
    # forward values inside differentiable() are those outside it, bit for bit
    with torch.enable_grad():
        plain = conv(_c(x["f"]).requires_grad_(True), _c(x["qp"]), _c(x["sp"]), _c(x["idx"]))
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, out)
    assert gf.shape == (c.n, c.cin) and gw.shape == (c.k, c.cin, c.cout) and (gb is None) == (not c.bias)
    # a second backward on the same inputs: the same bits
    _, gf2, gw2, gb2, _ = _hip_grads(c, x, go, chunk_rows)
    assert torch.equal(gf, gf2) and torch.equal(gw, gw2) and (gb is None or torch.equal(gb, gb2))
    go_np = go.cpu().numpy().astype(np.float64)
    _, *ref64 = kpconv_grads(x, c.sigma, go_np, torch.float64, "cuda")
    _, *ref32 = kpconv_grads(x, c.sigma, go_np, torch.float32, "cuda")
    for name, got, r64, r32 in zip(("grad_f", "grad_w", "grad_b"), (gf, gw, gb), ref64, ref32):
        if got is None:
            continue
        got = got.double().cpu().numpy()
        assert np.isfinite(got).all()
        scale = np.abs(r64).max() if r64.size else 0.0
        e_hip = np.abs(got - r64).max() if r64.size else 0.0
        e_ref = np.abs(r32 - r64).max() if r64.size else 0.0
        print(f"\nKPB {c.name} {kind} {name}: plan {plan} scale {scale:.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e} "
              f"e_hip/scale {e_hip / max(scale, 1e-300):.2e} e_hip/e_ref {e_hip / max(e_ref, 1e-300):.2f}")
        if plan & EMPTY and name != "grad_b":
            assert not got.any()
        assert e_hip <= 1e-5 * scale, f"{c.name} {name}: e_hip {e_hip:.3e} > 1e-5 * {scale:.3e}"
        assert e_hip <= 8 * e_ref + 1e-7 * scale, f"{c.name} {name}: e_hip {e_hip:.3e} > 8 * {e_ref:.3e} + 1e-7 * {scale:.3e}"
    if stress == "unreferenced":
        named = np.zeros(c.n + 1, bool)
        named[x["idx"].reshape(-1)] = True
        assert (~named[:c.n]).sum() >= 50 and not gf[_c(~named[:c.n])].any()      # exactly 0
    if c.special == "zero_rows":
        assert (x["f"][x["idx"][0][x["idx"][0] < c.n]] == 0).all()                # num fell back to 1 on row 0


def test_every_plan_bit_occurs():
    from gaussreg_amd import _lib
    L = _lib.lib()
    seen, groups = 0, set()
    for c, _, chunk_rows in CASES:
        plan = L.gr_kpconv_backward_plan(c.n, c.m, c.h, c.cin, c.cout, c.k, 3 | (4 if c.bias else 0), chunk_rows)
        seen |= plan
        if plan & FEATS:
            groups.add(plan & SUM_MASK)
        if c.name == "one-slab-m50":
            assert plan & WEIGHTS and not plan & SLABS
    assert groups == {G16, G32, G64}
    for bit in (MULTIPASS, FEATS, WEIGHTS, SLABS, BIAS, CHUNKED, EMPTY):
        assert seen & bit, bit
    assert L.gr_kpconv_backward_plan(900, 700, 20, 32, 16, 15, 2, 0) & (FEATS | WEIGHTS) == WEIGHTS
    assert L.gr_kpconv_backward_plan(900, 700, 20, 32, 16, 17, 7, 0) == -1       # more kernel points than the kernels hold


def test_inputs_without_grad_get_none_and_bias_is_optional():
    c, stress, _ = CASES[IDS.index("cin32-cout16-h4")]
    x = _build(c, stress)
    out, gf, gw, gb, conv = _hip_grads(c, x, _grad_out(c, "dense"), 0, f_grad=False)
    assert gf is None and gw is not None and gb is not None
    from gaussreg_amd.kpconv import differentiable
    conv.weights.requires_grad_(False)
    conv.weights.grad = conv.bias.grad = None
    f = _c(x["f"]).requires_grad_(True)
    with differentiable():
        conv(f, _c(x["qp"]), _c(x["sp"]), _c(x["idx"])).sum().backward()
    assert conv.weights.grad is None and f.grad is not None and conv.bias.grad is not None
    c2 = c._replace(bias=False)
    _, _, _, gb2, conv2 = _hip_grads(c2, x, _grad_out(c, "dense"), 0)
    assert gb2 is None and conv2.bias is None


def test_points_that_require_grad_are_refused():
    from gaussreg_amd.kpconv import differentiable
    c, stress, _ = CASES[IDS.index("cin4-cout3-h3")]
    x = _build(c, stress)
    conv = _conv(c, x)
    f, idx = _c(x["f"]).requires_grad_(True), _c(x["idx"])
    with differentiable():
        with pytest.raises(ValueError, match="q_points"):
            conv(f, _c(x["qp"]).requires_grad_(True), _c(x["sp"]), idx)
        with pytest.raises(ValueError, match="s_points"):
            conv(f, _c(x["qp"]), _c(x["sp"]).requires_grad_(True), idx)


def test_norm_segments_are_refused_inside_differentiable():
    from gaussreg_amd.kpconv import differentiable
    from gaussreg_amd.kpconv_blocks import GroupNorm, norm_segments
    norm = GroupNorm(4, 16).cuda()
    x = torch.randn(40, 16, device="cuda", requires_grad=True)
    table = {40: (torch.tensor([0, 25, 40], device="cuda"), 25)}
    with differentiable(), norm_segments(table):
        with pytest.raises(NotImplementedError, match="norm_segments"):
            norm(x)


def test_outside_the_context_nothing_carries_a_grad_fn():
    from gaussreg_amd.kpconv import maxpool, nearest_upsample
    c, stress, _ = CASES[IDS.index("cin32-cout16-h4")]
    x = _build(c, stress)
    conv = _conv(c, x)
    f, idx = _c(x["f"]).requires_grad_(True), _c(x["idx"])
    assert torch.is_grad_enabled() and conv.weights.requires_grad
    for y in (conv(f, _c(x["qp"]), _c(x["sp"]), idx), maxpool(f, idx), nearest_upsample(f, idx)):
        assert y.grad_fn is None and not y.requires_grad


# ---------------------------------------------------------------------------------------------- the two pools
def _pool_case(name, channels):
    c, stress, _ = CASES[IDS.index(name)]
    idx = _build(c, stress)["idx"]
    rng = np.random.default_rng(channels * 1000 + c.h)
    # distinct values of both signs: no ties between real rows; a shadow neighbour's 0 still beats the negative ones
    x = (rng.permutation(c.n * channels).reshape(c.n, channels).astype(np.float32) - c.n * channels / 2 + 0.5) / 64
    go = rng.normal(size=(c.m, channels)).astype(np.float32)
    return c, idx, x, go


@pytest.mark.parametrize("channels", [1, 5, 64])
@pytest.mark.parametrize("name", ["cin32-cout16-h4", "cin1-cout16-h37", "shadow-rows", "hub-row", "repeated-index",
                                  "unreferenced-rows"])
def test_pool_backward_vs_float64(name, channels):
    from gaussreg_amd.kpconv import differentiable, maxpool, nearest_upsample
    c, idx, x, go = _pool_case(name, channels)
    for fn, ref in ((maxpool, maxpool_ref), (nearest_upsample, nearest_upsample_ref)):
        xt = _c(x).requires_grad_(True)
        with differentiable():
            y = fn(xt, _c(idx))
        assert y.grad_fn is not None and torch.equal(y.detach(), fn(_c(x), _c(idx)))
        y.backward(_c(go))
        x2 = _c(x).requires_grad_(True)
        with differentiable():
            fn(x2, _c(idx)).backward(_c(go))
        assert torch.equal(xt.grad, x2.grad)                              # bit-identical
        r = {}
        for dt in (torch.float64, torch.float32):
            xr = _c(x).to(dt).requires_grad_(True)
            r[dt], = torch.autograd.grad(ref(xr, _c(idx)), [xr], _c(go).to(dt))
        r64 = r[torch.float64].cpu().numpy()
        if fn is nearest_upsample:                                        # index_add over column 0 in float64
            want = torch.zeros(c.n + 1, channels, dtype=torch.float64).index_add_(0, torch.from_numpy(idx[:, 0]),
                                                                               torch.from_numpy(go).double())[:c.n].numpy()
            assert np.abs(want - r64).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
        got = xt.grad.double().cpu().numpy()
        scale = np.abs(r64).max()
        e_hip, e_ref = np.abs(got - r64).max(), np.abs(r[torch.float32].double().cpu().numpy() - r64).max()
        print(f"\nKPB pool {fn.__name__} {name} C{channels}: scale {scale:.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e}")
        assert e_hip <= 1e-5 * scale and e_hip <= 8 * e_ref + 1e-7 * scale
        named = np.zeros(c.n + 1, bool)
        named[idx.reshape(-1) if fn is maxpool else idx[:, 0]] = True
        assert not got[~named[:c.n]].any()


def test_maxpool_ties_losers_and_the_shadow_row():
    from gaussreg_amd.kpconv import differentiable, maxpool
    x = torch.tensor([[1.0, -1.0], [1.0, -2.0], [0.5, -3.0], [7.0, 7.0]], device="cuda", requires_grad=True)
    idx = torch.tensor([[1, 0, 2], [2, 4, 4], [0, 0, 2]], device="cuda")    # 4 = the shadow row
    go = torch.tensor([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0]], device="cuda")
    with differentiable():
        maxpool(x, idx).backward(go)
    # query 0: channel 0 ties rows 1 and 0 at h = 0, 1 -> the lowest h (row 1); channel 1: row 0.
    # query 1: channel 0: row 2 (0.5 > 0); channel 1: the shadow row's 0 wins -> dropped.
    # query 2: row 0 twice -> the first column takes it all.  Row 3 is named by nobody; row 2 only loses in queries 0 and 2 and in channel 1.
    want = torch.tensor([[50.0, 20.0 + 60.0], [10.0, 0.0], [30.0, 0.0], [0.0, 0.0]], device="cuda")
    assert torch.equal(x.grad, want)
