"""GPU: the HIP GroupNorm of the training path -- kpconv_blocks.GroupNorm inside kpconv.differentiable(fused_norm=True):
gr_group_norm_train forward, gr_group_norm_backward -- against float64 autograd of the restatement in
tests/group_norm_grad_f64.py.

Bars, per gradient tensor (those of docs/kpconv_backward_f64_errors.md): with e_hip = max|HIP - f64|, e_ref = max|fp32 stock
composition autograd - f64| (transpose, group_norm, add, leaky_relu on the same GPU) and scale = max|f64|,
    e_hip <= 8 e_ref + 1e-7 scale   on every case, and
    e_hip <= 1e-5 scale             on every case without a zero-variance group, a single-row segment or a group of two
                                    values; there only the first bar applies.
The second bar assumes that grad_x is of the size of its terms rstd * dy * gamma.  It is not where the statistics leave the
normalised values no freedom: with zero variance rstd is eps^-1/2 = 316; a single row gives its groups C / G values; and a
group of two values (C / G = 1, two rows) normalises to +-sqrt(var / (var + eps)) whatever the input, so its exact gradient is
O(eps / var) of the terms it is the difference of (scale 2.6e-4 where the terms are O(1)) and no fp32 evaluation resolves it
to 1e-5 of that: the stock composition measures 6.2e-7 there, the kernels 2.2e-7.
The measured figures are in docs/group_norm_backward_f64_errors.md.
"""
import collections
import functools

import pytest
import torch

from group_norm_grad_f64 import grads, group_norm_ref, stock_composition

pytestmark = pytest.mark.gpu

SEG3 = (0, 25, 40)
SEG5 = (0, 0, 1, 300, 5000)     # an empty segment, a single-row segment
Case = collections.namedtuple("Case", "c g n seg slope res affine go const_col", defaults=(True, "dense", False))

CASES = [
    Case(4, 1, 1, None, None, False),
    Case(4, 1, 7, None, 0.1, True),
    Case(4, 1, 5000, None, 0.1, False),
    Case(8, 8, 2, None, 0.1, True),
    Case(8, 8, 40, SEG3, 0.1, True, go="zero-seg"),
    Case(8, 8, 5000, SEG5, None, False),
    Case(8, 8, 300, None, 0.1, True, const_col=True),
    Case(64, 32, 300, None, 0.1, True),
    Case(64, 32, 5000, SEG5, 0.1, True, go="zero-seg"),
    Case(64, 32, 40, SEG3, None, False, go="strided"),
    Case(16, 4, 7, None, None, True),
    Case(16, 4, 5000, None, 0.1, False, affine=False),
    Case(128, 32, 300, None, 0.1, True, go="strided"),
    Case(128, 32, 5000, SEG5, 0.1, False),
    Case(128, 32, 1, None, None, False),
    Case(1024, 32, 7, None, 0.1, True),
    Case(1024, 32, 300, None, None, False),
    Case(1024, 32, 40, SEG3, 0.1, True, go="zero-seg"),
    Case(1024, 32, 5000, SEG5, 0.1, True),
    Case(2048, 32, 2, None, 0.1, True),
    Case(2048, 32, 300, None, 0.1, False),
    Case(2048, 32, 40, SEG3, None, True),
    Case(2048, 32, 5000, None, 0.1, False),
]
ZERO_SEG = {SEG3: 1, SEG5: 3}    # the segment whose grad_out rows are zero in a "zero-seg" case
NAMES = ("grad_x", "grad_residual", "grad_gamma", "grad_beta")


def _id(c):
    return (f"c{c.c}-g{c.g}-n{c.n}-{'seg%d' % (len(c.seg) - 1) if c.seg else 'noseg'}-slope{c.slope}-{'res' if c.res else 'nores'}"
            f"{'' if c.affine else '-noaffine'}-{c.go}{'-constcol' if c.const_col else ''}")


def _table(c):
    if c.seg is None:
        return None
    off = torch.tensor(c.seg, dtype=torch.int64, device="cuda")
    return {c.n: (off, max(b - a for a, b in zip(c.seg[:-1], c.seg[1:])))}


def _inputs(c):
    from gaussreg_amd.kpconv_blocks import GroupNorm
    gen = torch.Generator(device="cuda").manual_seed(1000 * c.c + c.n)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    x = rnd(c.n, c.c) * 1.5 + 0.3
    if c.const_col:
        x[:, 3] = 0.75
    norm = GroupNorm(c.g, c.c).cuda()
    if c.affine:
        with torch.no_grad():
            norm.norm.weight.copy_(torch.rand(c.c, device="cuda", generator=gen) + 0.5)
            norm.norm.bias.copy_(rnd(c.c) * 0.2)
    else:
        norm.norm = torch.nn.GroupNorm(c.g, c.c, affine=False).cuda()
    res = rnd(c.n, c.c) if c.res else None
    if c.go == "strided":
        go = rnd(c.n, 2 * c.c)[:, ::2]
        assert not go.is_contiguous() or c.n * c.c == 1
    else:
        go = rnd(c.n, c.c)
        if c.go == "zero-seg":
            k = ZERO_SEG[c.seg]
            go[c.seg[k]:c.seg[k + 1]] = 0
    return x, norm, res, go


def _hip(c, x, norm, res, go, fused=True):
    """(out, [grad_x, grad_residual, grad_gamma, grad_beta] twice) through the module inside differentiable()."""
    import contextlib
    from gaussreg_amd.kpconv import differentiable
    from gaussreg_amd.kpconv_blocks import norm_segments
    xs = x.clone().requires_grad_(True)
    rs = None if res is None else res.clone().requires_grad_(True)
    table = _table(c)
    with differentiable(fused_norm=fused), (norm_segments(table) if table else contextlib.nullcontext()):
        out = norm(xs, c.slope, residual=rs)
    leaves = [t for t in (xs, rs, norm.norm.weight, norm.norm.bias) if t is not None]
    runs = []
    for _ in range(2):
        got = iter(torch.autograd.grad(out, leaves, go.reshape(out.shape), retain_graph=True))
        runs.append([next(got) if t is not None else None for t in (xs, rs, norm.norm.weight, norm.norm.bias)])
    return out, runs


@functools.lru_cache(maxsize=None)
def _run(c):
    x, norm, res, go = _inputs(c)
    out, runs = _hip(c, x, norm, res, go)
    args = (x, c.g, norm.norm.weight, norm.norm.bias, norm.norm.eps, c.slope, res, c.seg, go)
    r64 = grads(group_norm_ref, *args, torch.float64)
    r32 = grads(stock_composition, *args, torch.float32)
    return dict(x=x, norm=norm, res=res, go=go, out=out, runs=runs, r64=r64, r32=r32)


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    """The cases' inputs, results and references (about 1 GB) live as long as this module's tests, not as long as the session."""
    yield
    _run.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_gradients_vs_float64(c):
    r = _run(c)
    # zero variance / a single-row segment / groups of two values: the relative bar only (module docstring)
    loose = c.const_col or c.n == 1 or c.seg == SEG5 or c.n * (c.c // c.g) <= 2
    assert (r["out"].double().reshape(c.n, c.c) - r["r64"][0]).abs().max().item() <= 1e-4 * max(r["r64"][0].abs().max().item(), 1)
    for name, got, t64, t32 in zip(NAMES, r["runs"][0], r["r64"][1:], r["r32"][1:]):
        assert (got is None) == (t64 is None), name
        if got is None:
            continue
        assert torch.isfinite(got).all(), name
        scale = t64.abs().max().item()
        e_hip = (got.double().reshape(t64.shape) - t64).abs().max().item()
        e_ref = (t32 - t64).abs().max().item()
        print(f"\nGNB {_id(c)} {name}: scale {scale:.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e} "
              f"e_hip/scale {e_hip / max(scale, 1e-300):.2e} e_hip/e_ref {e_hip / max(e_ref, 1e-300):.2f}")
        assert e_hip <= 8 * e_ref + 1e-7 * scale, f"{name}: e_hip {e_hip:.3e} > 8 * {e_ref:.3e} + 1e-7 * {scale:.3e}"
        if not loose:
            assert e_hip <= 1e-5 * scale, f"{name}: e_hip {e_hip:.3e} > 1e-5 * {scale:.3e}"


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_forward_bits_and_reproducibility(c):
    import contextlib
    from gaussreg_amd.kpconv_blocks import norm_segments
    r = _run(c)
    table = _table(c)
    with torch.no_grad(), (norm_segments(table) if table else contextlib.nullcontext()):
        want = r["norm"](r["x"], c.slope, residual=r["res"])
    assert r["out"].grad_fn is not None and "GroupNorm" in type(r["out"].grad_fn).__name__ + str(r["out"].grad_fn.next_functions)
    assert r["out"].shape == want.shape and torch.equal(r["out"], want)
    for name, a, b in zip(NAMES, *r["runs"]):
        assert (a is None and b is None) or torch.equal(a, b), name
    if c.go == "zero-seg":      # a wrong segment offset would leak the neighbours' gradient in here
        k = ZERO_SEG[c.seg]
        rows = slice(c.seg[k], c.seg[k + 1])
        assert rows.stop > rows.start
        for got in r["runs"][0][:2]:
            if got is not None:
                assert (got[rows] == 0).all() and (got != 0).any()


@pytest.mark.parametrize("c,k", [(Case(64, 32, 5000, SEG5, 0.1, True), 3), (Case(8, 8, 40, SEG3, 0.1, True), 0),
                                 (Case(2048, 32, 40, SEG3, None, True), 1)], ids=lambda v: _id(v) if isinstance(v, Case) else f"seg{v}")
def test_a_segment_agrees_with_the_call_on_that_segment_alone(c, k):
    x, norm, res, go = _inputs(c)
    a, b = c.seg[k], c.seg[k + 1]
    mask = torch.zeros(c.n, 1, device="cuda")
    mask[a:b] = 1
    go = go * mask                      # the other segments send nothing to grad_gamma / grad_beta
    _, (whole, _) = _hip(c, x, norm, res, go)
    alone = c._replace(n=b - a, seg=None)
    _, (part, _) = _hip(alone, x[a:b], norm, None if res is None else res[a:b], go[a:b])
    for name, w, p in zip(NAMES, whole, part):
        w = w[a:b] if name in ("grad_x", "grad_residual") else w
        scale = p.abs().max().item()
        assert (w.reshape(p.shape) - p).abs().max().item() <= 1e-6 * scale, name


def test_inputs_without_requires_grad_get_none():
    from gaussreg_amd.kpconv import differentiable, fused_norm_active
    from gaussreg_amd.kpconv_blocks import GroupNorm
    norm = GroupNorm(4, 16).cuda()
    norm.norm.bias.requires_grad_(False)
    x = torch.randn(50, 16, device="cuda")
    res = torch.randn(50, 16, device="cuda", requires_grad=True)
    assert not fused_norm_active()
    with differentiable(fused_norm=True):
        assert fused_norm_active()
        with torch.no_grad():
            assert not fused_norm_active()
        out = norm(x, 0.1, residual=res)
    assert not fused_norm_active()
    out.sum().backward()
    assert x.grad is None and norm.norm.bias.grad is None
    assert res.grad is not None and norm.norm.weight.grad is not None
    want = torch.where(out > 0, 1.0, 0.1)
    assert torch.equal(res.grad, want)


def test_unsupported_channels_take_the_torch_path_and_refuse_segments():
    from gaussreg_amd.kpconv import differentiable
    from gaussreg_amd.kpconv_blocks import GroupNorm, norm_segments
    norm = GroupNorm(4, 24).cuda()
    x = torch.randn(40, 24, device="cuda", requires_grad=True)
    with differentiable(fused_norm=True):
        out = norm(x, 0.1)
    assert "GroupNormFunction" not in type(out.grad_fn).__name__
    out.sum().backward()
    assert x.grad is not None and norm.norm.weight.grad is not None
    table = {40: (torch.tensor([0, 25, 40], device="cuda"), 25)}
    with differentiable(fused_norm=True), norm_segments(table):
        with pytest.raises(NotImplementedError, match="norm_segments"):
            norm(x, 0.1)
    ok = GroupNorm(4, 16).cuda()
    with differentiable(), norm_segments(table):      # the default keeps refusing
        with pytest.raises(NotImplementedError, match="norm_segments"):
            ok(torch.randn(40, 16, device="cuda"), 0.1)
    with pytest.raises(TypeError):
        with differentiable(fused=True):
            pass


def test_invalid_arguments_are_refused_before_any_launch():
    from gaussreg_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, c, g = 40, 16, 4
    x, out, go = (torch.randn(n, c, device="cuda") for _ in range(3))
    stats = torch.cat([torch.zeros(1, 1, g), torch.ones(1, 1, g)], 1).cuda()
    outs = [torch.full((n, c), 7.0, device="cuda"), torch.full((n, c), 7.0, device="cuda"),
            torch.full((c,), 7.0, device="cuda"), torch.full((c,), 7.0, device="cuda")]
    ws = L.gr_group_norm_backward_workspace_bytes(c, g, 1)

    def call(x=x, groups=g, slope=0.1, ws=ws, cc=c):
        return _lib.call(dev, "gr_group_norm_backward", x, out, go, None, stats, n, cc, groups, slope, None, 1, n, *outs, ws=ws)

    for kwargs, text in ((dict(slope=0.0), "negative_slope"), (dict(slope=-0.1), "negative_slope"),
                         (dict(groups=65, cc=260), "bad sizes"), (dict(cc=24), "not supported"),
                         (dict(ws=torch.empty(64, dtype=torch.uint8, device="cuda")), "workspace too small"),
                         (dict(x=None), "null argument")):
        with pytest.raises(RuntimeError, match=text):
            call(**kwargs)
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in outs)
    call()                               # and the same arguments, valid, do run
    torch.cuda.synchronize()
    assert all((o != 7.0).any() for o in outs)
