"""CPU: the float64 restatement of tests/group_norm_grad_f64.py -- the truth of the GroupNorm gradient tests -- is pinned to
torch.nn.functional.group_norm on the transposed (1, C, N) form (what geotransformer/modules/kpconv/modules.py:32-50 runs),
segment by segment, and its gradients to finite differences."""
import torch

from group_norm_grad_f64 import group_norm_ref, stock_composition


def _inputs(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g, dtype=torch.float64) * 1.5 + 0.3
    w = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    b = torch.randn(c, generator=g, dtype=torch.float64) * 0.2
    r = torch.randn(n, c, generator=g, dtype=torch.float64)
    return x, w, b, r


def test_restatement_equals_functional_group_norm_per_segment():
    for n, c, groups, seg in ((40, 16, 4, None), (40, 16, 4, [0, 25, 40]), (300, 8, 8, [0, 0, 1, 300]), (7, 64, 32, None),
                              (1, 4, 1, None)):
        x, w, b, r = _inputs(n, c, 5)
        for wt, bs in ((w, b), (None, None)):
            for slope, res in ((None, None), (0.1, None), (0.1, r), (None, r)):
                got = group_norm_ref(x, groups, wt, bs, 1e-5, slope, res, seg)
                want = stock_composition(x, groups, wt, bs, 1e-5, slope, res, seg)
                assert got.shape == want.shape == (n, c)
                assert (got - want).abs().max().item() <= 1e-12, (n, c, groups, seg, slope)
    # the stock composition is torch.nn.functional.group_norm on the transposed form wherever that accepts the input
    x, w, b, _ = _inputs(40, 16, 6)
    want = torch.nn.functional.group_norm(x.t().unsqueeze(0), 4, w, b, 1e-5).squeeze(0).t()
    assert torch.equal(stock_composition(x, 4, w, b, 1e-5), want)
    assert (group_norm_ref(x, 4, w, b, 1e-5) - want).abs().max().item() <= 1e-12


def test_restatement_passes_gradcheck_on_two_segments():
    n, c, groups, seg = 8, 8, 4, [0, 5, 8]
    x, w, b, r = _inputs(n, c, 9)
    # away from the LeakyReLU kink: push every pre-activation at least 0.05 from zero through the residual
    with torch.no_grad():
        pre = group_norm_ref(x, groups, w, b, 1e-5, None, r, seg)
        r = r + torch.where(pre.abs() < 0.05, torch.sign(pre) * 0.1 + (pre == 0) * 0.1, torch.zeros_like(pre))
        assert group_norm_ref(x, groups, w, b, 1e-5, None, r, seg).abs().min().item() >= 0.05
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b, r)]
    fn = lambda xx, ww, bb, rr: group_norm_ref(xx, groups, ww, bb, 1e-5, 0.1, rr, seg)
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)
    # and the plain norm, without affine parameters
    xx = x.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: group_norm_ref(a, groups, None, None, 1e-5, None, None, seg), [xx], eps=1e-6,
                                    atol=1e-7, rtol=1e-5)
