"""GPU: KPConvFPN differentiable end to end inside gaussreg_amd.kpconv.differentiable().

A small backbone (input_dim 1, init_dim 16, 4 groups: the narrowest tensors have 8 entries) on a synthetic five-level pyramid of two clouds of 400 points, built
with the project's own grid_subsample / radius_search.  Loss: the sum of squares over all four outputs.  Truth: a float64
twin -- the module deep-copied to double with KPConv.forward / maxpool / nearest_upsample replaced by the torch restatement
of tests/kpconv_grad_f64.py; the same twin in float32 gives the error stock torch has.  Per parameter tensor the norm-wise
relative error of the HIP gradients is at most 8 times that of the fp32 twin, with a floor of 1e-6.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

from kpconv_grad_f64 import kpconv_ref, maxpool_ref, nearest_upsample_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyramid():
    from gaussreg_amd.data import precompute_data_stack_mode
    rng = np.random.default_rng(11)
    pts = torch.from_numpy(rng.random((800, 3)).astype(np.float32)).cuda()
    lengths = torch.tensor([400, 400])
    data = precompute_data_stack_mode(pts, lengths, 5, 0.04, 0.1, [24] * 5)
    sizes = [p.shape[0] for p in data["points"]]
    assert sizes[0] == 800 and sizes[-1] >= 4 and all(a >= b for a, b in zip(sizes, sizes[1:])), sizes
    return data


def _model(seed=3):
    from gaussreg_amd.kpconv_blocks import KPConvFPN
    torch.manual_seed(seed)
    np.random.seed(seed)
    return KPConvFPN(1, 8, 16, 15, 0.1, 0.08, 4).cuda()


@contextlib.contextmanager
def _restated():
    """KPConv.forward / maxpool / nearest_upsample of the blocks replaced by the torch restatement (any dtype)."""
    from gaussreg_amd import kpconv, kpconv_blocks
    saved = (kpconv.KPConv.forward, kpconv_blocks.maxpool, kpconv_blocks.nearest_upsample)
    kpconv.KPConv.forward = lambda self, f, q, s, nb: kpconv_ref(f, q.to(f.dtype), s.to(f.dtype), nb,
                                                                 self.kernel_points, self.weights, self.sigma, self.bias, self.inf)
    kpconv_blocks.maxpool, kpconv_blocks.nearest_upsample = maxpool_ref, nearest_upsample_ref
    try:
        yield
    finally:
        kpconv.KPConv.forward, kpconv_blocks.maxpool, kpconv_blocks.nearest_upsample = saved


def _loss(outs, targets=None):
    if targets is None:
        return sum((o ** 2).sum() for o in outs)
    return sum(((o - t) ** 2).sum() for o, t in zip(outs, targets))


def _twin_grads(model, data, dtype):
    twin = copy.deepcopy(model).to(dtype)
    feats = torch.ones(data["points"][0].shape[0], 1, device="cuda", dtype=dtype)
    with _restated(), torch.enable_grad():
        _loss(twin._forward(feats, data)).backward()
    return {n: p.grad.double() for n, p in twin.named_parameters()}


def test_backbone_gradients_vs_float64_twin(pyramid):
    from gaussreg_amd.kpconv import differentiable
    model = _model()
    feats = torch.ones(pyramid["points"][0].shape[0], 1, device="cuda")
    with differentiable():
        outs = model(feats, pyramid)
    assert len(outs) == 4 and all(o.grad_fn is not None for o in outs)
    _loss(outs).backward()
    g64, g32 = _twin_grads(model, pyramid, torch.float64), _twin_grads(model, pyramid, torch.float32)
    worst = 0.0
    for name, p in model.named_parameters():
        assert p.grad is not None, f"{name} received no gradient"
        assert torch.isfinite(p.grad).all(), name
        norm = g64[name].norm().item()
        r_hip = (p.grad.double() - g64[name]).norm().item() / max(norm, 1e-300)
        r_ref = (g32[name] - g64[name]).norm().item() / max(norm, 1e-300)
        print(f"\nKPB backbone {name}: |g64| {norm:.3e} rel_hip {r_hip:.3e} rel_ref {r_ref:.3e}")
        worst = max(worst, r_hip / max(8 * r_ref, 1e-6))
        assert r_hip <= max(8 * r_ref, 1e-6), f"{name}: rel_hip {r_hip:.3e} > max(8 * {r_ref:.3e}, 1e-6)"
    print(f"\nKPB backbone worst rel_hip / bar {worst:.3f}")


def test_backbone_backward_is_bit_reproducible(pyramid):
    from gaussreg_amd.kpconv import differentiable
    grads = []
    for _ in range(2):
        model = _model()
        feats = torch.ones(pyramid["points"][0].shape[0], 1, device="cuda")
        with differentiable():
            _loss(model(feats, pyramid)).backward()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if "KPConv" in n})
    assert grads[0] and all(torch.equal(grads[0][n], grads[1][n]) for n in grads[0])


def test_five_adam_steps_lower_the_loss(pyramid):
    from gaussreg_amd.kpconv import differentiable
    model = _model()
    feats = torch.ones(pyramid["points"][0].shape[0], 1, device="cuda")
    with torch.no_grad():
        gen = torch.Generator(device="cuda").manual_seed(7)
        targets = [torch.randn(o.shape, device="cuda", generator=gen) * 0.5 for o in model(feats, pyramid)]
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        with differentiable():
            loss = _loss(model(feats, pyramid), targets)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    print(f"\nKPB backbone Adam losses {losses}")
    assert losses[5] < losses[0]


def test_norm_segments_are_refused_by_the_backbone(pyramid):
    from gaussreg_amd.kpconv import differentiable
    from gaussreg_amd.kpconv_blocks import norm_segments, segment_table
    model = _model()
    feats = torch.ones(pyramid["points"][0].shape[0], 1, device="cuda")
    table = segment_table(pyramid["lengths"], torch.device("cuda"))
    with differentiable(), norm_segments(table):
        with pytest.raises(NotImplementedError, match="norm_segments"):
            model(feats, pyramid)
