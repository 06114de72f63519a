"""GPU: KPConvFPN trained inside kpconv.differentiable(fused_norm=True) -- every GroupNorm (with the residual add and the
LeakyReLU of a block's tail) runs the HIP forward that keeps its statistics and the HIP backward, and a norm_segments table is
accepted, so two pairs train in one pass with per-pair statistics.

The small backbone of tests/test_gpu_backbone_backward.py (input_dim 1, init_dim 16, 4 groups) on clouds of 400 points.  Truth:
the float64 twin of that test (KPConv / maxpool / nearest_upsample restated by tests/kpconv_grad_f64.py, torch's GroupNorm in
float64); the same twin in float32 gives the error stock torch has.  Bar per parameter tensor, as there:
rel_hip <= max(8 rel_ref, 1e-6) on the norm-wise relative error.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

from kpconv_grad_f64 import kpconv_ref, maxpool_ref, nearest_upsample_ref

pytestmark = pytest.mark.gpu


def _pyramid(pts, lengths, limit=24):
    from gaussreg_amd.data import precompute_data_stack_mode
    return precompute_data_stack_mode(pts, torch.tensor(lengths), 5, 0.04, 0.1, [limit] * 5)


def _untruncated(data, limit):
    """No search met its limit (a neighbour table is as wide as its fullest row, capped at the limit), so the neighbour SETS
    do not depend on the order in which a search finds them."""
    return all(idx.shape[1] < limit for key in ("neighbors", "subsampling", "upsampling") for idx in data[key])


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(11)
    return torch.from_numpy(rng.random((1600, 3)).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def pair_pyramids(clouds):
    """The two pairs alone (what the twin runs) and both in one stack (what the batched pass runs).  Two things make a pair
    the same network input alone and in the stack.  The limit of these pyramids is one no search meets, so no neighbour set
    depends on the order in which a search finds its neighbours.  And the index tables of the pairs alone are padded with
    their shadow index to the width the stack's tables have (a table is as wide as its fullest row, and the stack holds the
    fuller rows of both pairs): maxpool takes the maximum over the zero shadow row wherever a row has padding
    (functional.py:54-67), so a row that fills the table of its pair alone, but not the stack's, pools over a zero only in
    the stack."""
    alone = [_pyramid(clouds[:800].contiguous(), [400, 400], 160), _pyramid(clouds[800:].contiguous(), [400, 400], 160)]
    both = _pyramid(clouds, [400] * 4, 160)
    assert all(_untruncated(d, 160) for d in alone + [both])
    for d in alone:
        for key, src in (("neighbors", 0), ("subsampling", 0), ("upsampling", 1)):
            for lv, idx in enumerate(d[key]):
                pad = both[key][lv].shape[1] - idx.shape[1]
                assert pad >= 0
                shadow = idx.new_full((idx.shape[0], pad), d["points"][lv + src].shape[0])
                d[key][lv] = torch.cat([idx, shadow], 1).contiguous()
    for lv in range(5):     # the stack is the two pairs one after the other at every level
        assert torch.equal(both["points"][lv], torch.cat([alone[0]["points"][lv], alone[1]["points"][lv]], 0))
    return alone, both


def _model(seed=3):
    from gaussreg_amd.kpconv_blocks import KPConvFPN
    torch.manual_seed(seed)
    np.random.seed(seed)
    return KPConvFPN(1, 8, 16, 15, 0.1, 0.08, 4).cuda()


@contextlib.contextmanager
def _restated():
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


def _feats(data, dtype=torch.float32):
    return torch.ones(data["points"][0].shape[0], 1, device="cuda", dtype=dtype)


def _twin_grads(model, pyramids, dtype):
    """Gradients of the sum of the losses of every pyramid, each run alone through the restated twin."""
    twin = copy.deepcopy(model).to(dtype)
    with _restated(), torch.enable_grad():
        for data in pyramids:
            _loss(twin._forward(_feats(data, dtype), data)).backward()
    return {n: p.grad.double() for n, p in twin.named_parameters()}


def _check(model, g64, g32, tag):
    worst = 0.0
    for name, p in model.named_parameters():
        assert p.grad is not None, f"{name} received no gradient"
        assert torch.isfinite(p.grad).all(), name
        norm = g64[name].norm().item()
        r_hip = (p.grad.double() - g64[name]).norm().item() / max(norm, 1e-300)
        r_ref = (g32[name] - g64[name]).norm().item() / max(norm, 1e-300)
        print(f"\nGNB backbone {tag} {name}: |g64| {norm:.3e} rel_hip {r_hip:.3e} rel_ref {r_ref:.3e}")
        worst = max(worst, r_hip / max(8 * r_ref, 1e-6))
        assert r_hip <= max(8 * r_ref, 1e-6), f"{name}: rel_hip {r_hip:.3e} > max(8 * {r_ref:.3e}, 1e-6)"
    print(f"\nGNB backbone {tag} worst rel_hip / bar {worst:.3f}")


def _uses_the_fused_norm(outs):
    seen, todo = set(), [o.grad_fn for o in outs]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "_GroupNormFunction" in type(fn).__name__:
            return True
        todo.extend(f for f, _ in fn.next_functions)
    return False


def test_one_pair_gradients_vs_float64_twin(pair_pyramids):
    from gaussreg_amd.kpconv import differentiable
    data = pair_pyramids[0][0]
    model = _model()
    with differentiable(fused_norm=True):
        outs = model(_feats(data), data)
    assert len(outs) == 4 and _uses_the_fused_norm(outs)
    for o, w in zip(outs, model(_feats(data), data)):      # inference: outside the context
        assert w.grad_fn is None and torch.equal(o, w)
    with differentiable():
        assert not _uses_the_fused_norm(model(_feats(data), data))
    _loss(outs).backward()
    _check(model, _twin_grads(model, [data], torch.float64), _twin_grads(model, [data], torch.float32), "one pair")


def test_two_pairs_in_one_pass(pair_pyramids):
    from gaussreg_amd.kpconv import differentiable
    from gaussreg_amd.kpconv_blocks import norm_segments, segment_table
    alone, both = pair_pyramids
    table = segment_table(both["lengths"], torch.device("cuda"))
    model = _model()
    with differentiable(fused_norm=True), norm_segments(table):
        outs = model(_feats(both), both)
    with norm_segments(table):
        batched = model(_feats(both), both)
    for o, w in zip(outs, batched):
        assert o.grad_fn is not None and torch.equal(o, w)
    for o, a0, a1 in zip(outs, model(_feats(alone[0]), alone[0]), model(_feats(alone[1]), alone[1])):
        want = torch.cat([a0, a1], 0)      # a pair's rows are what the pair gets alone, up to the order of the KPConv sums
        err = (o - want).abs().max().item() / want.abs().max().item()
        print(f"\nGNB backbone two pairs: batched output against the pairs alone, max error / max {err:.2e}")
        assert o.shape == want.shape
    _loss(outs).backward()
    _check(model, _twin_grads(model, alone, torch.float64), _twin_grads(model, alone, torch.float32), "two pairs")


def test_five_adam_steps_on_the_two_pair_batch_lower_the_loss(pair_pyramids):
    from gaussreg_amd.kpconv import differentiable
    from gaussreg_amd.kpconv_blocks import norm_segments, segment_table
    both = pair_pyramids[1]
    table = segment_table(both["lengths"], torch.device("cuda"))
    model = _model()
    feats = _feats(both)
    with norm_segments(table):
        gen = torch.Generator(device="cuda").manual_seed(7)
        targets = [torch.randn(o.shape, device="cuda", generator=gen) * 0.5 for o in model(feats, both)]
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        with differentiable(fused_norm=True), norm_segments(table):
            loss = _loss(model(feats, both), targets)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    print(f"\nGNB backbone two-pair Adam losses {losses}")
    assert losses[5] < losses[0]


def test_peak_memory_is_below_the_torch_norm_path():
    from gaussreg_amd.kpconv import differentiable
    rng = np.random.default_rng(5)
    pts = torch.from_numpy(rng.random((12000, 3)).astype(np.float32)).cuda()
    data = _pyramid(pts, [6000, 6000])
    model = _model()
    feats = _feats(data)
    peak = {}
    for fused in (False, True, False, True):       # twice each: the second round has every workspace and plan in place
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        with differentiable(fused_norm=fused):
            loss = _loss(model(feats, data))
        loss.backward()
        torch.cuda.synchronize()
        peak[fused] = torch.cuda.max_memory_allocated()
        del loss
    print(f"\nGNB backbone peak memory forward + backward, 2 x 6 000 points: torch norms {peak[False] / 2**20:.1f} MB, "
          f"fused norms {peak[True] / 2**20:.1f} MB")
    assert peak[True] < peak[False]
