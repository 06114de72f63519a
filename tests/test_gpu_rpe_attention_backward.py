"""GPU: the HIP backward of RPEMultiHeadAttention (gr_rpe_attention_backward) through the module inside
gaussreg_amd.kpconv.differentiable(), against torch autograd of the float64 restatement (tests/rpe_attention_grad_f64.py,
the reference's association).

Bars, per gradient tensor (those of tests/test_gpu_kpconv_backward.py): with e_hip = max|HIP - f64|,
e_ref = max|fp32 autograd of the restatement - f64| and scale = max|f64|,  e_hip <= 1e-5 scale  and
e_hip <= 8 e_ref + 1e-7 scale.  The measured figures are in docs/rpe_attention_backward_f64_errors.md.
One exception to scale = max|f64|: without factors and weights the softmax is invariant under a shift of all its arguments,
so the gradients of proj_k.bias and proj_p.bias are exactly zero and their float64 value is rounding noise (1e-16).  Where
|f64| stays below ZERO_BY_SYMMETRY x the terms the gradient sums (max_c sum_rows |dY[row, c]| of the Linear's output, from the
restatement in float64), the scale is that of the terms -- what the error of any fp32 sum is relative to.
Inputs are built as tests/test_gpu_rpe_attention_paths.py builds them.
"""

import numpy as np
import pytest
import torch

from rpe_attention_grad_f64 import grads, rpe_attention, tapped, to_params

pytestmark = pytest.mark.gpu

PAIRS = [(c, h) for c in (64, 128, 256) for h in (1, 2, 4, 8)]
PAIR_IDS = [f"c{c}-h{h}" for c, h in PAIRS]
THREE = [(64, 8), (128, 2), (256, 4)]
THREE_IDS = ["c64-h8", "c128-h2", "c256-h4"]
EDGE_SHAPES = [(1, 1), (5, 3), (33, 65), (130, 257)]
PROJ = [f"proj_{p}.{w}" for p in "qkvp" for w in ("weight", "bias")]
ZERO_BY_SYMMETRY = 1e-9
CHECKED = ["input_q", "input_k", "input_v", "embed_qk"] + PROJ


def _module(c, h, seed):
    from gaussreg_amd.rpe_attention import RPEMultiHeadAttention
    torch.manual_seed(seed)
    att = RPEMultiHeadAttention(c, h)
    with torch.no_grad():
        for lin in (att.proj_q, att.proj_k, att.proj_v, att.proj_p):
            lin.bias.uniform_(-0.3, 0.3)
    sd = {k: v.detach().numpy().copy() for k, v in att.state_dict().items()}
    return att.cuda().eval(), sd


def _inputs(c, n, m, seed, options="none", batch=1):
    rng = np.random.default_rng(seed)
    x = {"q": rng.normal(size=(batch, n, c)), "k": rng.normal(size=(batch, m, c)), "v": rng.normal(size=(batch, m, c)),
         "emb": rng.normal(size=(batch, n, m, c)) * 0.7}
    x = {k: v.astype(np.float32) for k, v in x.items()}
    x["factors"] = x["weights"] = x["masks"] = None
    if options in ("factors", "all"):
        x["factors"] = rng.uniform(0.2, 1.5, (batch, n, m)).astype(np.float32)
    if options in ("weights", "all"):
        x["weights"] = rng.uniform(0.0, 1.0, (batch, m)).astype(np.float32)
    if options in ("masks", "all"):
        mk = rng.random((batch, m)) < 0.3
        mk[:, rng.integers(0, m)] = False                     # at least one key stays
        if m > 1:
            mk[:, (np.argmin(mk, 1) + 1) % m] = True          # and at least one goes
        x["masks"] = mk
    return x


def _upstream(x, h, seed):
    """Random upstream gradients on hidden (B,N,C) and scores (B,H,N,M)."""
    rng = np.random.default_rng(seed)
    b, n, c = x["q"].shape
    x["go_h"] = rng.normal(size=(b, n, c)).astype(np.float32)
    x["go_s"] = rng.normal(size=(b, h, n, x["k"].shape[1])).astype(np.float32)
    return x


def _g(a, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _hip(att, x, scores_upstream=True, emb_grad=True, alias=False):
    """One forward + backward inside differentiable() -> ({name: gradient tensor on the GPU}, hidden, scores)."""
    from gaussreg_amd.kpconv import differentiable
    att.zero_grad(set_to_none=True)
    q = _g(x["q"], True)
    k, v = (q, q) if alias else (_g(x["k"], True), _g(x["v"], True))
    emb = _g(x["emb"], emb_grad)
    with differentiable():
        hid, sc = att(q, k, v, emb, key_weights=_g(x["weights"]), key_masks=_g(x["masks"]), attention_factors=_g(x["factors"]))
    assert hid.grad_fn is not None
    outs, ups = [hid], [_g(x["go_h"])]
    if scores_upstream:
        outs.append(sc)
        ups.append(_g(x["go_s"]))
    torch.autograd.backward(outs, ups)
    torch.cuda.synchronize()
    got = {"input_q": q.grad, "input_k": k.grad, "input_v": v.grad, "embed_qk": emb.grad}
    got.update({n: p.grad for n, p in att.named_parameters()})
    return got, hid.detach(), sc.detach()


def _truth(sd, h, x, dtype, scores_upstream=True, alias=False, b=0):
    """Gradients of the restatement for batch element b in `dtype`, as float64 numpy arrays keyed like _hip's."""
    p = to_params(sd, dtype)
    t = lambda a, g=False: None if a is None else torch.from_numpy(np.asarray(a[b])).to(dtype if a.dtype != np.bool_ else torch.bool) \
        .requires_grad_(g)
    q = t(x["q"], True)
    k, v = (q, q) if alias else (t(x["k"], True), t(x["v"], True))
    emb = t(x["emb"], True)
    with tapped() as taps:
        hid, sc = rpe_attention(p, q, k, v, emb, t(x["weights"]), t(x["masks"]), t(x["factors"]), num_heads=h)
    outs, ups = ([hid, sc], [x["go_h"][b], x["go_s"][b]]) if scores_upstream else ([hid], [x["go_h"][b]])
    wrt = [q, emb] + [p[n] for n in PROJ] if alias else [q, k, v, emb] + [p[n] for n in PROJ]
    names = ["input_q", "embed_qk"] + PROJ if alias else CHECKED
    g, terms = grads(outs, ups, wrt, taps=taps)
    return dict(zip(names, g)), terms


def _bar(what, got, g32, g64, terms=None):
    got = got.detach().double().cpu().numpy().reshape(g64.shape)
    scale = np.abs(g64).max()
    if terms is not None and scale < ZERO_BY_SYMMETRY * terms:
        what, scale = what + " (zero by symmetry: scale of the terms)", terms
    e_hip, e_ref = np.abs(got - g64).max(), np.abs(g32 - g64).max()
    print(f"RPEBWD {what}: scale {scale:.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e} e_hip/scale {e_hip / max(scale, 1e-300):.2e} "
          f"e_hip/e_ref {e_hip / max(e_ref, 1e-300):.2f}")
    assert np.isfinite(got).all(), what
    assert e_hip <= 1e-5 * scale, what
    assert e_hip <= 8 * e_ref + 1e-7 * scale, what


def _check_all(tag, c, h, x, sd, got, scores_upstream=True, alias=False):
    g64, terms = _truth(sd, h, x, torch.float64, scores_upstream, alias)
    g32, _ = _truth(sd, h, x, torch.float32, scores_upstream, alias)
    print()
    for name in g64:
        _bar(f"c{c} h{h} {tag} {name}", got[name], g32[name], g64[name], terms.get(name))


@pytest.mark.parametrize("c,h", PAIRS, ids=PAIR_IDS)
def test_every_instantiation(c, h):
    att, sd = _module(c, h, seed=c + h)
    x = _upstream(_inputs(c, 37, 29, seed=100 * c + h, options="all"), h, seed=c - h)
    got, _, _ = _hip(att, x)
    _check_all("37x29 all", c, h, x, sd, got)


@pytest.mark.parametrize("n,m", EDGE_SHAPES, ids=[f"{n}x{m}" for n, m in EDGE_SHAPES])
@pytest.mark.parametrize("c,h", THREE, ids=THREE_IDS)
def test_edge_shapes(c, h, n, m):
    att, sd = _module(c, h, seed=c + h)
    x = _upstream(_inputs(c, n, m, seed=1000 * n + m + h, options="all" if m > 1 else "none"), h, seed=n + m)
    got, _, _ = _hip(att, x)
    _check_all(f"{n}x{m}", c, h, x, sd, got)


@pytest.mark.parametrize("options", ["none", "factors", "weights", "masks"])
@pytest.mark.parametrize("c,h", THREE, ids=THREE_IDS)
def test_options_each_alone(c, h, options):
    att, sd = _module(c, h, seed=7 * c + h)
    x = _upstream(_inputs(c, 37, 29, seed=c + 10 * h + len(options), options=options), h, seed=len(options))
    got, _, _ = _hip(att, x)
    _check_all(options, c, h, x, sd, got)


@pytest.mark.parametrize("c,h", THREE, ids=THREE_IDS)
def test_upstream_on_hidden_only(c, h):
    """The scores are not used: their gradient arrives as None and the kernel runs its null grad_scores path."""
    att, sd = _module(c, h, seed=c)
    x = _upstream(_inputs(c, 37, 29, seed=c + h, options="all"), h, seed=3)
    got, _, _ = _hip(att, x, scores_upstream=False)
    _check_all("hidden-only", c, h, x, sd, got, scores_upstream=False)


@pytest.mark.parametrize("c,h", THREE, ids=THREE_IDS)
def test_embedding_without_grad_leaves_the_rest_bit_equal(c, h):
    att, _ = _module(c, h, seed=c)
    x = _upstream(_inputs(c, 37, 29, seed=c + h, options="all"), h, seed=4)
    want, _, _ = _hip(att, x)
    want = {k: v.clone() for k, v in want.items()}
    got, _, _ = _hip(att, x, emb_grad=False)
    assert got["embed_qk"] is None
    for name in CHECKED:
        if name != "embed_qk":
            assert torch.equal(got[name], want[name]), name


@pytest.mark.parametrize("c,h", THREE, ids=THREE_IDS)
def test_self_attention_aliasing(c, h):
    """One tensor as input_q, input_k and input_v: its gradient is the sum of the three."""
    att, sd = _module(c, h, seed=c + 1)
    x = _upstream(_inputs(c, 31, 31, seed=c + h, options="masks"), h, seed=5)
    got, _, _ = _hip(att, x, alias=True)
    _check_all("aliased", c, h, x, sd, got, alias=True)


def test_large_lds_launch():
    c, h, n, m = 64, 8, 8, 2100
    att, sd = _module(c, h, seed=m)
    x = _upstream(_inputs(c, n, m, seed=m + 1, options="all"), h, seed=6)
    got, _, _ = _hip(att, x)
    _check_all(f"{n}x{m}", c, h, x, sd, got)


def test_lds_guard_inside_the_context():
    """The largest M differentiable() accepts for (64, 4) runs forward and backward; one key more is refused at forward
    time, although the forward alone would take it."""
    from gaussreg_amd import _lib
    from gaussreg_amd.kpconv import differentiable
    c, h = 64, 4
    m = _lib.lib().gr_rpe_attention_backward_max_keys(c, h)
    assert 4 * (h * m + 4 * (h + 1) * c) <= 150 * 1024 < 4 * (h * (m + 1) + 4 * (h + 1) * c) and m + 1 <= 9600
    att, sd = _module(c, h, seed=1)
    x = _upstream(_inputs(c, 2, m, seed=2, options="all"), h, seed=7)
    got, _, _ = _hip(att, x)
    _check_all(f"2x{m}", c, h, x, sd, got)
    x = _inputs(c, 2, m + 1, seed=2)
    with differentiable():
        with pytest.raises(RuntimeError, match="do not fit in LDS"):
            att(_g(x["q"], True), _g(x["k"]), _g(x["v"]), _g(x["emb"]))
    hid, _ = att(_g(x["q"]), _g(x["k"]), _g(x["v"]), _g(x["emb"]))       # outside the context: the forward's own guard
    assert hid.shape == (1, 2, c)


@pytest.mark.parametrize("c,h", [(128, 4)], ids=["c128-h4"])
def test_batch_of_three_equals_three_single_calls(c, h):
    att, _ = _module(c, h, seed=c * h)
    x = _upstream(_inputs(c, 41, 50, seed=9, options="all", batch=3), h, seed=8)
    got, _, _ = _hip(att, x)
    got = {k: v.clone() for k, v in got.items()}
    for b in range(3):
        one = {k: (None if v is None else v[b:b + 1]) for k, v in x.items()}
        gb, _, _ = _hip(att, one)
        for name in ("input_q", "input_k", "input_v", "embed_qk"):
            assert torch.equal(got[name][b], gb[name][0]), (name, b)


@pytest.mark.parametrize("c,h", [(64, 1), (256, 8)], ids=["c64-h1", "c256-h8"])
def test_ragged_lengths(c, h):
    """lengths=[23, 0, 40]: the gradients of the real rows are those of the unpadded calls, the padded rows get exactly 0."""
    from gaussreg_amd.kpconv import differentiable
    att, _ = _module(c, h, seed=c - h)
    lengths = [23, 0, 40]
    nmax = max(lengths)
    rng = np.random.default_rng(4)
    feats = rng.normal(size=(3, nmax, c)).astype(np.float32)
    embs = [(rng.normal(size=(n, n, c)) * 0.7).astype(np.float32) for n in lengths]
    go = rng.normal(size=(3, nmax, c)).astype(np.float32)
    f = _g(feats, True)
    ge = [_g(e, True) for e in embs]
    with differentiable():
        hid, sc = att(f, f, f, ge, lengths=lengths)
    assert sc is None and hid.grad_fn is not None
    hid.backward(_g(go))
    pgrads = {n: p.grad.clone() for n, p in att.named_parameters()}
    total = {n: torch.zeros_like(g) for n, g in pgrads.items()}
    for b, n in enumerate(lengths):
        assert not f.grad[b, n:].any()                           # padded rows exactly zero
        if n == 0:
            continue
        att.zero_grad(set_to_none=True)
        fb, eb = _g(feats[b:b + 1, :n], True), _g(embs[b][None], True)
        with differentiable():
            hb, _ = att(fb, fb, fb, eb)
        assert torch.equal(hb[0], hid[b, :n])
        hb.backward(_g(go[b:b + 1, :n]))
        assert torch.equal(fb.grad[0], f.grad[b, :n]) and torch.equal(eb.grad[0], ge[b].grad), b
        for name, p in att.named_parameters():
            total[name] += p.grad
    for name in total:                                           # parameters: the sum over the elements, up to its order
        scale = pgrads[name].abs().max().item()
        assert (total[name] - pgrads[name]).abs().max().item() <= 1e-5 * scale, name


@pytest.mark.parametrize("c,h", THREE, ids=THREE_IDS)
def test_two_runs_are_bitwise_identical(c, h):
    att, _ = _module(c, h, seed=c)
    x = _upstream(_inputs(c, 130, 257, seed=c + h, options="all"), h, seed=9)
    a, _, _ = _hip(att, x)
    a = {k: v.clone() for k, v in a.items()}
    b, _, _ = _hip(att, x)
    for name in CHECKED:
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("c,h", THREE, ids=THREE_IDS)
def test_forward_values_are_those_of_inference(c, h):
    att, _ = _module(c, h, seed=c)
    x = _upstream(_inputs(c, 37, 29, seed=c + h, options="all"), h, seed=10)
    _, hid, sc = _hip(att, x)
    kw = dict(key_weights=_g(x["weights"]), key_masks=_g(x["masks"]), attention_factors=_g(x["factors"]))
    with torch.enable_grad():
        plain_h, plain_s = att(_g(x["q"], True), _g(x["k"], True), _g(x["v"], True), _g(x["emb"], True), **kw)
    assert plain_h.grad_fn is None and plain_s.grad_fn is None and not plain_h.requires_grad
    assert torch.equal(plain_h, hid) and torch.equal(plain_s, sc)


def test_what_has_no_gradient_is_refused():
    from gaussreg_amd.kpconv import differentiable
    from gaussreg_amd.rpe_attention import RPEMultiHeadAttention
    att, _ = _module(64, 4, seed=0)
    x = _inputs(64, 5, 6, seed=0, options="all")
    q, k, v, emb = _g(x["q"], True), _g(x["k"]), _g(x["v"]), _g(x["emb"])
    with differentiable():
        with pytest.raises(ValueError, match="key_weights"):
            att(q, k, v, emb, key_weights=_g(x["weights"], True))
        with pytest.raises(ValueError, match="attention_factors"):
            att(q, k, v, emb, attention_factors=_g(x["factors"], True))
        drop = RPEMultiHeadAttention(64, 4, dropout=0.1).cuda().train()
        with pytest.raises(NotImplementedError):
            drop(q, k, v, emb)
        hid, _ = drop.eval()(q, k, v, emb)                       # dropout switched off by eval(): fine
        assert hid.grad_fn is not None
