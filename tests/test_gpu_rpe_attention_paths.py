"""GPU parity of gr_rpe_attention / gr_rpe_scores on every compiled (d_model, heads) instantiation against the float64
restatement of RPEMultiHeadAttention in the REFERENCE's association (tests/kpconv_rpe_f64.py projects the (N,M,C)
embedding through proj_p and then contracts with q; the HIP path re-associates to u = W_p^T q).

Bar: helpers.assert_as_exact_as_reference with ref32 = the float64 function evaluated in float32.  Only the softmax scores
under +-80 arguments use the form tests/test_gpu_transformer.py uses for amplified rounding (1e-5 * scale plus twice the
reference's own fp32 error)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import assert_as_exact_as_reference
from kpconv_rpe_f64 import rpe_attention_f64

pytestmark = pytest.mark.gpu

PAIRS = [(c, h) for c in (64, 128, 256) for h in (1, 2, 4, 8)]
PAIR_IDS = [f"c{c}-h{h}" for c, h in PAIRS]
SHAPES = [(37, 29), (1, 1), (5, 3), (64, 64), (33, 65), (130, 257)]   # N != M, M < 16, M straddling 16 and 64
OPTIONS = ["none", "factors", "weights", "masks", "all"]


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


def _g(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hip(att, x):
    hid, sc = att(_g(x["q"]), _g(x["k"]), _g(x["v"]), _g(x["emb"]), key_weights=_g(x["weights"]), key_masks=_g(x["masks"]),
                  attention_factors=_g(x["factors"]))
    torch.cuda.synchronize()
    return hid.cpu().numpy(), sc.cpu().numpy()


def _refs(sd, h, x, b=0, **kw):
    pick = lambda a: None if a is None else a[b]
    args = (sd, x["q"][b], x["k"][b], x["v"][b], x["emb"][b], pick(x["weights"]), pick(x["masks"]), pick(x["factors"]))
    return rpe_attention_f64(*args, num_heads=h, **kw), rpe_attention_f64(*args, num_heads=h, dtype=np.float32)


def _report(what, got, r32, r64):
    scale = np.abs(r64).max()
    e_hip, e_ref = np.abs(got - r64).max(), np.abs(r32.astype(np.float64) - r64).max()
    print(f"\nRPE {what}: scale {scale:.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e} e_hip/scale {e_hip / max(scale, 1e-300):.2e} "
          f"e_hip/e_ref {e_hip / max(e_ref, 1e-300):.2f}")


def _check(what, got, r32, r64):
    _report(what, got, r32, r64)
    assert_as_exact_as_reference(got, r32, r64, what=what)


@pytest.mark.parametrize("n,m", SHAPES, ids=[f"{n}x{m}" for n, m in SHAPES])
@pytest.mark.parametrize("c,h", PAIRS, ids=PAIR_IDS)
def test_every_instantiation_at_edge_shapes(c, h, n, m):
    att, sd = _module(c, h, seed=c + h)
    x = _inputs(c, n, m, seed=1000 * n + m + h, options="all" if m > 1 else "none")
    hid, sc = _hip(att, x)
    assert hid.shape == (1, n, c) and sc.shape == (1, h, n, m)
    (h64, s64, _), (h32, s32, _) = _refs(sd, h, x)
    _check(f"c{c} h{h} {n}x{m} hidden", hid[0], h32, h64)
    _check(f"c{c} h{h} {n}x{m} scores", sc[0], s32, s64)
    if x["masks"] is not None:
        assert (sc[0][:, :, x["masks"][0]] == 0).all()         # masked keys get exactly 0


@pytest.mark.parametrize("options", OPTIONS)
@pytest.mark.parametrize("c,h", PAIRS, ids=PAIR_IDS)
def test_factors_weights_masks_each_alone(c, h, options):
    att, sd = _module(c, h, seed=7 * c + h)
    x = _inputs(c, 37, 29, seed=c + 10 * h + len(options), options=options)
    if x["masks"] is not None:
        assert x["masks"].dtype == np.bool_                   # masks go in as bool, as the reference takes them
    hid, sc = _hip(att, x)
    (h64, s64, _), (h32, s32, _) = _refs(sd, h, x)
    _check(f"c{c} h{h} {options} hidden", hid[0], h32, h64)
    _check(f"c{c} h{h} {options} scores", sc[0], s32, s64)
    if x["masks"] is not None:
        assert (sc[0][:, :, x["masks"][0]] == 0).all() and (sc[0][:, :, ~x["masks"][0]] > 0).all()
    np.testing.assert_allclose(sc[0].sum(-1), 1.0, rtol=0, atol=2e-6)


@pytest.mark.parametrize("c,h", [(64, 8), (128, 2), (256, 4)], ids=["c64-h8", "c128-h2", "c256-h4"])
def test_every_key_masked_gives_nan_like_the_reference(c, h):
    att, sd = _module(c, h, seed=3)
    x = _inputs(c, 9, 21, seed=5, options="all")
    x["masks"][:] = True
    hid, sc = _hip(att, x)
    (h64, s64, _), _ = _refs(sd, h, x)
    assert np.isnan(h64).all() and np.isnan(s64).all()
    assert np.array_equal(np.isnan(hid[0]), np.isnan(h64)) and np.array_equal(np.isnan(sc[0]), np.isnan(s64))


@pytest.mark.parametrize("c,h", PAIRS, ids=PAIR_IDS)
def test_large_softmax_arguments(c, h):
    """Queries scaled until the scores reach +-80 before the softmax: nothing overflows, parity with float64.  The scores
    carry the fp32 rounding of arguments of that size on both sides, so they take the suite's amplified-rounding form (1e-5 of
    the scale plus twice the reference's own fp32 error); the hidden states keep the plain bar."""
    att, sd = _module(c, h, seed=11 * c + h)
    with torch.no_grad():
        att.proj_q.bias.zero_()                                # the scores are then linear in input_q
    sd["proj_q.bias"] = np.zeros_like(sd["proj_q.bias"])
    x = _inputs(c, 33, 65, seed=c + h)
    logits = rpe_attention_f64(sd, x["q"][0], x["k"][0], x["v"][0], x["emb"][0], num_heads=h, return_logits=True)[3]
    x["q"] = (x["q"] * np.float32(80.0 / np.abs(logits).max())).astype(np.float32)
    hid, sc = _hip(att, x)
    (h64, s64, _, l64), (h32, s32, _) = _refs(sd, h, x, return_logits=True)
    assert 79.0 < np.abs(l64).max() < 81.0 and l64.min() < -50 and l64.max() > 50
    assert np.isfinite(hid).all() and np.isfinite(sc).all()
    _report(f"c{c} h{h} +-80 scores", sc[0], s32, s64)
    scale = np.abs(s64).max()
    bar = 1e-5 * scale + 2.0 * np.abs(s32.astype(np.float64) - s64).max()
    assert np.abs(sc[0] - s64).max() <= bar and np.abs(sc[0] - s32.astype(np.float64)).max() <= bar
    _check(f"c{c} h{h} +-80 hidden", hid[0], h32, h64)


@pytest.mark.parametrize("c,h,n,m", [(64, 8, 8, 2100), (64, 4, 4, 9600)], ids=["67KB", "150KB-guard"])
def test_large_lds_launch(c, h, n, m):
    """heads * M * 4 bytes of scores per workgroup: above 64 KB the launch opts into the large LDS, up to the 150 KB guard."""
    assert 64 * 1024 < h * m * 4 <= 150 * 1024
    att, sd = _module(c, h, seed=m)
    x = _inputs(c, n, m, seed=m + 1, options="all")
    hid, sc = _hip(att, x)
    (h64, s64, _), (h32, s32, _) = _refs(sd, h, x)
    _check(f"c{c} h{h} {n}x{m} hidden", hid[0], h32, h64)
    _check(f"c{c} h{h} {n}x{m} scores", sc[0], s32, s64)


def test_one_key_past_the_lds_guard_is_refused():
    att, _ = _module(64, 4, seed=1)
    x = _inputs(64, 2, 9601, seed=2)
    with pytest.raises(RuntimeError, match="do not fit in LDS"):
        _hip(att, x)


@pytest.mark.parametrize("c,h", [(64, 2), (128, 8), (256, 1)], ids=["c64-h2", "c128-h8", "c256-h1"])
def test_batch_of_three_equals_three_single_calls(c, h):
    """B = 3 on the dense path, per-element masks, against three B = 1 calls, bit for bit.  (The module projects every element
    with the shapes it has alone: a BLAS product's last bit follows the operand shapes, so projections over the whole batch
    gave hidden states 1 ulp off the single call's, first seen here at c256-h1.)"""
    att, _ = _module(c, h, seed=c * h)
    x = _inputs(c, 41, 50, seed=9, options="all", batch=3)
    assert not np.array_equal(x["masks"][0], x["masks"][1])
    hid, sc = _hip(att, x)
    for b in range(3):
        one = {k: (None if v is None else v[b:b + 1]) for k, v in x.items()}
        hb, sb = _hip(att, one)
        assert np.array_equal(hid[b], hb[0]) and np.array_equal(sc[b], sb[0]), b


@pytest.mark.parametrize("c,h", [(64, 1), (128, 4), (256, 8)], ids=["c64-h1", "c128-h4", "c256-h8"])
def test_ragged_lengths_on_the_module(c, h):
    """`lengths=[n0, 0, n2]` on the module: real rows torch.equal to the unpadded call, padded rows zero, scores None, and
    the ValueErrors of _forward_ragged.  (Projections over the padded batch made c64-h1 and c128-h4 differ in the last bit.)"""
    att, sd = _module(c, h, seed=c - h)
    lengths = [23, 0, 40]
    nmax = max(lengths)
    rng = np.random.default_rng(4)
    feats = rng.normal(size=(3, nmax, c)).astype(np.float32)
    embs = [torch.from_numpy((rng.normal(size=(n, n, c)) * 0.7).astype(np.float32)).cuda() for n in lengths]
    f = _g(feats)
    hid, sc = att(f, f, f, embs, lengths=lengths)
    assert sc is None and hid.shape == (3, nmax, c)
    for b, n in enumerate(lengths):
        assert not hid[b, n:].any()                            # padded rows exactly zero
        if n:
            want, _ = att(f[b:b + 1, :n], f[b:b + 1, :n], f[b:b + 1, :n], embs[b][None])
            assert torch.equal(hid[b, :n], want[0])
            h64, _, _ = rpe_attention_f64(sd, feats[b, :n], feats[b, :n], feats[b, :n], embs[b].cpu().numpy(), num_heads=h)
            h32, _, _ = rpe_attention_f64(sd, feats[b, :n], feats[b, :n], feats[b, :n], embs[b].cpu().numpy(), num_heads=h,
                                          dtype=np.float32)
            _check(f"c{c} h{h} ragged element {b}", hid[b, :n].cpu().numpy(), h32, h64)
    with pytest.raises(ValueError):                            # wrong embedding shape
        att(f, f, f, [embs[0], embs[1], embs[2][:, :-1]], lengths=lengths)
    with pytest.raises(ValueError):                            # wrong dtype
        att(f, f, f, [embs[0].double(), embs[1], embs[2]], lengths=lengths)
    with pytest.raises(ValueError):                            # one embedding per element
        att(f, f, f, embs[:2], lengths=lengths)


@pytest.mark.parametrize("m", [255, 256, 257, 600])            # the kernel's grid splits the keys into slabs of 256
@pytest.mark.parametrize("c,h", PAIRS, ids=PAIR_IDS)
def test_rpe_scores_entry_vs_float64_positional_term(c, h, m):
    """gr_rpe_scores (the positional term alone: out[h][n][m] = emb[n][m] . u[n][h] + add[n][h]) through ctypes, with and
    without `add`, against the q . proj_p(emb) term of the float64 restatement."""
    from gaussreg_amd import _lib
    L = _lib.lib()
    n = 6
    att, sd = _module(c, h, seed=c + h + m)
    x = _inputs(c, n, m, seed=m + h)
    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.no_grad():
        q2 = att.proj_q(_g(x["q"][0])).view(n, h, c // h)
        u = torch.einsum("nhc,hcj->nhj", q2, att.proj_p.weight.view(h, c // h, c)).contiguous()
        add = torch.einsum("nhc,hc->nh", q2, att.proj_p.bias.view(h, c // h)).contiguous()
    emb = _g(x["emb"][0])
    for with_add in (True, False):
        out = torch.full((h, n, m), float("nan"), device=dev)
        _lib.check(L.gr_rpe_scores(_lib.ptr(emb), _lib.ptr(u), _lib.ptr(add) if with_add else ctypes.c_void_p(0), n, m, c, h,
                                   _lib.ptr(out), _lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        sdr = dict(sd)
        if not with_add:
            sdr["proj_p.bias"] = np.zeros_like(sd["proj_p.bias"])
        args = (sdr, x["q"][0], x["k"][0], x["v"][0], x["emb"][0])
        p64 = rpe_attention_f64(*args, num_heads=h)[2]
        p32 = rpe_attention_f64(*args, num_heads=h, dtype=np.float32)[2]
        _check(f"rpe_scores c{c} h{h} m{m} add={with_add}", out.cpu().numpy(), p32, p64)
