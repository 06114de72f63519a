"""CPU: the torch restatement the transformer gradient tests take their truth from (tests/rpe_attention_grad_f64.py).

  * its forward equals the NumPy float64 restatements of tests/kpconv_rpe_f64.py (attention) and tests/geo_embedding_f64.py
    (structure embedding) at 1e-12;
  * torch.autograd.gradcheck in float64 at tiny shapes (attention with factors, weights and masks; both layer kinds; the
    embedding's projections);
  * the 'max' cases of tests/transformer_grad_cases.py meet their admission rules on the restatement alone;
  * where the reference tree is present, the gradients equal those of the reference's own RPEMultiHeadAttention and
    GeometricTransformer in float64 (a child process imports the reference; skipped where it is absent).
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import geo_embedding_f64
import transformer_grad_cases as tc
from kpconv_rpe_f64 import rpe_attention_f64
from rpe_attention_grad_f64 import (geo_embedding, geometric_transformer, grads, rpe_attention, rpe_transformer_layer,
                                    to_params, transformer_layer)

REF = "/root/reference"


def _attention_case(c, h, n, m, seed, options=True):
    rng = np.random.default_rng(seed)
    b = 1.0 / np.sqrt(c)
    sd = {}
    for name in ("proj_q", "proj_k", "proj_v", "proj_p"):
        sd[name + ".weight"] = rng.uniform(-b, b, (c, c))
        sd[name + ".bias"] = rng.uniform(-0.3, 0.3, c)
    x = {"q": rng.normal(size=(n, c)), "k": rng.normal(size=(m, c)), "v": rng.normal(size=(m, c)),
         "emb": rng.normal(size=(n, m, c)) * 0.7, "factors": None, "weights": None, "masks": None}
    if options:
        x["factors"] = rng.uniform(0.2, 1.5, (n, m))
        x["weights"] = rng.uniform(0.1, 1.0, m)
        x["masks"] = np.zeros(m, bool)
        x["masks"][rng.integers(0, m)] = True
    return sd, x


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(np.asarray(a)).requires_grad_(grad)


@pytest.mark.parametrize("c,h,n,m,options", [(64, 4, 9, 7, True), (32, 8, 5, 11, False), (16, 1, 3, 4, True)])
def test_attention_forward_equals_numpy_float64(c, h, n, m, options):
    sd, x = _attention_case(c, h, n, m, seed=c + n, options=options)
    h64, s64, _ = rpe_attention_f64(sd, x["q"], x["k"], x["v"], x["emb"], x["weights"], x["masks"], x["factors"], num_heads=h)
    with torch.no_grad():
        hid, sc = rpe_attention(to_params(sd, torch.float64), _t(x["q"]), _t(x["k"]), _t(x["v"]), _t(x["emb"]), _t(x["weights"]),
                                _t(x["masks"]), _t(x["factors"]), num_heads=h)
    assert np.abs(hid.numpy() - h64).max() <= 1e-12 * np.abs(h64).max()
    assert np.abs(sc.numpy() - s64).max() <= 1e-12 * np.abs(s64).max()


@pytest.mark.parametrize("red", ["max", "mean"])
def test_embedding_forward_equals_numpy_float64(red):
    st = tc.embedding_state(5)
    pts = tc.cloud(tc.EMB_N, tc.EMB_CLOUD_SEED[red])
    params = {"w_d": st["proj_d.weight"], "b_d": st["proj_d.bias"], "w_a": st["proj_a.weight"], "b_a": st["proj_a.bias"],
              "div": st["embedding.div_term"]}
    want = geo_embedding_f64.embedding(pts, params, tc.SIGMA_D, tc.SIGMA_A, tc.ANGLE_K, red, np.float64)
    with torch.no_grad():
        got = geo_embedding(to_params(st, torch.float64), torch.from_numpy(pts), tc.SIGMA_D, tc.SIGMA_A, tc.ANGLE_K, red).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_gradcheck_attention_float64():
    sd, x = _attention_case(4, 2, 3, 4, seed=0)
    names = sorted(sd)
    fac, kw, km = _t(x["factors"]), _t(x["weights"]), _t(x["masks"])

    def fn(q, k, v, emb, *ws):
        return rpe_attention(dict(zip(names, ws)), q, k, v, emb, kw, km, fac, num_heads=2)

    args = [_t(x[n], True) for n in ("q", "k", "v", "emb")] + [_t(sd[n], True) for n in names]
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-8, rtol=1e-6)


def _layer_state(c, rng, rpe):
    sd = {}
    lin = lambda name, o, i: sd.update({name + ".weight": rng.uniform(-0.5, 0.5, (o, i)), name + ".bias": rng.uniform(-0.3, 0.3, o)})
    for name in ("proj_q", "proj_k", "proj_v") + (("proj_p",) if rpe else ()):
        lin("attention.attention." + name, c, c)
    lin("attention.linear", c, c)
    lin("output.expand", 2 * c, c)
    lin("output.squeeze", c, 2 * c)
    for name in ("attention.norm", "output.norm"):
        sd[name + ".weight"], sd[name + ".bias"] = rng.uniform(0.8, 1.2, c), rng.uniform(-0.2, 0.2, c)
    return sd


@pytest.mark.parametrize("rpe", [True, False], ids=["rpe-layer", "cross-layer"])
def test_gradcheck_layers_float64(rpe):
    rng = np.random.default_rng(3)
    c, n, m = 4, 3, 5
    sd = _layer_state(c, rng, rpe)
    names = sorted(sd)
    km = torch.tensor([False, True, False, False, False])
    x, mem, emb = _t(rng.normal(size=(n, c)), True), _t(rng.normal(size=(m, c)), True), _t(rng.normal(size=(n, m, c)), True)

    def fn(x, mem, emb, *ws):
        p = dict(zip(names, ws))
        if rpe:
            return rpe_transformer_layer(p, x, mem, emb, key_masks=km, num_heads=2)[0]
        return transformer_layer(p, x, mem, key_masks=km, num_heads=2)[0] + 0 * emb.sum()

    assert torch.autograd.gradcheck(fn, [x, mem, emb] + [_t(sd[n], True) for n in names], eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("red", ["mean", "max"])
def test_gradcheck_embedding_projections_float64(red):
    st = tc.embedding_state(9, C=8)
    pts = torch.from_numpy(tc.cloud(6, 3)).double()
    names = ["proj_d.weight", "proj_d.bias", "proj_a.weight", "proj_a.bias"]
    div = torch.from_numpy(st["embedding.div_term"])

    def fn(*ws):
        return geo_embedding({**dict(zip(names, ws)), "embedding.div_term": div}, pts, tc.SIGMA_D, tc.SIGMA_A, tc.ANGLE_K, red)

    assert torch.autograd.gradcheck(fn, [_t(st[n].astype(np.float64), True) for n in names], eps=1e-6, atol=1e-8, rtol=1e-6)


def test_embedding_max_case_zeroes_at_most_one_percent():
    """The seed of the embedding 'max' case: the near-tie share on the restatement alone stays under the cap."""
    p64 = to_params(tc.embedding_state(5), torch.float64)
    _, share = tc.near_tie_mask(p64, tc.cloud(tc.EMB_N, tc.EMB_CLOUD_SEED["max"]), prefix="")
    print(f"\nembedding max case: near-tie share {share:.3e}")
    assert share <= tc.NEAR_TIE_SHARE


def test_stack_max_case_has_the_margin():
    m = tc.stack_module("max", tc.STACK_CASES["max"][3])
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    worst, err = tc.assert_max_margin(to_params(sd, torch.float64), to_params(sd, torch.float32), tc.stack_clouds("max"))
    print(f"\nstack max case: smallest float64 margin {worst:.3e}, fp32 error of the angular values {err:.3e}")


CHILD = textwrap.dedent('''
    import sys, types
    import numpy as np
    import torch
    REF, fin, fout = sys.argv[1:4]
    sys.path.insert(0, REF)
    for name in ("ipdb", "IPython", "open3d", "coloredlogs", "easydict", "plyfile", "fpsample", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["IPython"].embed = lambda *a, **k: None
    sys.modules["geotransformer.ext"] = types.ModuleType("geotransformer.ext")
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(4)
    import geotransformer
    assert geotransformer.__file__.startswith(REF), geotransformer.__file__
    from geotransformer.modules.transformer.rpe_transformer import RPEMultiHeadAttention
    from geotransformer.modules.geotransformer.geotransformer import GeometricTransformer
    d = dict(np.load(fin))
    t = lambda n, g=False: torch.from_numpy(d[n]).requires_grad_(g)
    out = {}
    # --- RPEMultiHeadAttention with factors, weights and masks
    c, h = (int(v) for v in d["att/cfg"])
    att = RPEMultiHeadAttention(c, h)
    att.load_state_dict({k[7:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("att/sd/")})
    xs = [t("att/" + n, True)[None] for n in ("q", "k", "v", "emb")]
    xs = [x.detach().requires_grad_(True) for x in xs]
    hid, sc = att(*xs, key_weights=t("att/weights")[None], key_masks=t("att/masks")[None], attention_factors=t("att/factors")[None])
    names = [n for n, _ in att.named_parameters()]
    gs = torch.autograd.grad([hid, sc], xs + [p for _, p in att.named_parameters()], [t("att/go_h")[None], t("att/go_s")[None]])
    for n, g in zip(["q", "k", "v", "emb"] + names, gs):
        out["att/" + n] = g.numpy().reshape(g.shape[1:] if n in ("q", "k", "v", "emb") else g.shape)
    # --- GeometricTransformer, both reductions
    for red in ("mean", "max"):
        cfg = [int(v) for v in d[red + "/cfg"]]
        m = GeometricTransformer(cfg[0], cfg[1], cfg[2], cfg[3], ["self", "cross", "self", "cross"], 0.2, 15, 3, reduction_a=red)
        sd = {k[len(red) + 4:]: torch.from_numpy(v) for k, v in d.items() if k.startswith(red + "/sd/")}
        sd["embedding.embedding.div_term"] = sd["embedding.embedding.div_term"].float()
        m.load_state_dict(sd)
        f0, f1 = t(red + "/f0", True), t(red + "/f1", True)
        o0, o1 = m(t(red + "/p0")[None], t(red + "/p1")[None], f0[None], f1[None])
        ps = list(m.named_parameters())
        gs = torch.autograd.grad([o0, o1], [f0, f1] + [p for _, p in ps], [t(red + "/go0")[None], t(red + "/go1")[None]])
        for n, g in zip(["f0", "f1"] + [n for n, _ in ps], gs):
            out[red + "/" + n] = g.numpy()
    np.savez(fout, **out)
''')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "geotransformer")), reason="reference tree not present")
def test_gradients_equal_the_reference_modules(tmp_path):
    rng = np.random.default_rng(8)
    data = {}
    c, h, n, m = 16, 4, 7, 9
    sd, x = _attention_case(c, h, n, m, seed=21)
    go_h, go_s = rng.normal(size=(n, c)), rng.normal(size=(h, n, m))
    data.update({"att/cfg": np.array([c, h]), "att/go_h": go_h, "att/go_s": go_s})
    data.update({"att/sd/" + k: v for k, v in sd.items()})
    data.update({"att/" + k: v for k, v in x.items()})
    stacks = {}
    for red in ("mean", "max"):
        mod = tc.stack_module(red, 5, input_dim=6, output_dim=5, hidden_dim=16)
        ssd = {k: v.double().numpy() for k, v in mod.state_dict().items()}
        # dyadic clouds (a generic cloud leaves rounding noise of ~1e-8 in the diagonal distances, which the two sides
        # compute in different associations); nine lattice points have no distance ties for topk to order its own way
        p0, p1 = tc.cloud(9, 40).astype(np.float64), tc.cloud(8, 41).astype(np.float64)
        f0, f1, go0, go1 = rng.normal(size=(9, 6)), rng.normal(size=(8, 6)), rng.normal(size=(9, 5)), rng.normal(size=(8, 5))
        stacks[red] = (ssd, p0, p1, f0, f1, go0, go1)
        data.update({red + "/cfg": np.array([6, 5, 16, 4]), red + "/p0": p0, red + "/p1": p1, red + "/f0": f0, red + "/f1": f1,
                     red + "/go0": go0, red + "/go1": go1})
        data.update({red + "/sd/" + k: v for k, v in ssd.items()})
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **data)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", CHILD, REF, fin, fout], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = np.load(fout)

    def same(name, got, want):
        scale = np.abs(want).max()
        assert scale > 0 and np.abs(got - want).max() <= 1e-12 * scale, (name, np.abs(got - want).max() / scale)

    p = to_params(sd, torch.float64)
    ins = [_t(x[k], True) for k in ("q", "k", "v", "emb")]
    hid, sc = rpe_attention(p, *ins, _t(x["weights"]), _t(x["masks"]), _t(x["factors"]), num_heads=h)
    names = sorted(sd)
    for name, g in zip(["q", "k", "v", "emb"] + names, grads([hid, sc], [go_h, go_s], ins + [p[k] for k in names])):
        same("att/" + name, g, ref["att/" + name])
    for red, (ssd, p0, p1, f0, f1, go0, go1) in stacks.items():
        p = to_params(ssd, torch.float64)
        names = [k for k in ssd if not k.endswith("div_term")]
        tf0, tf1 = _t(f0, True), _t(f1, True)
        o0, o1 = geometric_transformer(p, _t(p0), _t(p1), tf0, tf1, num_heads=4, blocks=tc.STACK["blocks"], sigma_d=tc.SIGMA_D,
                                       sigma_a=tc.SIGMA_A, angle_k=tc.ANGLE_K, reduction_a=red)
        for name, g in zip(["f0", "f1"] + names, grads([o0, o1], [go0, go1], [tf0, tf1] + [p[k] for k in names])):
            same(red + "/" + name, g, ref[red + "/" + name])
