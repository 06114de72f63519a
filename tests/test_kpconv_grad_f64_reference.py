"""CPU: the torch restatement the KPConv gradient tests take their truth from (tests/kpconv_grad_f64.py).

  * its forward equals the NumPy float64 restatement of tests/kpconv_rpe_f64.py on cases of tests/kpconv_cases.py;
  * torch.autograd.gradcheck in float64 on a tiny shape, features away from the `sum > 0` flag boundary, pools tie-free;
  * where the reference tree is present, its gradients equal those of the reference's own KPConv module and
    functional.maxpool / nearest_upsample in float64 (a child process imports the reference; skipped where it is absent).
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import kpconv_cases
from kpconv_grad_f64 import kpconv_grads, kpconv_ref, maxpool_ref, nearest_upsample_ref
from kpconv_rpe_f64 import kpconv_f64

REF = "/root/reference"
FORWARD_CASES = ["mfma-cin16-h3", "mfma-cin32-h37", "generic-cin4", "k7-cin16", "shadow-rows-generic", "zero-feature-rows-mfma",
                 "small-sigma-generic", "h0-generic", "n0-bias"]


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_restatement_forward_equals_numpy_float64(name):
    c = kpconv_cases.CASES[kpconv_cases.CASE_IDS.index(name)]
    x = kpconv_cases.build(c)
    want = kpconv_f64(x["f"], x["qp"], x["sp"], x["idx"], x["kp"], x["w"], c.sigma, x["b"])
    t = lambda a: torch.from_numpy(a).double()
    got = kpconv_ref(t(x["f"]), t(x["qp"]), t(x["sp"]), torch.from_numpy(x["idx"]), t(x["kp"]), t(x["w"]), c.sigma,
                     None if x["b"] is None else t(x["b"])).numpy()
    scale = max(np.abs(want).max(), 1e-300)
    assert np.abs(got - want).max() <= 1e-12 * scale


def _tiny(seed=0):
    """M 5, N 7, H 3, Cin 2, Cout 3, K 15; every feature row positive with a sum far above the flag boundary."""
    rng = np.random.default_rng(seed)
    sp = rng.random((7, 3)) * 0.1
    qp = sp[:5] + rng.normal(0, 0.004, (5, 3))
    idx = rng.integers(0, 8, (5, 3))                      # 7 = the shadow point
    idx[0] = 7                                            # a row of shadows only
    f = rng.random((7, 2)) + 0.5
    kpconv_cases.assert_flag_margin(f)
    kp = rng.normal(size=(15, 3)) * 0.035
    kp[0] = 0
    w = rng.uniform(-0.3, 0.3, (15, 2, 3))
    b = rng.uniform(-0.5, 0.5, 3)
    return {"f": f, "qp": qp, "sp": sp, "idx": idx, "kp": kp, "w": w, "b": b}


def test_gradcheck_kpconv_float64():
    x = _tiny()
    t = lambda a, g=False: torch.from_numpy(a).double().requires_grad_(g)
    q, s, idx, kp = t(x["qp"]), t(x["sp"]), torch.from_numpy(x["idx"]), t(x["kp"])
    fn = lambda f, w, b: kpconv_ref(f, q, s, idx, kp, w, 0.045, b)
    assert torch.autograd.gradcheck(fn, (t(x["f"], True), t(x["w"], True), t(x["b"], True)), eps=1e-6, atol=1e-8, rtol=1e-6)


def _tie_free(seed=1):
    rng = np.random.default_rng(seed)
    x = rng.permutation(np.arange(1, 7 * 4 + 1)).reshape(7, 4).astype(np.float64) * 0.1 - 1.0   # distinct, both signs, no 0
    idx = np.stack([rng.permutation(8)[:3] for _ in range(5)])                                 # no index twice in a row
    return x, idx


def test_gradcheck_pools_float64():
    x, idx = _tie_free()
    xt, it = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(idx)
    assert torch.autograd.gradcheck(lambda v: maxpool_ref(v, it), (xt,), eps=1e-6, atol=1e-8)
    assert torch.autograd.gradcheck(lambda v: nearest_upsample_ref(v, it), (xt,), eps=1e-6, atol=1e-8)


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
    import geotransformer.modules.kpconv.kpconv as K
    from geotransformer.modules.kpconv import functional as F
    d = dict(np.load(fin))
    t = lambda n, g=False: torch.from_numpy(d[n]).requires_grad_(g)
    K.load_kernels = lambda *a, **k: d["kp"].astype(np.float32)
    m = K.KPConv(d["w"].shape[1], d["w"].shape[2], d["w"].shape[0], 0.0625, float(d["sigma"]), bias=True)
    m.kernel_points = torch.from_numpy(d["kp"])
    with torch.no_grad():
        m.weights.copy_(t("w")); m.bias.copy_(t("b"))
    f = t("f", True)
    out = m(f, t("qp"), t("sp"), torch.from_numpy(d["idx"]))
    gf, gw, gb = torch.autograd.grad(out, [f, m.weights, m.bias], t("go"))
    x = t("px", True)
    gmax, = torch.autograd.grad(F.maxpool(x, torch.from_numpy(d["pidx"])), [x], t("pgo"))
    gup, = torch.autograd.grad(F.nearest_upsample(x, torch.from_numpy(d["pidx"])), [x], t("pgo"))
    np.savez(fout, out=out.detach().numpy(), gf=gf.numpy(), gw=gw.numpy(), gb=gb.numpy(), gmax=gmax.numpy(), gup=gup.numpy())
''')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "geotransformer")), reason="reference tree not present")
def test_gradients_equal_the_reference_modules(tmp_path):
    c = kpconv_cases.case("grad-ref", 6, 5, 9, m=60, n=80, feats="mixed", bias=True)
    x = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in kpconv_cases.build(c).items()}
    rng = np.random.default_rng(5)
    go = rng.normal(size=(c.m, c.cout))
    px, pidx = _tie_free()
    pgo = rng.normal(size=(pidx.shape[0], px.shape[1]))
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, go=go, px=px, pidx=pidx, pgo=pgo, sigma=np.float64(c.sigma), **x)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", CHILD, REF, fin, fout], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = np.load(fout)
    out, gf, gw, gb = kpconv_grads(x, c.sigma, go, torch.float64)
    for name, got in (("out", out), ("gf", gf), ("gw", gw), ("gb", gb)):
        scale = np.abs(ref[name]).max()
        assert scale > 0 and np.abs(got - ref[name]).max() <= 1e-12 * scale, name
    xt, it = torch.from_numpy(px).requires_grad_(True), torch.from_numpy(pidx)
    gmax, = torch.autograd.grad(maxpool_ref(xt, it), [xt], torch.from_numpy(pgo))
    gup, = torch.autograd.grad(nearest_upsample_ref(xt, it), [xt], torch.from_numpy(pgo))
    assert np.array_equal(gmax.numpy(), ref["gmax"]) and np.array_equal(gup.numpy(), ref["gup"])
