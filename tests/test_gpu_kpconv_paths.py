"""GPU parity of gr_kpconv_forward on EVERY dispatch path against the float64 restatement (tests/kpconv_rpe_f64.py).

gr_kpconv_forward picks one of 8 gather variants (plus two inner branches of the generic one) and one of 7 product
variants by shape.  tests/kpconv_cases.py holds one table of cases; tests/test_kpconv_rpe_f64_reference.py proves on the
host (gr_kpconv_plan) that the table reaches all of them, and this file runs each case through gaussreg_amd.kpconv.KPConv.

Bar: helpers.assert_as_exact_as_reference -- |hip - f64| <= 1e-5 * scale, the same against the fp32 NumPy oracle, and
|hip - f64| <= 8 |oracle32 - f64| + 1e-7 * scale.  No output row is excluded: the generator keeps every feature row's sum
away from the rounding of the `sum > 0` neighbour flag (asserted before the GPU is touched).

maxpool / nearest_upsample ride along on the same neighbour tables (exact equality with a NumPy gather)."""
import numpy as np
import pytest
import torch

import kpconv_cases
from helpers import assert_as_exact_as_reference
from kpconv_rpe_f64 import kpconv_f64

pytestmark = pytest.mark.gpu


def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle32(x, c):
    """oracle.matching_np.kpconv (fp32) over chunks of query rows (rows are independent; the chunks bound its temporaries)."""
    from oracle import matching_np as M
    if c.m == 0:
        return np.zeros((0, c.cout), np.float32)
    step = max(1, int(2e7 // max(1, c.h * max(c.cin, 3 * c.k))))
    return np.concatenate([M.kpconv(x["f"], x["qp"][r:r + step], x["sp"], x["idx"][r:r + step], x["kp"], x["w"], c.sigma, x["b"])
                           for r in range(0, c.m, step)])


@pytest.mark.parametrize("c", kpconv_cases.CASES, ids=kpconv_cases.CASE_IDS)
def test_kpconv_path_vs_float64(c):
    from gaussreg_amd import _lib
    from gaussreg_amd.kpconv import KPConv
    x = kpconv_cases.build(c)
    kpconv_cases.assert_flag_margin(x["f"])
    ref64 = kpconv_f64(x["f"], x["qp"], x["sp"], x["idx"], x["kp"], x["w"], c.sigma, x["b"])
    ref32 = _oracle32(x, c)
    conv = KPConv(c.cin, c.cout, c.k, 0.0625, c.sigma, bias=c.bias, kernel_points=x["kp"]).cuda()
    with torch.no_grad():
        conv.weights.copy_(_c(x["w"]))
        if c.bias:
            conv.bias.copy_(_c(x["b"]))
    assert conv.weights.data_ptr() % 16 == 0  # the plan the CPU test asked for (operands_aligned = 1) is the one that runs
    y = conv(_c(x["f"]), _c(x["qp"]), _c(x["sp"]), _c(x["idx"]))
    torch.cuda.synchronize()
    assert y.shape == (c.m, c.cout) and y.dtype == torch.float32
    if c.m == 0:
        return
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    scale = np.abs(ref64).max()
    e_hip, e_ref = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max()
    plan = _lib.lib().gr_kpconv_plan(c.n, c.m, c.h, c.cin, c.cout, c.k, 1)
    print(f"\nKPCONV {c.name}: plan gather {plan & 0xff} product {plan >> 8} scale {scale:.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e} "
          f"e_hip/scale {e_hip / max(scale, 1e-300):.2e} e_hip/e_ref {e_hip / max(e_ref, 1e-300):.2f}")
    if c.special in ("n0", "h0"):  # nothing to convolve: the bias, exactly (zeros without one)
        want = np.broadcast_to(x["b"] if c.bias else np.zeros(c.cout, np.float32), got.shape)
        assert np.array_equal(got, want)
    if c.special == "shadow_rows":
        rows = (x["idx"] == c.n).all(1)
        assert rows.any() and np.array_equal(got[rows], np.broadcast_to(x["b"] if c.bias else np.zeros(c.cout, np.float32),
                                                                     (int(rows.sum()), c.cout)))
    assert_as_exact_as_reference(got, ref32, ref64, what=f"KPConv {c.name}")


def test_kpconv_null_arguments_are_refused_not_launched():
    """Support points present (n > 0) but no feature address: one clear error, no launch on a null pointer."""
    from gaussreg_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m, h, cin, cout, k = 10, 8, 4, 4, 8, 15
    t = lambda *s: torch.zeros(*s, device=dev)
    q, sp, kp, w, out = t(m, 3), t(n, 3), t(k, 3), t(k, cin, cout), t(m, cout)
    nb = torch.zeros(m, h, dtype=torch.int64, device=dev)
    ws = _lib.workspace(dev, L.gr_kpconv_workspace_bytes(n, m, k, cin))
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.check(L.gr_kpconv_forward(None, _lib.ptr(q), _lib.ptr(sp), _lib.ptr(nb), n, m, h, cin, cout, _lib.ptr(kp), k,
                                       _lib.ptr(w), None, 0.05, 1e6, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.check(L.gr_kpconv_forward(_lib.ptr(t(n, cin)), _lib.ptr(q), _lib.ptr(sp), None, n, m, h, cin, cout, _lib.ptr(kp), k,
                                       _lib.ptr(w), None, 0.05, 1e6, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))


# ---------------------------------------------------------------- maxpool / nearest_upsample on the same neighbour tables
POOL_CASES = ["mfma-cin16-h1", "mfma-cin32-h3", "mfma-cin64-h4", "mfma-cin128-h37", "generic-cin48", "shadow-rows-generic",
              "chunked-h300-cin48", "n0-bias"]


@pytest.mark.parametrize("channels", [1, 5, 8, 30, 64])          # C % 4 != 0: the scalar kernel; C % 4 == 0: four channels per thread
@pytest.mark.parametrize("name", POOL_CASES)
def test_pools_equal_a_numpy_gather(name, channels):
    from gaussreg_amd.kpconv import maxpool, nearest_upsample
    c = kpconv_cases.CASES[kpconv_cases.CASE_IDS.index(name)]
    idx = kpconv_cases.build(c)["idx"]
    rng = np.random.default_rng(channels * 1000 + c.h)
    x = rng.normal(size=(c.n, channels)).astype(np.float32)      # both signs: a shadow neighbour's 0 wins over negative features
    xs = np.concatenate([x, np.zeros((1, channels), np.float32)])
    got_max = maxpool(_c(x), _c(idx)).cpu().numpy()
    got_up = nearest_upsample(_c(x), _c(idx)).cpu().numpy()
    assert np.array_equal(got_max, xs[idx].max(1))
    assert np.array_equal(got_up, xs[idx[:, 0]])
    if c.n == 0:
        assert not got_max.any() and not got_up.any() and got_max.shape == (c.m, channels)
    if c.special == "shadow_rows":
        assert not got_max[(idx == c.n).all(1)].any()
