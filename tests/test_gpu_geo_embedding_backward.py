"""GPU: the HIP backward of the structure embedding (gr_geo_embedding_backward, csrc/geo_embedding_backward.hip) -- the
gradients of proj_d / proj_a -- against torch autograd of the float64 restatement (tests/rpe_attention_grad_f64.py).
Cases, the handling of reduction 'max' and the bars: tests/geo_embedding_grad_cases.py.

Bars, per gradient tensor: e_hip <= 1e-5 scale and e_hip <= 8 e_ref + 1e-7 scale (e_ref: the float32 restatement's own
error).  The printed GEBWD lines are the table of docs/geo_embedding_backward_f64_errors.md.

Measured on one MI355X, 2026-10-18 (the doc has every line): e_hip / scale at most 6.2e-07 and e_hip / e_ref at most 2.64 over
all lines; the homogeneity residual of test 5 between 7e-11 and 1.3e-9 of sum |go . out|.
"""
import numpy as np
import pytest
import torch

import geo_embedding_grad_cases as gc

pytestmark = pytest.mark.gpu

F64 = torch.float64
SHORT = ["grad_w_d", "grad_b_d", "grad_w_a", "grad_b_a"]


def _c(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared case arrays are read-only


def _module(c, k, red, mode="table", state=None):
    from gaussreg_amd.embedding import GeometricStructureEmbedding
    m = GeometricStructureEmbedding(c, gc.SIGMA_D, gc.SIGMA_A, k, reduction_a=red,
                                    mode="gemm" if mode == "gemm" else "table", fp32_mfma=mode == "fp32")
    st = gc.tc.embedding_state(5, c) if state is None else state
    m.load_state_dict({name: torch.from_numpy(v) for name, v in st.items()})
    return m.cuda()


def _direct(m, pts, go, accumulate=0, out=None, ws=None, k=None, c=None, n=None, null_a=False):
    """One gr_geo_embedding_backward through _lib.call with the module's weights and F_a table -> the four gradients."""
    from gaussreg_amd import _lib
    dev = pts.device
    c = m.proj_d.weight.shape[0] if c is None else c
    k = int(m.angle_k) if k is None else k
    n = pts.shape[0] if n is None else n
    if out is None:
        out = [torch.full(s, float("nan"), device=dev) for s in ((c, c), (c,), (c, c), (c,))]
    ta = m._function_tables(dev)[1] if m.reduction_a == "max" and k > 0 else None
    f = lambda t: t.detach().float().contiguous()
    if ws is None:
        ws = _lib.lib().gr_geo_embedding_backward_workspace_bytes(n, c, k)
    gwa, gba = (None, None) if null_a else out[2:]
    _lib.call(dev, "gr_geo_embedding_backward", pts, n, go, ta, 0 if ta is None else ta.shape[0], float(m.TABLE_INV_H),
              f(m.proj_a.weight), f(m.proj_a.bias), f(m.embedding.div_term), c, float(m.sigma_d), float(m.factor_a), k,
              1 if m.reduction_a == "mean" else 0, accumulate, out[0], out[1], gwa, gba, ws=ws)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ 1. the entry point
@pytest.mark.parametrize("red", ["mean", "max"])
@pytest.mark.parametrize("case", gc.CASES + [gc.CASE_MULTI_CHUNK], ids=lambda c: "n%d_c%d_k%d" % c[:3])
def test_entry_point_against_float64(case, red):
    n, c, k, _ = case
    d = gc.case(*case, red)
    if case == gc.CASE_MULTI_CHUNK:      # the shape is here for the path it takes: several chunks and MFMA steps per slab
        from gaussreg_amd import _lib
        import ctypes
        pairs = ctypes.c_int64(0)
        assert _lib.lib().gr_geo_embedding_backward_plan(n, c, k, None, ctypes.byref(pairs), None) == 0
        assert pairs.value > 128 and pairs.value % 128 != 0
    got = _direct(_module(c, k, red), _c(d["pts"]), _c(d["go"]))
    print(f"\nGEBWD direct N {n} C {c} k {k} {red}: near-tie share {d['share']:.4f}")
    for i, name in enumerate(SHORT):
        gc.bar("GEBWD", f"direct N {n} C {c} k {k} {red} {name}", got[i], d["truth"][torch.float32][i], d["truth"][F64][i])


@pytest.mark.parametrize("red", ["mean", "max"])
def test_entry_point_without_angles(red):
    """angle_k == 0: only proj_d has a gradient; null grad_w_a / grad_b_a are accepted, and given they receive zeros."""
    n, c, k, _ = gc.CASE_K0
    d = gc.case(*gc.CASE_K0, red)
    m = _module(c, k, red)
    got = _direct(m, _c(d["pts"]), _c(d["go"]), null_a=True)
    print()
    for i in (0, 1):
        gc.bar("GEBWD", f"direct N {n} C {c} k 0 {red} {SHORT[i]}", got[i], d["truth"][torch.float32][i], d["truth"][F64][i])
    assert torch.isnan(got[2]).all() and torch.isnan(got[3]).all()          # never touched
    full = _direct(m, _c(d["pts"]), _c(d["go"]))
    assert torch.equal(full[0], got[0]) and torch.equal(full[1], got[1])
    assert not full[2].any() and not full[3].any()


# ------------------------------------------------------------------------------------------------ 2. through the module
def _module_grads(m, pts, go):
    from gaussreg_amd.kpconv import differentiable
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        plain = m(pts)
    with differentiable():
        out = m(pts)
    assert out.grad_fn is not None and torch.equal(out, plain)
    out.backward(go)
    torch.cuda.synchronize()
    return [p.grad for p in (m.proj_d.weight, m.proj_d.bias, m.proj_a.weight, m.proj_a.bias)], out


def _raises(*a, **k):
    raise AssertionError("the HIP backward must not call embedding._projection_grads")


@pytest.mark.parametrize("mode", ["table", "gemm", "fp32"])
@pytest.mark.parametrize("red", ["mean", "max"])
@pytest.mark.parametrize("case", [gc.CASES[0], gc.CASES[1]], ids=lambda c: "n%d_c%d_k%d" % c[:3])
def test_module_backward_is_hip(case, red, mode, monkeypatch):
    from gaussreg_amd import embedding
    n, c, k, _ = case
    d = gc.case(*case, red)
    m = _module(c, k, red, mode)
    assert m.grad_impl == "hip"
    monkeypatch.setattr(embedding, "_projection_grads", _raises)
    got, _ = _module_grads(m, _c(d["pts"])[None], _c(d["go"])[None])
    print()
    for i, name in enumerate(SHORT):
        gc.bar("GEBWD", f"module {mode} N {n} C {c} k {k} {red} {name}", got[i], d["truth"][torch.float32][i], d["truth"][F64][i])


@pytest.mark.parametrize("red", ["mean", "max"])
@pytest.mark.parametrize("case", [gc.CASES[0], gc.CASES[1]], ids=lambda c: "n%d_c%d_k%d" % c[:3])
def test_grad_impl_torch_is_the_recomputation_and_agrees(case, red, monkeypatch):
    """grad_impl = "torch" calls _projection_grads, and the two paths agree within the bars: |hip - torch| <= 1e-5 scale and
    <= 8 e_ref + 1e-7 scale (scale and e_ref from the float64 / float32 restatement, as everywhere in this file).

    Measured: |hip - torch| is 1.1e-6 .. 3.7e-6 of the scale on the weight gradients and 1.5e-7 .. 2.6e-7 on the biases.  The
    torch path is the less exact of the two on the GPU (single library GEMM calls over all N^2 k rows: up to 8.59 e_ref against
    float64, the kernel 0.5 .. 2.1 e_ref), so its error decides the difference: the closest line is (45, 64, 3) 'mean'
    grad_w_a at 7.98 e_ref against the bar's 8 e_ref + 1e-7 scale = 8.22 e_ref.
    """
    from gaussreg_amd import embedding
    n, c, k, _ = case
    d = gc.case(*case, red)
    m = _module(c, k, red)
    pts, go = _c(d["pts"])[None], _c(d["go"])[None]
    hip, _ = _module_grads(m, pts, go)
    hip = [g.clone() for g in hip]
    calls = []
    real = embedding._projection_grads
    monkeypatch.setattr(embedding, "_projection_grads", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    monkeypatch.setattr(m, "grad_impl", "torch")
    ref, _ = _module_grads(m, pts, go)
    assert calls == [1]
    print()
    missed = []
    for i, name in enumerate(SHORT):
        g32, g64 = d["truth"][torch.float32][i], d["truth"][F64][i]
        scale, e_ref = np.abs(g64).max(), np.abs(g32 - g64).max()
        diff = (hip[i].double() - ref[i].double()).abs().max().item()
        e_torch = np.abs(ref[i].double().cpu().numpy() - g64).max()
        e_hip = np.abs(hip[i].double().cpu().numpy() - g64).max()
        print(f"GEBWD paths N {n} C {c} k {k} {red} {name}: scale {scale:.3e} |hip - torch| {diff:.3e} e_ref {e_ref:.3e} "
              f"diff/scale {diff / scale:.2e} diff/e_ref {diff / e_ref:.2f} (against float64: hip {e_hip / e_ref:.2f} e_ref, "
              f"torch path {e_torch / e_ref:.2f} e_ref)")
        if not (diff <= 1e-5 * scale and diff <= 8 * e_ref + 1e-7 * scale):
            missed.append(name)
    assert not missed, missed
    monkeypatch.setattr(m, "grad_impl", "eager")
    with pytest.raises(ValueError, match="grad_impl"):
        _module_grads(m, pts, go)


# ------------------------------------------------------------------------------------------------ 3. accumulate, batches
@pytest.mark.parametrize("red", ["mean", "max"])
def test_batch_is_cloud_0_then_cloud_1_accumulated(red):
    n, c, k = 24, 64, 3
    d0, d1 = gc.case(n, c, k, 102, red), gc.case(n, c, k, 101, red)
    m = _module(c, k, red)
    pts = torch.stack([_c(d0["pts"]), _c(d1["pts"])])
    go = torch.stack([_c(d0["go"]), _c(d1["go"])])
    batched, _ = _module_grads(m, pts, go)
    out = _direct(m, pts[0], go[0])
    first = [g.clone() for g in out]
    out = _direct(m, pts[1], go[1], accumulate=1, out=out)
    print()
    for i, name in enumerate(SHORT):
        assert torch.equal(batched[i], out[i]), name
        assert not torch.equal(first[i], out[i]), name
        g32 = d0["truth"][torch.float32][i] + d1["truth"][torch.float32][i]
        g64 = d0["truth"][F64][i] + d1["truth"][F64][i]
        gc.bar("GEBWD", f"batch of 2 N {n} C {c} k {k} {red} {name}", out[i], g32, g64)
    # an empty cloud: accumulate = 1 leaves the gradients as they are, accumulate = 0 zeroes them
    kept = [g.clone() for g in out]
    empty = torch.zeros((0, 3), device="cuda")
    out = _direct(m, empty, torch.zeros((0, 0, c), device="cuda"), accumulate=1, out=out, n=0)
    assert all(torch.equal(a, b) for a, b in zip(kept, out))
    out = _direct(m, empty, torch.zeros((0, 0, c), device="cuda"), accumulate=0, out=out, n=0)
    assert not any(g.any() for g in out)


# ------------------------------------------------------------------------------------------------ 4. reproducible
def test_two_runs_give_the_same_bits():
    case = gc.CASES[2]                                  # (45, 96, 3): ragged last slab, ragged c-tile and j-tile
    d = gc.case(*case, "max")
    m = _module(case[1], case[2], "max")
    a = _direct(m, _c(d["pts"]), _c(d["go"]))
    b = _direct(m, _c(d["pts"]), _c(d["go"]))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 5. forward consistency
def _lattice_cloud():
    """24 distinct points of an 8^3 integer lattice times float32(0.1): many neighbours are mathematically equidistant
    and none of the distances is exact in fp32, so rounding alone decides the neighbour sets."""
    rng = np.random.default_rng(2024)
    cells = rng.choice(8 ** 3, size=24, replace=False)
    ijk = np.stack([cells // 64, (cells // 8) % 8, cells % 8], axis=1).astype(np.float32)
    return ijk * np.float32(0.1)


@pytest.mark.parametrize("mode", ["table", "gemm", "fp32"])
@pytest.mark.parametrize("red", ["mean", "max"])
def test_backward_differentiates_what_the_forward_computed(red, mode):
    """out is positively homogeneous of degree 1 in theta = (W_d, b_d, W_a, b_a), so sum go . out = sum_theta <grad, theta>
    when the backward walks the forward's neighbours and winners.  Both sides in float64 on the host from the fp32 tensors.
    Bar 1e-6 of sum |go . out|: a consistent pair leaves 4e-10 .. 2e-9, one wrong neighbour in one row 3e-5 .. 1.5e-4."""
    c, k = 64, 3
    m = _module(c, k, red, mode)
    pts = _c(_lattice_cloud())[None]
    go = _c(np.random.default_rng(23).normal(size=(1, 24, 24, c)).astype(np.float32))
    grads, out = _module_grads(m, pts, go)
    prod = go.double().cpu() * out.detach().double().cpu()
    lhs, norm = prod.sum().item(), prod.abs().sum().item()
    theta = (m.proj_d.weight, m.proj_d.bias, m.proj_a.weight, m.proj_a.bias)
    rhs = sum((g.double().cpu() * t.detach().double().cpu()).sum().item() for g, t in zip(grads, theta))
    print(f"\nGEBWD homogeneity {mode} {red}: lhs {lhs:.9e} rhs {rhs:.9e} residual {abs(lhs - rhs) / norm:.3e} of sum|go.out| "
          f"{norm:.3e}")
    assert abs(lhs - rhs) <= 1e-6 * norm


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_any_launch():
    n, c, k = 24, 64, 3
    d = gc.case(n, c, k, 102, "max")
    m = _module(c, k, "max")
    pts, go = _c(d["pts"]), _c(d["go"])
    out = [torch.full(s, 7.0, device="cuda") for s in ((c, c), (c,), (c, c), (c,))]
    big = 1 << 22
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _direct(m, pts, go, out=out, c=48, ws=big)
    with pytest.raises(RuntimeError, match="angle_k"):
        _direct(m, pts, go, out=out, k=9, ws=big)
    with pytest.raises(RuntimeError, match="angle_k"):
        _direct(m, pts[:3].contiguous(), go, out=out, n=3, ws=big)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _direct(m, pts, go, out=out, ws=torch.empty(4096, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="aligned"):
        _direct(m, pts, torch.cat([go.flatten(), go.new_zeros(4)])[1:n * n * c + 1].view(n, n, c), out=out, ws=big)
    torch.cuda.synchronize()
    assert all((g == 7.0).all() for g in out)           # nothing ran
