"""GPU: gr_sinkhorn_backward (csrc/sinkhorn.hip) and the autograd path of LearnableLogOptimalTransport inside
`gaussreg_amd.differentiable()`, against the float64 references of tests/sinkhorn_grad_f64.py on the case table of
tests/sinkhorn_grad_cases.py (each case is admitted on the CPU first).

Errors (definitions in the case module): e_hip <= 8 e_ref + 1e-7 on every case, e_hip <= 1e-5 on every case but `wide` and
`mixed`.  Exact properties: zeros on masked rows / columns, NaN on masked grad_out entries changes no bit, drop_dustbin ==
zero-padded grad_out, a matrix alone == the matrix in its batch, two calls and a side stream leave the same bits, the
forward inside differentiable() is the inference forward.  Every case prints a line starting with SKBF64;
docs/sinkhorn_backward_f64_errors.md holds one run."""
import numpy as np
import pytest
import torch

import sinkhorn_grad_cases as C
import sinkhorn_grad_f64 as F

pytestmark = pytest.mark.gpu


def _c(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _backward(x, T, G, drop=False, sel=None):
    """gr_sinkhorn_backward on (a selection `sel` of the matrices of) a case -> (grad_scores, per-matrix grad_alpha), NumPy."""
    from gaussreg_amd import _lib
    pick = (lambda a: a) if sel is None else (lambda a: None if a is None else a[sel])
    s, rm, cm, g = (_c(pick(a)) for a in (x["scores"], x["row_masks"], x["col_masks"], G))
    B, M, N = s.shape
    alpha = torch.tensor([C.ALPHA], dtype=torch.float32, device="cuda")
    gs = torch.full((B, M, N), float("nan"), dtype=torch.float32, device="cuda")     # every element must be written
    ga = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    dev = s.device
    _lib.call(dev, "gr_sinkhorn_backward", s, B, M, N, rm, cm, alpha, T, 1e12, int(drop), g, gs, ga,
              ws=_lib.lib().gr_sinkhorn_backward_workspace_bytes(B, M, N, T))
    return gs.cpu().numpy(), ga.cpu().numpy()


def _live(case, x):
    return F.live_mask(case.B, case.M, case.N, x["row_masks"], x["col_masks"])[2].numpy()


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_against_float64(name):
    case = C.BY_NAME[name]
    e_ref = C.admitted(name)                               # on the CPU, before the kernel is called
    x, want, _ = C.reference(name)
    gs, ga = _backward(x, case.T, x["G"])
    assert np.isfinite(gs).all() and np.isfinite(ga).all()
    e_hip = C.errors(gs, ga.astype(np.float64).sum(), want)
    for what, eh, er in zip(("grad_scores", "grad_alpha"), e_hip, e_ref):
        print(f"\nSKBF64 {name} {what}: e_hip {eh:.2e}  e_ref {er:.2e}  ratio {eh / er if er else float('inf'):.2f}")
    live = _live(case, x)[:, :case.M, :case.N]
    assert not gs[~live].any() and not np.signbit(gs[~live]).any(), "exact +0.0 on masked rows and columns"
    for what, eh, er in zip(("grad_scores", "grad_alpha"), e_hip, e_ref):
        assert eh <= 8 * er + 1e-7, f"{name} {what}: e_hip {eh:.2e} > 8 x e_ref {er:.2e} + 1e-7"
        if case.absolute:
            assert eh <= C.ABS_BOUND, f"{name} {what}: e_hip {eh:.2e} > {C.ABS_BOUND:g}"
    # two calls leave the same bits
    gs2, ga2 = _backward(x, case.T, x["G"])
    assert np.array_equal(gs, gs2) and np.array_equal(ga, ga2)


def test_refused_before_any_launch():
    from gaussreg_amd import _lib
    x = dict(scores=np.zeros((2, 144, 5), np.float32), row_masks=None, col_masks=None)
    with pytest.raises(RuntimeError, match="larger than 143"):
        _backward(x, 10, np.zeros((2, 145, 6), np.float32))
    assert _lib.lib().gr_sinkhorn_backward_workspace_bytes(2, 144, 5, 10) == 0
    # a workspace that is too small; batch == 0 is fine without one
    s = torch.zeros((2, 5, 5), device="cuda")
    a = torch.ones(1, device="cuda")
    g, gs, ga = torch.zeros((2, 6, 6), device="cuda"), torch.zeros((2, 5, 5), device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call(s.device, "gr_sinkhorn_backward", s, 2, 5, 5, None, None, a, 3, 1e12, 0, g, gs, ga,
                  ws=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.call(s.device, "gr_sinkhorn_backward", s, 2, 5, 5, None, None, a, 3, 1e12, 0, None, gs, ga, ws=1 << 20)
    assert _lib.call(s.device, "gr_sinkhorn_backward", None, 0, 5, 5, None, None, None, 3, 1e12, 0, None, None, None,
                     ws=torch.zeros(16, dtype=torch.uint8, device="cuda")) == 0


@pytest.mark.parametrize("name", ["tiny", "demo_masked", "max"])
def test_nan_on_masked_grad_out_changes_no_bit(name):
    case = C.BY_NAME[name]
    x = C.reference(name)[0]
    G = np.array(x["G"])
    G[~_live(case, x)] = np.nan
    assert np.isnan(G).any()
    a, b = _backward(x, case.T, x["G"]), _backward(x, case.T, G)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["tiny", "mid", "demo", "over132"])
def test_drop_dustbin_equals_zero_padded_grad_out(name):
    case = C.BY_NAME[name]
    x = C.reference(name)[0]
    G = np.zeros_like(x["G"])
    G[:, :case.M, :case.N] = x["G"][:, :case.M, :case.N]
    a = _backward(x, case.T, G)
    b = _backward(x, case.T, np.ascontiguousarray(x["G"][:, :case.M, :case.N]), drop=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name,picks", [("many", (0, 255, 511, 512, 513, 599)), ("mixed", range(6))])
def test_a_matrix_alone_equals_the_matrix_in_its_batch(name, picks):
    case = C.BY_NAME[name]
    x = C.reference(name)[0]
    gs, ga = _backward(x, case.T, x["G"])
    for b in picks:
        one = _backward(x, case.T, x["G"], sel=slice(b, b + 1))
        assert np.array_equal(one[0][0], gs[b]) and one[1][0] == ga[b], b


def test_side_stream_is_bit_equal():
    case = C.BY_NAME["mid"]
    x = C.reference("mid")[0]
    a = _backward(x, case.T, x["G"])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = _backward(x, case.T, x["G"])
    st.synchronize()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ================================================================================================== the module
def _module(T):
    from gaussreg_amd.sinkhorn import LearnableLogOptimalTransport
    ot = LearnableLogOptimalTransport(T).cuda()
    with torch.no_grad():
        ot.alpha.fill_(C.ALPHA)
    return ot


@pytest.mark.parametrize("name,drop", [("mid", False), ("mid", True), ("one", False), ("demo", True)])
def test_module_gradients(name, drop):
    import gaussreg_amd
    case = C.BY_NAME[name]
    x, want, e_ref = C.reference(name)
    ot = _module(case.T)
    s = _c(x["scores"]).requires_grad_()
    inference = ot(s, _c(x["row_masks"]), _c(x["col_masks"]), drop_dustbin=drop)
    assert not inference.requires_grad and inference.grad_fn is None        # outside the context: as before
    with gaussreg_amd.differentiable():
        out = ot(s, _c(x["row_masks"]), _c(x["col_masks"]), drop_dustbin=drop)
        with pytest.raises(ValueError, match="out="):
            ot(s, _c(x["row_masks"]), _c(x["col_masks"]), drop_dustbin=drop, out=torch.empty_like(inference))
    assert out.grad_fn is not None and torch.equal(out, inference)          # the inference forward, bit for bit
    G = x["G"][:, :case.M, :case.N] if drop else x["G"]
    live = torch.from_numpy(_live(case, x)[:, :G.shape[1], :G.shape[2]]).cuda()
    (torch.where(live, out, torch.zeros_like(out)) * _c(G)).sum().backward()
    if drop:
        want = F.grads_autograd(x["scores"], C.ALPHA, x["row_masks"], x["col_masks"], case.T, G, drop=True)
    assert ot.alpha.grad.shape == ot.alpha.shape and ot.alpha.grad.dtype == ot.alpha.dtype
    e = C.errors(s.grad.cpu().numpy(), ot.alpha.grad.item(), want)
    print(f"\nSKBF64 module {name} drop={drop}: e {e[0]:.2e} {e[1]:.2e}")
    assert e[0] <= 8 * e_ref[0] + 1e-7 and e[1] <= 8 * e_ref[1] + 1e-7 and max(e) <= C.ABS_BOUND


def test_gradient_reaches_a_cpu_float64_tensor():
    import gaussreg_amd
    case = C.BY_NAME["tiny"]
    x, want, _ = C.reference("tiny")
    ot = _module(case.T)
    s = torch.tensor(x["scores"], dtype=torch.float64, requires_grad=True)
    with gaussreg_amd.differentiable():
        out = ot(s, torch.from_numpy(np.array(x["row_masks"])), torch.from_numpy(np.array(x["col_masks"])))
    assert out.device.type == "cpu"
    live = torch.from_numpy(_live(case, x))
    (torch.where(live, out, torch.zeros_like(out)) * torch.from_numpy(np.array(x["G"]))).sum().backward()
    assert s.grad.dtype == torch.float64 and s.grad.device.type == "cpu"
    assert C.errors(s.grad.numpy(), ot.alpha.grad.item(), want)[0] <= C.ABS_BOUND


def _fine_pair(rng, B=4, K=12):
    """A synthetic pair of B patches: src = ref moved by a rigid transform plus noise, partly masked, some points far away."""
    ref = rng.normal(size=(B, K, 3))
    ang = 0.4
    Rm = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    t = np.array([0.3, -0.2, 0.1])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    src = (ref - t) @ Rm + rng.normal(size=(B, K, 3)) * 0.01            # apply_transform(src, T) ~ ref
    src = src[:, rng.permutation(K)]
    src[:, :3] += 5.0                                                     # three points without a partner
    rm, sm = rng.random((B, K)) < 0.8, rng.random((B, K)) < 0.8
    rm[:, 0], sm[:, 5] = True, True
    return ref, src, rm, sm, T


def test_fine_matching_loss_value_and_gradient():
    import gaussreg_amd
    from gaussreg_amd.loss import FineMatchingLoss
    rng = np.random.default_rng(11)
    ref, src, rm, sm, T = _fine_pair(rng)
    scores = (rng.normal(size=(4, 12, 12)) * 2.0).astype(np.float32)
    ot = _module(20)
    s = _c(scores).requires_grad_()
    crit = FineMatchingLoss(0.1)
    od = dict(ref_node_corr_knn_points=_c(ref.astype(np.float32)), src_node_corr_knn_points=_c(src.astype(np.float32)),
              ref_node_corr_knn_masks=_c(rm), src_node_corr_knn_masks=_c(sm))
    with gaussreg_amd.differentiable():
        od["matching_scores"] = ot(s, od["ref_node_corr_knn_masks"], od["src_node_corr_knn_masks"])
        loss = crit(od, dict(transform=_c(T.astype(np.float32))))
    loss.backward()
    # the same composition in float64 on the CPU
    s64 = torch.tensor(scores, dtype=torch.float64, requires_grad=True)
    a64 = torch.tensor(C.ALPHA, dtype=torch.float64, requires_grad=True)
    keep = {}
    out64 = F.forward(s64, a64, rm, sm, 20, keep=keep)
    labels = FineMatchingLoss.labels(torch.from_numpy(ref), torch.from_numpy(src), torch.from_numpy(rm), torch.from_numpy(sm),
                                     torch.from_numpy(T), 0.1)
    assert labels[:, :-1, :-1].any() and labels[:, :-1, -1].any() and labels[:, -1, :-1].any()
    want = -out64[labels].mean()
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    gs = s64.grad.numpy()
    assert np.abs(s.grad.cpu().numpy() - gs).max() <= 1e-5 * np.abs(gs).max()
    dust = torch.zeros_like(labels)
    dust[:, -1, :], dust[:, :, -1] = True, True
    assert abs(ot.alpha.grad.item() - a64.grad.item()) <= 1e-5 * keep["Z"].grad[dust].abs().sum().item()


def test_five_adam_steps_lower_the_fine_loss():
    import gaussreg_amd
    from gaussreg_amd.loss import FineMatchingLoss
    rng = np.random.default_rng(12)
    ref, src, rm, sm, T = _fine_pair(rng)
    torch.manual_seed(0)
    lin = torch.nn.Linear(3, 16).cuda()
    ot = _module(20)
    crit = FineMatchingLoss(0.1)
    od = dict(ref_node_corr_knn_points=_c(ref.astype(np.float32)), src_node_corr_knn_points=_c(src.astype(np.float32)),
              ref_node_corr_knn_masks=_c(rm), src_node_corr_knn_masks=_c(sm))
    dd = dict(transform=_c(T.astype(np.float32)))
    moved = od["src_node_corr_knn_points"] @ dd["transform"][:3, :3].T + dd["transform"][:3, 3]
    opt = torch.optim.Adam(list(lin.parameters()) + [ot.alpha], lr=0.05)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        with gaussreg_amd.differentiable():
            scores = torch.einsum("bnc,bmc->bnm", lin(od["ref_node_corr_knn_points"]), lin(moved))
            od["matching_scores"] = ot(scores, od["ref_node_corr_knn_masks"], od["src_node_corr_knn_masks"])
            loss = crit(od, dd)
        losses.append(loss.item())
        loss.backward()
        assert ot.alpha.grad is not None and lin.weight.grad is not None
        opt.step()
    print("\nSKBF64 fine loss over five Adam steps:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0]
