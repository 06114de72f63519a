"""CPU: the float64 references of tests/test_gpu_sinkhorn_backward.py are pinned three ways -- the restatement's forward
against fine_matching_f64.sinkhorn (itself pinned to the reference's goldens), its autograd by torch.autograd.gradcheck,
and the explicit reverse recurrence of the kernel against that autograd -- and every case of the table passes admission."""
import numpy as np
import pytest
import torch

import fine_matching_f64 as FM
import sinkhorn_grad_cases as C
import sinkhorn_grad_f64 as F

SMALL = [c.name for c in C.CASES if c.B * c.M * c.N <= 50000]


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_forward_equals_the_pinned_restatement(name):
    case = C.BY_NAME[name]
    x = C.build(case)
    got = F.forward(torch.tensor(x["scores"], dtype=torch.float64), torch.tensor(C.ALPHA, dtype=torch.float64), x["row_masks"],
                    x["col_masks"], case.T).numpy()
    want = FM.sinkhorn(x["scores"], x["row_masks"], x["col_masks"], C.ALPHA, case.T)
    live = FM.live_entries(x["scores"].shape, x["row_masks"], x["col_masks"])
    assert np.abs(got - want)[live].max() <= 1e-12 * np.abs(want[live]).max()
    assert np.abs(got - want)[~live].max(initial=0.0) <= 1e-12 * 1e12        # the -inf stand-ins


def test_gradcheck_2x3x4_with_masks():
    rng = np.random.default_rng(5)
    s = torch.tensor(rng.normal(size=(2, 3, 4)) * 2.0, requires_grad=True)
    a = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
    rm = np.array([[1, 0, 1], [1, 1, 1]], bool)
    cm = np.array([[1, 1, 0, 1], [0, 1, 1, 1]], bool)
    live = F.live_mask(2, 3, 4, rm, cm)[2]
    assert torch.autograd.gradcheck(lambda s, a: torch.where(live, F.forward(s, a, rm, cm, 3), torch.zeros((), dtype=s.dtype)),
                                    (s, a), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("name", SMALL + ["demo_masked"])
def test_recurrence_equals_autograd(name, drop):
    case = C.BY_NAME[name]
    x = C.build(case)
    G = x["G"][:, :case.M, :case.N] if drop else x["G"]
    args = (x["scores"], C.ALPHA, x["row_masks"], x["col_masks"], case.T, G)
    ws, wa, dust = F.grads_autograd(*args, drop=drop)
    gs, ga = F.grads_recurrence(*args, drop=drop)
    assert np.abs(gs - ws).max() <= 1e-12 * np.abs(ws).max()
    assert abs(ga - wa) <= 1e-12 * dust
    live = F.live_mask(case.B, case.M, case.N, x["row_masks"], x["col_masks"])[2].numpy()
    assert not ws[~live[:, :case.M, :case.N]].any()                         # exact zeros on masked rows and columns


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_case_is_admitted(name):
    e_ref = C.admitted(name)
    print(f"{name}: e_ref grad_scores {e_ref[0]:.2e}  grad_alpha {e_ref[1]:.2e}")
    assert all(np.isfinite(e_ref))
