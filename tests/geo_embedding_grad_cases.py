"""Test helper (not collected): the seeded cases of tests/test_gpu_geo_embedding_backward.py -- the structure embedding's
projection gradients for any (N, C, angle_k), against torch autograd of the restatement (tests/rpe_attention_grad_f64.py)
in float64 (the truth) and float32 (the reference's own rounding error).

The rules are those of tests/transformer_grad_cases.py, whose `max_margin` reads module constants; here angle_k and C are
arguments.  Clouds: the dyadic grids `transformer_grad_cases.cloud(n, seed)` (distances, neighbour sets and angle arguments
exact in fp32).  Weights: `embedding_state(5, C)`.  For reduction 'max' the upstream gradient is zeroed where the float64
margin of the winner (over rivals whose angular index differs) is below NEAR_TIE x max|a|; at most NEAR_TIE_SHARE of the
entries may be zeroed -- a condition on the case, asserted, not a measurement.  A case is computed once per process and
shared by the tests; nothing in it is modified afterwards (the arrays are read-only).
"""
import functools

import numpy as np
import torch

import transformer_grad_cases as tc
from rpe_attention_grad_f64 import _lin, _sinusoid, embedding_indices, geo_embedding, grads, to_params

NEAR_TIE, NEAR_TIE_SHARE = tc.NEAR_TIE, tc.NEAR_TIE_SHARE
SIGMA_D, SIGMA_A = tc.SIGMA_D, tc.SIGMA_A
NAMES = ["proj_d.weight", "proj_d.bias", "proj_a.weight", "proj_a.bias"]
# (N, C, angle_k, cloud seed): the near-tie share of every 'max' case is below the cap (at (24, 64, 8) seeds 102 and 103 are not)
CASES = [(45, 64, 3, 102), (24, 256, 3, 102), (45, 96, 3, 101), (24, 64, 8, 104), (24, 64, 1, 101), (4, 64, 3, 102)]
CASE_K0 = (24, 64, 0, 101)
# the kernel's multi-chunk path, the only one the demo size (767 points, 6 144 pairs per slab) runs: at (128, 256) a slab has
# 192 pairs = one whole 128-pair chunk of indices and a ragged one of 64, i.e. 4 + 2 MFMA steps carried in the accumulators,
# and the last of the 86 slabs has 64 pairs.  Near-tie share of 'max' at seed 101: 0.0039 (seeds 101 .. 106: 0.0036 .. 0.0043).
CASE_MULTI_CHUNK = (128, 256, 3, 101)


def near_tie_mask(params64, points, angle_k):
    """(N, N, C) bool: the float64 margin of the 'max' winner is below NEAR_TIE x the scale of the values; and its share."""
    with torch.no_grad():
        _, a_idx = embedding_indices(torch.as_tensor(points).double(), SIGMA_D, SIGMA_A, angle_k)
        a = _lin(_sinusoid(a_idx, params64["embedding.div_term"].double()), params64, "proj_a")      # (N, N, k, C)
        top, win = a.max(dim=2)
        idx = a_idx[..., None].expand_as(a)
        idx_win = torch.gather(idx, 2, win.unsqueeze(2))
        rival = (idx - idx_win).abs() > 1e-9 * (1 + idx_win.abs())
        best = torch.where(rival, a, torch.full_like(a, float("-inf"))).max(dim=2)[0]
        mask = (top - best) < NEAR_TIE * a.abs().max()
    return mask, mask.double().mean().item()


@functools.lru_cache(maxsize=None)
def case(n, c, angle_k, seed, reduction):
    """-> dict: pts (n,3) fp32, go (n,n,c) fp32 (near ties zeroed for 'max'), state (numpy fp32 state dict), share, and
    truth[dtype] = [grad_wd, grad_bd, grad_wa, grad_ba] as float64 arrays (zeros for proj_a when angle_k == 0)."""
    pts = tc.cloud(n, seed)
    st = tc.embedding_state(5, c)
    go = np.random.default_rng(17).normal(size=(n, n, c)).astype(np.float32)
    share = 0.0
    if reduction == "max" and angle_k > 0:
        mask, share = near_tie_mask(to_params(st, torch.float64, requires_grad=False), pts, angle_k)
        assert share <= NEAR_TIE_SHARE, f"near-tie share {share:.4f} of case {(n, c, angle_k, seed)} exceeds the cap"
        go[mask.numpy()] = 0.0
    truth = {}
    for dtype in (torch.float64, torch.float32):
        p = to_params(st, dtype)
        o = geo_embedding(p, torch.from_numpy(pts), SIGMA_D, SIGMA_A, angle_k, reduction)
        truth[dtype] = grads([o], [go], [p[name] for name in NAMES])
    for a in (pts, go, *truth[torch.float64], *truth[torch.float32]):
        a.setflags(write=False)
    return dict(pts=pts, go=go, state=st, share=share, truth=truth)


def bar(tag, what, got, g32, g64):
    """The project's bars for one gradient tensor (tests/test_gpu_kpconv_backward.py): e_hip <= 1e-5 scale and
    e_hip <= 8 e_ref + 1e-7 scale; prints the line docs/geo_embedding_backward_f64_errors.md is made of."""
    got = got.detach().double().cpu().numpy().reshape(g64.shape)
    scale = np.abs(g64).max()
    e_hip, e_ref = np.abs(got - g64).max(), np.abs(g32 - g64).max()
    print(f"{tag} {what}: scale {scale:.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e} e_hip/scale {e_hip / max(scale, 1e-300):.2e} "
          f"e_hip/e_ref {e_hip / max(e_ref, 1e-300):.2f}")
    assert scale > 0 and np.isfinite(got).all(), what
    assert e_hip <= 1e-5 * scale, what
    assert e_hip <= 8 * e_ref + 1e-7 * scale, what
