"""Test helper (not collected): the seeded cases of tests/test_gpu_transformer_backward.py, shared with the CPU file
tests/test_rpe_attention_grad_f64_reference.py, which checks the admission rules of the 'max' cases without a GPU.

Clouds are the dyadic grids of tests/geo_embedding_cases.py (1/32 lattice over 4 m): distances, neighbour sets and angle
arguments are exact in fp32, so fp32 and float64 differentiate the same function -- except where reduction_a = 'max' picks
its winner among the angle_k projected values by a margin fp32 cannot resolve.  That is a property of the case, not a
rounding error of the code, and it is handled in the open:

  * embedding cases: the upstream gradient is zeroed where the float64 margin (max_margin below, on the restatement's
    values) is below NEAR_TIE x the values' scale; at most NEAR_TIE_SHARE of the entries may be zeroed;
  * whole-stack 'max' case: clouds and seed are chosen so that the float64 margin exceeds MARGIN_FACTOR x the fp32 error of
    the angular values at every entry (assert_max_margin), so no winner can flip.

The margin counts only rivals whose angular INDEX differs from the winner's: two neighbours at the same angle (always on
the diagonal, where every angle is atan2(0, 0); by symmetry elsewhere on a lattice) tie exactly, in every precision, and the
gradient does not depend on which of them wins.
"""
import numpy as np
import torch

import geo_embedding_cases
from rpe_attention_grad_f64 import _lin, _sinusoid, embedding_indices

NEAR_TIE = 1e-4
NEAR_TIE_SHARE = 0.01
MARGIN_FACTOR = 100.0
SIGMA_D, SIGMA_A, ANGLE_K = 0.2, 15, 3

EMB_N, EMB_C = 24, 64
EMB_CLOUD_SEED = {"mean": 101, "max": 102}

STACK = dict(input_dim=32, output_dim=32, hidden_dim=64, num_heads=4, blocks=["self", "cross", "self", "cross"],
             sigma_d=SIGMA_D, sigma_a=SIGMA_A, angle_k=ANGLE_K)
# (ref points, src points, cloud seed, module seed): 'mean' at the size the issue names; 'max' shrunk until a seed gives
# the margin (45 and 38 points have 2 x 10^5 entries: the smallest float64 margin among that many is below any fp32 bar)
STACK_CASES = {"mean": (45, 38, 7, 11), "max": (8, 6, 250, 11)}
PADDED = dict(lengths_ref=[19, 26], lengths_src=[22, 17], cloud_seed=31, module_seed=12)


def stack_clouds(reduction_a):
    n0, n1, seed, _ = STACK_CASES[reduction_a]
    return cloud(n0, seed), cloud(n1, seed + 1000)


def cloud(n, seed):
    """(n, 3) float32, exact dyadic values."""
    return geo_embedding_cases.build_cloud(("grid", n, 32, 128, seed)).astype(np.float32)


def max_margin(params, points, prefix="embedding."):
    """reduction 'max' in the dtype of `params`: (margin (N,N,C), values (N,N,k,C)).  margin = winner - best rival whose
    angular index differs from the winner's (inf where there is none)."""
    dtype = params[prefix + "proj_a.weight"].dtype
    with torch.no_grad():
        _, a_idx = embedding_indices(torch.as_tensor(points).to(dtype), SIGMA_D, SIGMA_A, ANGLE_K)
        a = _lin(_sinusoid(a_idx, params[prefix + "embedding.div_term"].to(dtype)), params, prefix + "proj_a")
        top, win = a.max(dim=2)                                                      # (N, N, C)
        idx_win = torch.gather(a_idx[..., None].expand_as(a), 2, win.unsqueeze(2))   # (N, N, 1, C)
        rival = (a_idx[..., None].expand_as(a) - idx_win).abs() > 1e-9 * (1 + idx_win.abs())
        best = torch.where(rival, a, torch.full_like(a, float("-inf"))).max(dim=2)[0]
        return top - best, a


def near_tie_mask(params64, points, prefix="embedding."):
    """True where the float64 margin is below NEAR_TIE x the scale of the values, and the share of such entries."""
    margin, a = max_margin(params64, points, prefix)
    mask = margin < NEAR_TIE * a.abs().max()
    return mask, mask.double().mean().item()


def assert_max_margin(params64, params32, clouds):
    """The whole-stack 'max' admission rule; returns (smallest margin, fp32 error) for the record."""
    worst, err = float("inf"), 0.0
    for pts in clouds:
        margin, a64 = max_margin(params64, pts)
        _, a32 = max_margin(params32, pts)
        worst = min(worst, margin.min().item())
        err = max(err, (a32.double() - a64).abs().max().item())
    assert worst > MARGIN_FACTOR * err, f"smallest float64 margin {worst:.3e} <= {MARGIN_FACTOR} x fp32 error {err:.3e}"
    return worst, err


def embedding_state(seed, C=EMB_C):
    """GeometricStructureEmbedding state dict (numpy fp32) with nn.Linear's default initialisation."""
    p = geo_embedding_cases.build_params(C, 1.0, seed)
    return {"embedding.div_term": p["div"], "proj_d.weight": p["w_d"], "proj_d.bias": p["b_d"], "proj_a.weight": p["w_a"],
            "proj_a.bias": p["b_a"]}


def stack_module(reduction_a, seed, **overrides):
    """gaussreg_amd's GeometricTransformer on the CPU (construction needs no GPU) with every bias and LayerNorm parameter
    moved off its initial value, so that each has a gradient worth checking."""
    from gaussreg_amd.transformer import GeometricTransformer
    torch.manual_seed(seed)
    m = GeometricTransformer(reduction_a=reduction_a, **{**STACK, **overrides})
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(1.0 + 0.2 * (torch.rand(p.shape, generator=g) - 0.5))
            elif name.endswith("bias"):
                p.copy_(0.3 * (torch.rand(p.shape, generator=g) - 0.5))
    return m
