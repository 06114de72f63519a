"""Test helper (not collected): the seeded case table of tests/test_gpu_sinkhorn_backward.py, shared with the CPU file
tests/test_sinkhorn_grad_f64_reference.py, which walks it through the admission rule.

Errors are e = max |got - f64| over the call / scale: for grad_scores scale = max |f64 grad_scores|; for grad_alpha scale =
the float64 sum of |gZ| over the live dustbin entries (the signed sum cancels).  e_ref is the float32 run of the
restatement (sinkhorn_grad_f64.forward under torch autograd) against its float64 run.  The kernel must hold
e_hip <= 8 e_ref + 1e-7 on every case (the rule of docs/kpconv_backward_f64_errors.md) and e_hip <= ABS_BOUND on every case
but `wide` and `mixed`; a case that claims the absolute bound is admitted only with e_ref <= ABS_BOUND / 4, as in
fine_matching_cases.py.  Measured figures: docs/sinkhorn_backward_f64_errors.md."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

import sinkhorn_grad_f64 as F

ABS_BOUND = 1e-5
ABS_ADMIT = ABS_BOUND / 4
Case = namedtuple("Case", "name B M N T valid sigmas absolute")

CASES = [
    Case("tiny", 3, 5, 7, 3, 0.7, 2.0, True),             # hand-sized, ragged lanes
    Case("one", 2, 1, 1, 5, None, 2.0, True),             # only dustbins besides one entry
    Case("mid", 4, 33, 29, 20, 0.5, 2.0, True),           # part-slices of unequal length
    Case("demo", 2, 128, 128, 100, None, 2.0, True),      # dustbins on the side waves, full history
    Case("demo_masked", 2, 128, 128, 100, 0.3, 2.0, True),
    Case("edge132", 2, 131, 131, 10, None, 2.0, True),    # the last shape with one side row per wave pair
    Case("over132", 2, 132, 131, 10, None, 2.0, True),
    Case("max", 2, 143, 143, 10, 0.9, 2.0, True),         # SK_MAXD
    Case("wide", 2, 128, 128, 100, 0.3, 40.0, False),     # score range far beyond what exp(S - rowmax) holds
    Case("mixed", 6, 64, 64, 20, 0.5, (2.0, 40.0), False),
    Case("many", 600, 9, 9, 5, 0.6, 2.0, True),           # more matrices than workgroups: history slots reused
    Case("T0", 2, 7, 5, 0, 0.5, 2.0, True),               # no iterations
]
BY_NAME = {c.name: c for c in CASES}
ALPHA = 0.8


def build(case):
    """-> dict(scores (B, M, N) float32, row_masks, col_masks (bool or None), G (B, M+1, N+1) float32)."""
    rng = np.random.default_rng(zlib.crc32(("sinkhorn_grad_" + case.name).encode()))
    B, M, N = case.B, case.M, case.N
    sig = np.resize(np.asarray(case.sigmas, np.float64), B)
    scores = (rng.normal(size=(B, M, N)) * sig[:, None, None]).astype(np.float32)
    rm = cm = None
    if case.valid is not None:
        rm, cm = rng.random((B, M)) < case.valid, rng.random((B, N)) < case.valid
        rm[np.arange(B), rng.integers(M, size=B)] = True      # at least one valid row and column
        cm[np.arange(B), rng.integers(N, size=B)] = True
    G = rng.normal(size=(B, M + 1, N + 1)).astype(np.float32)
    return dict(scores=scores, row_masks=rm, col_masks=cm, G=G)


def errors(gs, ga, want):
    """(e of grad_scores, e of grad_alpha) of a result against the float64 reference triple."""
    ws, wa, dust = want
    return (float(np.abs(np.asarray(gs, np.float64) - ws).max() / np.abs(ws).max()), abs(float(ga) - wa) / dust)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (inputs, (f64 grad_scores, f64 grad_alpha, f64 sum |gZ| over the dustbins), (e_ref scores, e_ref alpha))."""
    case = BY_NAME[name]
    x = build(case)
    args = (x["scores"], ALPHA, x["row_masks"], x["col_masks"], case.T, x["G"])
    want = F.grads_autograd(*args, dtype=torch.float64)
    got32 = F.grads_autograd(*args, dtype=torch.float32)
    for a in (x["scores"], x["G"], want[0]):
        a.setflags(write=False)
    return x, want, errors(got32[0], got32[1], want)


def admitted(name):
    e_ref = reference(name)[2]
    if BY_NAME[name].absolute:
        assert max(e_ref) <= ABS_ADMIT, f"{name}: the float32 restatement is {max(e_ref):.2e} from float64 (> {ABS_ADMIT:g})"
    return e_ref
