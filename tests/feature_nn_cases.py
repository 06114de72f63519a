"""Test helper (not collected): the seeded cases of tests/test_gpu_feature_nn.py, shared with the CPU file
tests/test_feature_nn_reference.py, and the reductions both compare against.

gr_feature_nn (csrc/feature_nn.hip) runs one kernel family for every shape: 128 x 128 tiles, a workgroup per (row tile,
strip of column tiles).  `strip_tiles` restates the host's strip rule; the strip boundary -- 128 * strip_tiles columns -- is
where a row's running minimum leaves the registers, and the 128-row tile is where a column's does.

Bits: the oracle is ops.pairwise_distance reduced by `reduce_matrix` ("minimum value, then smallest index holding it", NaN
as +inf).  Float64: `feature_nn_f64` holds the brute force and the comparison; a decision is clear when the float64 gap
between best and runner-up exceeds 2 * PD_BOUND * s (coarse_stage_cases.PD_BOUND, s = s_ij of the larger candidate)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from coarse_stage_cases import PD_BY_NAME, build_pairwise

TILE = 128
UNCLEAR_CAP = 0.02     # share of rows / of columns whose decision may be unclear in an admitted float64 case


def strip_tiles(n, m):
    """fn_strip_tiles of feature_nn.hip: column tiles per workgroup."""
    rt, ct = -(-n // TILE), -(-m // TILE)
    strips = min(max(-(-4096 // rt), 1), ct)
    by_target = -(-ct // strips)
    by_fill = min(8, rt * ct // 512)
    return min(max(by_target, by_fill, 1), ct)


# A shape whose sweep crosses the strip boundary (256 columns: strips of two tiles) many times, and the 128-row tile boundary
# of the columns' direction
STRIP_SHAPE = (4100, 4200, 8)
assert strip_tiles(*STRIP_SHAPE[:2]) == 2 and strip_tiles(1700, 1700) == 1

FnCase = namedtuple("FnCase", "name n m c kind f64 misaligned")


def _seed(name):
    return zlib.crc32(name.encode())


def _case(n, m, c, kind="gauss", f64=True, misaligned=False, tag=""):
    return FnCase(f"{n}x{m}x{c}_{kind}{tag}", n, m, c, kind, f64, misaligned)


# kind: "gauss" N(0,1) rows; "unit" / "room": the rows of coarse_stage_cases' case of that shape.  f64: admitted to the
# float64 comparison (the room kind is not: heavy cancellation leaves a third of one direction unclear; the strip case is
# there for the bits and would only repeat 1700 x 1700 x 16 at ten times the float64 work)
CASES = [_case(1, 1, 1), _case(1, 300, 7), _case(300, 1, 7), _case(64, 64, 32), _case(65, 63, 33), _case(127, 129, 16),
         _case(129, 257, 17), _case(200, 130, 256), _case(40, 50, 1024), _case(1700, 1700, 16),
         _case(1665, 1700, 3, "room", f64=False), _case(1300, 1200, 36, "unit"),
         _case(150, 140, 16, misaligned=True, tag="_off4"), _case(*STRIP_SHAPE, f64=False, tag="_strip"),
         _case(2000, 1500, 32)]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
F64_CASES = [c.name for c in CASES if c.f64]

_SHARED = {"1665x1700x3_room": "big_scalar_1x1665x1700x3_room", "1300x1200x36_unit": "big_vec_2x1300x1200x36_unit"}


@functools.lru_cache(maxsize=None)
def build(name):
    """-> x (n, c), y (m, c) float32, read-only."""
    case = BY_NAME[name]
    if name in _SHARED:
        x, y = (a[0].copy() for a in build_pairwise(PD_BY_NAME[_SHARED[name]]))
    else:
        rng = np.random.default_rng(_seed("fn_" + name))
        x = rng.normal(size=(case.n, case.c)).astype(np.float32)
        y = rng.normal(size=(case.m, case.c)).astype(np.float32)
    assert x.shape == (case.n, case.c) and y.shape == (case.m, case.c)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def unit_rows(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def reduce_matrix(d):
    """d (n, m) float32, numpy or torch -> (row_index, row_dist2, col_index, col_dist2): minimum value, then the smallest
    index holding it, NaN as +inf; -1 / +inf along an empty axis.  numpy arrays."""
    d = np.array(d.cpu().numpy() if hasattr(d, "cpu") else d, np.float32)
    d[np.isnan(d)] = np.inf
    n, m = d.shape
    if m:
        ri = d.argmin(1).astype(np.int64)      # (numpy's argmin returns the first of equal minima)
        rd = d[np.arange(n), ri]
    else:
        ri, rd = np.full(n, -1, np.int64), np.full(n, np.inf, np.float32)
    if n:
        ci = d.argmin(0).astype(np.int64)
        cd = d[ci, np.arange(m)]
    else:
        ci, cd = np.full(m, -1, np.int64), np.full(m, np.inf, np.float32)
    return ri, rd, ci, cd


def integer_features(n, m, c, seed):
    """Integer-valued features in [-4, 4]: with c <= 64 every product, sum and distance is exact in fp32."""
    assert c <= 64
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, (n, c)).astype(np.float32), rng.integers(-4, 5, (m, c)).astype(np.float32))


def reference_corr_indices(ref_nn, src_nn, n_ref, n_src, mutual, bilateral):
    """The index logic of the reference's extract_corr_indices_from_feats (utils/registration.py:228-243) over given
    neighbours."""
    if mutual or bilateral:
        ref_indices = np.arange(n_ref)
        if mutual:
            ref_masks = np.equal(src_nn[ref_nn], ref_indices)
            ref_corr = ref_indices[ref_masks]
            return ref_corr, ref_nn[ref_corr]
        src_indices = np.arange(n_src)
        return np.concatenate([ref_indices, src_nn], axis=0), np.concatenate([ref_nn, src_indices], axis=0)
    return np.arange(n_ref), ref_nn
