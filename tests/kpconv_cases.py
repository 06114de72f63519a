"""Test helper (not collected): the KPConv case table of tests/test_gpu_kpconv_paths.py and its seeded input generator.

The table lives here, outside the GPU-marked module, so that the non-GPU test in tests/test_kpconv_rpe_f64_reference.py
can ask gr_kpconv_plan which compiled variants every case reaches and fail when one has no case."""
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name cin cout h m n k feats bias sigma special")


def case(name, cin, cout, h, m=700, n=900, k=15, feats="relu", bias=False, sigma=0.045, special=None):
    return Case(name, cin, cout, h, m, n, k, feats, bias, sigma, special)


CASES = []
# matrix-core gather: every tile count NT = Cin / 16 at H = 1, 3, 4 (one step, partial and full), 37, 64 (the last step full)
_COUT = {16: 32, 32: 64, 64: 96, 128: 40, 256: 130}
for _cin in (16, 32, 64, 128, 256):
    for _i, _h in enumerate((1, 3, 4, 37, 64)):
        CASES.append(case(f"mfma-cin{_cin}-h{_h}", _cin, _COUT[_cin], _h, feats=("relu", "mixed")[(_i + _cin // 16) % 2],
                          bias=_i % 2 == 0))
CASES += [
    # generic gather
    case("generic-cin64-h65", 64, 64, 65, feats="mixed"),                       # an MFMA width, one neighbour too many
    case("generic-cin1-first-layer", 1, 64, 40, m=2500, n=3000),               # Kd = 15: less than one slab
    case("generic-cin4", 4, 64, 40, m=2500, n=3000, feats="mixed", bias=True),
    case("generic-cin48", 48, 32, 30, feats="mixed"),
    case("generic-cin96", 96, 48, 30, bias=True),
    case("generic-cin200", 200, 72, 25, feats="mixed"),
    case("flush-cin300", 300, 96, 20, m=2500, n=3000, feats="mixed"),           # Cin > 256 threads: partial sums in WF
    case("flush-cin512", 512, 64, 20, m=1000, n=1200, bias=True),               # Kd = 15 * 512
    case("chunked-h300-cin48", 48, 64, 300, m=300, n=640, feats="mixed"),       # H > 256: two staging chunks
    case("chunked-h300-cin300", 300, 40, 300, m=260, n=640),                    # ... with the read-modify-write flush
    case("chunked-h600-cin4", 4, 20, 600, m=200, n=900, feats="mixed", bias=True),  # three chunks
    # product: the small kernel
    case("small-m100", 32, 64, 20, m=100, n=300, bias=True),
    case("small-cout3", 64, 3, 30, m=2500, n=3000, feats="mixed"),
    case("small-cout16", 20, 16, 30, m=2500, n=3000, bias=True),
    # product: 128 x 64, aligned / bounds-checked
    case("p128x64-aligned", 32, 64, 30, m=2500, n=3000, feats="mixed", bias=True),
    case("p128x64-checked-kd60", 4, 34, 30, m=2500, n=3000),
    case("p128x64-checked-cout30", 32, 30, 30, m=1281, n=1500, feats="mixed"),  # Kd % 16 == 0, Cout % 4 != 0
    # product: 64 x 128
    case("p64x128-aligned-cout96", 64, 96, 30, m=2500, n=3000, bias=True),
    case("p64x128-aligned-cout256", 64, 256, 30, m=2500, n=3000, feats="mixed"),
    case("p64x128-checked-cout130", 20, 130, 30, m=2500, n=3000, feats="mixed", bias=True),  # Kd = 300: a 12-wide tail slab
    case("p64x128-aligned-ragged-m257", 16, 100, 20, m=257, n=400),
    case("p64x128-checked-ragged-m255", 20, 201, 20, m=255, n=400, feats="mixed", bias=True),
    # product: 128 x 128 (768 tiles or more)
    case("p128x128-aligned", 16, 1024, 16, m=12300, n=2000, bias=True),
    case("p128x128-checked", 16, 1022, 16, m=12300, n=2000, feats="mixed"),
    case("p128x128-aligned-ragged-m12289", 16, 1000, 12, m=12289, n=2000, feats="mixed"),   # 128 * 96 + 1 rows
    case("p128x128-checked-ragged-m12415", 20, 1001, 12, m=12415, n=2000, bias=True),       # 128 * 97 - 1 rows, Kd = 300
    # kernel sizes
    case("k1-cin4", 4, 64, 20, k=1, feats="mixed"),                             # Kd = 4
    case("k1-cin64", 64, 64, 20, k=1, bias=True),
    case("k7-cin16", 16, 64, 20, k=7, feats="mixed"),
    case("k7-cin100", 100, 130, 20, k=7, m=1000, n=1200),
    case("k16-cin32", 32, 96, 20, k=16, bias=True),                             # KP_MAX
    case("k16-cin48", 48, 40, 20, k=16, feats="mixed"),
    # degenerate inputs
    case("n0-bias", 32, 40, 5, m=300, n=0, bias=True, special="n0"),
    case("n0-nobias", 4, 64, 5, m=300, n=0, special="n0"),
    case("m0", 32, 40, 5, m=0, n=300, bias=True, special="m0"),
    case("h0-mfma-width", 32, 40, 0, m=300, n=300, bias=True, special="h0"),
    case("h0-generic", 5, 7, 0, m=300, n=300, special="h0"),
    case("shadow-rows-mfma", 64, 64, 30, feats="mixed", bias=True, special="shadow_rows"),
    case("shadow-rows-generic", 48, 64, 30, special="shadow_rows"),
    case("zero-feature-rows-mfma", 32, 64, 30, bias=True, special="zero_rows"),
    case("zero-feature-rows-generic", 200, 64, 30, feats="mixed", special="zero_rows"),
    # most influences clamp to 0
    case("small-sigma-mfma", 64, 64, 30, sigma=0.008, feats="mixed", bias=True),
    case("small-sigma-generic", 4, 34, 30, m=2500, n=3000, sigma=0.008),
]
CASE_IDS = [c.name for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)

RADIUS = 0.07
FLAG_MARGIN = 1e-3  # rows are all-zero or |sum_c f| >= FLAG_MARGIN * sum_c |f|: the `sum > 0` flag cannot flip in fp32


def neighbors(qp, sp, h, radius=RADIUS):
    """Brute-force radius query: the h nearest support points of every query, index N (the shadow point) beyond the radius."""
    n = sp.shape[0]
    out = np.full((qp.shape[0], h), n, np.int64)
    if n == 0 or h == 0:
        return out
    hh = min(h, n)
    for r0 in range(0, qp.shape[0], 1024):
        d = ((qp[r0:r0 + 1024, None, :].astype(np.float64) - sp[None].astype(np.float64)) ** 2).sum(-1)
        idx = np.argsort(d, axis=1, kind="stable")[:, :hh]
        out[r0:r0 + 1024, :hh] = np.where(np.take_along_axis(d, idx, 1) > radius ** 2, n, idx)
    return out


def features(rng, n, cin, flavour):
    if flavour == "relu":                                      # ReLU-like, some rows all zero
        f = np.maximum(rng.normal(size=(n, cin)), 0).astype(np.float32)
    else:                                                      # GroupNorm + LeakyReLU-like: both signs, row sums of both signs
        x = rng.normal(size=(n, cin)) + rng.normal(size=(n, 1)) * 0.8
        f = np.where(x >= 0, x, 0.1 * x).astype(np.float32)
    f[::11] = 0
    f64 = f.astype(np.float64)
    f[np.abs(f64.sum(1)) < 2 * FLAG_MARGIN * np.abs(f64).sum(1)] = 0   # a row sum within rounding of 0: made a zero row
    return f


def assert_flag_margin(f):
    f64 = np.asarray(f, np.float64)
    s, a = f64.sum(1), np.abs(f64).sum(1)
    assert ((a == 0) | (np.abs(s) >= FLAG_MARGIN * a)).all(), "a feature row's sum is within fp32 rounding of 0"


def build(c):
    """Seeded inputs of a case: dict of float32 / int64 NumPy arrays (f, qp, sp, idx, kp, w, b or None)."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    # density chosen so that most queries have between a few and > h neighbours inside the radius
    side = 0.6 if c.n >= 2000 else 0.4 if c.n >= 800 else 0.3
    sp = (rng.random((c.n, 3)) * side).astype(np.float32)
    if c.n > 0:
        qp = sp[rng.integers(0, c.n, c.m)] + rng.normal(0, 0.004, (c.m, 3)).astype(np.float32)
    else:
        qp = (rng.random((c.m, 3)) * side).astype(np.float32)
    qp = qp.astype(np.float32)
    radius = RADIUS if c.h <= 64 else 10.0                     # the long rows take every point they can get
    idx = neighbors(qp, sp, c.h, radius)
    f = features(rng, c.n, c.cin, c.feats)
    if c.special == "shadow_rows":
        idx[::7] = c.n                                         # rows with only shadow neighbours
        idx[-1] = c.n
    if c.special == "zero_rows":
        for r in range(0, c.m, 97):                            # rows whose neighbours all have zero features: num -> 1
            real = idx[r][idx[r] < c.n]
            f[real] = 0
    kp = (rng.normal(size=(c.k, 3)) * 0.035).astype(np.float32)
    kp[0] = 0
    bound = 1.0 / np.sqrt(c.k * c.cin)
    w = rng.uniform(-bound, bound, (c.k, c.cin, c.cout)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, c.cout).astype(np.float32) if c.bias else None
    return {"f": f, "qp": qp, "sp": sp, "idx": idx, "kp": kp, "w": w, "b": b}
