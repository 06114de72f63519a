"""CPU model of the top-digit buckets of the depth sort at the headline shape (1 M Gaussians, 640 x 480, 32 views, bench.py's
scene and cameras): per view the shift of the top-digit pass, how large the 512 buckets are, which share of the entries sits
in buckets above each candidate cap of the small bucket class, and the largest bucket against the 7 936 entries of the large
class.  No GPU: the depth fields are computed as the preprocess does (fp32 fma chain of the view transform, float bits of
the depth minus those of 0.125), visibility by the float64 restatement of the preprocess in tests/raster_torch64.py (a few
Gaussians on a threshold may decide the other way than the fp32 kernel: nothing a histogram sees).
    python tools/depth_buckets_model.py [P W H V]"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import raster_torch64
from gaussreg_amd import synthetic

BINS, BIG_CAP, CAPS = 512, 7936, (1024, 1536, 2048, 3072, 4096)
KEY_BASE = 0x3E000000


def depth_field(view_t, p):
    """float bits of fma(M2, x, fma(M6, y, fma(M10, z, M14))) minus those of 0.125 (viewmatrix stored transposed)"""
    m = view_t.reshape(-1).astype(np.float64)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    t = (m[10] * z + m[14]).astype(np.float32).astype(np.float64)
    t = (m[6] * y + t).astype(np.float32).astype(np.float64)
    d = (m[2] * x + t).astype(np.float32)
    return d.view(np.uint32).astype(np.int64) - KEY_BASE


def main(P=1_000_000, W=640, H=480, V=32):
    g = synthetic.gaussians_c2(P, seed=0, sh_degree=3)
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    grey = torch.zeros((P, 3), dtype=torch.float64)
    print(f"P {P}  {W} x {H}  views {V}  buckets per view {BINS}  large class {BIG_CAP}")
    print("view  visible  shift  used  mean  p50  p90  p99  largest   share of entries above cap " + " ".join(f"{c:>6d}" for c in CAPS))
    sizes_all, worst, vis_all = [], 0, 0
    for v, c in enumerate(synthetic.camera_ring(V, W, H, seed=0)):
        cam = dict(c, W=W, H=H)
        pre = raster_torch64.preprocess(cam, t["means3D"], t["opacities"], colors_precomp=grey, scales=t["scales"],
                                        rotations=t["rotations"])
        vis = pre["radii"].numpy() > 0
        f = depth_field(c["viewmatrix"], g["means3D"])[vis]
        assert f.size == 0 or (f.min() > 0 and f.max() < (1 << 27))
        span = int(f.max() - f.min()) if f.size else 0
        shift = max(0, span.bit_length() - 9) if span else 0
        n = np.bincount((f - f.min()) >> shift, minlength=BINS) if f.size else np.zeros(BINS, np.int64)
        used = n[n > 0]
        share = [100.0 * n[n > cap].sum() / max(1, n.sum()) for cap in CAPS]
        print(f"{v:4d} {int(vis.sum()):8d} {shift:6d} {used.size:5d} {int(used.mean()):5d} " +
              " ".join(f"{int(x):4d}" for x in np.percentile(used, [50, 90, 99])) + f" {int(n.max()):8d}   " + " " * 27 +
              " ".join(f"{s:5.1f}%" for s in share))
        sizes_all.append(n)
        worst = max(worst, int(n.max()))
        vis_all += int(vis.sum())
    n = np.concatenate(sizes_all)
    print(f"all views: visible {vis_all}  non-empty buckets {int((n > 0).sum())}  largest {worst} "
          f"({'OVERFLOWS' if worst > BIG_CAP else 'fits'} the large class of {BIG_CAP})")
    edges = [0, 1, 256, 512, 1024, 1536, 2048, 3072, 4096, 6144, BIG_CAP, 1 << 30]
    hist = np.histogram(n, bins=edges)[0]
    for lo, hi, k in zip(edges[:-1], edges[1:], hist):
        ent = int(n[(n >= lo) & (n < hi)].sum())
        print(f"  buckets of [{lo:5d}, {hi if hi < (1 << 30) else 'inf':>5}) entries: {int(k):6d}  holding {ent:9d} entries ({100.0 * ent / max(1, n.sum()):5.1f} %)")
    for cap in CAPS:
        big = n > cap
        print(f"  small cap {cap:5d}: {int(big.sum()):5d} listed buckets ({int(big.sum()) / V:6.1f} per view), "
              f"{100.0 * n[big].sum() / max(1, n.sum()):5.1f} % of the entries")


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:]])
