"""Instance totals of the binning chunks at the headline shape (1 M Gaussians, 640 x 480, 32 views, bench.py's scene and
cameras): how large the chunks are and how many of them do not fit the scatter's LDS staging block for a given number of
resident workgroups per CU.     python tools/binning_chunks.py [P W H V]"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
from gaussreg_amd import _lib, synthetic
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch

CHUNK, TILE, MARKER = 2048, 16, 127 | (127 << 7)


def main(P=1_000_000, W=640, H=480, V=32):
    L = _lib.lib()
    g = synthetic.gaussians_c2(P, seed=0, sh_degree=3)
    t = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
    sets = [GaussianRasterizationSettings(H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3), 1.0, torch.from_numpy(c["viewmatrix"]),
                                          torch.from_numpy(c["projmatrix"]), 3, torch.from_numpy(c["campos"]), False, False)
            for c in synthetic.camera_ring(V, W, H, seed=0)]
    vb = ViewBatch(sets)
    gbytes = L.gr_raster_geom_bytes(P, V, W, H)
    geom = torch.empty(gbytes, dtype=torch.uint8, device="cuda")
    radii = torch.empty((V, P), dtype=torch.int32, device="cuda")
    nr = (ctypes.c_int64 * (V + 1))()
    _lib.check(L.gr_raster_preprocess(P, 16, _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None, _lib.ptr(t["opacities"]),
                                      _lib.ptr(t["scales"]), _lib.ptr(t["rotations"]), None, vb.array, V, _lib.ptr(radii),
                                      _lib.ptr(geom), gbytes, nr, _lib.stream_ptr(torch.device("cuda"))))
    torch.cuda.synchronize()
    off = (ctypes.c_int64 * 4)()
    L.gr_raster_debug_geom_layout(P, V, W, H, off)
    gh = geom.cpu().numpy()
    rects = gh[off[2]: off[2] + 4 * V * P].view(np.uint32).reshape(V, P).astype(np.int64)
    nvis = gh[off[3]: off[3] + 4 * V].view(np.int32)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    nchunk = (P + CHUNK - 1) // CHUNK
    tot = np.zeros((V, nchunk), np.int64)
    for v in range(V):
        r = rects[v, : nvis[v]]
        assert not (r == MARKER).any()  # (none at this image size: rectangles fit the packing)
        cnt = ((r >> 14) & 63) * ((r >> 20) & 63)
        tot[v] = np.bincount(np.arange(nvis[v]) // CHUNK, weights=cnt, minlength=nchunk)[:nchunk]
    tiles = gx * gy
    cur = 4 * ((tiles + 1) & ~1) * 2
    print(f"chunks {V * nchunk}  instances {int(tot.sum())}  largest chunk {int(tot.max())} (host figure {int(nr[V])})")
    print("percentiles 50/90/99/99.9:", [int(x) for x in np.percentile(tot, [50, 90, 99, 99.9])])
    for wgs in (2, 3, 4, 5, 6, 7, 8):
        cap = (160 * 1024 // wgs - 512 - cur) // 2
        over = tot > cap
        print(f"{wgs} workgroups per CU: stage_cap {cap:6d}  chunks over it {int(over.sum()):5d}  their instances "
              f"{int(tot[over].sum()):9d} ({100.0 * tot[over].sum() / tot.sum():.1f} %)")


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:]])
