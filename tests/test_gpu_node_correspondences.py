"""GPU: gr_node_correspondences (csrc/node_correspondences.hip) and gaussreg_amd.matching.get_node_correspondences against
the float64 restatement of tests/node_corr_f64.py on the case table of tests/node_corr_cases.py (each case is admitted on
the CPU by tests/test_training_targets_reference.py).

Per case: wherever the float64 counts at r^2 - tau and r^2 + tau agree, the emitted set, its row-major order and the
overlaps equal the float64 answer bit for bit (the overlap through the fp32 formula); elsewhere overlap_lo <= hip <=
overlap_hi.  The dense matrix agrees with the list, two calls and a side stream leave the same bits, NaN-filled outputs are
overwritten up to C and untouched behind it.  K = 257, null pointers and a short workspace are refused before any launch.
Every case prints a line starting with NCF64; docs/coarse_targets_f64_errors.md holds one run."""
import ctypes

import numpy as np
import pytest
import torch

import node_corr_cases as C
import node_corr_f64 as F
from helpers import load_golden

pytestmark = pytest.mark.gpu


def _c(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(case, capacity=None, dense=True, fill=float("nan")):
    """One call of the entry point on NaN-filled outputs -> (indices, overlaps, C, dense matrix), NumPy, whole buffers."""
    from gaussreg_amd import _lib
    rn, sn, rp, sp, T = (_c(case[k]) for k in ("ref_nodes", "src_nodes", "ref_knn_points", "src_knn_points", "transform"))
    masks = [_c(case[k]) for k in ("ref_masks", "src_masks", "ref_knn_masks", "src_knn_masks")]
    M, N, K = rn.shape[0], sn.shape[0], rp.shape[1]
    cap = M * N if capacity is None else capacity
    idx = torch.full((cap, 2), -7, dtype=torch.int64, device="cuda")
    ov = torch.full((cap,), fill, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    dm = torch.full((M, N), fill, dtype=torch.float32, device="cuda") if dense else None
    r2 = float(F.radius_sq_f32(case["pos_radius"]))
    _lib.call(rn.device, "gr_node_correspondences", rn, sn, rp, sp, M, N, K, T, r2, *masks, idx, ov, cap, cnt, dm,
              ws=_lib.lib().gr_node_correspondences_workspace_bytes(M, N, K))
    return idx.cpu().numpy(), ov.cpu().numpy(), int(cnt.item()), None if dm is None else dm.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", C.NAMES)
def test_against_float64(name):
    case, ref = C.build(name), C.reference(name)
    idx, ov, n, dense = _raw(case)
    M, N, K = case["ref_nodes"].shape[0], case["src_nodes"].shape[0], case["ref_knn_points"].shape[1]
    decided = ref["decided"]
    want_idx, _ = F.emitted(np.where(decided, ref["ov_lo"], 0))
    print(f"\nNCF64 {name}: {M} x {N} nodes, K {K}: C {n}  float64 pairs {len(F.emitted(ref['ov_lo'])[0])} .. "
          f"{len(F.emitted(ref['ov_hi'])[0])}  undecided node pairs {int((~decided).sum())}  tau {ref['tau']:.2e}")
    # the dense matrix: every element written; decided entries bit-equal, the others inside their interval
    assert np.isfinite(dense).all()
    assert np.array_equal(_bits(dense[decided]), _bits(ref["ov_lo"][decided]))
    assert np.all((ref["ov_lo"] <= dense) & (dense <= ref["ov_hi"]))
    # the list is the dense matrix's positive entries in row-major order, written up to C and nowhere else
    l_idx, l_ov = F.emitted(dense)
    assert n == len(l_idx) and np.array_equal(idx[:n], l_idx) and np.array_equal(_bits(ov[:n]), _bits(l_ov))
    assert np.all(idx[n:] == -7) and np.isnan(ov[n:]).all()
    # on the decided pairs the emitted set and its order are the float64 ones
    keep = decided[idx[:n, 0], idx[:n, 1]]
    assert np.array_equal(idx[:n][keep], want_idx)
    # two calls, and one without the dense matrix, leave the same bits
    idx2, ov2, n2, _ = _raw(case, dense=False, fill=0.0)
    assert n2 == n and np.array_equal(idx2[:n], idx[:n]) and np.array_equal(_bits(ov2[:n]), _bits(ov[:n]))
    if name == "far":
        assert n == 0
    if name.startswith("golden"):
        g = load_golden("training.npz")
        prefix = {"golden_lattice": "nc_lattice", "golden_self": "nc_self"}[name]
        assert np.array_equal(idx[:n], g[f"{prefix}_indices"]) and np.array_equal(_bits(ov[:n]), _bits(g[f"{prefix}_overlaps"]))
        if name == "golden_self":
            assert np.all(dense[np.arange(M), np.arange(M)][case["ref_masks"]] == np.float32(1.0))


@pytest.mark.parametrize("name", ["far", "partial_masks", "room"])
def test_python_wrapper(name):
    from gaussreg_amd.matching import get_node_correspondences
    case = C.build(name)
    idx, ov, n, dense = _raw(case)
    args = [_c(case[k]) for k in ("ref_nodes", "src_nodes", "ref_knn_points", "src_knn_points", "transform")]
    masks = {k: _c(case[k]) for k in ("ref_masks", "src_masks", "ref_knn_masks", "src_knn_masks")}
    gi, go, gd = get_node_correspondences(*args, case["pos_radius"], return_dense=True, **masks)
    assert gi.dtype == torch.int64 and go.dtype == torch.float32 and gi.shape == (n, 2) and go.shape == (n,)
    assert np.array_equal(gi.cpu().numpy(), idx[:n]) and np.array_equal(_bits(go.cpu().numpy()), _bits(ov[:n]))
    assert np.array_equal(_bits(gd.cpu().numpy()), _bits(dense))
    # a side stream leaves the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        si, so = get_node_correspondences(*args, case["pos_radius"], **masks)
    side.synchronize()
    assert torch.equal(si, gi) and np.array_equal(_bits(so.cpu().numpy()), _bits(go.cpu().numpy()))
    # CPU tensors come back on the CPU
    ci, co = get_node_correspondences(*[a.cpu() for a in args], case["pos_radius"], **{k: None if v is None else v.cpu()
                                                                                          for k, v in masks.items()})
    assert ci.device.type == "cpu" and torch.equal(ci, gi.cpu()) and torch.equal(co, go.cpu())


def test_capacity_bounds_the_writes_and_the_count_is_whole():
    case = C.build("5x70")
    idx, ov, n, _ = _raw(case)
    assert n > 8
    idx2, ov2, n2, _ = _raw(case, capacity=8)
    assert n2 == n and np.array_equal(idx2, idx[:8]) and np.array_equal(_bits(ov2), _bits(ov[:8]))


def test_empty_shapes_give_zero_pairs():
    from gaussreg_amd.matching import get_node_correspondences
    T = torch.eye(4, device="cuda")
    for M, N, K in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (0, 0, 0)):
        i, o, d = get_node_correspondences(torch.zeros(M, 3, device="cuda"), torch.zeros(N, 3, device="cuda"),
                                           torch.zeros(M, K, 3, device="cuda"), torch.zeros(N, K, 3, device="cuda"), T, 0.05,
                                           return_dense=True)
        assert i.shape == (0, 2) and o.shape == (0,) and i.dtype == torch.int64 and d.shape == (M, N) and not d.any()


def test_refusals_come_before_any_launch():
    from gaussreg_amd import _lib
    L = _lib.lib()
    M = N = 4
    z = lambda *s: torch.zeros(*s, device="cuda")
    T = torch.eye(4, device="cuda")
    idx = torch.full((M * N, 2), -7, dtype=torch.int64, device="cuda")
    ov, cnt = z(M * N), torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.gr_node_correspondences_workspace_bytes(M, N, 256) + 4096, dtype=torch.uint8, device="cuda")

    bufs = {K: (z(M, 3), z(N, 3), z(M, K, 3), z(N, K, 3)) for K in (8, 257)}

    def call(K, count=cnt, ws_bytes=None):
        p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
        rn, sn, rp, sp = bufs[K]
        return L.gr_node_correspondences(p(rn), p(sn), p(rp), p(sp), M, N, K, p(T), 0.0025, None, None, None, None, p(idx), p(ov),
                                         M * N, p(count), None, p(ws), ws.numel() if ws_bytes is None else ws_bytes, None)
    assert call(257) != 0 and b"not supported" in L.gr_last_error()
    assert L.gr_node_correspondences(None, None, None, None, M, N, 8, None, 0.0025, None, None, None, None, None, None, 0,
                                     ctypes.c_void_p(cnt.data_ptr()), None, ctypes.c_void_p(ws.data_ptr()), ws.numel(), None) != 0
    assert b"null argument" in L.gr_last_error()
    assert call(8, count=None) != 0 and b"null argument" in L.gr_last_error()
    assert call(8, ws_bytes=64) != 0 and b"workspace too small" in L.gr_last_error()
    torch.cuda.synchronize()
    assert int(cnt.item()) == -1 and bool((idx == -7).all())          # nothing ran
    assert call(8) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == M * N                                    # 16 coincident patches: every pair overlaps fully
