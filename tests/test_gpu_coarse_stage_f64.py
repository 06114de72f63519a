"""GPU: the two dense operators between the backbone and fine matching -- gr_pairwise_distance(_batch)
(csrc/superpoint_matching.hip: pairwise_kernel, pairwise_big_kernel<ALIGNED> and its vec / scalar fetch) and
gr_point_to_node_partition(_batch) (csrc/point_to_node.hip: assign_kernel's LDS rounds, select_kernel's three regimes) --
against the float64 restatements of tests/coarse_stage_f64.py on the case tables of tests/coarse_stage_cases.py.

Pairwise distance: |gpu - f64| <= PD_BOUND * s_ij entrywise, every entry finite and >= 0; a matrix of a batch on the
128 x 128 kernel equals, bit for bit, the same matrix computed alone on the 64 x 64 kernel; a NaN row gives NaN on its row
or column and nowhere else.  Point to node: owners, masks, rows and knn masks exact wherever the float64 geometry is
clear (everywhere, in the planted clouds); the float32 oracle passes the same comparison on the CPU before the kernel is
called.  Every case prints its figure on a line starting with CSF64; docs/coarse_stage_f64_errors.md holds one run."""
import numpy as np
import pytest
import torch

import coarse_stage_cases as C
import coarse_stage_f64 as F

pytestmark = pytest.mark.gpu

GR_ERR_WORKSPACE = -3  # include/gaussreg_hip.h


def _c(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared references are read-only)


def _names(kernels):
    return [c.name for c in C.PD_CASES if c.kernel in kernels]


# ================================================================================================== pairwise distance
def _off4(t):
    """The same values in a view that starts one float into its storage."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _inputs(case, x, y):
    xt, yt = _c(x), _c(y)
    if case.misaligned:
        xt, yt = _off4(xt), _off4(yt)
    return xt, yt


def _distance(case, xt, yt, normalized):
    from gaussreg_amd.ops import pairwise_distance
    if case.channel_first:
        return pairwise_distance(xt.transpose(1, 2).contiguous(), yt.transpose(1, 2).contiguous(), normalized, channel_first=True)
    return pairwise_distance(xt, yt, normalized)


def _same_bits(case, xt, yt, out, normalized):
    """Every matrix (batches), or every 128 x 128 block (the 1700-sized cases), against a call of its own: one tile of
    128 x 128 at the most, so that call runs the 64 x 64 kernel.  -> number of comparisons."""
    from gaussreg_amd.ops import pairwise_distance
    assert C.kernel_of(1, min(case.n, 128), min(case.m, 128), case.C) == "small"
    blocks, equal = [], []
    for b in range(case.B):
        for i0 in range(0, case.n, 128):
            for j0 in range(0, case.m, 128):
                alone = pairwise_distance(xt[b, i0:i0 + 128], yt[b, j0:j0 + 128], normalized)
                blocks.append((b, i0, j0))
                equal.append((alone == out[b, i0:i0 + 128, j0:j0 + 128]).all())
    equal = torch.stack(equal).cpu().numpy()                # (one synchronisation for all of them)
    bad = [blocks[k] for k in np.nonzero(~equal)[0]]
    assert not bad, f"{case.name}: {len(bad)} of {len(blocks)} (matrix, row, column) blocks differ from the 64 x 64 kernel's bits: {bad[:5]}"
    return len(blocks)


def _check_pairwise(name, normalized):
    case = C.PD_BY_NAME[name]
    x, y, want, scale = C.pairwise_reference(name, normalized)
    xt, yt = _inputs(case, x, y)
    assert C.kernel_of(case.B, case.n, case.m, case.C, xt.data_ptr() % 16 == 0 and yt.data_ptr() % 16 == 0) == case.kernel
    out = _distance(case, xt, yt, normalized)
    assert out.dtype == torch.float32 and tuple(out.shape) == (case.B, case.n, case.m)
    ratio = C.pairwise_ratio(out.cpu().numpy(), want, scale)
    print(f"\nCSF64 pairwise {case.kernel} {name} normalized={int(normalized)}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: |gpu - f64| reaches {ratio:.3f} of {C.PD_BOUND:g} * s_ij (or an entry is negative / not finite)"
    if normalized and case.kind == "gauss" and case.n * case.m * case.B > 100:
        assert (want == 0).any() and (out.cpu().numpy()[want == 0] == 0).all()  # xy > 1: the clamp fires
    return case, xt, yt, out


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("name", _names(["small"]))
def test_pairwise_64_tile_kernel(name, normalized):
    """Fewer than 192 tiles of 128 x 128: pairwise_kernel.  One element, exact tiles, tiles with tails on both sides,
    k-slab tails of 32 (C = 1, 3, 17, 20, 33), many slabs (C = 1024), channel_first, and 191 matrices of one tile."""
    _check_pairwise(name, normalized)


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("name", _names(["big_aligned", "big_vec", "big_scalar"]))
def test_pairwise_128_tile_kernel_and_its_bits(name, normalized):
    """192 tiles or more: pairwise_big_kernel -- ALIGNED (C % 16 == 0), vec (C % 4 == 0) and scalar fetches, the k-slab
    tails of 16, a single row / column, tile tails, x and y one float off 16 bytes.  Each matrix or 128 x 128 block is
    also computed alone, on the 64 x 64 kernel: same bits (include/gaussreg_hip.h)."""
    case, xt, yt, out = _check_pairwise(name, normalized)
    calls = _same_bits(case, xt, yt, out, normalized)
    print(f"CSF64 same-bits {name} normalized={int(normalized)}: {calls} matrices / blocks equal the 64 x 64 kernel's bits")


def test_pairwise_wrapper_passes_the_misaligned_pointers(monkeypatch):
    from gaussreg_amd import _lib, ops
    case = C.PD_BY_NAME["big_scalar_192x5x7x16_gauss_off4"]
    x, y, _, _ = C.pairwise_reference(case.name, False)
    xt, yt = _inputs(case, x, y)
    seen = []
    inner = _lib.call

    def spy(dev, name, *args, **kw):
        seen.append((name, args[0].data_ptr(), args[1].data_ptr()))
        return inner(dev, name, *args, **kw)
    monkeypatch.setattr(ops._lib, "call", spy)
    ops.pairwise_distance(xt, yt)
    assert seen == [("gr_pairwise_distance_batch", xt.data_ptr(), yt.data_ptr())] and seen[0][1] % 16 == 4 and seen[0][2] % 16 == 4


@pytest.mark.parametrize("name", C.PD_NAN_CASES)
@pytest.mark.parametrize("normalized", [False, True])
def test_pairwise_nan_rows_stay_nan(name, normalized):
    """One NaN in the last channel of one row of x and of one row of y (of another matrix, where there is one): the
    reference's clamp(min=0) keeps NaN, so the output is NaN on exactly that row and that column -- not 0, the best
    possible match -- and within the bound everywhere else."""
    case = C.PD_BY_NAME[name]
    x, y, _, _ = C.pairwise_reference(name, normalized)
    x, y = x.copy(), y.copy()
    bx, by = 0, case.B - 1
    i, j = case.n // 2, case.m - 1
    x[bx, i, -1], y[by, j, -1] = np.nan, np.nan
    want = F.pairwise_distance(x, y, normalized)
    nan = np.zeros(want.shape, bool)
    nan[bx, i, :], nan[by, :, j] = True, True
    assert np.array_equal(np.isnan(want), nan)
    got = _distance(case, *_inputs(case, x, y), normalized).cpu().numpy()
    assert np.array_equal(np.isnan(got), nan), f"{int(np.isnan(got).sum())} NaN entries, {int(nan.sum())} expected"
    scale = F.pairwise_scale(np.nan_to_num(x), np.nan_to_num(y), normalized)
    assert C.pairwise_ratio(got[~nan], want[~nan], scale[~nan]) <= 1.0


@pytest.mark.parametrize("name", ["small_1x65x63x33_gauss", "big_aligned_192x5x7x16_gauss", "big_scalar_192x5x7x17_gauss",
                                  "big_vec_192x5x7x20_gauss"])
def test_pairwise_c_entry_with_exactly_the_header_workspace(name):
    """gr_pairwise_distance_batch with a workspace of exactly gr_pairwise_distance_batch_workspace_bytes: accepted, same
    bits as the wrapper (whose shared workspace is larger); one byte less is GR_ERR_WORKSPACE when un-normalised; the
    normalised form takes a null workspace."""
    from gaussreg_amd import _lib
    L = _lib.lib()
    case = C.PD_BY_NAME[name]
    x, y, _, _ = C.pairwise_reference(name, False)
    xt, yt = _inputs(case, x, y)
    B, n, m, c = case.B, case.n, case.m, case.C
    nbytes = L.gr_pairwise_distance_batch_workspace_bytes(B, n, m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((B, n, m), float("nan"), device="cuda")

    def entry(normalized, ws_ptr, nb):
        return L.gr_pairwise_distance_batch(_lib.ptr(xt), _lib.ptr(yt), B, n, m, c, normalized, _lib.ptr(out), ws_ptr, nb,
                                            _lib.stream_ptr(xt.device))
    _lib.check(entry(0, _lib.ptr(ws), nbytes))
    assert torch.equal(out, _distance(case, xt, yt, False))
    assert entry(0, _lib.ptr(ws), nbytes - 1) == GR_ERR_WORKSPACE
    assert entry(0, _lib.ptr(None), 0) == GR_ERR_WORKSPACE
    out.fill_(float("nan"))
    _lib.check(entry(1, _lib.ptr(None), 0))
    assert torch.equal(out, _distance(case, xt, yt, True))


def test_pairwise_empty_shapes():
    from gaussreg_amd.ops import pairwise_distance
    for B, n, m in ((1, 0, 5), (1, 5, 0), (0, 5, 7), (3, 0, 0), (200, 0, 7)):
        for normalized in (False, True):
            out = pairwise_distance(torch.zeros(B, n, 8, device="cuda"), torch.zeros(B, m, 8, device="cuda"), normalized)
            assert tuple(out.shape) == (B, n, m) and out.dtype == torch.float32
    out = pairwise_distance(torch.zeros(0, 8, device="cuda"), torch.zeros(4, 8, device="cuda"))
    assert tuple(out.shape) == (0, 4)


# ================================================================================================== point to node
def _partition(pts, nodes, K):
    from gaussreg_amd.ops import point_to_node_partition
    out = point_to_node_partition(_c(pts), _c(nodes), K)
    assert [t.dtype for t in out] == [torch.int64, torch.bool, torch.int64, torch.bool]
    return [t.cpu().numpy() for t in out]


def _check_partition(name, K):
    unclear, loose = C.p2n_admitted(name, K)                # the float32 oracle, on the CPU, before the kernel is called
    pts, nodes = C.cloud(C.P2N_CASES[name][0])
    got = _partition(pts, nodes, K)
    g_unclear, g_loose = C.p2n_check(name, K, got)
    print(f"\nCSF64 p2n {name} K={K}: N={pts.shape[0]} M={nodes.shape[0]}, {g_unclear} unclear points, {g_loose} rows compared "
          f"as sets (oracle: {unclear}, {loose})")
    return got, C.p2n_reference(name)


@pytest.mark.parametrize("K", C.P2N_CASES["planted"][1])
def test_point_to_node_planted_cloud(K):
    """2049 nodes: assign_kernel stages them in three LDS rounds and the owners of most points sit in the second and
    third (node indices 1023, 1024, 1025, 2048).  Node sizes 63 / 64 / 65 (one wave | LDS sort), 127 / 128 / 129 (K), 2047
    / 2048 / 2049 (one sort | a second round), 3968 / 3969 (two rounds | a third), 1 and 0; K = 1024 is the limit, where a
    round appends as many keys as it keeps.  Nothing is unclear: every owner, mask, index and knn mask is compared."""
    got, ref = _check_partition("planted", K)
    idx, mask = F.knn_tables(ref, K)
    assert np.array_equal(got[0], ref["owner"]) and np.array_equal(got[1], ref["node_masks"])
    assert np.array_equal(got[2], idx) and np.array_equal(got[3], mask)
    sizes = np.array([len(m) for m in ref["members"]])
    assert sorted(sizes[[1023, 1024, 2048, 0, 1025]].tolist()) == [2047, 2048, 2049, 3968, 3969]
    assert (ref["owner"] >= 1024).mean() > 0.5 and (ref["owner"] >= 2048).sum() >= 2049
    assert {63, 64, 65, 127, 128, 129, 1, 0} <= set(sizes.tolist())


@pytest.mark.parametrize("K", C.P2N_CASES["ties"][1])
def test_point_to_node_exact_ties(K):
    """Points repeated inside a one-wave node (40 members), an LDS-sort node (70) and a multi-round node (2100): equal
    distances, listed in ascending index.  Nodes 40, 41, 42 repeat nodes 17, 3, 17: the first minimum wins, so they own
    nothing -- mask False, a row of padding."""
    got, ref = _check_partition("ties", K)
    idx, mask = F.knn_tables(ref, K)
    assert np.array_equal(got[0], ref["owner"]) and np.array_equal(got[1], ref["node_masks"])
    assert np.array_equal(got[2], idx) and np.array_equal(got[3], mask)
    N = ref["N"]
    for m in (40, 41, 42, 43):
        assert not got[1][m] and (got[2][m] == N).all() and not got[3][m].any()
    assert got[1][17] and got[1][3]
    tied = 0
    for m in (17, 3, 30):
        d, mem = ref["member_d"][m], ref["members"][m]
        eq = np.nonzero(np.diff(d) == 0)[0]
        assert len(eq) >= 5 and (mem[eq] < mem[eq + 1]).all()
        tied += int((eq < K - 1).sum())
    if K > 1:
        assert tied > 0  # some of them inside the rows compared above


def test_point_to_node_room_up_to_ties():
    """1500 nodes sampled from 6000 random points: owners are not obvious, so the expanded-form arithmetic decides them."""
    _check_partition("room", 64)


def test_point_to_node_two_lds_rounds_small():
    _check_partition("n1030", 128)
    _check_partition("small3", 128)


def test_point_to_node_stack_mode_equals_single_calls():
    """The planted cloud, 130 points / 3 nodes, points without nodes, an empty cloud and 1030 nodes in one call: every
    cloud's slice equals its own call bit for bit; the padding is that cloud's own point count."""
    from gaussreg_amd.ops import point_to_node_partition_batch
    clouds = [C.cloud(n) for n in C.STACK]
    n_pts, n_nodes = [p.shape[0] for p, _ in clouds], [nd.shape[0] for _, nd in clouds]
    got = point_to_node_partition_batch(_c(np.concatenate([p for p, _ in clouds])), n_pts,
                                        _c(np.concatenate([nd for _, nd in clouds])), n_nodes, C.STACK_K)
    got = [t.cpu().numpy() for t in got]
    po, no = np.concatenate([[0], np.cumsum(n_pts)]), np.concatenate([[0], np.cumsum(n_nodes)])
    assert got[0].shape == (po[-1],) and got[2].shape == (no[-1], C.STACK_K)
    for c, (pts, nodes) in enumerate(clouds):
        if nodes.shape[0] == 0:
            continue                                        # (no node: nothing is returned for its points)
        want = _partition(pts, nodes, C.STACK_K)
        assert np.array_equal(got[0][po[c]:po[c + 1]], want[0]), f"cloud {c}: point_to_node"
        for k in (1, 2, 3):
            assert np.array_equal(got[k][no[c]:no[c + 1]], want[k]), f"cloud {c}: output {k}"
        pad = got[2][no[c]:no[c + 1]][~got[3][no[c]:no[c + 1]]]
        assert (pad == pts.shape[0]).all() and (got[2][no[c]:no[c + 1]][got[3][no[c]:no[c + 1]]] < pts.shape[0]).all()


def test_point_to_node_refusals_and_no_nodes():
    from gaussreg_amd.ops import point_to_node_partition
    pts, nodes = (_c(a) for a in C.cloud("small3"))
    with pytest.raises(RuntimeError, match=r"point_limit must be in \[1, 1024\]"):
        point_to_node_partition(_c(C.cloud("planted")[0]), nodes, 1025)
    with pytest.raises(RuntimeError, match="need at least point_limit points"):
        point_to_node_partition(pts, nodes, 131)
    out = point_to_node_partition(pts, torch.zeros(0, 3, device="cuda"), 16)
    assert tuple(out[1].shape) == (0,) and tuple(out[2].shape) == (0, 16) and tuple(out[3].shape) == (0, 16)


@pytest.mark.parametrize("K", [16, 128])
def test_point_to_node_nan_point(K):
    """A point with a NaN coordinate has no finite distance: it is assigned to node 0 (torch.min returns index 0 for
    a NaN column), sets that node's mask and is never listed -- with K = 128 node 0 has room left, and it stays padding --
    while every other point is where it was.  (fmaxf turned its distances into 0: it used to come FIRST in node 0.)"""
    pts, nodes = C.cloud("small3")
    base = F.partition(pts, nodes)
    i = int(base["members"][1][3])                          # a member of node 1, fourth of its row
    assert base["owner"][i] == 1
    pts = pts.copy()
    pts[i, 1] = np.nan
    ref = F.partition(pts, nodes)
    assert ref["owner"][i] == 0 and i not in ref["members"][0] and len(ref["members"][1]) == len(base["members"][1]) - 1
    got = _partition(pts, nodes, K)
    F.compare_partition(got, pts, nodes, ref, K, C.PD_BOUND)
    idx, mask = F.knn_tables(ref, K)
    assert got[0][i] == 0 and np.array_equal(got[0], ref["owner"])
    assert np.array_equal(got[2], idx) and np.array_equal(got[3], mask) and not (got[2] == i).any()
    # the only member of a node: the node's mask is set, its row is padding
    far = np.concatenate([np.full((1, 3), 50.0, np.float32), nodes])
    lone = _partition(pts, far, K)
    assert lone[0][i] == 0 and (lone[0] > 0).sum() == len(pts) - 1
    assert lone[1][0] and (lone[2][0] == len(pts)).all() and not lone[3][0].any()
