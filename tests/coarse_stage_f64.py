"""Test helper (not collected): float64 restatements of the two dense operators between the backbone and fine matching,
for tests/test_gpu_coarse_stage_f64.py (csrc/superpoint_matching.hip: gr_pairwise_distance(_batch); csrc/point_to_node.hip:
gr_point_to_node_partition(_batch)) and the CPU file tests/test_coarse_stage_f64_reference.py, which pins them against the
goldens that the reference's own modules produced, oracle/matching_np.py and the reference's modules themselves.

  pairwise_distance        geotransformer/modules/ops/pairwise_distance.py:4-31 in float64; clamp(min=0) keeps NaN
  pairwise_scale           s_ij of the entrywise bound: |x_i|^2 + |y_j|^2, or 2 + 2 |x_i| |y_j| when `normalized`
  pairwise_fp32_torch      the reference's own expression on float32 torch tensors            } admission only
  pairwise_fp32_chain      float32 with the dot product as an ascending-k chain (the kernels)  }
  partition                geotransformer/modules/ops/pointcloud_partition.py:61-111 in float64, without the (M, N) matrix
  compare_partition        a partition result against `partition`, exact wherever the float64 geometry is clear

Rules the reference leaves open and the kernels promise (include/gaussreg_hip.h): the owner of a point is the FIRST node
at the minimum distance, so a node repeated at a higher index owns nothing; a node's members are listed by ascending
(distance, point index), so members at equal distance appear in ascending index; a point without a finite distance (a
NaN coordinate) is assigned to node 0, as torch.min does, sets that node's mask and is never listed."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ pairwise distance
def _clamp0(d):
    return np.where(d < 0, 0.0, d)  # torch.clamp(min=0): NaN stays NaN


def pairwise_distance(x, y, normalized=False):
    """(*, N, C) x (*, M, C) -> (*, N, M) float64.  pairwise_distance.py:23-31."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore"):
        xy = np.matmul(x, np.swapaxes(y, -1, -2))
        if normalized:
            return _clamp0(2.0 - 2.0 * xy)
        x2 = (x * x).sum(-1)[..., :, None]
        y2 = (y * y).sum(-1)[..., None, :]
        return _clamp0(x2 - 2.0 * xy + y2)


def pairwise_scale(x, y, normalized=False):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x2, y2 = (x * x).sum(-1)[..., :, None], (y * y).sum(-1)[..., None, :]
    return 2.0 + 2.0 * np.sqrt(x2) * np.sqrt(y2) if normalized else x2 + y2


def pairwise_fp32_torch(x, y, normalized=False):
    """The lines of pairwise_distance.py:23-30 on float32 CPU tensors."""
    x, y = torch.from_numpy(np.array(x, np.float32)), torch.from_numpy(np.array(y, np.float32))  # (copies: the inputs may be read-only)
    xy = torch.matmul(x, y.transpose(-1, -2))
    if normalized:
        d = 2.0 - 2.0 * xy
    else:
        d = torch.sum(x ** 2, dim=-1).unsqueeze(-1) - 2 * xy + torch.sum(y ** 2, dim=-1).unsqueeze(-2)
    return d.clamp(min=0.0).numpy()


def pairwise_fp32_chain(x, y, normalized=False):
    """float32, every sum an ascending-k chain acc = float32(float64(acc) + float64(a) * float64(b)) -- one rounding per
    term, the order of the kernels' MFMA chain -- then (x2 - 2 xy) + y2 in float32."""
    f32, f64 = np.float32, np.float64
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    C = x.shape[-1]

    def chain(a, b):
        acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), f32)
        for k in range(C):
            acc = (acc.astype(f64) + a[..., k].astype(f64) * b[..., k].astype(f64)).astype(f32)
        return acc
    xy = chain(x[..., :, None, :], y[..., None, :, :])
    if normalized:
        d = f32(2.0) - f32(2.0) * xy
    else:
        d = (chain(x, x)[..., :, None] - f32(2.0) * xy) + chain(y, y)[..., None, :]
    return np.where(d < 0, f32(0.0), d).astype(f32)


# ------------------------------------------------------------------------------------------------ point to node
def partition(points, nodes, chunk=2048):
    """-> dict: owner (N,) the argmin over the nodes, first minimum; owner_d (N,) its squared distance; second (N,) the
    nearest node other than the owner and gap (N,) its distance minus owner_d (inf with one node); node_masks (M,);
    members: per node its listed members by ascending (distance, index), with their distances in member_d.  The distance
    is the reference's expanded form in float64."""
    p, nd = np.asarray(points, np.float64), np.asarray(nodes, np.float64)
    N, M = p.shape[0], nd.shape[0]
    owner, owner_d = np.zeros(N, np.int64), np.full(N, np.nan)
    second, gap = np.zeros(N, np.int64), np.full(N, np.inf)
    for a in range(0, N, chunk):
        d = pairwise_distance(nd, p[a:a + chunk])                    # (M, n)
        cols = np.arange(d.shape[1])
        o = d.argmin(0)                                              # first minimum; a NaN column gives 0, like torch.min
        owner[a:a + chunk], owner_d[a:a + chunk] = o, d[o, cols]
        if M > 1:
            d[o, cols] = np.inf
            s = d.argmin(0)
            second[a:a + chunk] = s
            with np.errstate(invalid="ignore"):
                gap[a:a + chunk] = d[s, cols] - owner_d[a:a + chunk]
    node_masks = np.zeros(M, bool)
    node_masks[owner] = True
    listed = np.nonzero(np.isfinite(owner_d))[0]
    order = listed[np.lexsort((listed, owner_d[listed], owner[listed]))]
    starts = np.searchsorted(owner[order], np.arange(M + 1))
    members = [order[starts[m]:starts[m + 1]] for m in range(M)]
    return dict(N=N, M=M, owner=owner, owner_d=owner_d, second=second, gap=gap, node_masks=node_masks, members=members,
                member_d=[owner_d[mem] for mem in members])


def knn_tables(ref, K):
    """node_knn_indices (M, K) padded with N, node_knn_masks (M, K).  pointcloud_partition.py:97-102."""
    idx = np.full((ref["M"], K), ref["N"], np.int64)
    mask = np.zeros((ref["M"], K), bool)
    for m, mem in enumerate(ref["members"]):
        c = min(K, len(mem))
        idx[m, :c], mask[m, :c] = mem[:c], True
    return idx, mask


def clarity(points, nodes, ref, B):
    """Which decisions the float64 geometry leaves open at an entrywise error of B * (|node|^2 + |p|^2) per distance.
    -> (unclear_points (N,) bool, per node a bool array over its consecutive member pairs).  Two distances may each be off by
    the bound, so a gap is clear above 2 B s with s the larger of the two scales.  Bit-equal operands (a repeated node, a
    repeated point) give bit-equal distances in any arithmetic: such a tie is decided by the index and is clear."""
    p, nd = np.asarray(points, np.float64), np.asarray(nodes, np.float64)
    p2, n2 = (p * p).sum(1), (nd * nd).sum(1)
    o, s = ref["owner"], ref["second"]
    thr = 2.0 * B * (np.maximum(n2[o], n2[s]) + p2)
    with np.errstate(invalid="ignore"):
        unclear = np.isfinite(ref["gap"]) & (ref["gap"] <= thr)
    unclear &= ~((nodes[o] == nodes[s]).all(1))
    pairs = []
    for m, (mem, d) in enumerate(zip(ref["members"], ref["member_d"])):
        if len(mem) < 2:
            pairs.append(np.zeros(0, bool))
            continue
        t = 2.0 * B * (n2[m] + np.maximum(p2[mem[:-1]], p2[mem[1:]]))
        same = (points[mem[:-1]] == points[mem[1:]]).all(1)
        pairs.append((np.diff(d) <= t) & ~same)
    return unclear, pairs


def compare_partition(got, points, nodes, ref, K, B):
    """got = (point_to_node, node_masks, node_knn_indices, node_knn_masks) as NumPy.  Asserts:
      * a clear point has the reference's owner; an unclear one a node within its threshold of the nearest;
      * masks and rows are consistent with got's own owners (a row lists min(K, count) members of its node, the rest N / False);
      * a node none of whose candidate points is unclear has the reference's mask and row, position by position, except
        that a run of members whose consecutive gaps are unclear is compared as a set (cut at K: a subset of the run).
    -> (number of unclear points, number of rows not compared position by position)."""
    p2n, masks, idx, kmask = got
    N, M = ref["N"], ref["M"]
    assert p2n.shape == (N,) and masks.shape == (M,) and idx.shape == (M, K) and kmask.shape == (M, K)
    unclear, pairs = clarity(points, nodes, ref, B)
    clear = ~unclear
    assert np.array_equal(p2n[clear], ref["owner"][clear]), "owner of a clear point"
    p, nd = np.asarray(points, np.float64), np.asarray(nodes, np.float64)
    touched = np.zeros(M, bool)
    for i in np.nonzero(unclear)[0]:
        d = pairwise_distance(nd, p[i:i + 1])[:, 0]
        n2 = (nd * nd).sum(1)
        near = d - ref["owner_d"][i] <= 2.0 * B * (np.maximum(n2, n2[ref["owner"][i]]) + (p[i] * p[i]).sum())
        assert near[p2n[i]], f"point {i}: owner {p2n[i]} is not among its nearest nodes"
        touched |= near
    counts = np.bincount(p2n, minlength=M)
    assert np.array_equal(masks, counts > 0), "node_masks against the returned owners"
    finite = np.isfinite(ref["owner_d"])
    listed = np.bincount(p2n[finite], minlength=M)
    assert np.array_equal(kmask, np.arange(K)[None, :] < np.minimum(listed, K)[:, None]), "knn masks are a prefix of min(K, count)"
    assert np.array_equal(idx[~kmask], np.full((~kmask).sum(), N)), "padding value"
    assert np.array_equal(p2n[idx[kmask]], np.nonzero(kmask)[0]), "a row lists members of its own node"
    loose = 0
    for m in range(M):
        if touched[m]:
            row = idx[m][kmask[m]]
            assert len(set(row.tolist())) == len(row)
            loose += 1
            continue
        mem, un = ref["members"][m], pairs[m]
        assert masks[m] == ref["node_masks"][m]
        c = min(K, len(mem))
        if not un[:max(c - 1, 0)].any() and not (c == K and len(mem) > K and un[K - 1]):
            assert np.array_equal(idx[m, :c], mem[:c]), f"node {m}: row differs from the float64 order"
            continue
        loose += 1
        edges = np.concatenate([[0], np.nonzero(~un)[0] + 1, [len(mem)]])   # runs of members tied within the threshold
        for s, e in zip(edges[:-1], edges[1:]):
            if s >= c:
                break
            if e <= c:
                assert set(idx[m, s:e].tolist()) == set(mem[s:e].tolist()), f"node {m}: positions {s}..{e}"
            else:
                part = idx[m, s:c].tolist()
                assert len(set(part)) == len(part) and set(part) <= set(mem[s:e].tolist()), f"node {m}: positions {s}..{c}"
    return int(unclear.sum()), loose
