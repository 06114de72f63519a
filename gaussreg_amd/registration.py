"""Correspondence-based RANSAC with a similarity model on the GPU -- the step GaussReg delegates to Open3D
(geotransformer/utils/open3d.py:169-198, called from model.py:209-215).  PARITY UNPINNED (Open3D is not in
the reference tree, and its sampler is unseeded): behaviour is judged on registration error, see tests."""
import torch

from . import _lib


@torch.no_grad()
def registration_with_ransac_from_correspondences(src_points, ref_points, correspondences=None, distance_threshold=0.05,
                                                  ransac_n=3, num_iterations=10000, with_scaling=True, refine=True,
                                                  seed=0, return_stats=False):
    """Same positional signature as the reference wrapper (open3d.py:169-176); returns a (4,4) float32 tensor
    (the reference returns a float64 numpy array).  `correspondences` (C,2) selects rows of src / ref."""
    dev = _lib.require_gpu()
    s = _lib.to_device(torch.as_tensor(src_points, dtype=torch.float32), dev)
    r = torch.as_tensor(ref_points, dtype=torch.float32)
    dev = s.device
    r = r.to(dev).contiguous()
    if correspondences is not None:
        c = torch.as_tensor(correspondences, dtype=torch.int64, device=dev)
        s, r = s[c[:, 0]].contiguous(), r[c[:, 1]].contiguous()
    n = s.shape[0]
    out = torch.empty((4, 4), dtype=torch.float32, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.call(dev, "gr_ransac_similarity", s, r, n, int(ransac_n), int(num_iterations), int(seed), float(distance_threshold),
              int(bool(with_scaling)), int(bool(refine)), out, stats,
              ws=_lib.lib().gr_ransac_workspace_bytes(int(num_iterations)))
    return (out, stats) if return_stats else out


@torch.no_grad()
def registration_with_ransac_from_feats(src_points, ref_points, src_feats, ref_feats, distance_threshold=0.05, ransac_n=3,
                                        num_iterations=50000, mutual=False, seed=0):
    """The reference wrapper of Open3D's registration_ransac_based_on_feature_matching (open3d.py:133-166), rigid: every
    source point is paired with the reference point whose descriptor is nearest (gaussreg_amd.feature_nn, fp32 features on
    the GPU; `mutual`: only the pairs that are each other's nearest), then gr_ransac_similarity without scaling runs on
    the pairs.  Returns a (4,4) float32 tensor; fewer than ransac_n pairs raise.  PARITY UNPINNED: Open3D is not in the
    reference tree and its sampler is unseeded, and its edge-length checker (CorrespondenceCheckerBasedOnEdgeLength) is not
    reproduced -- hypotheses are judged by their inlier count alone."""
    from . import feature_nn
    src_idx, ref_idx = feature_nn.extract_corr_indices_from_feats(src_feats, ref_feats, mutual=mutual)
    if src_idx.shape[0] < int(ransac_n):
        raise ValueError(f"registration_with_ransac_from_feats: {src_idx.shape[0]} pairs, fewer than ransac_n = {ransac_n}")
    corr = torch.stack([src_idx, ref_idx], dim=1)
    return registration_with_ransac_from_correspondences(src_points, ref_points, corr, distance_threshold, ransac_n,
                                                         num_iterations, with_scaling=False, seed=seed)


@torch.no_grad()
def registration_with_ransac_batch(src_points, ref_points, row_offsets, fallback_transforms=None, distance_threshold=0.05,
                                   ransac_n=3, num_iterations=10000, with_scaling=True, refine=True, seed=0,
                                   return_stats=False):
    """registration_with_ransac_from_correspondences for a batch of scene pairs in one call (gr_ransac_similarity_seg):
    row i of src_points corresponds to row i of ref_points; pair b owns rows [row_offsets[b], row_offsets[b+1]) (int32
    tensor on the device, B + 1 entries) and uses seed + b.  A pair with fewer than ransac_n rows keeps
    fallback_transforms[b] (model.py:209-220; default identity).  Returns (B,4,4) float32 on the device, no host
    synchronisation."""
    s = src_points.contiguous()
    r = ref_points.contiguous()
    dev = s.device
    off = row_offsets.to(device=dev, dtype=torch.int32).contiguous()
    B = off.shape[0] - 1
    out = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    stats = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    fb = None if fallback_transforms is None else fallback_transforms.to(device=dev, dtype=torch.float32).contiguous()
    if B > 0:
        _lib.call(dev, "gr_ransac_similarity_seg", s, r, off, B, int(ransac_n), int(num_iterations), int(seed),
                  float(distance_threshold), int(bool(with_scaling)), int(bool(refine)), fb, out, stats,
                  ws=_lib.lib().gr_ransac_seg_workspace_bytes(int(num_iterations), B))
    return (out, stats) if return_stats else out


@torch.no_grad()
def farthest_point_sampling(points, lengths, num_samples, start_indices=None, gather=False):
    """Exact FPS in stack mode (stand-in for fpsample.bucket_fps_kdline_sampling, demo.py:46; parity unpinned).
    points (N,3); lengths / num_samples: per-cloud sizes (lists or 1-D tensors).  Returns a list of int64
    CUDA tensors with LOCAL indices, one per cloud, in sampling order (first = start index, default 0).
    `gather=True`: returns the sampled POINTS instead, a list of (k_b, 3) views of one stacked tensor (one row gather for
    the whole call instead of one indexing launch per cloud)."""
    dev = _lib.require_gpu()
    p = _lib.to_device(torch.as_tensor(points, dtype=torch.float32), dev)
    dev = p.device
    lens = [int(x) for x in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    ks = [int(x) for x in (num_samples.tolist() if hasattr(num_samples, "tolist") else num_samples)]
    st = None if start_indices is None else _lib.host_i64([int(x) for x in start_indices])
    out = torch.empty((sum(ks),), dtype=torch.int64, device=dev)
    _lib.call(dev, "gr_fps", p, _lib.host_i64(lens), _lib.host_i64(ks), st, p.shape[0], len(lens), out,
              ws=_lib.lib().gr_fps_workspace_bytes(p.shape[0], len(lens)))
    if gather:
        from .ops import index_select
        base = torch.tensor([0] + lens[:-1], dtype=torch.int64).cumsum(0).to(dev)        # first row of every cloud in the stack
        glob = out + torch.repeat_interleave(base, torch.tensor(ks, device=dev))
        return list(torch.split(index_select(p, glob, 0), ks))
    return list(torch.split(out, ks))
