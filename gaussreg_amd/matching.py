"""Mirror of the reference's matching nn.Modules, bodies replaced by fused HIP kernels.

    SuperPointMatching   geotransformer/modules/geotransformer/superpoint_matching.py:7-50
    PointMatching        geotransformer/modules/geotransformer/point_matching.py:5-115
                         (compute_correspondence_matrix is also what LocalGlobalRegistration uses,
                          local_global_registration.py:49-83)

    SuperPointTargetGenerator   geotransformer/modules/geotransformer/superpoint_target.py:6-46
    get_node_correspondences    geotransformer/modules/registration/matching.py:231-315 (training: the ground-truth
                                superpoint correspondences, one fused HIP call -- csrc/node_correspondences.hip)

Same constructor arguments, same forward signatures and return tuples; no parameters or buffers
(no state-dict keys), like the reference.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib


_F32 = dict(dtype=torch.float32, cast=False)  # _lib.to_device: these modules insist on float tensors, they do not cast


class SuperPointMatching(nn.Module):
    def __init__(self, num_correspondences, dual_normalization=True):
        super().__init__()
        self.num_correspondences = num_correspondences
        self.dual_normalization = dual_normalization

    @torch.no_grad()
    def forward(self, ref_feats, src_feats, ref_masks=None, src_masks=None):
        """-> (ref_corr_indices (k,) i64, src_corr_indices (k,) i64, corr_scores (k,) f32 descending)."""
        dev = _lib.require_gpu()
        out_device = ref_feats.device
        rf = _lib.to_device(ref_feats, dev, **_F32)
        dev = rf.device
        sf = _lib.to_device(src_feats, dev, **_F32)
        rm = None if ref_masks is None else _lib.to_device_bool(ref_masks, dev)
        sm = None if src_masks is None else _lib.to_device_bool(src_masks, dev)
        nr, c = rf.shape
        ns = sf.shape[0]
        k = int(self.num_correspondences)
        ri = torch.empty((k,), dtype=torch.int64, device=dev)
        si = torch.empty((k,), dtype=torch.int64, device=dev)
        sc = torch.empty((k,), dtype=torch.float32, device=dev)
        n_out = ctypes.c_int64(0)
        _lib.call(dev, "gr_superpoint_matching", rf, sf, nr, ns, c, rm, sm, k, int(bool(self.dual_normalization)), ri, si, sc,
                  ctypes.byref(n_out), ws=_lib.lib().gr_superpoint_matching_workspace_bytes(nr, ns))
        n = n_out.value
        return _lib.like_input((ri[:n], si[:n], sc[:n]), out_device)

    @torch.no_grad()
    def forward_batch(self, feats, node_lengths, masks=None):
        """The same for a batch of scene pairs in one call (gr_superpoint_matching_batch): `feats` (sum M, C) stacks the
        L2-normalised superpoint features as [ref_0, src_0, ref_1, src_1, ...], `node_lengths` their 2 B sizes, `masks`
        (sum M,) likewise.  -> (ref_corr_indices (B, k), src_corr_indices (B, k), corr_scores (B, k), counts: list of B ints
        -- row b is valid up to counts[b]).  One host read-back for the whole batch."""
        dev = _lib.require_gpu()
        f = _lib.to_device(feats, dev, **_F32)
        dev = f.device
        m = None if masks is None else _lib.to_device_bool(masks, dev)
        off = _lib.offsets(node_lengths)
        if len(off) % 2 != 1 or off[-1] != f.shape[0]:
            raise ValueError("node_lengths must list ref and src sizes of every pair and sum to feats.shape[0]")
        B = (len(off) - 1) // 2
        k = int(self.num_correspondences)
        ri = torch.zeros((B, k), dtype=torch.int64, device=dev)
        si = torch.zeros((B, k), dtype=torch.int64, device=dev)
        sc = torch.zeros((B, k), dtype=torch.float32, device=dev)
        h_off = _lib.host_i64(off)
        h_n = _lib.host_i64([0] * B)
        _lib.call(dev, "gr_superpoint_matching_batch", f, h_off, B, f.shape[1], m, k, int(bool(self.dual_normalization)),
                  ri, si, sc, h_n, ws=_lib.lib().gr_superpoint_matching_batch_workspace_bytes(h_off, B))
        return ri, si, sc, [int(h_n[b]) for b in range(B)]


class PointMatching(nn.Module):
    def __init__(self, k: int, mutual: bool = True, confidence_threshold: float = 0.05, use_dustbin: bool = False,
                 use_global_score: bool = False, remove_duplicate: bool = False):
        super().__init__()
        self.k = k
        self.mutual = mutual
        self.confidence_threshold = confidence_threshold
        self.use_dustbin = use_dustbin
        self.use_global_score = use_global_score
        self.remove_duplicate = remove_duplicate
        if use_dustbin:
            # the reference's dustbin branch slices corr_mat[:, -1:, -1] (point_matching.py:61-62), which
            # yields a (B, 1) tensor and cannot be combined with the (B, K, K) mask on the next line;
            # GaussReg never enables it (model.py:51-65 uses LocalGlobalRegistration with use_dustbin False)
            raise NotImplementedError("use_dustbin=True is not supported (unusable in the reference as well)")

    def _corr(self, score_mat, ref_knn_masks, src_knn_masks, want_count, scores_are_exp=False):
        dev = _lib.require_gpu()
        s = _lib.to_device(score_mat, dev, **_F32)
        dev = s.device
        rm, sm = _lib.to_device_bool(ref_knn_masks, dev), _lib.to_device_bool(src_knn_masks, dev)
        B, K1, K2 = s.shape
        corr = torch.empty((B, K1, K2), dtype=torch.bool, device=dev)
        n = ctypes.c_int64(0)
        # the workspace keeps the per-patch counts: gr_corr_gather and gr_lgr_register_* read them, so it goes back to the caller
        ws = _lib.workspace(dev, _lib.lib().gr_point_matching_workspace_bytes(B))
        _lib.call(dev, "gr_corr_matrix_exp" if scores_are_exp else "gr_corr_matrix", s, B, K1, K2, rm, sm, int(self.k),
                  int(bool(self.mutual)), float(self.confidence_threshold), corr, ctypes.byref(n) if want_count else None,
                  ws=ws)
        return s, corr, n.value, ws

    @torch.no_grad()
    def compute_correspondence_matrix(self, score_mat, ref_knn_masks, src_knn_masks):
        """`score_mat` here is exp(log-scores), as in the reference call sites (point_matching.py:98,
        local_global_registration.py:211): it is thresholded as given (gr_corr_matrix_exp), no log/exp round trip."""
        s, corr, _, _ = self._corr(score_mat, ref_knn_masks, src_knn_masks, False, scores_are_exp=True)
        return _lib.like_input(corr, score_mat.device)

    @torch.no_grad()
    def forward(self, ref_knn_points, src_knn_points, ref_knn_masks, src_knn_masks, ref_knn_indices, src_knn_indices,
                score_mat, global_scores):
        out_device = score_mat.device
        s, corr, n, ws = self._corr(score_mat, ref_knn_masks, src_knn_masks, True)
        dev = s.device
        B, K1, K2 = s.shape
        rp, sp = _lib.to_device(ref_knn_points, dev, **_F32), _lib.to_device(src_knn_points, dev, **_F32)
        ri = ref_knn_indices.to(dev).contiguous()
        si = src_knn_indices.to(dev).contiguous()
        gs = _lib.to_device(global_scores, dev, **_F32) if (self.use_global_score and global_scores is not None) else None
        o_rp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        o_sp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        o_ri = torch.empty((n,), dtype=torch.int64, device=dev)
        o_si = torch.empty((n,), dtype=torch.int64, device=dev)
        o_sc = torch.empty((n,), dtype=torch.float32, device=dev)
        if n > 0:
            _lib.call(dev, "gr_corr_gather", s, B, K1, K2, corr, rp, sp, ri, si, gs, int(gs is not None), o_rp, o_sp, o_ri,
                      o_si, o_sc, ws=ws)
        return _lib.like_input((o_rp, o_sp, o_ri, o_si, o_sc), out_device)


class LocalGlobalRegistration(nn.Module):
    """Mirror of geotransformer/modules/geotransformer/local_global_registration.py:11-235 (forward,
    inference).  Correspondence extraction = the PointMatching kernels; hypothesis generation, verification
    and refinement run in three more launches with no GPU->CPU SVD round trips (the reference does
    1 + num_refinement_steps of them, registration/procrustes.py:59)."""

    def __init__(self, k: int, acceptance_radius: float, mutual: bool = True, confidence_threshold: float = 0.05,
                 use_dustbin: bool = False, use_global_score: bool = False, correspondence_threshold: int = 3,
                 correspondence_limit=None, num_refinement_steps: int = 5):
        super().__init__()
        self.k = k
        self.acceptance_radius = acceptance_radius
        self.mutual = mutual
        self.confidence_threshold = confidence_threshold
        self.use_dustbin = use_dustbin
        self.use_global_score = use_global_score
        self.correspondence_threshold = correspondence_threshold
        self.correspondence_limit = correspondence_limit
        self.num_refinement_steps = num_refinement_steps
        if use_dustbin:
            raise NotImplementedError("use_dustbin=True is not supported (GaussReg sets it False, config.py:121)")
        self._pm = PointMatching(k, mutual, confidence_threshold, False, use_global_score)

    @torch.no_grad()
    def compute_correspondence_matrix(self, score_mat, ref_knn_masks, src_knn_masks):
        return self._pm.compute_correspondence_matrix(score_mat, ref_knn_masks, src_knn_masks)

    @torch.no_grad()
    def forward(self, ref_knn_points, src_knn_points, ref_knn_masks, src_knn_masks, score_mat, global_scores):
        """-> (ref_corr_points (C,3), src_corr_points (C,3), corr_scores (C,), estimated_transform (4,4))."""
        out_device = score_mat.device
        s, corr, n, pm_ws = self._pm._corr(score_mat, ref_knn_masks, src_knn_masks, True)
        dev = s.device
        B, K1, K2 = s.shape
        rp, sp = _lib.to_device(ref_knn_points, dev, **_F32), _lib.to_device(src_knn_points, dev, **_F32)
        gs = _lib.to_device(global_scores, dev, **_F32) if (self.use_global_score and global_scores is not None) else None
        o_rp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        o_sp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        o_sc = torch.empty((n,), dtype=torch.float32, device=dev)
        idx_dummy = torch.zeros((B, max(K1, K2)), dtype=torch.int64, device=dev)
        o_i = torch.empty((2, max(n, 1)), dtype=torch.int64, device=dev)
        transform = torch.eye(4, dtype=torch.float32, device=dev)
        if n > 0:
            _lib.call(dev, "gr_corr_gather", s, B, K1, K2, corr, rp, sp, idx_dummy, idx_dummy, gs, int(gs is not None), o_rp,
                      o_sp, o_i[0], o_i[1], o_sc, ws=pm_ws)
            # (a buffer of its own: pm_ws, the shared workspace, is an input of the registration)
            ws2 = torch.empty(_lib.lib().gr_lgr_workspace_bytes(B) + 256, dtype=torch.uint8, device=dev)
            v_rp, v_sp, v_sc = o_rp, o_sp, o_sc
            if self.correspondence_limit is not None and n > int(self.correspondence_limit):
                # verification set = top-`limit` global scores (local_global_registration.py:145-148)
                v_sc, sel = o_sc.topk(k=int(self.correspondence_limit), largest=True)
                v_rp, v_sp, v_sc = o_rp[sel].contiguous(), o_sp[sel].contiguous(), v_sc.contiguous()
            _lib.call(dev, "gr_lgr_register_verify", o_rp, o_sp, o_sc, n, B, pm_ws, v_rp, v_sp, v_sc, v_sc.shape[0],
                      float(self.acceptance_radius), int(self.correspondence_threshold), int(self.num_refinement_steps),
                      transform, ws=ws2)
        return _lib.like_input((o_rp, o_sp, o_sc, transform), out_device)

    @torch.no_grad()
    def forward_batch(self, ref_knn_points, src_knn_points, ref_knn_masks, src_knn_masks, score_mat, global_scores,
                      patches_per_pair):
        """forward for a batch of scene pairs in one pass: the P patches of all pairs are stacked along dim 0, pair b owning
        the next patches_per_pair[b] of them.  -> (ref_corr_points (C,3), src_corr_points (C,3), corr_scores (C,),
        estimated_transforms (B,4,4), row_offsets (B+1,) int32 on the device: pair b's correspondences are rows
        [row_offsets[b], row_offsets[b+1]) -- the single-pair outputs concatenated).  ONE host read-back (C, which sizes the
        outputs) for the whole batch; correspondence_limit is not supported here (the GaussReg config leaves it None)."""
        if self.correspondence_limit is not None:
            raise NotImplementedError("forward_batch: correspondence_limit must be None")
        s, corr, n, pm_ws = self._pm._corr(score_mat, ref_knn_masks, src_knn_masks, True)
        dev = s.device
        P, K1, K2 = s.shape
        poff = _lib.offsets(patches_per_pair)
        if poff[-1] != P:
            raise ValueError("patches_per_pair must sum to the number of patches")
        B = len(poff) - 1
        rp, sp = _lib.to_device(ref_knn_points, dev, **_F32), _lib.to_device(src_knn_points, dev, **_F32)
        gs = _lib.to_device(global_scores, dev, **_F32) if (self.use_global_score and global_scores is not None) else None
        o_rp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        o_sp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        o_sc = torch.empty((n,), dtype=torch.float32, device=dev)
        transforms = torch.eye(4, dtype=torch.float32, device=dev).repeat(B, 1, 1)
        rows = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
        if P > 0 and B > 0:
            idx_dummy = torch.zeros((P, max(K1, K2)), dtype=torch.int64, device=dev)
            o_i = torch.empty((2, max(n, 1)), dtype=torch.int64, device=dev)
            d_poff = torch.tensor(poff, dtype=torch.int32).to(dev, non_blocking=False)
            if n > 0:
                _lib.call(dev, "gr_corr_gather", s, P, K1, K2, corr, rp, sp, idx_dummy, idx_dummy, gs, int(gs is not None),
                          o_rp, o_sp, o_i[0], o_i[1], o_sc, ws=pm_ws)
            ws2 = torch.empty(_lib.lib().gr_lgr_workspace_bytes(P) + 256, dtype=torch.uint8, device=dev)
            _lib.call(dev, "gr_lgr_register_seg", o_rp, o_sp, o_sc, n, P, pm_ws, d_poff, B, float(self.acceptance_radius),
                      int(self.correspondence_threshold), int(self.num_refinement_steps), transforms, rows, ws=ws2)
        return o_rp, o_sp, o_sc, transforms, rows


@torch.no_grad()
def get_node_correspondences(ref_nodes, src_nodes, ref_knn_points, src_knn_points, transform, pos_radius, ref_masks=None,
                             src_masks=None, ref_knn_masks=None, src_knn_masks=None, return_dense=False):
    """registration/matching.py:231-315 -> (corr_indices (C, 2) int64, corr_overlaps (C,) float32): the pairs of patches
    that share at least one point pair closer than `pos_radius` under `transform`, in row-major (ref, src) order, with
    overlap = (matched ref points / valid ref points + matched src points / valid src points) / 2.
    One call of gr_node_correspondences: no (B, K, K) tensor, the transform stays on the device, one host read-back (C).
    The distance is evaluated as differences, then squares (the reference expands x^2 - 2xy + y^2, whose fp32 error at room
    scale is a visible fraction of pos_radius^2); the threshold is the reference's: float(pos_radius) ** 2 rounded once to
    float32, which is what torch.lt(fp32 tensor, python scalar) compares against.
    `return_dense=True` (extension) also returns the dense (M, N) overlap matrix (0 where a pair does not overlap): what
    CoarseMatchingLoss scatters the list into."""
    dev = _lib.require_gpu()
    out_device = ref_nodes.device
    rn = _lib.to_device(ref_nodes, dev, **_F32)
    dev = rn.device
    sn = _lib.to_device(src_nodes, dev, **_F32)
    rp, sp = _lib.to_device(ref_knn_points, dev, **_F32), _lib.to_device(src_knn_points, dev, **_F32)
    T = _lib.to_device(transform, dev, torch.float32)
    M, N = rn.shape[0], sn.shape[0]
    K = rp.shape[1]
    if tuple(rp.shape) != (M, K, 3) or tuple(sp.shape) != (N, K, 3) or tuple(T.shape) != (4, 4):
        raise ValueError("get_node_correspondences: expected knn points of shape (M, K, 3) / (N, K, 3) and a (4, 4) transform")
    masks = [None if m is None else _lib.to_device_bool(m, dev) for m in (ref_masks, src_masks, ref_knn_masks, src_knn_masks)]
    for m, shape in zip(masks, ((M,), (N,), (M, K), (N, K))):
        if m is not None and tuple(m.shape) != shape:
            raise ValueError("get_node_correspondences: a mask of shape %s was expected, got %s" % (shape, tuple(m.shape)))
    cap = M * N
    idx = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    ov = torch.empty((cap,), dtype=torch.float32, device=dev)
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    dense = torch.empty((M, N), dtype=torch.float32, device=dev) if return_dense else None
    r2 = ctypes.c_float(float(pos_radius) ** 2).value
    _lib.call(dev, "gr_node_correspondences", rn, sn, rp, sp, M, N, K, T, r2, *masks, idx, ov, cap, count, dense,
              ws=_lib.lib().gr_node_correspondences_workspace_bytes(M, N, K))
    c = int(count.item())
    res = (idx[:c].clone(), ov[:c].clone())       # (clones: the views would keep the M * N buffers alive)
    if return_dense:
        res += (dense,)
    return _lib.like_input(res, out_device)


class SuperPointTargetGenerator(nn.Module):
    """superpoint_target.py:6-46: at most `num_targets` of the ground-truth correspondences whose overlap exceeds
    `overlap_threshold`, drawn without replacement; when none exceeds it, the ones of the largest overlap.  No parameters.
    The reference draws from numpy's global RNG; `generator=` (a numpy Generator or RandomState, or an int seed) makes the
    draw reproducible -- None keeps the reference's source.  An empty correspondence set raises ValueError (the
    reference fails inside `.max()` of an empty tensor there)."""

    def __init__(self, num_targets, overlap_threshold, generator=None):
        super().__init__()
        self.num_targets = num_targets
        self.overlap_threshold = overlap_threshold
        import numpy as np
        self.generator = np.random.default_rng(generator) if isinstance(generator, int) else generator

    @torch.no_grad()
    def forward(self, gt_corr_indices, gt_corr_overlaps):
        """(N, 2) int64, (N,) -> (ref indices, src indices, overlaps) of the selected correspondences."""
        import numpy as np
        if gt_corr_indices.shape[0] == 0:
            raise ValueError("SuperPointTargetGenerator: no ground-truth superpoint correspondence (the two clouds do not "
                             "overlap under the given transform)")
        masks = torch.gt(gt_corr_overlaps, self.overlap_threshold)
        if masks.sum() == 0:
            masks = gt_corr_overlaps == gt_corr_overlaps.max()
        gt_corr_overlaps, gt_corr_indices = gt_corr_overlaps[masks], gt_corr_indices[masks]
        n = gt_corr_indices.shape[0]
        if n > self.num_targets:
            rng = np.random if self.generator is None else self.generator
            sel = torch.from_numpy(np.asarray(rng.choice(np.arange(n), self.num_targets, replace=False)))
            sel = sel.to(device=gt_corr_indices.device, dtype=torch.int64)
            gt_corr_indices, gt_corr_overlaps = gt_corr_indices[sel], gt_corr_overlaps[sel]
        return gt_corr_indices[:, 0], gt_corr_indices[:, 1], gt_corr_overlaps
