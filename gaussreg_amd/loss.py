"""Training losses and metrics of the registration network, mirrors of the experiment's loss.py and of
geotransformer/modules/loss/circle_loss.py in plain torch: none has a hot path of its own.

    WeightedCircleLoss   modules/loss/circle_loss.py:44-86, 111-132
    CoarseMatchingLoss   loss.py:10-40   -- circle loss on the superpoint feature distances, weighted by the ground-truth
                                            patch overlaps of gaussreg_amd.matching.get_node_correspondences (HIP)
    FineMatchingLoss     loss.py:43-71   -- selects entries of the Sinkhorn output, whose gradient is the HIP backward of
                                            gaussreg_amd.sinkhorn (inside `gaussreg_amd.differentiable()`)
    OverallLoss          loss.py:74-92
    Evaluator            loss.py:95-162

Constructors take the reference's `cfg` (gaussreg_amd.model.make_cfg() has the sections).  The numerics are the
reference's, including its singular point: the feature distance is sqrt(clamp(2 - 2 x y^T, 0)), whose derivative at an
exactly zero distance is infinite -- a positive pair with identical features gives a NaN gradient, here as there."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def weighted_circle_loss(pos_masks, neg_masks, feat_dists, pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale,
                         pos_scales=None, neg_scales=None):
    """circle_loss.py:44-86.  The weights are detached; anchors (rows, columns) need a positive and a negative."""
    row_masks = (torch.gt(pos_masks.sum(-1), 0) & torch.gt(neg_masks.sum(-1), 0)).detach()
    col_masks = (torch.gt(pos_masks.sum(-2), 0) & torch.gt(neg_masks.sum(-2), 0)).detach()
    pos_weights = feat_dists - 1e5 * (~pos_masks).to(feat_dists.dtype)
    pos_weights = pos_weights - pos_optimal
    pos_weights = torch.maximum(torch.zeros_like(pos_weights), pos_weights)
    if pos_scales is not None:
        pos_weights = pos_weights * pos_scales
    pos_weights = pos_weights.detach()
    neg_weights = feat_dists + 1e5 * (~neg_masks).to(feat_dists.dtype)
    neg_weights = neg_optimal - neg_weights
    neg_weights = torch.maximum(torch.zeros_like(neg_weights), neg_weights)
    if neg_scales is not None:
        neg_weights = neg_weights * neg_scales
    neg_weights = neg_weights.detach()
    loss_pos_row = torch.logsumexp(log_scale * (feat_dists - pos_margin) * pos_weights, dim=-1)
    loss_pos_col = torch.logsumexp(log_scale * (feat_dists - pos_margin) * pos_weights, dim=-2)
    loss_neg_row = torch.logsumexp(log_scale * (neg_margin - feat_dists) * neg_weights, dim=-1)
    loss_neg_col = torch.logsumexp(log_scale * (neg_margin - feat_dists) * neg_weights, dim=-2)
    loss_row = F.softplus(loss_pos_row + loss_neg_row) / log_scale
    loss_col = F.softplus(loss_pos_col + loss_neg_col) / log_scale
    return (loss_row[row_masks].mean() + loss_col[col_masks].mean()) / 2


class WeightedCircleLoss(nn.Module):
    def __init__(self, pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale):
        super().__init__()
        self.pos_margin, self.neg_margin = pos_margin, neg_margin
        self.pos_optimal, self.neg_optimal = pos_optimal, neg_optimal
        self.log_scale = log_scale

    def forward(self, pos_masks, neg_masks, feat_dists, pos_scales=None, neg_scales=None):
        return weighted_circle_loss(pos_masks, neg_masks, feat_dists, self.pos_margin, self.neg_margin, self.pos_optimal,
                                    self.neg_optimal, self.log_scale, pos_scales=pos_scales, neg_scales=neg_scales)


class CoarseMatchingLoss(nn.Module):
    """loss.py:10-40.  The feature distance is torch (sqrt(clamp(2 - 2 x y^T, 0)): pairwise_distance(normalized=True)), so
    autograd carries it; its gradient at an exactly zero distance of a positive pair is NaN, as in the reference.  When
    `output_dict` has `gt_node_corr_overlap_matrix` -- the dense (M, N) matrix gr_node_correspondences writes -- it is used
    as it is instead of scattering the list into zeros (the same values)."""

    def __init__(self, cfg):
        super().__init__()
        c = cfg.coarse_loss
        self.weighted_circle_loss = WeightedCircleLoss(c.positive_margin, c.negative_margin, c.positive_optimal,
                                                       c.negative_optimal, c.log_scale)
        self.positive_overlap = c.positive_overlap

    def forward(self, output_dict):
        ref_feats, src_feats = output_dict['ref_feats_c'], output_dict['src_feats_c']
        feat_dists = torch.sqrt((2.0 - 2.0 * torch.matmul(ref_feats, src_feats.transpose(-1, -2))).clamp(min=0.0))
        overlaps = output_dict.get('gt_node_corr_overlap_matrix')
        if overlaps is None:
            idx = output_dict['gt_node_corr_indices'].to(feat_dists.device)
            overlaps = torch.zeros_like(feat_dists)
            overlaps[idx[:, 0], idx[:, 1]] = output_dict['gt_node_corr_overlaps'].to(feat_dists)
        else:
            overlaps = overlaps.to(feat_dists)
        pos_masks = torch.gt(overlaps, self.positive_overlap)
        neg_masks = torch.eq(overlaps, 0)
        pos_scales = torch.sqrt(overlaps * pos_masks.float())
        return self.weighted_circle_loss(pos_masks, neg_masks, feat_dists, pos_scales)


class FineMatchingLoss(nn.Module):
    def __init__(self, positive_radius):
        """`positive_radius`: the radius, or the reference's `cfg` (cfg.fine_loss.positive_radius is read)."""
        super().__init__()
        fine = getattr(positive_radius, 'fine_loss', None)
        self.positive_radius = positive_radius if fine is None else fine.positive_radius

    @staticmethod
    @torch.no_grad()
    def labels(ref_points, src_points, ref_masks, src_masks, transform, positive_radius):
        """(B, K1, 3), (B, K2, 3), (B, K1), (B, K2), (4, 4) -> (B, K1+1, K2+1) bool: the point pairs closer than
        `positive_radius` under the ground-truth transform, and the dustbin entry of every valid point without a partner
        (loss.py:56-67)."""
        src_points = src_points @ transform[:3, :3].T + transform[:3, 3]                     # apply_transform
        dists = ((ref_points ** 2).sum(-1).unsqueeze(2) - 2.0 * ref_points @ src_points.transpose(1, 2)
                 + (src_points ** 2).sum(-1).unsqueeze(1)).clamp(min=0.0)                    # pairwise_distance (B, K1, K2)
        gt_corr_map = (dists < positive_radius ** 2) & ref_masks.unsqueeze(2) & src_masks.unsqueeze(1)
        B, K1, K2 = gt_corr_map.shape
        labels = torch.zeros((B, K1 + 1, K2 + 1), dtype=torch.bool, device=gt_corr_map.device)
        labels[:, :-1, :-1] = gt_corr_map
        labels[:, :-1, -1] = (gt_corr_map.sum(2) == 0) & ref_masks
        labels[:, -1, :-1] = (gt_corr_map.sum(1) == 0) & src_masks
        return labels

    def forward(self, output_dict, data_dict):
        matching_scores = output_dict['matching_scores']
        dev = matching_scores.device
        labels = self.labels(output_dict['ref_node_corr_knn_points'].to(dev), output_dict['src_node_corr_knn_points'].to(dev),
                             output_dict['ref_node_corr_knn_masks'].to(dev), output_dict['src_node_corr_knn_masks'].to(dev),
                             data_dict['transform'].to(dev), self.positive_radius)
        return -matching_scores[labels].mean()


class OverallLoss(nn.Module):
    """loss.py:74-92 -> {'loss', 'c_loss', 'f_loss'}."""

    def __init__(self, cfg):
        super().__init__()
        self.coarse_loss = CoarseMatchingLoss(cfg)
        self.fine_loss = FineMatchingLoss(cfg)
        self.weight_coarse_loss = cfg.loss.weight_coarse_loss
        self.weight_fine_loss = cfg.loss.weight_fine_loss

    def forward(self, output_dict, data_dict):
        coarse_loss = self.coarse_loss(output_dict)
        fine_loss = self.fine_loss(output_dict, data_dict)
        loss = self.weight_coarse_loss * coarse_loss + self.weight_fine_loss * fine_loss
        return {'loss': loss, 'c_loss': coarse_loss, 'f_loss': fine_loss}


def _split_similarity(transform):
    """get_rotation_translation_from_transform_w_scale (modules/ops/transformation.py:110-123): (R, t / s, s)."""
    A = transform[..., :3, :3]
    scale = torch.matmul(A, A.transpose(-1, -2))[..., 0:1, 0:1] ** 0.5
    return A / scale, transform[..., :3, 3] / scale, scale


def isotropic_transform_error(gt_transform, transform):
    """modules/registration/metrics.py:97-125 -> (RRE in degrees, RTE relative to |t_gt|, RSE relative to s_gt)."""
    gR, gt, gs = _split_similarity(gt_transform)
    R, t, s = _split_similarity(transform)
    mat = torch.matmul(R.transpose(-1, -2), gR)
    x = (0.5 * (mat[..., 0, 0] + mat[..., 1, 1] + mat[..., 2, 2] - 1.0)).clamp(min=-1.0, max=1.0)
    rre = 180.0 * torch.arccos(x) / math.pi
    rte = torch.linalg.norm(gt - t, dim=-1) / torch.linalg.norm(gt, dim=-1)
    rse = torch.linalg.norm(gs - s, dim=-1) / torch.linalg.norm(gs, dim=-1)
    return rre.mean(), rte.mean(), rse


class Evaluator(nn.Module):
    """loss.py:95-162.  `evaluate_registration` undoes the data loader's normalisation like the reference (`ref_adjust_scale`,
    `src_adjust_scale`, `ref_center`, `src_center` of `data_dict`; absent keys count as 1 and 0) -- on copies: the reference
    rescales `data_dict['transform']` and `output_dict['estimated_transform']` in place."""

    def __init__(self, cfg):
        super().__init__()
        self.acceptance_overlap = cfg.eval.acceptance_overlap
        self.acceptance_radius = cfg.eval.acceptance_radius
        self.acceptance_rmse = cfg.eval.rmse_threshold

    @torch.no_grad()
    def evaluate_coarse(self, output_dict):
        """The share of the predicted superpoint correspondences that are ground-truth ones (overlap > acceptance_overlap)."""
        overlaps, idx = output_dict['gt_node_corr_overlaps'], output_dict['gt_node_corr_indices']
        idx = idx[torch.gt(overlaps, self.acceptance_overlap)]
        corr_map = torch.zeros(output_dict['ref_points_c'].shape[0], output_dict['src_points_c'].shape[0], device=idx.device)
        corr_map[idx[:, 0], idx[:, 1]] = 1.0
        return corr_map[output_dict['ref_node_corr_indices'], output_dict['src_node_corr_indices']].mean()

    @torch.no_grad()
    def evaluate_fine(self, output_dict, data_dict):
        T = data_dict['transform'].to(output_dict['src_corr_points'])
        src = output_dict['src_corr_points'] @ T[:3, :3].T + T[:3, 3]
        dist = torch.linalg.norm(output_dict['ref_corr_points'] - src, dim=1)
        return torch.lt(dist, self.acceptance_radius).float().mean()

    @torch.no_grad()
    def evaluate_registration(self, output_dict, data_dict):
        est = output_dict['estimated_transform'].clone()
        gt = data_dict['transform'].to(est).clone()
        rs, ss = data_dict.get('ref_adjust_scale', 1.0), data_dict.get('src_adjust_scale', 1.0)
        zero = torch.zeros(3, dtype=est.dtype, device=est.device)
        rc = torch.as_tensor(data_dict.get('ref_center', zero)).to(est)
        sc = torch.as_tensor(data_dict.get('src_center', zero)).to(est)
        gt[:3, :3] = gt[:3, :3] / rs * ss
        gt[:3, 3] = gt[:3, 3] / rs
        est[:3, :3] = est[:3, :3] / rs * ss
        est[:3, 3] = est[:3, 3] / rs + rc - torch.matmul(est[:3, :3], sc)
        rre, rte, rse = isotropic_transform_error(gt, est)
        realign = torch.matmul(torch.inverse(gt), est)
        src = output_dict['src_points']
        moved = src @ realign[:3, :3].T + realign[:3, 3]
        rmse = torch.linalg.norm(moved - src, dim=1).mean()
        return rre, rte, rse, rmse, torch.lt(rmse, self.acceptance_rmse).float()

    def forward(self, output_dict, data_dict):
        rre, rte, rse, rmse, recall = self.evaluate_registration(output_dict, data_dict)
        return {'RRE': rre, 'RTE': rte, 'RSE': rse, 'RMSE': rmse, 'RR': recall}
