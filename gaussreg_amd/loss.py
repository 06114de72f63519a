"""Training losses.  `FineMatchingLoss` mirrors FineMatchingLoss of the experiment's loss.py (:43-71) in plain torch: it has
no hot path of its own -- it selects entries of the Sinkhorn output, whose gradient is the HIP backward of
gaussreg_amd.sinkhorn (inside `gaussreg_amd.differentiable()`)."""
import torch
import torch.nn as nn


class FineMatchingLoss(nn.Module):
    def __init__(self, positive_radius):
        super().__init__()
        self.positive_radius = positive_radius

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
