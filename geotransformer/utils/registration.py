"""utils/registration.py of the reference: the functions that ask scipy's cKDTree for neighbours there -- compute_overlap,
get_correspondences, compute_modified_chamfer_distance, evaluate_correspondences -- and the correspondence metrics beside
them run on gaussreg_amd.cloud_nn, with the reference's signatures: numpy in, numpy out; tensors in, tensors out.
get_correspondences orders its pairs by (ref index, src index) ascending.  The descriptor matching of the same file --
extract_corr_indices_from_feats, extract_correspondences_from_feats -- runs on gaussreg_amd.feature_nn, a fused
distance-and-argmin kernel, in the same way; its neighbour of a row is the smallest under (distance, index).  Every other
name of the reference's file (the transform-error metrics, ...) is the reference's own when its checkout is on sys.path:
the file runs in this module first, then the names below replace its searches."""
from gaussreg_amd._alias import inline_shadowed as _inline

_inline(globals())

from gaussreg_amd import cloud_nn as _nn  # noqa: E402

compute_overlap = _nn.array_api(_nn.compute_overlap, 2)
get_correspondences = _nn.array_api(_nn.get_correspondences, 2)
compute_modified_chamfer_distance = _nn.array_api(_nn.compute_modified_chamfer_distance, 3)
compute_inlier_ratio = _nn.array_api(_nn.compute_inlier_ratio, 2)
compute_correspondence_residual = _nn.array_api(_nn.compute_correspondence_residual, 2)
evaluate_correspondences = _nn.array_api(_nn.evaluate_correspondences, 2)
compute_registration_rmse = _nn.array_api(_nn.compute_registration_rmse, 1)

from gaussreg_amd import feature_nn as _fnn  # noqa: E402

extract_corr_indices_from_feats = _nn.array_api(_fnn.extract_corr_indices_from_feats, 2)
extract_correspondences_from_feats = _nn.array_api(_fnn.extract_correspondences_from_feats, 4)
