"""gaussreg_amd -- MI355X-native implementation of GaussReg's two data-parallel hot paths.

Host side: Python on PyTorch-ROCm (device memory, streams, torch.distributed only).
Device side: hand-written HIP kernels for gfx950 behind the C ABI in include/gaussreg_hip.h
(gaussreg_amd/lib/libgaussreg_hip.so, built by `python -m gaussreg_amd.build`).

There is no CPU fallback: every op raises if the HIP library or a GPU is missing.
"""
__version__ = "0.1.0"


def differentiable(chunk_rows=0, fused_norm=False):
    """`with gaussreg_amd.differentiable():` -- the one switch that makes the KPConv backbone and the transformer stack
    differentiable (gaussreg_amd.kpconv.differentiable; imported on use so that `import gaussreg_amd` stays light).
    `fused_norm=True`: the backbone's GroupNorm layers run in HIP in training as well."""
    from .kpconv import differentiable as ctx
    return ctx(chunk_rows, fused_norm)


_LOSSES = ("WeightedCircleLoss", "CoarseMatchingLoss", "FineMatchingLoss", "OverallLoss", "Evaluator")

# the reference's overlap / correspondence / evaluation functions on the cross-cloud search (gaussreg_amd.cloud_nn)
_CLOUD_NN = ("compute_overlap", "get_correspondences", "compute_modified_chamfer_distance", "compute_inlier_ratio",
             "compute_correspondence_residual", "evaluate_correspondences", "compute_registration_rmse")

# point-to-point ICP (gaussreg_amd.icp).  `gaussreg_amd.icp` is the submodule, which is callable as its function `icp`:
# `gaussreg_amd.icp(src, ref, ...)` and `from gaussreg_amd import icp; icp(src, ref, ...)` both run it.
_ICP = ("icp", "evaluate_registration", "IcpResult", "icp_point_to_plane", "icp_generalized")

# PCA normals from a neighbour table (gaussreg_amd.normals), what point-to-plane ICP takes for its reference cloud
_NORMALS = ("normals_from_neighbors", "estimate_normals")

# the covariances generalised ICP takes: from normals, from a scene's own Gaussians, or estimated (gaussreg_amd.covariances)
_COVARIANCES = ("covariances_from_normals", "covariances_from_gaussians", "estimate_covariances")

# nearest neighbours in feature space and the reference's descriptor matching on them (gaussreg_amd.feature_nn)
_FEATURE_NN = ("feature_nn", "extract_corr_indices_from_feats", "extract_correspondences_from_feats")


def __getattr__(name):
    """The training losses and metrics (gaussreg_amd.loss), the evaluation functions (gaussreg_amd.cloud_nn), ICP
    (gaussreg_amd.icp), normals (gaussreg_amd.normals), covariances (gaussreg_amd.covariances) and descriptor matching (gaussreg_amd.feature_nn), imported on first use like `differentiable`."""
    if name in _FEATURE_NN:
        import importlib
        module = importlib.import_module(".feature_nn", __name__)
        return module if name == "feature_nn" else getattr(module, name)
    if name in _COVARIANCES:
        import importlib
        return getattr(importlib.import_module(".covariances", __name__), name)
    if name in _NORMALS:
        import importlib
        return getattr(importlib.import_module(".normals", __name__), name)
    if name in _ICP:
        import importlib
        module = importlib.import_module(".icp", __name__)
        return module if name == "icp" else getattr(module, name)
    if name in _LOSSES:
        from . import loss
        return getattr(loss, name)
    if name in _CLOUD_NN:
        from . import cloud_nn
        return getattr(cloud_nn, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
