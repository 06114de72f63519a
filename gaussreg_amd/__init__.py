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


def __getattr__(name):
    """The training losses and metrics (gaussreg_amd.loss), imported on first use like `differentiable`."""
    if name in _LOSSES:
        from . import loss
        return getattr(loss, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
