"""``diff_gaussian_rasterization`` drop-in (differentiable: forward and backward), backed by the gfx950 rasterizer.
``GaussianRasterizer(settings, render_depth=True)`` returns ``(color, radii, depth, alpha)`` (extension)."""
from gaussreg_amd.rasterizer import (  # noqa: F401
    GaussianRasterizationSettings,
    GaussianRasterizer,
    ViewBatch,
    rasterize_gaussians,
    rasterize_views,
)
