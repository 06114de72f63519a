"""Camera tensors as differentiable functions of a pose, for render-and-compare refinement through the rasterizer.

The rasterizer returns gradients for `viewmatrix`, `projmatrix` and `campos` as three independent inputs
(gaussreg_amd/rasterizer.py).  The functions here compose the three from one pose in torch, so autograd chains the three
gradients into dL/d(pose).  Conventions are those of `synthetic.camera` (3DGS): `R_c2w` rotates camera axes to world
axes, `C` is the camera centre in the world, the matrices are stored TRANSPOSED (a row vector times the tensor), so the
world-to-view map of a point X is `[X, 1] @ viewmatrix`.

    camera_tensors(R_c2w, C, tanfovx, tanfovy)      -> viewmatrix (4,4), projmatrix (4,4), campos (3)
    similarity_camera(viewmatrix, s, R, t)          -> the camera that sees the UNMOVED scene as the original camera sees
                                                       the scene moved by x -> s R x + t
    so3_exp(w)                                      -> rotation matrix of the rotation vector w (axis * angle)
"""
import torch


def so3_exp(w):
    """Rotation matrix exp([w]_x) of a rotation vector w (3,), differentiable everywhere (w = 0 included)."""
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    return torch.linalg.matrix_exp(K)


def _projection_t(tanfovx, tanfovy, znear, zfar, dtype, device):
    """Transposed perspective matrix of synthetic.camera."""
    Pm = torch.zeros((4, 4), dtype=dtype, device=device)
    Pm[0, 0] = 1.0 / tanfovx
    Pm[1, 1] = 1.0 / tanfovy
    Pm[2, 2] = zfar / (zfar - znear)
    Pm[2, 3] = -zfar * znear / (zfar - znear)
    Pm[3, 2] = 1.0
    return Pm.T


def camera_tensors(R_c2w, C, tanfovx, tanfovy, znear=0.01, zfar=100.0):
    """-> (viewmatrix, projmatrix, campos) of the pinhole camera with camera-to-world rotation `R_c2w` (3,3) and centre
    `C` (3,), differentiable in both, in their dtype and on their device: what `synthetic.camera` returns for the same
    pose (there in numpy fp32)."""
    R_c2w = torch.as_tensor(R_c2w)
    C = torch.as_tensor(C, dtype=R_c2w.dtype, device=R_c2w.device)
    dtype, device = R_c2w.dtype, R_c2w.device
    # transposed world-to-view matrix [[R, 0], [-C R, 1]]: x_view = X R - C R = R^T (X - C)
    top = torch.cat([R_c2w, torch.zeros((3, 1), dtype=dtype, device=device)], 1)
    bottom = torch.cat([-(C @ R_c2w), torch.ones(1, dtype=dtype, device=device)])[None]
    viewmatrix = torch.cat([top, bottom], 0)
    projmatrix = viewmatrix @ _projection_t(float(tanfovx), float(tanfovy), float(znear), float(zfar), dtype, device)
    return viewmatrix, projmatrix, C


def similarity_camera(viewmatrix, s, R, t, projmatrix=None):
    """The camera under which the unmoved scene renders as the scene moved by x -> s R x + t renders from `viewmatrix`.

    With x_view = R_v x + t_v the old camera sees the moved point at R_v (s R x + t) + t_v = s (R_v R x + (R_v t + t_v) / s):
    a rigid camera (R_v R, (R_v t + t_v) / s) whose view-space coordinates are 1 / s of the old ones.  A perspective image
    does not change under a uniform scaling about the camera centre, so the colour and alpha images agree and the depth map
    of the new camera times `s` is the old camera's (up to the near-plane cull, which acts on the unscaled depth).

    -> (viewmatrix', projmatrix', campos', s): projmatrix' = viewmatrix' viewmatrix^-1 projmatrix when the old
    `projmatrix` is given (same intrinsics), else None.  Differentiable in s (a scalar tensor or float), R (3,3), t (3,)."""
    Vt = viewmatrix
    dtype, device = Vt.dtype, Vt.device
    s = torch.as_tensor(s, dtype=dtype, device=device)
    R = torch.as_tensor(R, dtype=dtype, device=device)
    t = torch.as_tensor(t, dtype=dtype, device=device)
    Rv_t, tv = Vt[:3, :3], Vt[3, :3]  # transposed storage: x_view = X Rv_t + tv
    new_Rt = R.T @ Rv_t
    new_tv = (t @ Rv_t + tv) / s
    top = torch.cat([new_Rt, torch.zeros((3, 1), dtype=dtype, device=device)], 1)
    bottom = torch.cat([new_tv, torch.ones(1, dtype=dtype, device=device)])[None]
    new_view = torch.cat([top, bottom], 0)
    campos = -(new_tv @ new_Rt.T)
    new_proj = None
    if projmatrix is not None:
        inv = torch.cat([torch.cat([Rv_t.T, torch.zeros((3, 1), dtype=dtype, device=device)], 1),
                         torch.cat([-(tv @ Rv_t.T), torch.ones(1, dtype=dtype, device=device)])[None]], 0)
        new_proj = new_view @ (inv @ projmatrix.to(dtype=dtype, device=device))
    return new_view, new_proj, campos, s
