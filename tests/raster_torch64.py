"""Test helper (not collected): a dense float64 torch restatement of the rasterizer forward, written from the algorithm
(Kerbl et al. 2023, the rules oracle/rasterizer_np64.py lists), so that autograd through it gives reference gradients for
the HIP backward.

Rules kept from the forward: near cull z <= 0.2 and depth order by fp32 view-space z (ties: index); +0.3 px^2 dilation;
radius = ceil(3 sqrt(lambda_max)); a pixel sees a Gaussian only if its 16 x 16 tile lies in the tile rectangle of
(centre +- radius); skip power > 0 and alpha < 1/255; stop BEFORE blending once T (1 - alpha) < 1e-4; final colour
C + T bg.  alpha = min(opacity G, 0.99) is straight-through for the gradient (upstream's backward); the 1.3 tan(fov)
clamp and the SH max(., 0) are torch.clamp (zero gradient where active).  Everything is float64; decisions (visibility,
rectangle, skip and stop rules) are taken on the float64 values, so a few isolated pixels may decide a threshold the
other way than the fp32 kernels do.

Compositing is dense over (pixels x visible Gaussians) in depth order; `grads()` runs it over chunks of pixels and
calls backward() per chunk (the loss is a sum over pixels), so memory stays bounded on larger scenes.
"""
import torch

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)
NAMES = ("means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


def _f32(x):
    return x.to(torch.float32).to(torch.float64)


def sh_basis(d, degree):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    cols = [torch.full_like(x, SH_C0)]
    if degree > 0:
        cols += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        cols += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
        if degree > 2:
            cols += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
                     SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
                     SH_C3[6] * x * (xx - 3 * yy)]
    return torch.stack(cols, 1)


def preprocess(cam, means3D, opacities, means2D=None, shs=None, colors_precomp=None, scales=None, rotations=None,
               cov3D_precomp=None, sh_degree=0, scale_modifier=1.0):
    """Per-Gaussian quantities (differentiable float64) of the visible Gaussians, in depth order."""
    dev = means3D.device
    f8 = torch.float64
    p = means3D.to(f8)
    P = p.shape[0]
    W, H = int(cam["W"]), int(cam["H"])
    Vm = torch.as_tensor(cam["viewmatrix"], dtype=f8, device=dev).reshape(4, 4).T
    PM = torch.as_tensor(cam["projmatrix"], dtype=f8, device=dev).reshape(4, 4).T
    campos = torch.as_tensor(cam["campos"], dtype=f8, device=dev).reshape(3)
    tanx, tany = float(cam["tanfovx"]), float(cam["tanfovy"])
    ph = torch.cat([p, torch.ones((P, 1), dtype=f8, device=dev)], 1)
    pv = ph @ Vm.T
    hom = ph @ PM.T
    ndc = hom[:, :2] / (hom[:, 3:4] + 1e-7)
    if means2D is not None:
        ndc = ndc + means2D.to(f8)[:, :2]  # upstream's screen-space handle: its gradient is dL/dNDC
    with torch.no_grad():  # depth in fp32, as the kernels order by it
        pd = p.detach().to(torch.float32).to(f8)
        Vf = Vm.to(torch.float32).to(f8)
        z32 = _f32(Vf[2, 0] * pd[:, 0] + _f32(Vf[2, 1] * pd[:, 1] + _f32(Vf[2, 2] * pd[:, 2] + Vf[2, 3])))
    visible = z32 > 0.2
    if cov3D_precomp is not None:
        c = cov3D_precomp.to(f8)
        S3 = torch.stack([torch.stack([c[:, 0], c[:, 1], c[:, 2]], 1), torch.stack([c[:, 1], c[:, 3], c[:, 4]], 1),
                          torch.stack([c[:, 2], c[:, 4], c[:, 5]], 1)], 1)
    else:
        q = rotations.to(f8)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                         torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                         torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
        s = scales.to(f8) * float(scale_modifier)
        M = R * s[:, None, :]
        S3 = M @ M.transpose(1, 2)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    tz = torch.where(visible, pv[:, 2], torch.ones_like(pv[:, 2]))
    tx = torch.clamp(pv[:, 0] / tz, -1.3 * tanx, 1.3 * tanx) * tz
    ty = torch.clamp(pv[:, 1] / tz, -1.3 * tany, 1.3 * tany) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -fx * tx / (tz * tz)], 1),
                     torch.stack([zero, fy / tz, -fy * ty / (tz * tz)], 1)], 1)
    T = J @ Vm[:3, :3][None]
    cov = T @ S3 @ T.transpose(1, 2)
    a, b, c2 = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c2 - b * b
    with torch.no_grad():
        ok = visible & (det != 0)
        mid = 0.5 * (a + c2)
        lam = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
        radius = torch.ceil(3.0 * torch.sqrt(lam))
    det_s = torch.where(ok, det, torch.ones_like(det))
    conic = torch.stack([c2 / det_s, -b / det_s, a / det_s], 1)
    px = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    py = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    gx, gy = (W + 15) // 16, (H + 15) // 16
    with torch.no_grad():
        def tile(v, g):
            return torch.clamp(torch.trunc(torch.nan_to_num(v) / 16.0), 0, g).to(torch.int64)
        pxd, pyd = torch.where(ok, px, zero), torch.where(ok, py, zero)
        x0, x1 = tile(pxd - radius, gx), tile(pxd + radius + 15, gx)
        y0, y1 = tile(pyd - radius, gy), tile(pyd + radius + 15, gy)
        ok = ok & (x1 > x0) & (y1 > y0)
    if colors_precomp is not None:
        rgb = colors_precomp.to(f8)
    else:
        sh = shs.to(f8).reshape(P, -1, 3)
        d = p - campos[None]
        d = d / torch.linalg.norm(d, dim=1, keepdim=True)
        B = sh_basis(d, int(sh_degree))
        rgb = torch.clamp(torch.einsum('nk,nkc->nc', B, sh[:, :B.shape[1], :]) + 0.5, min=0.0)
    idx = torch.nonzero(ok).reshape(-1)
    order = idx[torch.argsort(z32[idx], stable=True)]  # idx ascending: ties keep the index order
    radii = torch.where(ok, radius, zero).to(torch.int64)
    return dict(order=order, px=px[order], py=py[order], conic=conic[order], op=opacities.to(f8).reshape(-1)[order],
                rgb=rgb[order], x0=x0[order], x1=x1[order], y0=y0[order], y1=y1[order], radii=radii, W=W, H=H)


def composite(pre, bg, pix):
    """Colours (3, n) of the pixels with flat indices `pix` (differentiable)."""
    W = pre["W"]
    pxf = (pix % W).to(torch.float64)
    pyf = (pix // W).to(torch.float64)
    tx, ty = (pix % W) // 16, (pix // W) // 16
    member = ((tx[:, None] >= pre["x0"][None]) & (tx[:, None] < pre["x1"][None]) &
              (ty[:, None] >= pre["y0"][None]) & (ty[:, None] < pre["y1"][None]))
    dx = pre["px"][None] - pxf[:, None]
    dy = pre["py"][None] - pyf[:, None]
    cn = pre["conic"]
    power = -0.5 * (cn[None, :, 0] * dx * dx + cn[None, :, 2] * dy * dy) - cn[None, :, 1] * dx * dy
    raw = pre["op"][None] * torch.exp(torch.clamp(power, max=0.0))
    alpha = raw - (raw - torch.clamp(raw, max=0.99)).detach()  # straight-through clamp
    with torch.no_grad():
        valid = member & (power <= 0.0) & (alpha >= 1.0 / 255.0)
        t_incl = torch.cumprod(1.0 - torch.where(valid, alpha, torch.zeros_like(alpha)), 1)
        stop = valid & (t_incl < 1e-4)
        blend = valid & (torch.cumsum(stop.to(torch.int32), 1) == 0)
    a = torch.where(blend, alpha, torch.zeros_like(alpha))
    t_incl = torch.cumprod(1.0 - a, 1)
    t_excl = torch.cat([torch.ones_like(t_incl[:, :1]), t_incl[:, :-1]], 1)
    w = a * t_excl
    col = w @ pre["rgb"]  # (n, 3)
    t_fin = t_incl[:, -1] if t_incl.shape[1] > 0 else torch.ones(pix.shape[0], dtype=torch.float64, device=pix.device)
    bg = torch.as_tensor(bg, dtype=torch.float64, device=pix.device).reshape(1, 3)
    return (col + t_fin[:, None] * bg).T


def render(cam, bg, chunk=4096, **inputs):
    """-> (image (3, H, W) float64, differentiable, radii (P,))."""
    pre = preprocess(cam, **inputs)
    W, H = pre["W"], pre["H"]
    dev = inputs["means3D"].device
    cols = [composite(pre, bg, torch.arange(s, min(s + chunk, H * W), device=dev)) for s in range(0, H * W, chunk)]
    return torch.cat(cols, 1).reshape(3, H, W), pre["radii"]


def grads(cam, bg, grad_output, chunk=4096, pixels=None, **inputs):
    """Reference gradients of sum(image * grad_output): dict name -> float64 tensor (None for absent inputs), and the
    float64 image.  Inputs are copied into float64 leaves; `means2D` is added as a zero (P, 3) leaf.
    `pixels` (flat indices): composite only these -- grad_output must be zero everywhere else (large scenes: the
    gradient is exact, only the returned image is left unset, NaN, outside them)."""
    leaves = {}
    for k, v in inputs.items():
        if k in NAMES and v is not None:
            leaves[k] = v.detach().to(torch.float64).clone().requires_grad_(True)
    P = inputs["means3D"].shape[0]
    dev = inputs["means3D"].device
    leaves["means2D"] = torch.zeros((P, 3), dtype=torch.float64, device=dev, requires_grad=True)
    other = {k: v for k, v in inputs.items() if k not in NAMES}
    pre = preprocess(cam, **leaves, **other)
    W, H = pre["W"], pre["H"]
    go = grad_output.detach().to(torch.float64).reshape(3, H * W)
    img = torch.full((3, H * W), float("nan"), dtype=torch.float64, device=dev)
    tensors = [t for t in leaves.values()]
    acc = [torch.zeros_like(t) for t in tensors]
    allpix = torch.arange(H * W, device=dev) if pixels is None else torch.as_tensor(pixels, device=dev).reshape(-1)
    for s in range(0, allpix.numel(), chunk):
        pix = allpix[s:s + chunk]
        c = composite(pre, bg, pix)
        img[:, pix] = c.detach()
        gs = torch.autograd.grad((c * go[:, pix]).sum(), tensors, retain_graph=True, allow_unused=True)
        for a, g in zip(acc, gs):
            if g is not None:
                a += g
    out = {k: None for k in NAMES}
    for k, a in zip(leaves, acc):
        out[k] = a
    return out, img.reshape(3, H, W), pre["radii"]


def camera_dict(cam, W, H):
    """synthetic.camera(...) output -> the dict preprocess() reads."""
    d = dict(cam)
    d["W"], d["H"] = W, H
    return d
