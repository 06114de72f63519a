"""Optimiser of a Gaussian scene on the HIP kernels of csrc/scene_optim.hip.

    opt = GaussianAdam([{"params": [xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [f_dc], "lr": 2.5e-3, "name": "f_dc"}, ...])
    stats = DensifyStats(P, device)
    ...
    loss.backward()
    opt.step(visibility=radii)               # None | (P,) bool / uint8 mask | (P,) or (V, P) int32 radii
    stats.update(means2D.grad, radii)
    opt.zero_grad(set_to_none=True)

`GaussianAdam` is torch.optim.Adam (no weight decay, no amsgrad) whose whole step is ONE launch over all parameter tensors
of the scene, and which leaves the Gaussians that `visibility` marks invisible untouched: parameters and both moments
keep their bits.  The bias corrections follow the optimiser's step count, as in torch, so without `visibility` the step
is torch's Adam; INTEGRATION.md has the definition.  State keys and layout are torch's.  `reindex(index)` on both
classes gathers rows (prune with a subset, clone with a repeated index).  There is no CPU fallback.
"""
import torch

from . import _lib


def _check_param(p, P, dev, what):
    if not isinstance(p, torch.Tensor):
        raise ValueError(f"{what}: not a tensor")
    if p.dtype != torch.float32:
        raise ValueError(f"{what}: dtype {p.dtype}, must be float32")
    if not p.is_cuda:
        raise ValueError(f"{what}: on {p.device}; every tensor must be on one GPU (there is no CPU fallback)")
    if dev is not None and p.device != dev:
        raise ValueError(f"{what}: on {p.device}, the other tensors are on {dev}")
    if p.dim() < 1:
        raise ValueError(f"{what}: a scalar has no Gaussian dimension")
    if not p.is_contiguous():
        raise ValueError(f"{what}: not contiguous")
    if P is not None and p.shape[0] != P:
        raise ValueError(f"{what}: leading dimension {p.shape[0]}, the other tensors have {P}")


def _visibility(visibility, P, dev):
    """-> (mask uint8 (P,) or None, radii int32 (V, P) or None, V)"""
    if visibility is None:
        return None, None, 0
    t = visibility
    if not isinstance(t, torch.Tensor):
        raise ValueError("visibility: not a tensor")
    if t.device != dev:
        raise ValueError(f"visibility: on {t.device}, the parameters are on {dev}")
    if not t.is_contiguous():
        raise ValueError("visibility: not contiguous")
    if t.dtype in (torch.bool, torch.uint8):
        if tuple(t.shape) != (P,):
            raise ValueError(f"visibility: mask of shape {tuple(t.shape)}, must be ({P},)")
        return t.view(torch.uint8), None, 0
    if t.dtype == torch.int32:
        if t.dim() == 1:
            t = t[None]
        if t.dim() != 2 or t.shape[1] != P or t.shape[0] < 1:
            raise ValueError(f"visibility: radii of shape {tuple(visibility.shape)}, must be ({P},) or (V, {P})")
        return None, t, int(t.shape[0])
    raise ValueError(f"visibility: dtype {t.dtype}, must be bool, uint8 (mask) or int32 (radii)")


class GaussianAdam(torch.optim.Optimizer):
    """Adam over the parameter tensors of one Gaussian scene; one tensor per group, all (P, ...) fp32 on one GPU."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-15):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid lr {lr}, betas {betas} or eps {eps}")
        # torch.optim.Adam's own group keys (weight_decay, amsgrad, ...) at their inert defaults, so that a state_dict of
        # this optimiser loads into torch's Adam and steps there
        defaults = dict(torch.optim.Adam([torch.zeros(1)], foreach=False).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps)
        super().__init__(params, defaults)
        self._layout()

    def _layout(self):
        """Validate every group; -> (P, device)."""
        P, dev = None, None
        for gi, group in enumerate(self.param_groups):
            what = f"param group {group.get('name', gi)}"
            if len(group["params"]) != 1:
                raise ValueError(f"{what}: {len(group['params'])} tensors, GaussianAdam takes one tensor per group")
            p = group["params"][0]
            _check_param(p, P, dev, what)
            P, dev = p.shape[0], p.device
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
                raise ValueError(f"{what}: weight_decay, amsgrad and maximize are not supported")
        return P, dev

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, visibility=None, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        P, dev = self._layout()
        if P is None:
            return loss
        mask, radii, V = _visibility(visibility, P, dev)
        # one launch per distinct (step count, betas, eps): one launch unless groups were given different ones
        active = []
        for gi, group in enumerate(self.param_groups):
            p = group["params"][0]
            if p.grad is None:
                continue
            what = f"gradient of param group {group.get('name', gi)}"
            if p.grad.is_sparse:
                raise ValueError(f"{what}: sparse")
            _check_param(p.grad, P, dev, what)
            if p.grad.shape != p.shape:
                raise ValueError(f"{what}: shape {tuple(p.grad.shape)}, the parameter has {tuple(p.shape)}")
            active.append((gi, group, p))
        launches = {}
        for gi, group, p in active:  # state is created only once every group has passed
            st = self._state_of(p)
            for key in ("exp_avg", "exp_avg_sq"):
                _check_param(st[key], P, dev, f"{key} of param group {group.get('name', gi)}")
                if st[key].shape != p.shape:
                    raise ValueError(f"{key} of param group {group.get('name', gi)}: shape {tuple(st[key].shape)}")
            t = int(st["step"].item() if isinstance(st["step"], torch.Tensor) else st["step"]) + 1
            beta1, beta2 = group["betas"]
            K = p.numel() // P if P else 0
            what = f"gr_gs_adam_step: param group {group.get('name', gi)}"
            entry = _lib.GsAdamGroup(*(_lib.device_ptr(t, dev, what) for t in (p, p.grad, st["exp_avg"], st["exp_avg_sq"])),
                                     float(group["lr"]), K)
            launches.setdefault((t, float(beta1), float(beta2), float(group["eps"])), []).append((entry, st))
        if not launches:
            return loss
        for (t, beta1, beta2, eps), entries in launches.items():
            bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
            for i in range(0, len(entries), _lib.GS_ADAM_MAX_GROUPS):
                chunk = entries[i:i + _lib.GS_ADAM_MAX_GROUPS]
                table = (_lib.GsAdamGroup * len(chunk))(*[e for e, _ in chunk])
                _lib.call(dev, "gr_gs_adam_step", table, len(chunk), P, beta1, beta2, eps, bc1, bc2, mask, radii, V)
            for _, st in entries:
                if isinstance(st["step"], torch.Tensor):
                    st["step"] += 1
                else:
                    st["step"] = torch.tensor(float(t), dtype=torch.float32)
        return loss

    @torch.no_grad()
    def reindex(self, index):
        """Gather the rows `index` (int64) of every parameter and of its moments: a subset prunes, a repeated index
        clones.  New tensors replace the old ones in param_groups (same class, same requires_grad); -> the new tensors."""
        if index.dtype != torch.int64 or index.dim() != 1:
            raise ValueError("reindex: index must be a 1-D int64 tensor")
        out = []
        for group in self.param_groups:
            old = group["params"][0]
            new = old.detach()[index].contiguous()
            if isinstance(old, torch.nn.Parameter):
                new = torch.nn.Parameter(new, requires_grad=old.requires_grad)
            else:
                new.requires_grad_(old.requires_grad)
            st = self.state.pop(old, None)
            if st:
                self.state[new] = {"step": st["step"], "exp_avg": st["exp_avg"][index].contiguous(),
                                   "exp_avg_sq": st["exp_avg_sq"][index].contiguous()}
            group["params"][0] = new
            out.append(new)
        return out


class DensifyStats:
    """Per-Gaussian statistics of 3DGS densification: the accumulated norm of the screen-space gradient, the number of
    views that saw the Gaussian, and its largest screen radius."""

    def __init__(self, P, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.HipLibraryError("gaussreg_amd.scene_optim needs tensors on an MI355X; there is no CPU fallback")
        self.grad_accum = torch.zeros(P, dtype=torch.float32, device=device)
        self.denom = torch.zeros(P, dtype=torch.int32, device=device)
        self.max_radii = torch.zeros(P, dtype=torch.int32, device=device)

    @torch.no_grad()
    def update(self, means2D_grad, radii):
        """means2D_grad (V, P, 3) fp32 with radii (V, P) int32, or upstream's (P, 3) and (P,) of one camera."""
        P, dev = self.grad_accum.shape[0], self.grad_accum.device
        g, r = means2D_grad, radii
        if g.dim() == 2 and r.dim() == 1:
            g, r = g[None], r[None]
        if g.dtype != torch.float32 or r.dtype != torch.int32:
            raise ValueError(f"means2D_grad must be float32 and radii int32 (got {g.dtype}, {r.dtype})")
        if g.dim() != 3 or tuple(g.shape[1:]) != (P, 3) or tuple(r.shape) != (g.shape[0], P):
            raise ValueError(f"means2D_grad {tuple(means2D_grad.shape)} and radii {tuple(radii.shape)} must be (V, {P}, 3) and "
                             f"(V, {P}), or ({P}, 3) and ({P},)")
        if g.device != dev or r.device != dev:
            raise ValueError(f"means2D_grad and radii must be on {dev}")
        if not (g.is_contiguous() and r.is_contiguous()):
            raise ValueError("means2D_grad and radii must be contiguous")
        _lib.call(dev, "gr_gs_densify_stats", g, r, P, int(g.shape[0]), self.grad_accum, self.denom, self.max_radii)

    def mean_grad(self):
        """grad_accum / max(denom, 1): upstream's average screen-space gradient norm per Gaussian."""
        return self.grad_accum / self.denom.clamp(min=1).to(torch.float32)

    def reset(self):
        self.grad_accum.zero_()
        self.denom.zero_()
        self.max_radii.zero_()

    def reindex(self, index):
        if index.dtype != torch.int64 or index.dim() != 1:
            raise ValueError("reindex: index must be a 1-D int64 tensor")
        self.grad_accum = self.grad_accum[index].contiguous()
        self.denom = self.denom[index].contiguous()
        self.max_radii = self.max_radii[index].contiguous()
