"""Densify and prune a Gaussian scene on the HIP kernels of csrc/scene_densify.hip: upstream 3DGS's densify_and_prune (clone
the small Gaussians with a large screen-space gradient, split the large ones into two children, prune the transparent and
the oversized) and reset_opacity, on a `GaussianAdam` and its `DensifyStats`.

    r = densify_and_prune(opt, stats, max_grad=2e-4, min_opacity=5e-3, extent=extent, max_screen_size=20)
    xyz, scaling = r.tensors["xyz"], r.tensors["scaling"]     # the new leaf tensors, already in opt.param_groups
    ...
    reset_opacity(opt)

One classification pass and one gather pass rebuild every parameter and both of its moments; the new Gaussian count is
the only value read back.  The groups named `xyz`, `opacity`, `scaling` and `rotation` are upstream's raw parameters;
every other group is carried row by row.  INTEGRATION.md has the definition.  There is no CPU fallback.
"""
from dataclasses import dataclass

import torch

from . import _lib
from .scene_optim import DensifyStats, GaussianAdam, _check_param

ROLE_SHAPES = {"xyz": (3,), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


@dataclass
class DensifyResult:
    tensors: dict           # group name (or index, for a group without a name) -> the new parameter tensor
    P_new: int
    source: torch.Tensor    # (P_new,) int32: the Gaussian a row comes from
    kind: torch.Tensor      # (P_new,) uint8: 0 original, 1 clone, 2 / 3 child 0 / 1
    counts: tuple           # (originals kept, clones, children 0, children 1)


def _roles(opt):
    """-> (P, device, {role name: parameter}) of a validated GaussianAdam."""
    if not isinstance(opt, GaussianAdam):
        raise ValueError(f"opt: {type(opt).__name__}, must be a GaussianAdam")
    P, dev = opt._layout()
    if P is None:
        raise ValueError("opt: no parameter groups")
    roles = {}
    for group in opt.param_groups:
        name = group.get("name")
        if name in ROLE_SHAPES:
            if name in roles:
                raise ValueError(f"param group {name}: named twice")
            p = group["params"][0]
            if tuple(p.shape[1:]) != ROLE_SHAPES[name]:
                raise ValueError(f"param group {name}: shape {tuple(p.shape)}, must be {(P,) + ROLE_SHAPES[name]}")
            roles[name] = p
    return P, dev, roles


def _check_state(opt, P, dev):
    for gi, group in enumerate(opt.param_groups):
        p = group["params"][0]
        st = opt.state.get(p)
        if st:
            for key in ("exp_avg", "exp_avg_sq"):
                what = f"{key} of param group {group.get('name', gi)}"
                _check_param(st[key], P, dev, what)
                if st[key].shape != p.shape:
                    raise ValueError(f"{what}: shape {tuple(st[key].shape)}, the parameter has {tuple(p.shape)}")


@torch.no_grad()
def densify_and_prune(opt, stats, max_grad, min_opacity, extent, max_screen_size=None, percent_dense=0.01, noise=None,
                      generator=None):
    """Upstream's densify_and_prune on `opt` (GaussianAdam) and `stats` (DensifyStats); -> DensifyResult.  `noise` (P, 2, 3)
    fp32: the standard normals of the two children of every SOURCE Gaussian (default: torch.randn with `generator`)."""
    P, dev, roles = _roles(opt)
    missing = [n for n in ROLE_SHAPES if n not in roles]
    if missing:
        raise ValueError(f"opt: no param group named {', '.join(missing)} (groups are found by their 'name')")
    if not isinstance(stats, DensifyStats):
        raise ValueError(f"stats: {type(stats).__name__}, must be a DensifyStats")
    for key, dtype in (("grad_accum", torch.float32), ("denom", torch.int32), ("max_radii", torch.int32)):
        t = getattr(stats, key)
        if tuple(t.shape) != (P,):
            raise ValueError(f"stats.{key}: shape {tuple(t.shape)}, the scene has {P} Gaussians")
        if t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise ValueError(f"stats.{key}: must be a contiguous {dtype} tensor on {dev}")
    if noise is None:
        noise = torch.randn((P, 2, 3), generator=generator, device=dev, dtype=torch.float32)
    else:
        if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (P, 2, 3):
            raise ValueError(f"noise: must be a tensor of shape ({P}, 2, 3)")
        if noise.dtype != torch.float32 or noise.device != dev or not noise.is_contiguous():
            raise ValueError(f"noise: must be a contiguous float32 tensor on {dev}")
    _check_state(opt, P, dev)
    source = torch.empty(2 * P, dtype=torch.int32, device=dev)
    kind = torch.empty(2 * P, dtype=torch.uint8, device=dev)
    counts_dev = torch.empty(4, dtype=torch.int32, device=dev)
    h_counts = _lib.host_i64([0] * 4)
    _lib.call(dev, "gr_gs_densify_plan", roles["scaling"], roles["opacity"], stats.grad_accum, stats.denom, stats.max_radii, P,
              float(max_grad), float(min_opacity), float(extent), float(percent_dense), int(max_screen_size is not None),
              float(max_screen_size or 0.0), source, kind, counts_dev, h_counts,
              ws=_lib.lib().gr_gs_densify_plan_workspace_bytes(P))
    counts = tuple(int(c) for c in h_counts[:4])
    P_new = sum(counts)
    # new tensors and the group table; nothing of opt or stats is replaced before every launch has been accepted
    entries, rebuilt = [], []
    for group in opt.param_groups:
        old = group["params"][0]
        st = opt.state.get(old)
        new = torch.empty((P_new,) + tuple(old.shape[1:]), dtype=torch.float32, device=dev)
        new_m = torch.empty_like(new) if st else None
        new_v = torch.empty_like(new) if st else None
        name = group.get("name")
        role = {"xyz": _lib.GS_DENSIFY_XYZ, "scaling": _lib.GS_DENSIFY_SCALING}.get(name, _lib.GS_DENSIFY_CARRIED)
        fields = (old, new, st["exp_avg"] if st else None, new_m, st["exp_avg_sq"] if st else None, new_v)
        entries.append(_lib.GsDensifyGroup(*(_lib.device_ptr(t, dev, f"gr_gs_densify_apply: param group {name}") for t in fields),
                                           old.numel() // P if P else 0, role))
        rebuilt.append((group, old, st, new, new_m, new_v))
    for i in range(0, len(entries), _lib.GS_ADAM_MAX_GROUPS):
        chunk = entries[i:i + _lib.GS_ADAM_MAX_GROUPS]
        table = (_lib.GsDensifyGroup * len(chunk))(*chunk)
        _lib.call(dev, "gr_gs_densify_apply", table, len(chunk), P, P_new, source, kind, roles["scaling"], roles["rotation"],
                  noise)
    tensors = {}
    for gi, (group, old, st, new, new_m, new_v) in enumerate(rebuilt):
        if isinstance(old, torch.nn.Parameter):
            new = torch.nn.Parameter(new, requires_grad=old.requires_grad)
        else:
            new.requires_grad_(old.requires_grad)
        opt.state.pop(old, None)
        if st:
            opt.state[new] = {"step": st["step"], "exp_avg": new_m, "exp_avg_sq": new_v}
        group["params"][0] = new
        tensors[group.get("name", gi)] = new
    stats.grad_accum = torch.zeros(P_new, dtype=torch.float32, device=dev)
    stats.denom = torch.zeros(P_new, dtype=torch.int32, device=dev)
    stats.max_radii = torch.zeros(P_new, dtype=torch.int32, device=dev)
    return DensifyResult(tensors, P_new, source[:P_new], kind[:P_new], counts)


@torch.no_grad()
def reset_opacity(opt, ceiling=0.01):
    """Upstream's reset_opacity: opacity <- logit(min(sigmoid(opacity), ceiling)) in place, its two moments zeroed."""
    if not 0.0 < ceiling < 1.0:
        raise ValueError(f"ceiling {ceiling} outside (0, 1)")
    P, dev, roles = _roles(opt)
    if "opacity" not in roles:
        raise ValueError("opt: no param group named opacity")
    p = roles["opacity"]
    o = torch.sigmoid(p).clamp_(max=ceiling)
    p.copy_(torch.log(o / (1.0 - o)))
    st = opt.state.get(p)
    if st:
        st["exp_avg"].zero_()
        st["exp_avg_sq"].zero_()
    return p
