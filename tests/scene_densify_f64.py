"""Float64 restatement of upstream 3DGS's densify_and_prune (two children per split) and reset_opacity, in upstream's own
sequence: clone by `cat`; split on the zero-padded gradient by `cat`, then mask out the split originals; prune by mask.
Moments, radii and the bookkeeping (`source`, `kind`) go through the same `cat`s and masks.  The only departures from
upstream's text are the ones INTEGRATION.md states: the gradient of a Gaussian with denom = 0 is 0, the radii of new rows
are 0, and the noise is an input indexed by (source Gaussian, child).

tests/test_scene_densify_f64_reference.py pins this file against a per-Gaussian loop written from the definition.
"""
import torch

MARGIN = 1e-4  # relative distance every s, s', o and non-dyadic g keeps from its threshold (fp32 exp / sigmoid err ~1e-7)
ROLES = ("xyz", "opacity", "scaling", "rotation")


def build_rotation(q):
    """upstream utils/general_utils.py build_rotation, in q's dtype; q (n, 4) in (r, x, y, z) order, unnormalised."""
    norm = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    q = q / norm[:, None]
    R = torch.zeros((q.shape[0], 3, 3), dtype=q.dtype, device=q.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def children(xyz, scaling, rotation, noise_k):
    """Upstream's densify_and_split arithmetic for selected rows, in the dtype of its arguments: -> (new xyz, new scaling).
    noise_k (n, 3): the standard normals of these children."""
    stds = torch.exp(scaling)
    samples = stds * noise_k  # torch.normal(mean=0, std=stds)
    new_xyz = torch.bmm(build_rotation(rotation), samples.unsqueeze(-1)).squeeze(-1) + xyz
    new_scaling = torch.log(stds / (0.8 * 2))
    return new_xyz, new_scaling


def mean_grad(grad_accum, denom):
    g = grad_accum.to(torch.float64) / denom.to(torch.float64)
    g[denom == 0] = 0.0
    return g


def assert_margin(params, stats, max_grad, min_opacity, extent, percent_dense):
    """The inputs keep MARGIN (relative) from every threshold, so fp32 and float64 classify alike.  A gradient EXACTLY on
    max_grad is allowed (dyadic test values: the comparison is >=)."""
    def clear(values, threshold, what):
        rel = (values - threshold).abs() / threshold
        assert bool((rel >= MARGIN).all()), f"{what}: {int((rel < MARGIN).sum())} values within {MARGIN} of {threshold}"
    s = torch.exp(params["scaling"].to(torch.float64)).max(dim=1).values
    clear(s, percent_dense * extent, "s against percent_dense * extent")
    clear(s, 0.1 * extent, "s against 0.1 * extent")
    clear(s / 1.6, 0.1 * extent, "s' against 0.1 * extent")
    clear(torch.sigmoid(params["opacity"].to(torch.float64)), min_opacity, "o against min_opacity")
    g = mean_grad(stats[0], stats[1])
    clear(g[g != max_grad], max_grad, "g against max_grad")


def densify_and_prune(params, moments, stats, max_grad, min_opacity, extent, max_screen_size, percent_dense, noise):
    """params: {name: (P, ...) tensor}; moments: {name: (exp_avg, exp_avg_sq)} for the groups with state; stats:
    (grad_accum, denom, max_radii); noise (P, 2, 3).  Everything is taken to float64.  -> dict with params, moments,
    stats (zeros), source, kind (int64 tensors), counts."""
    f64 = torch.float64
    params = {n: p.detach().to(f64).clone() for n, p in params.items()}
    moments = {n: [m.detach().to(f64).clone(), v.detach().to(f64).clone()] for n, (m, v) in moments.items()}
    noise = noise.to(f64)
    P = params["xyz"].shape[0]
    radii = stats[2].clone().to(torch.int64)
    source = torch.arange(P, dtype=torch.int64)
    kind = torch.zeros(P, dtype=torch.int64)
    grads = mean_grad(stats[0], stats[1])

    def postfix(new_params, new_source, new_kind):
        nonlocal radii, source, kind
        n = new_source.shape[0]
        for name in params:
            params[name] = torch.cat((params[name], new_params[name]), dim=0)
            if name in moments:
                moments[name] = [torch.cat((t, torch.zeros_like(new_params[name])), dim=0) for t in moments[name]]
        radii = torch.cat((radii, torch.zeros(n, dtype=torch.int64)))
        source = torch.cat((source, new_source))
        kind = torch.cat((kind, new_kind))

    def prune(mask):
        nonlocal radii, source, kind
        keep = ~mask
        for name in params:
            params[name] = params[name][keep]
            if name in moments:
                moments[name] = [t[keep] for t in moments[name]]
        radii, source, kind = radii[keep], source[keep], kind[keep]

    def world():
        return torch.exp(params["scaling"]).max(dim=1).values

    # densify_and_clone
    sel = (grads >= max_grad) & (world() <= percent_dense * extent)
    postfix({n: p[sel] for n, p in params.items()}, source[sel], torch.ones(int(sel.sum()), dtype=torch.int64))
    # densify_and_split
    padded = torch.zeros(params["xyz"].shape[0], dtype=f64)
    padded[:P] = grads
    sel = (padded >= max_grad) & (world() > percent_dense * extent)
    src = source[sel]
    n = src.shape[0]
    new = {name: p[sel].repeat((2,) + (1,) * (p.dim() - 1)) for name, p in params.items()}
    new["xyz"], new["scaling"] = children(new["xyz"], new["scaling"], new["rotation"], torch.cat((noise[src, 0], noise[src, 1])))
    postfix(new, src.repeat(2), torch.cat((torch.full((n,), 2, dtype=torch.int64), torch.full((n,), 3, dtype=torch.int64))))
    prune(torch.cat((sel, torch.zeros(2 * n, dtype=torch.bool))))
    # prune
    mask = torch.sigmoid(params["opacity"]).squeeze(-1) < min_opacity
    if max_screen_size is not None:
        mask = mask | (radii > max_screen_size) | (world() > 0.1 * extent)
    prune(mask)
    P_new = source.shape[0]
    counts = tuple(int((kind == k).sum()) for k in range(4))
    zeros = (torch.zeros(P_new, dtype=f64), torch.zeros(P_new, dtype=torch.int64), torch.zeros(P_new, dtype=torch.int64))
    return {"params": params, "moments": moments, "stats": zeros, "source": source, "kind": kind, "counts": counts,
            "P_new": P_new}


def reset_opacity(opacity, moments, ceiling=0.01):
    """-> (new opacity logits, (zeros, zeros)) in float64."""
    o = torch.minimum(torch.sigmoid(opacity.to(torch.float64)), torch.full_like(opacity, ceiling, dtype=torch.float64))
    return torch.log(o / (1 - o)), tuple(torch.zeros_like(m, dtype=torch.float64) for m in moments)


# ---- seeded test scenes (shared by the CPU and the GPU tests) ---------------------------------------------------------
EXTENT, MAX_GRAD, MIN_OPACITY, MAX_SCREEN, PERCENT_DENSE = 4.0, 2e-4, 5e-3, 20, 0.01
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "aux", "frozen")  # `frozen` never stepped: no state


def shapes(P, degree):
    return {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, (degree + 1) ** 2 - 1, 3), "opacity": (P, 1), "scaling": (P, 3),
            "rotation": (P, 4), "aux": (P, 2), "frozen": (P, 3)}


def make_case(P, degree, seed=0):
    """-> (params fp32, moments fp32 (all groups but `frozen`), (grad_accum fp32, denom int32, max_radii int32), noise fp32).
    Against EXTENT = 4 the largest world scale of a Gaussian is drawn from four bands that stay clear of 0.04 (clone / split),
    0.4 (oversized) and 0.64 (children still oversized): about 40 % small, 35 % middle, 12 % in (0.4, 0.64), 13 % above 0.64;
    the mean gradient from (2.5e-4, 1e-3) for two thirds and from (1e-6, 1.5e-4) for the rest, so that about a third each
    are clone candidates, split candidates and neither; a fifth have sigmoid(opacity) in (5e-4, 4e-3) < MIN_OPACITY; one in
    eight has a radius above MAX_SCREEN, one in sixteen exactly MAX_SCREEN; one in sixteen was never seen (denom = 0, with a
    non-zero accumulated gradient in half of them); quaternion norms in [0.1, 10]; moments are non-zero normals."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * P + degree)

    def rand(*shape):
        return torch.rand(shape, generator=g, dtype=torch.float64)

    band = rand(P)
    u = rand(P)
    smax = torch.where(band < 0.40, 0.005 + 0.030 * u,
                       torch.where(band < 0.75, 0.05 + 0.30 * u, torch.where(band < 0.87, 0.45 + 0.15 * u, 0.70 + 0.80 * u)))
    scales = smax[:, None] * (0.2 + 0.8 * rand(P, 3))
    scales[torch.arange(P), torch.randint(0, 3, (P,), generator=g)] = smax
    o = torch.where(rand(P) < 0.2, 5e-4 + 3.5e-3 * rand(P), 0.01 + 0.98 * rand(P))
    q = torch.randn((P, 4), generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True) * 10.0 ** (2.0 * rand(P, 1) - 1.0)
    params = {n: torch.randn(s, generator=g, dtype=torch.float64) for n, s in shapes(P, degree).items()}
    params["scaling"], params["opacity"], params["rotation"] = torch.log(scales), torch.logit(o)[:, None], q
    params = {n: p.to(torch.float32) for n, p in params.items()}
    moments = {n: (torch.randn(p.shape, generator=g) * 1e-2, torch.rand(p.shape, generator=g) * 1e-4 + 1e-9)
               for n, p in params.items() if n != "frozen"}
    denom = torch.randint(1, 11, (P,), generator=g, dtype=torch.int32)
    mean = torch.where(rand(P) < 2.0 / 3.0, 2.5e-4 + 7.5e-4 * rand(P), 1e-6 + 1.49e-4 * rand(P))
    grad_accum = (mean * denom).to(torch.float32)
    unseen = rand(P) < 1.0 / 16.0
    denom[unseen] = 0
    grad_accum[unseen & (rand(P) < 0.5)] = 0.0
    r = rand(P)
    max_radii = torch.where(r < 1.0 / 8.0, torch.randint(MAX_SCREEN + 1, 64, (P,), generator=g),
                            torch.where(r < 3.0 / 16.0, torch.full((P,), MAX_SCREEN), torch.randint(0, MAX_SCREEN, (P,), generator=g))
                            ).to(torch.int32)
    noise = torch.randn((P, 2, 3), generator=g)
    return params, moments, (grad_accum, denom, max_radii), noise
