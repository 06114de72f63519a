"""GPU: gaussreg_amd.scene_densify (csrc/scene_densify.hip) against the float64 restatement tests/scene_densify_f64.py.

Exact (bit patterns): P_new, the four counts, source, kind; every copied row; zero moments of new rows; the statistics;
step; the stateless group; a second run; unaligned tensors.  The inputs keep a 1e-4 relative margin from every threshold
(asserted by the reference on the generated inputs), so the fp32 and the float64 classification agree.
Accuracy (children's xyz and scaling, reset_opacity), per tensor in max-norm: e_hip <= max(4 e_t32, floor), e_t32 = the
error of upstream's formula composed from stock torch fp32 ops on the same GPU, floor = one fp32 ulp of the float64
tensor's largest magnitude; every ratio is printed before it is asserted (docs/scene_densify_f64_errors.md).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import scene_densify_f64 as R
from gaussreg_amd import _lib
from gaussreg_amd.scene_densify import densify_and_prune, reset_opacity
from gaussreg_amd.scene_optim import DensifyStats, GaussianAdam

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FACTOR = 4.0
SIZES = [1, 63, 64, 65, 257, 1000, 4099]
DEGREES = [0, 1, 2, 3]
# 65 858 is the smallest P whose last Gaussian has a non-zero prefix at every level of the plan's scan:
# workgroup 257 = second round of the one-workgroup scan (carry), second workgroup of that round, second wave, second lane.
# One more, so that a kept-and-cloned Gaussian and a split one both sit there.
P_ALL_LEVELS = 256 * 256 + 256 + 64 + 3
CASES = [(P, degree) for P in SIZES for degree in DEGREES] + [(P_ALL_LEVELS, 0)]
STEP = 7.0
# the example's scene at 64 x 48: the mean screen-space gradient after 10 steps has its 99 % quantile at 6.4e-3 and its
# maximum at 1.4e-2, so this threshold clones about one Gaussian in a hundred at every densification
DENSIFY_GRAD_THRESHOLD = 6e-3


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def offset_copy(t):
    """A contiguous copy of t that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    skip = next(i for i in range(5) if (buf.data_ptr() + 4 * i) % 16 == 4)
    out = buf[skip:skip + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 or t.numel() == 0
    return out


def build(case, unaligned=False, names=R.NAMES, extra=None):
    """-> (params, opt, stats, noise) on the GPU from a make_case tuple; every group but `frozen` has state at step STEP."""
    params, moments, st, noise = case
    place = offset_copy if unaligned else (lambda t: t.clone())
    dev = torch.device("cuda")
    tensors = {n: place(params[n].to(dev)).requires_grad_(True) for n in names}
    if extra:
        tensors.update({n: t.to(dev).requires_grad_(True) for n, t in extra.items()})
    opt = GaussianAdam([{"params": [t], "lr": 1e-3, "name": n} for n, t in tensors.items()], eps=1e-15)
    for n, t in tensors.items():
        if n in moments:
            opt.state[t] = {"step": torch.tensor(STEP), "exp_avg": place(moments[n][0].to(dev)),
                            "exp_avg_sq": place(moments[n][1].to(dev))}
    stats = DensifyStats(params["xyz"].shape[0], dev)
    stats.grad_accum, stats.denom, stats.max_radii = (place(t.to(dev)) for t in st)
    return tensors, opt, stats, place(noise.to(dev))


def run(case, screen=R.MAX_SCREEN, max_grad=R.MAX_GRAD, min_opacity=R.MIN_OPACITY, **kw):
    tensors, opt, stats, noise = build(case, **kw)
    old_state = {n: opt.state.get(t) for n, t in tensors.items()}
    r = densify_and_prune(opt, stats, max_grad, min_opacity, R.EXTENT, max_screen_size=screen, percent_dense=R.PERCENT_DENSE,
                          noise=noise)
    torch.cuda.synchronize()
    return tensors, old_state, opt, stats, r


def reference(case, screen=R.MAX_SCREEN, max_grad=R.MAX_GRAD, min_opacity=R.MIN_OPACITY):
    params, moments, st, noise = case
    R.assert_margin(params, st, max_grad, min_opacity, R.EXTENT, R.PERCENT_DENSE)
    return R.densify_and_prune(params, moments, st, max_grad, min_opacity, R.EXTENT, screen, R.PERCENT_DENSE, noise)


@functools.lru_cache(maxsize=None)
def solved(P, degree):
    """One case, computed once and left unchanged: (make_case tuple, float64 reference, library run)."""
    case = R.make_case(P, degree)
    if P == P_ALL_LEVELS:  # the last Gaussian is kept and cloned, the one before it split: both use every prefix
        params, moments, (grad_accum, denom, max_radii), noise = case
        params["opacity"][-2:] = 1.0
        params["scaling"][-1], params["scaling"][-2] = -5.0, -2.0
        grad_accum[-2:], denom[-2:], max_radii[-2:] = 1.0, 1, 0
    return case, reference(case), run(case)


def check_exact(case, ref, out):
    """Every exact statement of the module docstring for one run."""
    old, old_state, opt, stats, r = out
    P = case[0]["xyz"].shape[0]
    assert r.P_new == ref["P_new"] and tuple(r.counts) == ref["counts"] and sum(r.counts) == r.P_new
    assert r.source.dtype == torch.int32 and r.kind.dtype == torch.uint8
    assert r.source.cpu().tolist() == ref["source"].tolist()
    assert r.kind.cpu().tolist() == ref["kind"].tolist()
    src, kind = r.source.long(), r.kind
    copied, child = kind <= 1, kind >= 2
    assert len(opt.param_groups) == len(old)
    for group in opt.param_groups:
        n = group["name"]
        new = group["params"][0]
        assert new is r.tensors[n] and type(new) is type(old[n]) and new.requires_grad and new.grad is None
        assert new.shape == (r.P_new,) + old[n].shape[1:] and new.is_contiguous()
        assert same_bits(new[copied], old[n][src[copied]]), n
        if n not in ("xyz", "scaling"):
            assert same_bits(new[child], old[n][src[child]]), n
        assert old[n] not in opt.state
        if old_state[n] is None:
            assert new not in opt.state, n  # a group that never stepped stays stateless
            continue
        st = opt.state[new]
        assert float(st["step"]) == STEP
        for key in ("exp_avg", "exp_avg_sq"):
            assert st[key].shape == new.shape
            assert same_bits(st[key][kind == 0], old_state[n][key][src[kind == 0]]), (n, key)
            assert not bits(st[key][kind != 0]).any(), (n, key)
    for t, dtype in ((stats.grad_accum, torch.float32), (stats.denom, torch.int32), (stats.max_radii, torch.int32)):
        assert t.shape == (r.P_new,) and t.dtype == dtype and not t.any()
    assert 0 <= r.P_new <= 2 * P


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("P", SIZES)
def test_plan_and_copies_are_exact(P, degree):
    case, ref, out = solved(P, degree)
    check_exact(case, ref, out)
    if P >= 257:
        assert all(c > 0 for c in ref["counts"]) and ref["counts"][0] < P


def test_every_scan_level_carries_a_prefix():
    case, ref, out = solved(P_ALL_LEVELS, 0)
    check_exact(case, ref, out)
    # their rows used the carry of the scan's second round, a workgroup prefix, a wave prefix and a lane prefix
    rows = list(zip(out[4].source.cpu().tolist(), out[4].kind.cpu().tolist()))
    for want in ((P_ALL_LEVELS - 1, 0), (P_ALL_LEVELS - 1, 1), (P_ALL_LEVELS - 2, 2), (P_ALL_LEVELS - 2, 3)):
        assert want in rows[-1:] + [rows[i - 1] for i in np.cumsum(out[4].counts)], want


def children_t32(case, src, k):
    """Upstream's split arithmetic from stock torch fp32 ops on the GPU for the child rows (src, k)."""
    params, _, _, noise = case
    dev = torch.device("cuda")
    xyz, scaling, rotation = (params[n].to(dev)[src] for n in ("xyz", "scaling", "rotation"))
    return R.children(xyz, scaling, rotation, noise.to(dev)[src, k])


def bound(label, got, t32, f64):
    e_hip, e_t32 = float((got.double() - f64).abs().max()), float((t32.double() - f64).abs().max())
    floor = float(np.spacing(np.float32(f64.abs().max().item())))
    ratio = e_hip / e_t32 if e_t32 > 0 else (0.0 if e_hip == 0 else float("inf"))
    print(f"{label} e_hip {e_hip:.3e} e_t32 {e_t32:.3e} ratio {ratio:.3f} floor {floor:.3e}"
          f"{' (floor binds)' if floor > FACTOR * e_t32 else ''}")
    return e_hip <= max(FACTOR * e_t32, floor), (label, e_hip, e_t32, floor)


@pytest.mark.parametrize("P,degree", CASES)
def test_children_accuracy(P, degree):
    case, ref, out = solved(P, degree)
    r = out[4]
    child = (r.kind >= 2).cpu()
    if not bool(child.any()):
        assert not bool((ref["kind"] >= 2).any())
        return
    src, k = ref["source"][child], ref["kind"][child] - 2
    t32_xyz, t32_scaling = children_t32(case, src.cuda(), k.cuda())
    results = [bound(f"P={P} degree={degree} xyz    ", r.tensors["xyz"].detach()[child.cuda()].cpu(), t32_xyz.cpu(),
                     ref["params"]["xyz"][child]),
               bound(f"P={P} degree={degree} scaling", r.tensors["scaling"].detach()[child.cuda()].cpu(), t32_scaling.cpu(),
                     ref["params"]["scaling"][child])]
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]


@pytest.mark.parametrize("P", [1, 65, 4099])
def test_reset_opacity(P):
    case = R.make_case(P, 0)
    tensors, opt, _, _ = build(case)
    before = {n: t.detach().clone() for n, t in tensors.items()}
    moments_before = {n: {k: v.clone() for k, v in opt.state[t].items()} for n, t in tensors.items() if t in opt.state}
    p = reset_opacity(opt, 0.01)
    assert p is tensors["opacity"]
    want, _ = R.reset_opacity(case[0]["opacity"], case[1]["opacity"])
    o = torch.sigmoid(case[0]["opacity"].cuda()).clamp(max=0.01)
    t32 = torch.log(o / (1 - o))
    ok, info = bound(f"reset_opacity P={P}", p.detach().cpu(), t32.cpu(), want)
    assert ok, info
    st = opt.state[p]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == STEP
    for n, t in tensors.items():
        if n != "opacity":
            assert same_bits(t, before[n])
            if t in opt.state:
                assert same_bits(opt.state[t]["exp_avg"], moments_before[n]["exp_avg"])
                assert same_bits(opt.state[t]["exp_avg_sq"], moments_before[n]["exp_avg_sq"])


def all_bits(out):
    _, _, opt, _, r = out
    items = [r.source, r.kind.to(torch.int32)]
    for group in opt.param_groups:
        p = group["params"][0]
        items.append(bits(p))
        if p in opt.state:
            items += [bits(opt.state[p]["exp_avg"]), bits(opt.state[p]["exp_avg_sq"])]
    return items


@pytest.mark.parametrize("P,degree", [(65, 1), (4099, 3)])
def test_second_run_and_unaligned_tensors_give_the_same_bits(P, degree):
    case, _, out = solved(P, degree)
    first = all_bits(out)
    for kw in ({}, {"unaligned": True}):
        other = all_bits(run(case, **kw))
        assert len(other) == len(first)
        for a, b in zip(first, other):
            assert torch.equal(a, b), kw


def test_more_groups_than_one_launch_holds():
    case = R.make_case(257, 1)
    extra = {f"extra{i}": torch.randn((257, 5), generator=torch.Generator().manual_seed(i)) for i in range(3)}
    tensors, opt, stats, noise = build(case, extra=extra)
    assert len(opt.param_groups) > _lib.GS_ADAM_MAX_GROUPS
    r = densify_and_prune(opt, stats, R.MAX_GRAD, R.MIN_OPACITY, R.EXTENT, R.MAX_SCREEN, noise=noise)
    want = solved(257, 1)[2][4]
    assert torch.equal(r.source, want.source) and torch.equal(r.kind, want.kind)
    for n in R.NAMES:
        assert same_bits(r.tensors[n], want.tensors[n]), n
    for n in extra:
        assert same_bits(r.tensors[n], tensors[n][r.source.long()]), n


def edited(P, degree, **changes):
    """make_case with whole tensors replaced: scaling / opacity (params), grad_accum / denom / max_radii (statistics)."""
    params, moments, st, noise = R.make_case(P, degree)
    params, st = dict(params), list(st)
    for key, value in changes.items():
        if key in params:
            params[key] = value.to(torch.float32)
        else:
            st[("grad_accum", "denom", "max_radii").index(key)] = value
    return params, moments, tuple(st), noise


def test_nothing_selected_nothing_pruned():
    P = 1000
    case = edited(P, 2, scaling=torch.full((P, 3), -3.0), opacity=torch.full((P, 1), 1.0), grad_accum=torch.zeros(P),
                  max_radii=torch.zeros(P, dtype=torch.int32))
    old, old_state, opt, stats, r = out = run(case)
    check_exact(case, reference(case), out)
    assert r.P_new == P and tuple(r.counts) == (P, 0, 0, 0)
    for group in opt.param_groups:
        n, new = group["name"], group["params"][0]
        assert same_bits(new, old[n]) and new is not old[n]
        if old_state[n]:
            assert same_bits(opt.state[new]["exp_avg"], old_state[n]["exp_avg"])
            assert same_bits(opt.state[new]["exp_avg_sq"], old_state[n]["exp_avg_sq"])


def test_everything_pruned():
    P = 257
    case = edited(P, 1, opacity=torch.full((P, 1), -9.0))
    _, _, opt, stats, r = out = run(case)
    check_exact(case, reference(case), out)
    assert r.P_new == 0 and tuple(r.counts) == (0, 0, 0, 0) and r.source.shape == (0,)
    shapes = R.shapes(0, 1)
    for group in opt.param_groups:
        p = group["params"][0]
        assert tuple(p.shape) == shapes[group["name"]]
        if p in opt.state:
            assert opt.state[p]["exp_avg"].shape == p.shape
    assert stats.denom.shape == (0,)


def test_everything_cloned():
    P = 1000
    case = edited(P, 0, scaling=torch.full((P, 3), -5.0), opacity=torch.full((P, 1), 1.0), grad_accum=torch.full((P,), 1.0),
                  denom=torch.ones(P, dtype=torch.int32), max_radii=torch.zeros(P, dtype=torch.int32))
    _, _, _, _, r = out = run(case)
    check_exact(case, reference(case), out)
    assert tuple(r.counts) == (P, P, 0, 0)
    assert r.source.cpu().tolist() == list(range(P)) * 2


def test_everything_split():
    P = 1000
    case = edited(P, 0, scaling=torch.full((P, 3), -2.0), opacity=torch.full((P, 1), 1.0), grad_accum=torch.full((P,), 1.0),
                  denom=torch.ones(P, dtype=torch.int32), max_radii=torch.zeros(P, dtype=torch.int32))
    _, _, _, _, r = out = run(case)
    check_exact(case, reference(case), out)
    assert tuple(r.counts) == (0, 0, P, P)
    assert r.kind.cpu().tolist() == [2] * P + [3] * P


def test_without_max_screen_size_radii_and_world_size_are_ignored():
    case, _, with_screen = solved(1000, 1)
    out = run(case, screen=None)
    ref = reference(case, screen=None)
    check_exact(case, ref, out)
    params, _, st, _ = case
    big = (st[2] > R.MAX_SCREEN) | (torch.exp(params["scaling"]).max(1).values > 0.1 * R.EXTENT)
    low = torch.sigmoid(params["opacity"][:, 0]) < R.MIN_OPACITY
    emitted = set(out[4].source.cpu().tolist())
    assert bool((big & ~low).any()) and all(i in emitted for i in torch.nonzero(big & ~low)[:, 0].tolist())
    assert out[4].P_new > with_screen[4].P_new


def test_threshold_comparisons():
    """g == max_grad is selected (>=); radius == max_screen_size is kept (strict >); denom = 0 is never selected; a clone
    candidate of low opacity emits nothing."""
    P = 6
    max_grad = 2.0 ** -12
    scaling = torch.full((P, 3), -5.0)  # small: clone candidates
    opacity = torch.full((P, 1), 1.0)
    grad_accum = torch.tensor([2.0 ** -10, 2.0 ** -10 * (1 - 2.0 ** -10), 5.0, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10])
    denom = torch.tensor([4, 4, 0, 4, 4, 4], dtype=torch.int32)
    max_radii = torch.tensor([0, 0, 0, R.MAX_SCREEN, R.MAX_SCREEN + 1, 0], dtype=torch.int32)
    opacity[5] = -9.0
    case = edited(P, 0, scaling=scaling, opacity=opacity, grad_accum=grad_accum, denom=denom, max_radii=max_radii)
    _, _, _, _, r = out = run(case, max_grad=max_grad)
    check_exact(case, reference(case, max_grad=max_grad), out)
    rows = list(zip(r.source.cpu().tolist(), r.kind.cpu().tolist()))
    # 0: on the threshold, cloned; 1: just below, kept only; 2: never seen, kept only; 3: radius on the limit, kept and
    # cloned; 4: radius above it, the original goes and its clone (radius 0) stays; 5: low opacity, nothing
    assert rows == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (3, 1), (4, 1)]


def test_errors_leave_everything_in_place():
    case = R.make_case(65, 1)
    args = (R.MAX_GRAD, R.MIN_OPACITY, R.EXTENT)

    def refused(mutate, match, names=R.NAMES):
        tensors, opt, stats, noise = build(case, names=names)
        kw = {"noise": noise}
        mutate(tensors, opt, stats, kw)
        before = [g["params"][0] for g in opt.param_groups]
        stat_tensors = (stats.grad_accum, stats.denom, stats.max_radii)
        with pytest.raises(ValueError, match=match):
            densify_and_prune(opt, stats, *args, **kw)
        assert all(g["params"][0] is t for g, t in zip(opt.param_groups, before))
        assert all(a is b for a, b in zip((stats.grad_accum, stats.denom, stats.max_radii), stat_tensors))

    for missing in R.ROLES:
        refused(lambda *a: None, f"no param group named {missing}", names=[n for n in R.NAMES if n != missing])
    refused(lambda t, o, s, kw: o.param_groups[0].__setitem__("params", [torch.zeros((65, 4), device="cuda")]), "xyz: shape")
    refused(lambda t, o, s, kw: o.param_groups[1].__setitem__("params", [t["f_dc"].detach().double()]), "dtype")
    refused(lambda t, o, s, kw: o.param_groups[1].__setitem__("params", [t["f_dc"].detach().cpu()]), "cpu")
    refused(lambda t, o, s, kw: o.param_groups[2].__setitem__("params", [torch.zeros((65, 4, 6), device="cuda")[:, :, :3]]),
            "not contiguous")
    refused(lambda t, o, s, kw: o.param_groups[6].__setitem__("params", [torch.zeros((64, 2), device="cuda")]), "leading dimension")
    refused(lambda t, o, s, kw: setattr(s, "denom", s.denom[:64].contiguous()), "stats.denom: shape")
    refused(lambda t, o, s, kw: setattr(s, "grad_accum", s.grad_accum.double()), "stats.grad_accum")
    refused(lambda t, o, s, kw: setattr(s, "max_radii", s.max_radii.cpu()), "stats.max_radii")
    refused(lambda t, o, s, kw: kw.__setitem__("noise", kw["noise"][:, :1].contiguous()), "noise")
    refused(lambda t, o, s, kw: kw.__setitem__("noise", kw["noise"].double()), "noise")
    refused(lambda t, o, s, kw: kw.__setitem__("noise", kw["noise"].cpu()), "noise")
    refused(lambda t, o, s, kw: o.state[t["xyz"]].__setitem__("exp_avg", torch.zeros((64, 3), device="cuda")), "exp_avg")
    with pytest.raises(ValueError, match="GaussianAdam"):
        tensors, opt, stats, noise = build(case)
        densify_and_prune(torch.optim.Adam(list(tensors.values())), stats, *args)
    with pytest.raises(ValueError, match="ceiling"):
        reset_opacity(build(case)[1], 1.5)


def test_c_abi_refuses_bad_arguments():
    L = _lib.lib()
    dev = torch.device("cuda")
    P = 8
    f = torch.zeros((P, 3), device=dev)
    i32 = torch.zeros(2 * P, dtype=torch.int32, device=dev)
    u8 = torch.zeros(2 * P, dtype=torch.uint8, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    stream = _lib.stream_ptr(dev)
    assert L.gr_gs_densify_plan_workspace_bytes(-1) == 0 and L.gr_gs_densify_plan_workspace_bytes(P) > 0
    plan = lambda scaling, n: L.gr_gs_densify_plan(scaling, _lib.ptr(f), _lib.ptr(f), _lib.ptr(i32), _lib.ptr(i32), n, 1.0, 0.1, 1.0,
                                                   0.01, 0, 0.0, _lib.ptr(i32), _lib.ptr(u8), _lib.ptr(i32), None, _lib.ptr(ws), 4096,
                                                   stream)
    assert plan(_lib.ptr(None), P) == -1 and b"null" in L.gr_last_error()
    assert plan(_lib.ptr(f), -1) == -1
    assert L.gr_gs_densify_plan(_lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(i32), _lib.ptr(i32), P, 1.0, 0.1, 1.0, 0.01, 0, 0.0,
                                _lib.ptr(i32), _lib.ptr(u8), _lib.ptr(i32), None, _lib.ptr(ws), 8, stream) == -3
    h = _lib.host_i64([7] * 4)
    assert L.gr_gs_densify_plan(None, None, None, None, None, 0, 1.0, 0.1, 1.0, 0.01, 0, 0.0, None, None, None, h, None, 0,
                                stream) == 0 and list(h[:4]) == [0, 0, 0, 0]

    def apply(group, n=P, n_new=P, roles=(f, f, f), source=i32):
        table = (_lib.GsDensifyGroup * 1)(group)
        return L.gr_gs_densify_apply(table, 1, n, n_new, _lib.ptr(source), _lib.ptr(u8), *[_lib.ptr(t) for t in roles], stream)

    out = torch.full((P, 3), 5.0, device=dev)
    G = _lib.GsDensifyGroup
    z = _lib.ptr(None)
    assert apply(G(_lib.ptr(f), _lib.ptr(out), z, z, z, z, 3, 0), n=-1) == -1
    assert apply(G(_lib.ptr(f), _lib.ptr(out), z, z, z, z, 3, 0), n_new=2 * P + 1) == -1
    assert apply(G(z, _lib.ptr(out), z, z, z, z, 3, 0)) == -1
    assert apply(G(_lib.ptr(f), _lib.ptr(out), _lib.ptr(f), z, z, z, 3, 0)) == -1  # some moment pointers but not all
    assert apply(G(_lib.ptr(f), _lib.ptr(out), z, z, z, z, 3, 1), roles=(f, None, f)) == -1 and b"xyz" in L.gr_last_error()
    assert apply(G(_lib.ptr(f), _lib.ptr(out), z, z, z, z, 3, 0), source=None) == -1
    assert apply(G(_lib.ptr(f), _lib.ptr(out), z, z, z, z, 1 << 30, 0)) == -1 and b"32-bit" in L.gr_last_error()
    assert apply(G(_lib.ptr(f), _lib.ptr(out), z, z, z, z, 3, 0), n_new=0) == 0  # launches nothing
    assert apply(G(z, z, z, z, z, z, 0, 0)) == 0                                 # K = 0: skipped
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())  # no refused or empty call wrote anything


def test_finetune_example_with_densification():
    spec = importlib.util.spec_from_file_location("finetune_scene", os.path.join(ROOT, "examples", "finetune_scene.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    P, steps = 2000, 40
    lines = []
    r = example.finetune(points=P, views=4, steps=steps, width=64, height=48, optimizer="hip", densify_every=10,
                         densify_grad_threshold=DENSIFY_GRAD_THRESHOLD, log=lines.append)
    print(f"finetune + densify: loss {r['before'][0]:.6f} -> {r['after'][0]:.6f}, counts {r['counts']}")
    assert r["after"][0] < r["before"][0]
    events = r["densifications"]
    assert [e["step"] for e in events] == [10, 20, 30]
    assert any(e["P_new"] != e["P_old"] for e in events)
    assert r["counts"] == [e["P_new"] for e in events]
    assert sum("Gaussians" in line for line in lines) == len(events)
    opt, count = r["optimizer"], events[-1]["P_new"]
    for group in opt.param_groups:
        p = group["params"][0]
        assert p.shape[0] == count and p is r["raw"][group["name"]]
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
    st = r["stats"]
    assert st.grad_accum.shape == (count,) and st.denom.shape == (count,) and st.max_radii.shape == (count,)
    # one more step on the rebuilt scene
    raw = r["raw"]
    means2D = torch.zeros((1, count, 3), device="cuda", requires_grad=True)
    image, radii = example.render(raw, r["one_view"][0], means2D)
    image.sum().backward()
    before = raw["xyz"].detach().clone()
    opt.step(visibility=radii)
    torch.cuda.synchronize()
    assert not same_bits(before, raw["xyz"])
