"""GPU: gaussreg_amd.scene_optim (csrc/scene_optim.hip) against the float64 restatement tests/scene_optim_f64.py.

Bound.  Per tensor (parameter, exp_avg, exp_avg_sq of every group), in max-norm: e_hip = max |library - float64| and
e_t32 = max |torch.optim.Adam(foreach=False) in fp32 on the same device, same inputs - float64|.  Asserted:
e_hip <= max(4 e_t32, floor), floor = one fp32 ulp of the float64 tensor's largest magnitude.  The same rule bounds
grad_accum of the statistics against torch's fp32 `norm` composition.  Every ratio e_hip / e_t32 is printed before it is
asserted (docs/scene_optim_f64_errors.md has the recorded table).  Everything else is exact: bit patterns are compared.
"""
import copy
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import scene_optim_f64 as R
from gaussreg_amd import _lib
from gaussreg_amd.scene_optim import DensifyStats, GaussianAdam

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FACTOR = 4.0
SIZES = [1, 63, 64, 65, 257, 1000, 4099]
DEGREES = [0, 1, 2, 3]
# upstream's groups, plus `aux` (K = 2: a row length without a compile-time divisor) and `frozen` (never has a gradient)
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3, "aux": 1e-2,
       "frozen": 1e-2}
NAMES = list(LRS)


def shapes(P, degree):
    return {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, (degree + 1) ** 2 - 1, 3), "opacity": (P, 1), "scaling": (P, 3),
            "rotation": (P, 4), "aux": (P, 2), "frozen": (P, 3)}


def initial(P, degree, seed=0):
    rng = np.random.default_rng(seed)
    return {n: rng.normal(0.0, 1.0, s).astype(np.float32) for n, s in shapes(P, degree).items()}


def grads_of(P, degree, step):
    """Seeded per group and step; `frozen` has none; `rotation` has none at step 2 (its count then lags the others)."""
    out = {}
    for i, (n, s) in enumerate(shapes(P, degree).items()):
        out[n] = None if n == "frozen" or (n == "rotation" and step == 2) else R.seeded_grad(s, 1000 * step + 10 * i + degree)
    return out


def lrs_of(step):
    return {n: lr * 0.97 ** step for n, lr in LRS.items()}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def make_optimizer(kind, init, **kw):
    params = {n: torch.from_numpy(a).cuda().requires_grad_(True) for n, a in init.items()}
    groups = [{"params": [params[n]], "lr": LRS[n], "name": n} for n in NAMES if n in params]
    if kind == "hip":
        return params, GaussianAdam(groups, eps=1e-15, **kw)
    return params, torch.optim.Adam(groups, eps=1e-15, foreach=False, **kw)


def run_steps(kind, params, opt, P, degree, first, last, visibility=None):
    for s in range(first, last):
        g, lrs = grads_of(P, degree, s), lrs_of(s)
        for group in opt.param_groups:
            group["lr"] = lrs[group["name"]]
        for n, p in params.items():
            p.grad = None if g[n] is None else torch.from_numpy(g[n]).cuda()
        if kind == "hip":
            opt.step(visibility=None if visibility is None else visibility(s))
        else:
            opt.step()


def state_of(params, opt):
    """name -> (p, exp_avg, exp_avg_sq) as float64 numpy (zeros where the optimiser holds no state yet)."""
    out = {}
    for n, p in params.items():
        st = opt.state.get(p, {})
        out[n] = tuple(t.detach().double().cpu().numpy() for t in
                       (p, st.get("exp_avg", torch.zeros_like(p)), st.get("exp_avg_sq", torch.zeros_like(p))))
    return out


def f64_run(init, P, degree, steps, visible=None):
    ref = R.AdamF64([init[n] for n in NAMES])
    for s in range(steps):
        g, lrs = grads_of(P, degree, s), lrs_of(s)
        ref.step([g[n] for n in NAMES], [lrs[n] for n in NAMES], None if visible is None else visible(s))
    return {n: (ref.p[i], ref.m[i], ref.v[i]) for i, n in enumerate(NAMES)}


def check_bound(label, got, t32, f64):
    """Prints every ratio, then asserts the bound for all of them; -> the worst ratio."""
    failures, worst = [], 0.0
    for n in NAMES:
        for what, a, b, c in zip(("p", "exp_avg", "exp_avg_sq"), got[n], t32[n], f64[n]):
            if c.size == 0:
                continue
            e_hip, e_t32 = np.abs(a - c).max(), np.abs(b - c).max()
            floor = float(np.spacing(np.float32(np.abs(c).max())))
            bound = max(FACTOR * e_t32, floor)
            ratio = e_hip / e_t32 if e_t32 > 0 else (0.0 if e_hip == 0 else float("inf"))
            print(f"{label} {n:9s} {what:10s} e_hip {e_hip:.3e} e_t32 {e_t32:.3e} ratio {ratio:.3f} floor {floor:.3e}"
                  f"{' (floor binds)' if floor > FACTOR * e_t32 else ''}")
            worst = max(worst, ratio if np.isfinite(ratio) else 0.0)
            if not e_hip <= bound:
                failures.append((n, what, e_hip, e_t32, floor))
    assert not failures, failures
    return worst


@functools.lru_cache(maxsize=None)
def dense_case(P, degree):
    """After 1 and after 20 steps: (library, torch fp32, float64) states."""
    init = initial(P, degree)
    out = {}
    hip, t32 = make_optimizer("hip", init), make_optimizer("t32", init)
    for first, last in ((0, 1), (1, 20)):
        run_steps("hip", *hip, P, degree, first, last)
        run_steps("t32", *t32, P, degree, first, last)
        out[last] = (state_of(*hip), state_of(*t32), f64_run(init, P, degree, last))
    return out


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("P", SIZES)
def test_dense_accuracy(P, degree):
    case = dense_case(P, degree)
    for steps in (1, 20):
        check_bound(f"dense P={P} deg={degree} steps={steps}", *case[steps])


def mask_of(P, step, frac=0.4):
    rng = np.random.default_rng(77 + step)
    m = rng.random(P) < frac
    if P > 1:
        m[0], m[-1] = True, False
    return m


@pytest.mark.parametrize("P,degree", [(1, 3), (65, 1), (257, 2), (4099, 3)])
def test_masked_accuracy(P, degree):
    """The masked step against the float64 definition; the fp32 yardstick is torch's dense step composed with the same
    definition (rows restored where the mask is off), which is what torch code without this kernel would do."""
    init = initial(P, degree)
    hip = make_optimizer("hip", init)
    run_steps("hip", *hip, P, degree, 0, 20, visibility=lambda s: torch.from_numpy(mask_of(P, s)).cuda())
    params, opt = make_optimizer("t32", init)
    for s in range(20):
        keep = ~torch.from_numpy(mask_of(P, s)).cuda()
        before = {n: tuple(t.clone() for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]))
                  for n, p in params.items() if opt.state.get(p)}
        run_steps("t32", params, opt, P, degree, s, s + 1)
        with torch.no_grad():
            for n, p in params.items():
                st = opt.state.get(p)
                if st:
                    old = before.get(n, (torch.from_numpy(init[n]).cuda(), torch.zeros_like(p), torch.zeros_like(p)))
                    for t, o in zip((p, st["exp_avg"], st["exp_avg_sq"]), old):
                        t[keep] = o[keep]
    check_bound(f"masked P={P} deg={degree} steps=20", state_of(*hip), state_of(params, opt),
                f64_run(init, P, degree, 20, visible=lambda s: mask_of(P, s)))


def snapshot(params, opt):
    return {n: tuple(t.detach().clone() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])) if opt.state.get(p)
            else (p.detach().clone(),) for n, p in params.items()}


def assert_same_snapshots(a, b):
    for n in a:
        assert len(a[n]) == len(b[n])
        for x, y in zip(a[n], b[n]):
            assert same_bits(x, y), n


@pytest.mark.parametrize("P,degree", [(65, 1), (1000, 3)])
def test_invisible_rows_keep_their_bits(P, degree):
    init = initial(P, degree)
    params, opt = make_optimizer("hip", init)
    run_steps("hip", params, opt, P, degree, 0, 2)  # non-trivial moments
    for s in range(2, 5):
        before = snapshot(params, opt)
        m = mask_of(P, s)
        run_steps("hip", params, opt, P, degree, s, s + 1, visibility=lambda _: torch.from_numpy(m).cuda())
        after = snapshot(params, opt)
        off, on = torch.from_numpy(~m).cuda(), torch.from_numpy(m).cuda()
        g = grads_of(P, degree, s)
        for n in NAMES:
            for x, y in zip(before[n], after[n]):
                assert same_bits(x[off], y[off]), (n, s)
            if g[n] is not None and before[n][0].numel() and len(before[n]) == 3:
                assert not same_bits(before[n][1][on], after[n][1][on]), (n, s)  # visible rows did move


@pytest.mark.parametrize("P,degree", [(63, 2), (1000, 3)])
def test_mask_forms_agree_bit_for_bit(P, degree):
    init = initial(P, degree)
    rng = np.random.default_rng(3)
    results = {}
    for V in (1, 3):
        radii = rng.integers(-1, 4, (V, P)).astype(np.int32)
        radii[:, P // 2] = 0
        byte = (radii > 0).any(0)
        forms = {"radii": torch.from_numpy(radii).cuda(), "bool": torch.from_numpy(byte).cuda(),
                 "uint8": torch.from_numpy(byte.astype(np.uint8) * 7).cuda()}  # any non-zero byte is "visible"
        if V == 1:
            forms["radii1d"] = torch.from_numpy(radii[0]).cuda()
        for name, vis in forms.items():
            params, opt = make_optimizer("hip", init)
            run_steps("hip", params, opt, P, degree, 0, 3, visibility=lambda _: vis)
            results[(V, name)] = snapshot(params, opt)
        for name in forms:
            assert_same_snapshots(results[(V, "bool")], results[(V, name)])
    # all ones == no mask == a second run of the same
    runs = []
    for vis in (None, torch.ones(P, dtype=torch.bool, device="cuda"), torch.ones((3, P), dtype=torch.int32, device="cuda"), None):
        params, opt = make_optimizer("hip", init)
        run_steps("hip", params, opt, P, degree, 0, 3, visibility=None if vis is None else (lambda _: vis))
        runs.append(snapshot(params, opt))
    for r in runs[1:]:
        assert_same_snapshots(runs[0], r)


def test_zero_lr_and_zero_gradient():
    P, degree = 257, 1
    init = initial(P, degree)
    params, opt = make_optimizer("hip", init)
    g = grads_of(P, degree, 0)
    for group in opt.param_groups:
        group["lr"] = 0.0 if group["name"] in ("xyz", "f_rest") else LRS[group["name"]]
    for n, p in params.items():
        p.grad = None if g[n] is None else torch.from_numpy(g[n]).cuda()
    opt.step()
    for n in ("xyz", "f_rest"):
        assert same_bits(params[n], torch.from_numpy(init[n]).cuda()), n
        assert opt.state[params[n]]["exp_avg"].abs().max() > 0 and opt.state[params[n]]["exp_avg_sq"].max() > 0
    assert not same_bits(params["scaling"], torch.from_numpy(init["scaling"]).cuda())
    # zero gradient on zero state: nothing moves
    params, opt = make_optimizer("hip", init)
    for p in params.values():
        p.grad = torch.zeros_like(p)
    opt.step()
    for n, p in params.items():
        assert same_bits(p, torch.from_numpy(init[n]).cuda()), n
        for k in ("exp_avg", "exp_avg_sq"):
            assert same_bits(opt.state[p][k], torch.zeros_like(p)), (n, k)


@pytest.mark.parametrize("P,degree", [(65, 3), (4099, 2)])
def test_permutation_equivariance(P, degree):
    init = initial(P, degree)
    perm = np.random.default_rng(11).permutation(P)
    m = mask_of(P, 0)

    def run(order):
        params = {n: torch.from_numpy(a[order]).cuda().requires_grad_(True) for n, a in init.items()}
        opt = GaussianAdam([{"params": [params[n]], "lr": LRS[n], "name": n} for n in NAMES], eps=1e-15)
        for s in range(3):
            g = grads_of(P, degree, s)
            for n, p in params.items():
                p.grad = None if g[n] is None else torch.from_numpy(g[n][order]).cuda()
            opt.step(visibility=torch.from_numpy(m[order]).cuda() if s == 1 else None)
        return snapshot(params, opt)

    straight, permuted = run(np.arange(P)), run(perm)
    idx = torch.from_numpy(perm).cuda()
    for n in NAMES:
        for x, y in zip(straight[n], permuted[n]):
            assert same_bits(x[idx], y), n


def test_null_gradient_and_empty_group_through_the_c_abi():
    P = 130
    L = _lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    t = [torch.randn((P, 3), generator=gen, device="cuda") for _ in range(4)]
    t[3].abs_()
    before = [x.clone() for x in t]
    table = (_lib.GsAdamGroup * 3)(
        _lib.GsAdamGroup(_lib.ptr(t[0]), None, _lib.ptr(t[2]), _lib.ptr(t[3]), 1e-2, 3),           # no gradient: skipped
        _lib.GsAdamGroup(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), 1e-2, 0),  # K = 0: skipped
        _lib.GsAdamGroup(None, None, None, None, 1e-2, 0))
    _lib.check(L.gr_gs_adam_step(table, 3, P, 0.9, 0.999, 1e-15, 0.1, 0.001, None, None, 0, _lib.stream_ptr(t[0].device)))
    torch.cuda.synchronize()
    for a, b in zip(t, before):
        assert same_bits(a, b)
    # both visibility forms at once, too many groups, an element count past the 32-bit index: refused, nothing launched
    mask = torch.ones(P, dtype=torch.uint8, device="cuda")
    radii = torch.ones(P, dtype=torch.int32, device="cuda")
    one = (_lib.GsAdamGroup * 1)(_lib.GsAdamGroup(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), 1e-2, 3))
    stream = _lib.stream_ptr(t[0].device)
    assert L.gr_gs_adam_step(one, 1, P, 0.9, 0.999, 1e-15, 0.1, 0.001, _lib.ptr(mask), _lib.ptr(radii), 1, stream) != 0
    assert L.gr_gs_adam_step(one, 9, P, 0.9, 0.999, 1e-15, 0.1, 0.001, None, None, 0, stream) != 0
    assert L.gr_gs_adam_step(one, 1, (1 << 31) - 1, 0.9, 0.999, 1e-15, 0.1, 0.001, None, None, 0, stream) != 0
    assert b"32-bit" in L.gr_last_error()
    torch.cuda.synchronize()
    for a, b in zip(t, before):
        assert same_bits(a, b)


def test_unaligned_views_take_the_element_path():
    """Tensors that start 4 bytes into an allocation (contiguous, but not 16-byte aligned) give the same bits."""
    P, degree = 257, 3
    init = initial(P, degree)
    aligned = make_optimizer("hip", init)
    run_steps("hip", *aligned, P, degree, 0, 2)
    params = {}
    for n, a in init.items():
        buf = torch.zeros(a.size + 1, device="cuda")
        buf[1:] = torch.from_numpy(a).cuda().flatten()
        params[n] = buf[1:].view(a.shape).requires_grad_(True)
        assert params[n].is_contiguous() and (params[n].data_ptr() % 16 != 0 or a.size == 0)
    opt = GaussianAdam([{"params": [params[n]], "lr": LRS[n], "name": n} for n in NAMES], eps=1e-15)
    run_steps("hip", params, opt, P, degree, 0, 2)
    assert_same_snapshots(snapshot(*aligned), snapshot(params, opt))


@pytest.mark.parametrize("direction", ["torch_to_hip", "hip_to_torch"])
def test_state_dict_round_trip(direction):
    P, degree = 257, 2
    init = initial(P, degree)
    kinds = ("t32", "hip") if direction == "torch_to_hip" else ("hip", "t32")
    p1, o1 = make_optimizer(kinds[0], init)
    run_steps(kinds[0], p1, o1, P, degree, 0, 3)
    p2, o2 = make_optimizer(kinds[1], {n: p.detach().cpu().numpy() for n, p in p1.items()})
    o2.load_state_dict(copy.deepcopy(o1.state_dict()))
    for n in NAMES:
        if n != "frozen":
            st1, st2 = o1.state[p1[n]], o2.state[p2[n]]
            assert int(st1["step"]) == int(st2["step"]) == (2 if n == "rotation" else 3)
            assert same_bits(st1["exp_avg"], st2["exp_avg"]) and same_bits(st1["exp_avg_sq"], st2["exp_avg_sq"])
    run_steps(kinds[1], p2, o2, P, degree, 3, 6)
    t32 = make_optimizer("t32", init)
    run_steps("t32", *t32, P, degree, 0, 6)
    check_bound(f"state_dict {direction}", state_of(p2, o2), state_of(*t32), f64_run(init, P, degree, 6))


def test_lr_scheduler_drives_the_step():
    P = 64
    p = torch.ones((P, 3), device="cuda", requires_grad=True)
    opt = GaussianAdam([{"params": [p], "lr": 0.1, "name": "xyz"}])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    moved = []
    for _ in range(3):
        before = p.detach().clone()
        p.grad = torch.ones_like(p)
        opt.step()
        sched.step()
        moved.append((before - p.detach()).max().item())
    assert moved == pytest.approx([0.1, 0.05, 0.025], rel=1e-4)


def _stats_inputs(P, V, seed):
    rng = np.random.default_rng(seed)
    grad = (rng.normal(0.0, 1.0, (V, P, 3)) * 10.0 ** rng.uniform(-6, -2, (V, P, 1))).astype(np.float32)
    radii = rng.integers(-1, 40, (V, P)).astype(np.int32)
    radii[rng.random((V, P)) < 0.4] = 0
    return grad, radii


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("P", [1, 65, 4099])
def test_densify_stats(P, V):
    st, one, t_acc = DensifyStats(P, "cuda"), DensifyStats(P, "cuda"), torch.zeros(P, device="cuda")
    acc, den, rad = np.zeros(P), np.zeros(P, np.int64), np.zeros(P, np.int64)
    for call in range(2):  # the second call accumulates onto the first
        grad, radii = _stats_inputs(P, V, 10 * P + call)
        g, r = torch.from_numpy(grad).cuda(), torch.from_numpy(radii).cuda()
        st.update(g, r)
        for v in range(V):
            one.update(g[v], r[v])  # upstream's (P, 3) and (P,) of one camera
            t_acc = t_acc + torch.where(r[v] > 0, g[v, :, :2].norm(dim=-1), torch.zeros((), device="cuda"))
        acc, den, rad = R.densify_stats(acc, den, rad, grad, radii)
    assert np.array_equal(st.denom.cpu().numpy(), den) and np.array_equal(st.max_radii.cpu().numpy(), rad)
    for a, b in ((st.grad_accum, one.grad_accum), (st.denom, one.denom), (st.max_radii, one.max_radii)):
        assert same_bits(a, b)
    e_hip = np.abs(st.grad_accum.double().cpu().numpy() - acc).max()
    e_t32 = np.abs(t_acc.double().cpu().numpy() - acc).max()
    floor = float(np.spacing(np.float32(np.abs(acc).max())))
    print(f"stats P={P} V={V} e_hip {e_hip:.3e} e_t32 {e_t32:.3e} ratio {e_hip / e_t32 if e_t32 else 0.0:.3f} floor {floor:.3e}"
          f"{' (floor binds)' if floor > FACTOR * e_t32 else ''}")
    assert e_hip <= max(FACTOR * e_t32, floor)
    want = acc / np.maximum(den, 1)
    assert np.allclose(st.mean_grad().cpu().numpy(), want, rtol=1e-5, atol=0)
    st.reset()
    assert not st.grad_accum.any() and not st.denom.any() and not st.max_radii.any()


@pytest.mark.parametrize("index", ["subset", "repeated"])
def test_reindex(index):
    P, degree = 257, 1
    init = initial(P, degree)
    params, opt = make_optimizer("hip", init)
    run_steps("hip", params, opt, P, degree, 0, 2)
    stats = DensifyStats(P, "cuda")
    stats.update(*(torch.from_numpy(a).cuda() for a in _stats_inputs(P, 2, 5)))
    rng = np.random.default_rng(9)
    idx = np.sort(rng.choice(P, 100, replace=False)) if index == "subset" else rng.integers(0, P, P + 50)
    idx = torch.from_numpy(idx.astype(np.int64)).cuda()
    old = snapshot(params, opt)
    old_stats = (stats.grad_accum.clone(), stats.denom.clone(), stats.max_radii.clone())
    steps_before = {n: float(opt.state[p]["step"]) for n, p in params.items() if opt.state.get(p)}
    new = dict(zip(NAMES, opt.reindex(idx)))
    stats.reindex(idx)
    for group in opt.param_groups:
        p = group["params"][0]
        n = group["name"]
        assert p is new[n] and p.requires_grad and p.is_contiguous() and p.shape[0] == idx.numel()
        assert same_bits(p, old[n][0][idx])
        if len(old[n]) == 3:
            assert same_bits(opt.state[p]["exp_avg"], old[n][1][idx]) and same_bits(opt.state[p]["exp_avg_sq"], old[n][2][idx])
            assert float(opt.state[p]["step"]) == steps_before[n]
    assert len(opt.state) == len(steps_before)
    for a, b in zip((stats.grad_accum, stats.denom, stats.max_radii), old_stats):
        assert same_bits(a, b[idx])
    # and the optimiser goes on at the new size
    for n, p in new.items():
        p.grad = None if n == "frozen" else torch.full_like(p, 1e-3)
    opt.step(visibility=torch.ones(idx.numel(), dtype=torch.bool, device="cuda"))
    assert not same_bits(new["xyz"], old["xyz"][0][idx])


def test_value_errors():
    P = 16
    ok = lambda: torch.zeros((P, 3), device="cuda", requires_grad=True)  # noqa: E731
    group = lambda t, name: {"params": [t], "lr": 1e-3, "name": name}  # noqa: E731
    for bad in (torch.zeros((P, 3), device="cuda", dtype=torch.float64), torch.zeros((P, 3), device="cuda", dtype=torch.float16),
                torch.zeros((P, 3)), torch.zeros((3, P), device="cuda").t(), torch.zeros((P + 1, 3), device="cuda"),
                torch.zeros((), device="cuda")):
        with pytest.raises(ValueError):
            GaussianAdam([group(ok(), "a"), group(bad.requires_grad_(True), "b")])
    with pytest.raises(ValueError):
        GaussianAdam([{"params": [ok(), ok()], "lr": 1e-3}])
    a, b = ok(), ok()
    opt = GaussianAdam([group(a, "a"), group(b, "b")])
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    for vis in (torch.ones(P + 1, dtype=torch.bool, device="cuda"), torch.ones(P, dtype=torch.bool),
                torch.ones((2, P + 1), dtype=torch.int32, device="cuda"), torch.ones(P, dtype=torch.int64, device="cuda"),
                torch.ones((P, 2), dtype=torch.int32, device="cuda").t()[:, :P], torch.ones(P, device="cuda"), [1] * P):
        with pytest.raises(ValueError):
            opt.step(visibility=vis)
    b.grad = torch.ones((3, P), device="cuda").t()
    with pytest.raises(ValueError):
        opt.step()
    # nothing was launched by any of the refused calls
    assert not a.detach().any() and not b.detach().any() and len(opt.state) == 0
    stats = DensifyStats(P, "cuda")
    for g, r in ((torch.zeros((P, 2), device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")),
                 (torch.zeros((P, 3), device="cuda"), torch.zeros(P, dtype=torch.int64, device="cuda")),
                 (torch.zeros((2, P, 3), device="cuda"), torch.zeros((3, P), dtype=torch.int32, device="cuda")),
                 (torch.zeros((P, 3)), torch.zeros(P, dtype=torch.int32))):
        with pytest.raises(ValueError):
            stats.update(g, r)


def test_finetune_loop_through_the_rasterizer():
    spec = importlib.util.spec_from_file_location("finetune_scene", os.path.join(ROOT, "examples", "finetune_scene.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    P, steps = 2000, 20
    r = example.finetune(points=P, views=4, steps=steps, width=64, height=48, optimizer="hip")
    print(f"finetune: loss {r['before'][0]:.6f} -> {r['after'][0]:.6f}, PSNR {r['before'][1]:.2f} -> {r['after'][1]:.2f} dB")
    assert r["after"][0] < r["before"][0]
    seen = r["seen"]
    never = ~seen.any(0)
    assert 0 < int(never.sum()) < P  # the ring of cameras leaves some Gaussians out of every view
    for n in r["start"]:
        assert same_bits(r["start"][n][never], r["end"][n][never]), n
        assert not same_bits(r["start"][n][~never], r["end"][n][~never]), n
    opt = r["optimizer"]
    for group in opt.param_groups:
        st = opt.state[group["params"][0]]
        assert int(st["step"]) == steps
        assert not st["exp_avg"][never].any() and not st["exp_avg_sq"][never].any()
    assert torch.equal(r["stats"].denom, seen.sum(0).to(torch.int32))
    assert int(r["stats"].max_radii[never].max()) == 0 and float(r["stats"].grad_accum[never].max()) == 0.0
