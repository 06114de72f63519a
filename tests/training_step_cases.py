"""Test helper (not collected): the cases of tests/test_gpu_training_step_f64.py and its yardstick, shared with the CPU file
tests/test_training_step_f64_reference.py and with tests/golden/gen_golden_training_step.py.

One small network for all cases (case_cfg): KPConvFPN 1 -> 16 -> 32 with 4 groups, GeometricTransformer 512 -> 64 -> 32 with
4 heads and four blocks, 32-point patches, 32 targets, 100 Sinkhorn iterations: every width is one the HIP GroupNorm
accepts, (64, 4) is an instantiated RPE backward.  Parameters come from numpy's default_rng (init_state), every bias and
every norm weight off its initial value; kernel points are the stored disposition scaled by the layer's radius.

Clouds (clouds): a wavy sheet sampled at random; the source is a subset of the same physical points plus its own, jittered
and taken through the inverse of a similarity transform.  The cloud seeds below were chosen by the generator's search
(gen_golden_training_step.py --search), whose conditions are the ones asserted by check_case / check_feature_distances /
check_admission / check_self_distance here; what the search found is recorded in docs/training_step_f64_errors.md.

'max' picks the winner of the angular maximum: a winner float32 cannot resolve is a property of the case, so its clouds are
small enough (at most 8 superpoints per cloud) for transformer_grad_cases.assert_max_margin to hold.  With 8 x 8 candidate
pairs the 'mean' case's floor of 20 superpoints and 20 ground-truth pairs cannot apply: its floors are 3 and 4.
"""
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import demo_inputs  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "training_step.npz")

VOXEL, RADIUS, STAGES = 0.025, 0.0625, 5
LIMIT = 64                      # neighbour limit of every level: one no search of these clouds meets
STATE_SEED = 5
TARGET_SEED = 5                 # np.random.RandomState(TARGET_SEED) draws the targets
CAP = 1e-4                      # admission: float32 twin against float64 twin, per tensor
ZERO_BY_SYMMETRY = 1e-9         # tests/test_gpu_transformer_backward.py
MIN_FEATURE_DISTANCE = 1e-3
N_PROBES = 8

CASES = {
    "mean": dict(reduction_a="mean", cloud_seed=1, n_base=760, n_cloud=600, extent=2.0, superpoints=(20, 60), min_pairs=20),
    "max": dict(reduction_a="max", cloud_seed=4, n_base=250, n_cloud=200, extent=0.5, superpoints=(3, 8), min_pairs=4),
}
KPCONV_RADIUS_FACTOR = {"encoder1_1": 1, "encoder1_2": 1, "encoder2_1": 1, "encoder2_2": 2, "encoder2_3": 2, "encoder3_1": 2,
                        "encoder3_2": 4, "encoder3_3": 4, "encoder4_1": 4, "encoder4_2": 8, "encoder4_3": 8, "encoder5_1": 8,
                        "encoder5_2": 16, "encoder5_3": 16}       # backbone.py:104-131
CASE_KEYS_LEVELS = ("points", "neighbors", "subsampling", "upsampling")
CASE_KEYS = ("lengths", "features", "transform", "ref_knn_idx", "src_knn_idx", "ref_knn_masks", "src_knn_masks", "overlaps",
             "gt_indices", "gt_overlaps", "ref_ci", "src_ci", "labels", "ref_corr_knn_points", "src_corr_knn_points")


# ------------------------------------------------------------------------------------------------------ configuration
def case_cfg(name):
    from gaussreg_amd.model import make_cfg
    cfg = make_cfg()
    b, g = cfg.backbone, cfg.geotransformer
    b.input_dim, b.init_dim, b.output_dim, b.group_norm = 1, 16, 32, 4
    b.init_voxel_size = VOXEL
    b.init_radius, b.init_sigma = b.base_radius * VOXEL, b.base_sigma * VOXEL
    g.input_dim, g.hidden_dim, g.output_dim, g.num_heads = 512, 64, 32, 4
    g.blocks = ["self", "cross", "self", "cross"]
    g.reduction_a = CASES[name]["reduction_a"]
    cfg.model.num_points_in_patch = 32
    cfg.coarse_matching.num_targets = 32
    assert cfg.model.num_sinkhorn_iterations == 100 and abs(b.init_radius - RADIUS) < 1e-12
    return cfg


def hyper(cfg):
    """What training_step_f64.training_step reads, as plain dicts."""
    return {"group_norm": cfg.backbone.group_norm, "init_sigma": cfg.backbone.init_sigma,
            "geotransformer": dict(vars(cfg.geotransformer)), "coarse_loss": dict(vars(cfg.coarse_loss)),
            "loss": dict(vars(cfg.loss)), "num_sinkhorn_iterations": cfg.model.num_sinkhorn_iterations,
            "positive_radius": cfg.fine_loss.positive_radius, "overlap_threshold": cfg.coarse_matching.overlap_threshold,
            "matching_radius": cfg.model.ground_truth_matching_radius}


def init_state(template, cfg, seed=STATE_SEED):
    """A state dict with the names and shapes of `template` (a GeoTransformer state dict), filled from default_rng(seed) in
    sorted-name order: weights uniform in +-1/sqrt(fan_in) (torch's default bound), norm weights 1 +- 0.1, biases +- 0.15
    (a KPConv bias +- its default bound), alpha 0.7, kernel points the stored disposition x the layer's radius; the
    sinusoid's div_term is the template's."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in sorted(template):
        shape = tuple(template[name].shape)
        u = lambda: rng.random(shape) * 2.0 - 1.0
        if name.endswith("kernel_points"):
            radius = cfg.backbone.init_radius * KPCONV_RADIUS_FACTOR[name.split(".")[1]]
            v = demo_inputs.K015 * radius
            assert v.shape == shape
        elif name.endswith("div_term"):
            v = np.asarray(template[name].detach().cpu().numpy() if torch.is_tensor(template[name]) else template[name])
        elif name == "optimal_transport.alpha":
            v = np.full(shape, 0.7)
        elif name.endswith("norm.weight"):
            v = 1.0 + 0.1 * u()
        elif name.endswith("KPConv.bias"):
            v = u() / np.sqrt(shape[0])
        elif name.endswith("bias"):
            v = 0.15 * u()
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) == 3 else shape[1]
            v = u() / np.sqrt(fan_in)
        out[name] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return out


def state_checksums(state):
    return np.array([float(state[k].double().sum()) for k in sorted(state)], np.float64)


# ------------------------------------------------------------------------------------------------------------- clouds
def clouds(name, seed=None):
    """-> ref (n, 3), src (n, 3) float32 and the (4, 4) float32 similarity transform that takes src onto ref."""
    spec = CASES[name]
    rng = np.random.default_rng(1000 + (spec["cloud_seed"] if seed is None else seed))
    L, nb, nc = spec["extent"], spec["n_base"], spec["n_cloud"]
    xy = (rng.random((nb, 2)) - 0.5) * L
    z = 0.12 * np.sin(3.0 * xy[:, 0] + 0.3) * np.cos(2.0 * xy[:, 1]) + 0.01 * rng.standard_normal(nb)
    base = np.concatenate([xy, z[:, None]], 1)
    perm = rng.permutation(nb)
    ref = base[perm[:nc]]
    src_in_ref = base[perm[nb - nc:]] + 0.003 * rng.standard_normal((nc, 3))
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    angle = 0.6 + 0.4 * rng.random()
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    s = 1.08
    t = np.array([0.2, -0.1, 0.15])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * R, t
    src = (src_in_ref - t) @ R / s               # x_ref = s R x_src + t
    return ref.astype(np.float32), src.astype(np.float32), T.astype(np.float32)


def features(name, n):
    return (0.5 + np.random.default_rng(77).random((n, 1))).astype(np.float32)


def voxel_radius():
    return VOXEL, RADIUS, [LIMIT] * STAGES


# ---------------------------------------------------------------------------------------------------- case conditions
def untruncated(case):
    """The `_untruncated` rule of tests/test_gpu_backbone_fused_norm.py: no search met its limit."""
    return all(np.asarray(idx).shape[1] < LIMIT for key in ("neighbors", "subsampling", "upsampling") for idx in case[key])


def check_case(name, case, hp):
    """The conditions on the discrete side of a case; returns figures for the record."""
    import training_step_f64 as ts
    spec = CASES[name]
    assert untruncated(case), "a radius search met its limit"
    lengths = np.asarray(case["lengths"])
    assert max(lengths[0]) <= 600
    lo, hi = spec["superpoints"]
    assert all(lo <= int(n) <= hi for n in lengths[-1]), f"superpoints per cloud {lengths[-1]} outside [{lo}, {hi}]"
    pairs = int((np.asarray(case["gt_overlaps"]) > hp["overlap_threshold"]).sum())
    assert pairs >= spec["min_pairs"], f"{pairs} ground-truth pairs above the overlap threshold"
    labels = np.asarray(case["labels"])
    matched, dustbin = int(labels[:, :-1, :-1].sum()), int(labels[:, :-1, -1].sum() + labels[:, -1, :-1].sum())
    assert matched >= 1 and dustbin >= 1 and not labels[:, -1, -1].any()
    # the labels are a decision float32 and float64 take alike, with room to spare: no squared distance of a valid pair
    # within 4 float32 errors of the threshold
    t = lambda a, dt: torch.as_tensor(np.asarray(a)).to(dt)
    ref_m, src_m = torch.as_tensor(np.asarray(case["ref_knn_masks"]))[np.asarray(case["ref_ci"])], \
        torch.as_tensor(np.asarray(case["src_knn_masks"]))[np.asarray(case["src_ci"])]
    lab, d2 = {}, {}
    for dt in (torch.float64, torch.float32):
        lab[dt], d2[dt] = ts.fine_labels(t(case["ref_corr_knn_points"], dt), t(case["src_corr_knn_points"], dt), ref_m, src_m,
                                         t(case["transform"], dt), hp["positive_radius"])
    valid = ref_m[:, :, None] & src_m[:, None, :]
    err = float((d2[torch.float32].double() - d2[torch.float64]).abs()[valid].max())
    margin = float((d2[torch.float64] - hp["positive_radius"] ** 2).abs()[valid].min())
    assert np.array_equal(lab[torch.float64].numpy(), labels) and np.array_equal(lab[torch.float32].numpy(), labels)
    assert margin > 4 * err, f"a label is decided by {margin:.2e}, float32 error of the squared distance {err:.2e}"
    order_margin, order_err = patch_margin(case)
    assert order_margin > 4 * order_err, (f"a patch's membership is decided by {order_margin:.2e}, float32 error of the "
                                          f"squared distance {order_err:.2e}")
    return dict(superpoints=[int(n) for n in lengths[-1]], pairs=pairs, targets=int(labels.shape[0]), matched=matched,
                dustbin=dustbin, label_margin=margin, label_err=err, patch_margin=order_margin, patch_err=order_err)


def patch_margin(case):
    """point_to_node_partition assigns every fine point to its nearest superpoint and keeps a superpoint's K nearest points
    (pointcloud_partition.py:84-102), in float32 by the expanded form x^2 - 2xy + y^2.  The patch tables are an input of the
    twin, so float32 and float64 must build the same patches: -> (the smallest float64 gap that decides an assignment or the
    cut after the K-th point, the float32 error of the expanded form).
    The ORDER of the points inside a patch is not such a decision.  A superpoint is the barycentre of its cell, so the two
    points of a two-point cell are equidistant from it by construction -- an exact tie that every precision and every
    evaluation order breaks its own way, in every seed of these sparse clouds -- and the step does not depend on it: Sinkhorn
    is equivariant under permutations of rows and columns, and masks, points and labels move with the rows.  (The same stance
    as transformer_grad_cases.max_margin, which does not count rivals at the winner's own angle.)  Patches are therefore
    compared as sets: same_decisions."""
    lengths = np.asarray(case["lengths"])
    n_c, n_f = int(lengths[-1][0]), int(lengths[1][0])
    pc, pf = np.asarray(case["points"][-1]), np.asarray(case["points"][1])
    margin, err = float("inf"), 0.0
    for side, c, f in (("ref", pc[:n_c], pf[:n_f]), ("src", pc[n_c:], pf[n_f:])):
        c64, f64 = torch.from_numpy(c).double(), torch.from_numpy(f).double()
        d64 = ((c64[:, None, :] - f64[None, :, :]) ** 2).sum(-1)
        c32, f32 = torch.from_numpy(c), torch.from_numpy(f)
        d32 = ((c32 ** 2).sum(1)[:, None] - 2.0 * c32 @ f32.t() + (f32 ** 2).sum(1)[None, :]).clamp(min=0.0)
        err = max(err, float((d32.double() - d64).abs().max()))
        two = torch.sort(d64, 0)[0][:2]
        margin = min(margin, float((two[1] - two[0]).min()))
        owner = d64.argmin(0)
        idx, masks = np.asarray(case[side + "_knn_idx"]), np.asarray(case[side + "_knn_masks"])
        K = idx.shape[1]
        for m in range(c.shape[0]):
            own = torch.nonzero(owner == m)[:, 0]
            dist, order = torch.sort(d64[m][own])
            if own.numel() > K:
                margin = min(margin, float(dist[K] - dist[K - 1]))
            k = min(own.numel(), K)
            assert np.array_equal(np.sort(idx[m, :k]), np.sort(own[order][:k].numpy())) and (idx[m, k:] == f.shape[0]).all(), (side, m)
            assert masks[m, :k].all() and not masks[m, k:].any(), (side, m)
    return margin, err


def same_decisions(got, want):
    """The decisions of two runs of one case are the same: overlap matrix, correspondences, target pairs and patch masks bit
    for bit; the patches, their points and the labels bit for bit once every patch is listed in ascending point index (see
    patch_margin for why the order inside a patch is left free).  Raises AssertionError naming what differs."""
    for k in ("overlaps", "gt_indices", "gt_overlaps", "ref_ci", "src_ci", "ref_knn_masks", "src_knn_masks"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), f"{k} differs"
    assert np.asarray(got["overlaps"]).dtype == np.asarray(want["overlaps"]).dtype == np.float32
    canon = {}
    for tag, d in (("got", got), ("want", want)):
        for side in ("ref", "src"):
            idx = np.asarray(d[side + "_knn_idx"]).astype(np.int64)
            assert np.array_equal(np.sort(idx, 1), np.sort(np.asarray(want[side + "_knn_idx"]).astype(np.int64), 1)), \
                f"{side}_knn_idx differs (as sets)"
            order = np.argsort(idx[np.asarray(d[side + "_ci"])], axis=1, kind="stable")              # (P, K)
            canon[tag, side] = order
            canon[tag, side + "_points"] = np.take_along_axis(np.asarray(d[side + "_corr_knn_points"]), order[:, :, None], 1)
        r, c = canon[tag, "ref"], canon[tag, "src"]
        P, K = r.shape
        dust = np.full((P, 1), K)
        lab = np.asarray(d["labels"])
        lab = np.take_along_axis(lab, np.concatenate([r, dust], 1)[:, :, None], 1)
        canon[tag, "labels"] = np.take_along_axis(lab, np.concatenate([c, dust], 1)[:, None, :], 2)
    for k in ("ref_points", "src_points", "labels"):
        assert np.array_equal(canon["got", k], canon["want", k]), f"{k if k == 'labels' else k[:4] + 'corr_knn_points'} differs"


def check_feature_distances(case, hp, keep64):
    """No positive pair next to the singular point of sqrt(2 - 2 x y) at initialisation."""
    pos = torch.as_tensor(np.asarray(case["overlaps"])) > hp["coarse_loss"]["positive_overlap"]
    smallest = float(keep64["feat_dists"].detach()[pos].min())
    assert smallest >= MIN_FEATURE_DISTANCE, f"a positive pair at feature distance {smallest:.2e}"
    return smallest


def max_margin(state, case):
    """The admission rule of reduction_a = 'max' (transformer_grad_cases.assert_max_margin) on the superpoints."""
    import training_step_f64 as ts
    import transformer_grad_cases as tc
    sub = lambda dt: {k[len("transformer."):]: v for k, v in ts.to_params(state, dt).items() if k.startswith("transformer.")}
    pts = np.asarray(case["points"][-1], np.float32)
    n = int(np.asarray(case["lengths"])[-1][0])
    return tc.assert_max_margin(sub(torch.float64), sub(torch.float32), [pts[:n], pts[n:]])


# ---------------------------------------------------------------------------------------------------------- yardstick
def bar(rel_ref):
    """tests/test_gpu_backbone_fused_norm.py: rel_hip <= max(8 rel_ref, 1e-6)."""
    return max(8.0 * rel_ref, 1e-6)


def orderings(case):
    """The case three times, for the float32 twin: as stored, with the columns of every neighbour and subsampling table
    reversed, and with them shuffled (default_rng(2)).  The same neighbour SETS, so the same function (float64: equal to
    1.8e-14) summed in another order.  Why: rel_ref is one draw of a rounding error.  On the tensors whose gradient is a
    cancelling sum (a bias or an affine parameter next to a GroupNorm over groups of two channels) one draw of the float32
    twin moves 1.4e-6 .. 3.7e-6 between these orders, and 1.6x between two runs of one order on a threaded CPU, while the
    HIP step's own draw moves as far between its configurations; a bar of 8 x one draw then fails one run in a few with no
    code changed.  rel_ref is therefore the MEDIAN of the three draws: the same quantity, estimated with less scatter."""
    out = [case]
    for k in (1, 2):
        c = dict(case)
        for key in ("neighbors", "subsampling"):
            tables = []
            for a in case[key]:
                a = np.asarray(a)
                perm = np.arange(a.shape[1])[::-1] if k == 1 else np.random.default_rng(k).permutation(a.shape[1])
                tables.append(np.ascontiguousarray(a[:, perm]))
            c[key] = tables
        out.append(c)
    return out


def _median(values):
    return float(np.median(values))


def relative_errors(name, got, g64, g32, terms):
    """-> (|g64|, rel_got, rel_ref, scale, by_symmetry).  Norm-wise relative errors against the float64 gradient; a bias whose
    gradient is zero by the softmax's shift invariance takes the scale of the terms it sums, entry-wise.  `g32`: the float32
    twin's gradient, or a list of them (the draws of `orderings`): rel_ref is the median of their errors."""
    draws = g32 if isinstance(g32, (list, tuple)) else [g32]
    norm = float(g64.norm())
    tm = terms.get(name)
    if tm is not None and float(g64.abs().max()) < ZERO_BY_SYMMETRY * tm:
        return (norm, float((got - g64).abs().max()) / tm, _median([float((g - g64).abs().max()) / tm for g in draws]),
                tm * g64.numel() ** 0.5, True)
    assert norm > 0, f"{name}: the float64 gradient is zero"
    return norm, float((got - g64).norm()) / norm, _median([float((g - g64).norm()) / norm for g in draws]), norm, False


def _of(g32, name):
    return [g[name] for g in g32] if isinstance(g32, (list, tuple)) else g32[name]


def compare(tag, got, g64, g32, terms, emit=print):
    """The comparison of the GPU test.  got / g64 / g32: {name: float64 CPU tensor or None}.  Every parameter of g64 must be in
    `got`; where the float64 twin has no gradient (the loss does not reach the parameter) `got` must have none either.
    Raises AssertionError naming every tensor outside its bar; returns {name: (|g64|, rel_hip, rel_ref, rel_hip / bar)}."""
    rows, failures = {}, []
    for name, truth in g64.items():
        assert name in got, f"{name}: not among the gradients"
        g = got[name]
        if truth is None:
            if g is not None:
                failures.append(f"{name}: has a gradient, the loss does not reach it")
            continue
        if g is None:
            failures.append(f"{name}: received no gradient")
            continue
        g = g.detach().double().cpu().reshape(truth.shape)
        if not bool(torch.isfinite(g).all()):
            failures.append(f"{name}: not finite")
            continue
        norm, r_hip, r_ref, _, sym = relative_errors(name, g, truth, _of(g32, name), terms)
        rows[name] = (norm, r_hip, r_ref, r_hip / bar(r_ref))
        emit(f"TRSTEP {tag} {name}{' (zero by symmetry: scale of the terms)' if sym else ''}: |g64| {norm:.3e} "
             f"rel_hip {r_hip:.3e} rel_ref {r_ref:.3e}")
        if not r_hip <= bar(r_ref):
            failures.append(f"{name}: rel_hip {r_hip:.3e} > max(8 * {r_ref:.3e}, 1e-6)")
    worst = max(rows, key=lambda k: rows[k][3])
    emit(f"TRSTEP {tag} worst rel_hip / bar {rows[worst][3]:.3f} ({worst}); median rel_hip "
         f"{np.median([r[1] for r in rows.values()]):.3e} rel_ref {np.median([r[2] for r in rows.values()]):.3e}")
    assert not failures, f"{tag}: " + "; ".join(failures)
    return rows


def compare_losses(tag, got, l64, l32, emit=print):
    """|c_loss - c64| and |f_loss - f64| at most max(8 x the float32 twin's error, 1e-6 x value)."""
    draws = l32 if isinstance(l32, (list, tuple)) else [l32]
    for k in ("c_loss", "f_loss"):
        e_hip, e_ref = abs(got[k] - l64[k]), _median([abs(l[k] - l64[k]) for l in draws])
        emit(f"TRSTEP {tag} {k}: value {l64[k]:.12f} e_hip {e_hip:.3e} e_ref {e_ref:.3e}")
        assert e_hip <= max(8 * e_ref, 1e-6 * abs(l64[k])), (tag, k, e_hip, e_ref)


def check_admission(g64, g32, terms, cap=CAP):
    """The condition on the case: the float32 twin against the float64 twin, no code under test involved.
    -> (worst rel_ref, its tensor)."""
    worst, which = 0.0, None
    for name, truth in g64.items():
        if truth is None or float(truth.norm()) == 0.0:
            continue
        _, _, r_ref, _, _ = relative_errors(name, truth, truth, _of(g32, name), terms)
        if r_ref > worst:
            worst, which = r_ref, name
    assert worst <= cap, f"rel_ref {worst:.3e} of {which} above the admission cap {cap:g}"
    return worst, which


SELF_DISTANCE_FACTOR = 4.0


def check_self_distance(state, case, hp, g64, g32, terms):
    """The structure embedding takes sqrt(x^2 - 2xy + y^2) of every superpoint pair, the pair (i, i) included
    (geotransformer.py:37-39): float64 gives 0 there, float32 the square root of whatever the three terms leave -- some
    1e-4..1e-3 of sigma_d instead of 0, a rounding error of 1e-8 amplified by sqrt at its singular point.  What it leaves
    depends on how the dot product is rounded (with or without fma: one BLAS or kernel against another), so a bar that this
    residue decides is not a property of float32 arithmetic.  Rule: no tensor's bar may move by more than
    SELF_DISTANCE_FACTOR (half the bar's own factor 8) when the float32 twin is given the exact self-distance 0.
    -> (worst ratio of the bars, its tensor).  With N superpoints the diagonal is 1/N of all pairs: the rule refuses the small
    clouds of 'max' far more often than the 'mean' case."""
    import rpe_attention_grad_f64 as tf64
    import training_step_f64 as ts
    original = tf64.embedding_indices

    def exact_self_distance(points, *args):
        d_idx, a_idx = original(points, *args)
        d_idx = d_idx.clone()
        d_idx.fill_diagonal_(0.0)
        return d_idx, a_idx
    tf64.embedding_indices = exact_self_distance
    try:
        g32_exact = [ts.run(state, c, hp, torch.float32)[1] for c in orderings(case)]
    finally:
        tf64.embedding_indices = original
    worst, which = 0.0, None
    for name, truth in g64.items():
        if truth is None:
            continue
        r = relative_errors(name, truth, truth, _of(g32, name), terms)[2]
        r_exact = relative_errors(name, truth, truth, _of(g32_exact, name), terms)[2]
        if bar(r) / bar(r_exact) > worst:
            worst, which = bar(r) / bar(r_exact), name
    assert worst <= SELF_DISTANCE_FACTOR, (f"the bar of {which} moves {worst:.1f}x with the float32 residue of the superpoints' "
                                           f"self-distance")
    return worst, which


# ------------------------------------------------------------------------------------------- the reference's gradients
def probes(name, numel):
    """8 unit vectors from default_rng(crc32(name)): a gradient is stored as its norm and its 8 projections."""
    v = np.random.default_rng(zlib.crc32(name.encode())).standard_normal((N_PROBES, numel))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def summarise(name, grad):
    g = np.asarray(grad, np.float64).reshape(-1)
    return np.concatenate([[np.linalg.norm(g)], probes(name, g.size) @ g])


def compare_golden(tag, got, golden, g64, g32, terms, emit=print):
    """Norm and projections of `got` against the reference's, within the bar of `compare` (the scale is the gradient's norm;
    for a bias zero by symmetry, the scale of its terms)."""
    worst, failures = 0.0, []
    for name, want in golden.items():
        g = got[name].detach().double().cpu()
        _, _, r_ref, scale, _ = relative_errors(name, g, g64[name], _of(g32, name), terms)
        err = float(np.abs(summarise(name, g.numpy()) - want).max()) / scale
        worst = max(worst, err / bar(r_ref))
        if not err <= bar(r_ref):
            failures.append(f"{name}: {err:.3e} > max(8 * {r_ref:.3e}, 1e-6)")
    emit(f"TRSTEP {tag} against the reference's norms and projections: worst error / bar {worst:.3f}")
    assert not failures, f"{tag}: " + "; ".join(failures)
    return worst


# ------------------------------------------------------------------------------------------------------------ fixture
def load_case(name, path=GOLDEN):
    """The stored case -> (case dict for the twin, reference results {'losses': (3,), 'grads': {name: (9,)}, ...})."""
    z = np.load(path)
    pre = name + "_"
    case = {k: [z[f"{pre}{k}_{i}"] for i in range(STAGES - (k in ("subsampling", "upsampling")))] for k in CASE_KEYS_LEVELS}
    case.update({k: z[pre + k] for k in CASE_KEYS})
    ref = {"losses": z[pre + "losses"], "param_sums": z[pre + "param_sums"], "div_term": z[pre + "div_term"],
           "grads": dict(zip([str(n) for n in z[pre + "grad_names"]], z[pre + "grad_summaries"]))}
    return case, ref
