"""CPU: the yardsticks of the training targets and losses against the reference's own outputs (tests/golden/training.npz,
written by tests/golden/gen_golden_training.py from the reference's modules).

* The float64 restatement of get_node_correspondences (node_corr_f64.py) reproduces the reference exactly on the two exact
  inputs -- lattice clouds on which float32 is exact in either distance form -- indices, order and overlaps bit for bit.
* The torch losses of gaussreg_amd.loss match the reference's values and gradients: 1e-12 in float64, 1e-5 of the scale in
  float32; gradcheck on a 5 x 6 circle loss.
* SuperPointTargetGenerator repeats the reference's draw, and refuses an empty set.
* Every case of node_corr_cases.py is admitted: the node pairs the float64 thresholds r^2 -+ tau do not decide are at most
  1 % of the emitted pairs."""
import numpy as np
import pytest
import torch

import node_corr_cases as cases
import node_corr_f64 as f64
from helpers import load_golden

G = load_golden("training.npz")
MARGINS = dict(pos_margin=0.1, neg_margin=1.4, pos_optimal=0.1, neg_optimal=1.4, log_scale=24)


@pytest.mark.parametrize("name", ["golden_lattice", "golden_self"])
def test_restatement_reproduces_the_reference_on_exact_inputs(name):
    prefix = {"golden_lattice": "nc_lattice", "golden_self": "nc_self"}[name]
    r = cases.reference(name)
    assert r["decided"].all() and np.array_equal(r["ov_lo"], r["ov_hi"])
    idx, ov = f64.emitted(r["ov_lo"])
    assert np.array_equal(idx, G[f"{prefix}_indices"])
    assert ov.dtype == np.float32 and np.array_equal(ov.view(np.uint32), G[f"{prefix}_overlaps"].view(np.uint32))
    if name == "golden_self":
        diag = r["ov_lo"][np.arange(32), np.arange(32)]
        assert np.all(diag[cases.build(name)["ref_masks"]] == np.float32(1.0))


def test_golden_inputs_are_small_and_on_the_lattice():
    for prefix in ("nc_lattice", "nc_self"):
        rp, sp = G[f"{prefix}_ref_knn_points"], G[f"{prefix}_src_knn_points"]
        assert rp.shape[0] <= 40 and sp.shape[0] <= 40 and rp.shape[1] <= 16
        for a in (rp, sp, G[f"{prefix}_transform"]):
            assert np.array_equal(a.astype(np.float64) * 64, np.round(a.astype(np.float64) * 64))


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_is_admitted(name):
    r = cases.reference(name)
    idx, _ = f64.emitted(r["ov_hi"])
    undecided = int((~r["decided"]).sum())
    print(f"{name}: emitted {len(idx)}  undecided {undecided}  tau {r['tau']:.3e}  S {r['S']:.3f}")
    assert np.all(r["ov_lo"] <= r["ov_hi"])
    assert undecided <= cases.ADMIT * len(idx), (name, undecided, len(idx))
    if name == "far":
        assert len(idx) == 0
    else:
        assert len(idx) > 0


def test_mask_cases_would_differ_without_their_masks():
    """The padded points of `partial_masks` sit where an implementation that ignored the point masks would count them."""
    c = dict(cases.build("partial_masks"))
    with_masks = cases.reference("partial_masks")
    without = f64.node_correspondences_f64(c["ref_nodes"], c["src_nodes"], c["ref_knn_points"], c["src_knn_points"],
                                           c["transform"], c["pos_radius"])
    assert not np.array_equal(with_masks["ov_lo"], without["ov_lo"])
    assert np.abs(without["counts"][:, 0, :] - with_masks["counts"][:, 0, :]).max() > 0    # padded source points on T 0 = t
    assert np.abs(without["counts"][:, :, 1] - with_masks["counts"][:, :, 1]).max() > 0    # padded reference points on 0


def _circle(dtype):
    from gaussreg_amd.loss import weighted_circle_loss
    x = torch.from_numpy(G["wcl_feat_dists"]).to(dtype).requires_grad_(True)
    v = weighted_circle_loss(torch.from_numpy(G["wcl_pos_masks"]), torch.from_numpy(G["wcl_neg_masks"]), x,
                             pos_scales=torch.from_numpy(G["wcl_pos_scales"]).to(dtype), **MARGINS)
    v.backward()
    return float(v.detach()), x.grad.numpy()


def test_weighted_circle_loss_matches_the_reference():
    v, g = _circle(torch.float64)
    assert abs(v - float(G["wcl_value64"])) <= 1e-12 and np.abs(g - G["wcl_grad64"]).max() <= 1e-12
    v, g = _circle(torch.float32)
    assert abs(v - float(G["wcl_value32"])) <= 1e-5 * abs(float(G["wcl_value64"]))
    assert np.abs(g - G["wcl_grad32"]).max() <= 1e-5 * np.abs(G["wcl_grad64"]).max()
    assert np.abs(g - G["wcl_grad64"]).max() <= 1e-5 * np.abs(G["wcl_grad64"]).max()


def test_weighted_circle_loss_module_and_gradcheck():
    """The weights of the circle loss are detached (circle_loss.py:66,73), so the autograd gradient is by design not the
    derivative of the value: finite differences are taken of the same formula with the weights frozen at x0 -- written
    out here -- and the module's gradient must be that one."""
    from gaussreg_amd.loss import WeightedCircleLoss
    g = torch.Generator().manual_seed(3)
    ov = torch.rand(5, 6, generator=g, dtype=torch.float64) * (torch.rand(5, 6, generator=g) < 0.5)
    pos, neg = ov > 0.1, ov == 0
    scales = torch.sqrt(ov * pos)
    x0 = torch.rand(5, 6, generator=g, dtype=torch.float64) * 1.5 + 0.05
    pw = (x0 - 1e5 * (~pos).double() - 0.1).clamp(min=0) * scales
    nw = (1.4 - (x0 + 1e5 * (~neg).double())).clamp(min=0)
    rows = (pos.sum(1) > 0) & (neg.sum(1) > 0)
    cols = (pos.sum(0) > 0) & (neg.sum(0) > 0)
    assert rows.any() and cols.any()

    def frozen(x):
        p, n = 24 * (x - 0.1) * pw, 24 * (1.4 - x) * nw
        lr = torch.nn.functional.softplus(torch.logsumexp(p, 1) + torch.logsumexp(n, 1)) / 24
        lc = torch.nn.functional.softplus(torch.logsumexp(p, 0) + torch.logsumexp(n, 0)) / 24
        return (lr[rows].mean() + lc[cols].mean()) / 2
    x = x0.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(frozen, (x,), eps=1e-7, atol=1e-6)
    want, = torch.autograd.grad(frozen(x), x)
    mod = WeightedCircleLoss(0.1, 1.4, 0.1, 1.4, 24)
    v = mod(pos, neg, x, scales)
    got, = torch.autograd.grad(v, x)
    assert abs(float(v.detach()) - float(frozen(x0))) <= 1e-12 and (got - want).abs().max() <= 1e-12 and want.abs().max() > 1e-3


def _cfg():
    from gaussreg_amd.model import make_cfg
    return make_cfg()


def _loss_dicts(dtype, dense=False):
    t = lambda k: torch.from_numpy(G[k])
    od = dict(ref_feats_c=t("loss_ref_feats_c").to(dtype), src_feats_c=t("loss_src_feats_c").to(dtype),
              gt_node_corr_indices=t("loss_gt_indices"), gt_node_corr_overlaps=t("loss_gt_overlaps").to(dtype),
              ref_node_corr_knn_points=t("loss_ref_knn_points").to(dtype), src_node_corr_knn_points=t("loss_src_knn_points").to(dtype),
              ref_node_corr_knn_masks=t("loss_ref_knn_masks"), src_node_corr_knn_masks=t("loss_src_knn_masks"),
              matching_scores=t("loss_matching_scores").to(dtype))
    if dense:
        m = torch.zeros(od["ref_feats_c"].shape[0], od["src_feats_c"].shape[0], dtype=dtype)
        idx = od["gt_node_corr_indices"]
        m[idx[:, 0], idx[:, 1]] = od["gt_node_corr_overlaps"]
        od["gt_node_corr_overlap_matrix"] = m
    return od, dict(transform=t("loss_transform").to(dtype))


@pytest.mark.parametrize("dense", [False, True], ids=["list", "dense"])
def test_overall_loss_matches_the_reference(dense):
    from gaussreg_amd.loss import OverallLoss
    crit = OverallLoss(_cfg())
    for tag, dtype, tol in (("64", torch.float64, 1e-12), ("32", torch.float32, 1e-5)):
        res = crit(*_loss_dicts(dtype, dense))
        got = np.array([float(res["loss"]), float(res["c_loss"]), float(res["f_loss"])])
        want = G[f"loss_values{tag}"]
        assert np.abs(got - want).max() <= tol * max(1.0, np.abs(G["loss_values64"]).max()), (tag, got, want)
    assert sorted(res) == ["c_loss", "f_loss", "loss"]


def test_make_cfg_has_the_training_sections():
    c = _cfg()
    assert (c.coarse_loss.positive_margin, c.coarse_loss.negative_margin, c.coarse_loss.positive_optimal,
            c.coarse_loss.negative_optimal, c.coarse_loss.log_scale, c.coarse_loss.positive_overlap) == (0.1, 1.4, 0.1, 1.4, 24, 0.1)
    assert c.fine_loss.positive_radius == 0.05
    assert (c.loss.weight_coarse_loss, c.loss.weight_fine_loss) == (1.0, 1.0)
    assert (c.eval.acceptance_overlap, c.eval.acceptance_radius, c.eval.rmse_threshold) == (0.0, 0.1, 0.2)
    import gaussreg_amd
    for name in ("WeightedCircleLoss", "CoarseMatchingLoss", "FineMatchingLoss", "OverallLoss", "Evaluator"):
        assert hasattr(gaussreg_amd, name), name


def test_zero_positive_distance_gives_a_nan_gradient_as_in_the_reference():
    from gaussreg_amd.loss import CoarseMatchingLoss
    f = torch.nn.functional.normalize(torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float64), dim=1)
    rf = f.clone().requires_grad_(True)
    od = dict(ref_feats_c=rf, src_feats_c=f[:2].clone(), gt_node_corr_indices=torch.tensor([[0, 0]]),
              gt_node_corr_overlaps=torch.tensor([0.5], dtype=torch.float64))
    CoarseMatchingLoss(_cfg())(od).backward()
    assert torch.isnan(rf.grad).any()


def test_target_generator_repeats_the_reference_draw():
    from gaussreg_amd.matching import SuperPointTargetGenerator
    idx, ov = torch.from_numpy(G["tg_indices"]), torch.from_numpy(G["tg_overlaps"])
    gen = SuperPointTargetGenerator(128, 0.1, generator=np.random.RandomState(123))
    assert list(gen.state_dict()) == []
    a, b, o = gen(idx, ov)
    assert np.array_equal(a.numpy(), G["tg_ref"]) and np.array_equal(b.numpy(), G["tg_src"])
    assert np.array_equal(o.numpy(), G["tg_sel_overlaps"])
    a, b, o = SuperPointTargetGenerator(128, 0.1, generator=5)(idx, ov * 0.05)             # nothing above the threshold
    assert np.array_equal(a.numpy(), G["tg_low_ref"]) and np.array_equal(b.numpy(), G["tg_low_src"])
    assert np.array_equal(o.numpy(), G["tg_low_overlaps"])
    x, y = SuperPointTargetGenerator(16, 0.1, generator=7)(idx, ov), SuperPointTargetGenerator(16, 0.1, generator=7)(idx, ov)
    assert all(torch.equal(p, q) for p, q in zip(x, y)) and x[0].shape == (16,)
    with pytest.raises(ValueError, match="no ground-truth superpoint correspondence"):
        gen(idx[:0], ov[:0])


def test_evaluator_metrics_on_a_known_transform():
    from gaussreg_amd.loss import Evaluator
    ev = Evaluator(_cfg())
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([0.3, -0.2, 0.1])
    src = torch.rand(50, 3, generator=torch.Generator().manual_seed(1))
    od = dict(estimated_transform=T.clone(), src_points=src, ref_corr_points=src[:10] + T[:3, 3], src_corr_points=src[:10],
              ref_points_c=src[:4], src_points_c=src[:5], gt_node_corr_indices=torch.tensor([[0, 1], [2, 3]]),
              gt_node_corr_overlaps=torch.tensor([0.5, 0.2]), ref_node_corr_indices=torch.tensor([0, 1]),
              src_node_corr_indices=torch.tensor([1, 1]))
    dd = dict(transform=T.clone())
    res = ev(od, dd)
    assert sorted(res) == ["RMSE", "RR", "RRE", "RSE", "RTE"]
    assert float(res["RRE"]) < 0.1 and float(res["RTE"]) < 1e-6 and float(res["RMSE"]) < 1e-6 and float(res["RR"]) == 1.0
    assert torch.equal(dd["transform"], T) and torch.equal(od["estimated_transform"], T)   # nothing rescaled in place
    assert float(ev.evaluate_fine(od, dd)) == 1.0 and float(ev.evaluate_coarse(od)) == 0.5
