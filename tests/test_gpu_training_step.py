"""GPU: one training step of the registration network, end to end.

* `ops.index_select` inside `gaussreg_amd.differentiable()`: its gradient (gr_neighbor_pool_backward in mode 1 through the
  inverted index, no atomics) against torch's index_select gradient in float64, with repeated and padded indices:
  e_hip <= 8 e_ref + 1e-7 of the scale, e_ref being stock torch in float32.  Outside the context the output and its
  `requires_grad` are what they were.
* `model.GeoTransformer` in `.train()` mode on a 2 x 6000-point room pair with its ground-truth transform: the reference's
  output keys, ground-truth correspondences equal to the stand-alone call, a finite loss, a finite gradient in every
  parameter, five Adam steps that lower OverallLoss on the fixed pair, and an `.eval()` output that a no-op
  `differentiable()` block leaves bit-equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LIMITS = [38, 36, 36, 38, 38]
REFERENCE_KEYS = {   # experiments/geotransformer.gaussian_splatting.indoor/model.py:69-222, training branch
    "ref_points_c", "src_points_c", "ref_points_f", "src_points_f", "ref_points", "src_points", "gt_node_corr_indices",
    "gt_node_corr_overlaps", "ref_feats_c", "src_feats_c", "ref_feats_f", "src_feats_f", "ref_node_corr_indices",
    "src_node_corr_indices", "ref_node_corr_knn_points", "src_node_corr_knn_points", "ref_node_corr_knn_masks",
    "src_node_corr_knn_masks", "matching_scores", "ref_corr_points", "src_corr_points", "corr_scores", "estimated_transform"}
EXTRA_KEYS = {"lgr_transform", "gt_node_corr_overlap_matrix"}   # documented additions of gaussreg_amd.model


def test_index_select_gradient_against_float64():
    import gaussreg_amd
    from gaussreg_amd.ops import index_select
    g = torch.Generator().manual_seed(11)
    n, c = 50, 7
    data = torch.randn(n, c, generator=g)
    data[-1] = 0                                                    # the padded zero row the model appends
    index = torch.randint(0, n - 1, (40, 6), generator=g)
    index[torch.rand(40, 6, generator=g) < 0.3] = n - 1             # padded slots
    index[:5] = 3                                                   # one row named 30 times
    up = torch.randn(40, 6, c, generator=g)

    def torch_grad(dtype):
        x = data.clone().to(dtype).requires_grad_(True)
        y = x.index_select(0, index.reshape(-1)).reshape(40, 6, c)
        y.backward(up.to(dtype))
        return y.detach(), x.grad
    y64, g64 = torch_grad(torch.float64)
    _, g32 = torch_grad(torch.float32)
    x = data.cuda().requires_grad_(True)
    with gaussreg_amd.differentiable():
        y = index_select(x, index.cuda(), 0)
        assert y.requires_grad and y.shape == (40, 6, c) and torch.equal(y.detach().cpu().double(), y64)
        y.backward(up.cuda())
        with torch.no_grad():                                        # grad mode off inside the context: inference
            assert not index_select(x, index.cuda(), 0).requires_grad
    scale = float(g64.abs().max())
    e_hip = float((x.grad.cpu().double() - g64).abs().max()) / scale
    e_ref = float((g32.double() - g64).abs().max()) / scale
    print(f"\nindex_select grad: e_hip {e_hip:.2e}  e_ref {e_ref:.2e}")
    assert e_hip <= 8 * e_ref + 1e-7, (e_hip, e_ref)
    x2 = data.cuda().requires_grad_(True)
    with gaussreg_amd.differentiable():
        index_select(x2, index.cuda(), 0).backward(up.cuda())
    assert torch.equal(x2.grad, x.grad)                              # a fixed summation order: the same bits
    # outside the context nothing changes: the values, and no graph
    out = index_select(x, index.cuda(), 0)
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out, y.detach())
    # a CPU tensor gets its gradient on the CPU
    xc = data.clone().requires_grad_(True)
    with gaussreg_amd.differentiable():
        index_select(xc, index, 0).backward(up)
    assert xc.grad.device.type == "cpu" and torch.equal(xc.grad, x.grad.cpu())


@pytest.fixture(scope="module")
def step():
    import gaussreg_amd
    from gaussreg_amd.loss import Evaluator, OverallLoss
    from gaussreg_amd.model import GeoTransformer, make_cfg
    from gaussreg_amd.pair_pipeline import synthetic_room_pair
    from geotransformer.utils.data import precompute_data_stack_mode
    n_per = 6000
    ref, src, T = synthetic_room_pair(21, n_per, torch.device("cuda"))
    d = precompute_data_stack_mode(torch.cat([ref, src]), torch.tensor([n_per, n_per]), 5, 0.025, 0.0625, LIMITS)
    d["features"] = torch.ones((2 * n_per, 4), device="cuda")
    d["transform"] = T
    cfg = make_cfg()
    torch.manual_seed(3)
    np.random.seed(3)                                  # (the kernel points of a fresh KPConv come from numpy's global RNG)
    net = GeoTransformer(cfg).cuda()
    res = {"cfg": cfg, "data": d, "net": net}
    net.eval()
    res["eval_before"] = net(d)
    with gaussreg_amd.differentiable():
        pass
    res["eval_after"] = net(d)
    net.train()
    crit, opt = OverallLoss(cfg), torch.optim.Adam(net.parameters(), lr=1e-4)
    losses = []
    for it in range(6):                                 # five updates; the sixth forward measures the last one
        net.coarse_target.generator = np.random.RandomState(5)       # the same targets every step: a fixed problem
        opt.zero_grad(set_to_none=True)
        with gaussreg_amd.differentiable():
            out = net(d)
            loss = crit(out, d)
        losses.append({k: float(v.detach()) for k, v in loss.items()})
        if it == 5:
            break
        loss["loss"].backward()
        if it == 0:
            res["out"], res["grads"] = out, {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
            res["params"] = [k for k, _ in net.named_parameters()]
            res["metrics"] = Evaluator(cfg)(out, d)
            res["coarse_precision"] = float(Evaluator(cfg).evaluate_coarse(out))
        opt.step()
    res["losses"] = losses
    print("\ntraining step losses:", " ".join(f"{l['loss']:.4f}" for l in losses))
    return res


def test_training_output_keys_are_the_references(step):
    assert set(step["out"]) == REFERENCE_KEYS | EXTRA_KEYS
    assert step["out"]["matching_scores"].requires_grad and step["out"]["ref_feats_c"].requires_grad
    for k in ("ref_corr_points", "corr_scores", "estimated_transform", "gt_node_corr_overlaps"):
        assert not step["out"][k].requires_grad, k
    assert set(step["metrics"]) == {"RRE", "RTE", "RSE", "RMSE", "RR"} and 0.0 <= step["coarse_precision"] <= 1.0


def test_ground_truth_correspondences_equal_the_standalone_call(step):
    from gaussreg_amd.matching import get_node_correspondences
    from gaussreg_amd.ops import index_select, point_to_node_partition
    o, d = step["out"], step["data"]
    sides = []
    for side in ("ref", "src"):
        pf, pc = o[f"{side}_points_f"], o[f"{side}_points_c"]
        _, nm, idx, km = point_to_node_partition(pf, pc, 128)
        sides.append((pc, index_select(torch.cat([pf, torch.zeros_like(pf[:1])], 0), idx, dim=0), nm, km))
    (rc, rk, rnm, rkm), (sc, sk, snm, skm) = sides
    gi, go, gd = get_node_correspondences(rc, sc, rk, sk, d["transform"], 0.05, rnm, snm, rkm, skm, return_dense=True)
    assert gi.shape[0] > 100
    assert torch.equal(gi, o["gt_node_corr_indices"]) and torch.equal(go, o["gt_node_corr_overlaps"])
    assert torch.equal(gd, o["gt_node_corr_overlap_matrix"])
    # the targets are ground-truth pairs above the overlap threshold
    assert o["matching_scores"].shape[0] == min(128, int((go > 0.1).sum())) == o["ref_node_corr_knn_points"].shape[0]


def test_loss_and_every_gradient_are_finite(step):
    first = step["losses"][0]
    assert all(np.isfinite(v) for v in first.values()) and first["c_loss"] > 0 and first["f_loss"] > 0
    assert abs(first["loss"] - (first["c_loss"] + first["f_loss"])) <= 1e-5 * first["loss"]
    missing = [k for k in step["params"] if k not in step["grads"]]
    assert not missing, missing
    bad = [k for k, g in step["grads"].items() if not bool(torch.isfinite(g).all())]
    assert not bad, bad
    for k in ("optimal_transport.alpha", "backbone.encoder1_1.KPConv.weights", "transformer.in_proj.weight"):
        assert bool(step["grads"][k].any()), k     # the gradient reaches Sinkhorn's alpha, the first KPConv, the transformer


def test_five_adam_steps_lower_the_loss(step):
    losses = [l["loss"] for l in step["losses"]]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_eval_output_is_untouched_by_a_differentiable_block(step):
    a, b = step["eval_before"], step["eval_after"]
    assert set(a) == set(b) == (REFERENCE_KEYS | {"lgr_transform"}) - {"gt_node_corr_indices", "gt_node_corr_overlaps"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert not a[k].requires_grad, k


def test_training_outside_differentiable_is_refused(step):
    net = step["net"]
    assert net.training
    with pytest.raises(RuntimeError, match="inference branch only.*differentiable"):
        net(step["data"])
    import gaussreg_amd
    with gaussreg_amd.differentiable(), torch.no_grad(), pytest.raises(RuntimeError, match="inference branch only"):
        net(step["data"])
