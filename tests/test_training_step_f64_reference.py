"""CPU: the float64 twin of the training step (tests/training_step_f64.py) and the yardstick of
tests/test_gpu_training_step_f64.py (tests/training_step_cases.py), pinned without a GPU and without the reference checkout.

* The twin in float64 on the stored cases reproduces what the reference's own GeoTransformer + OverallLoss gave in float64
  (tests/golden/training_step.npz): the three losses to 1e-12 relative, every gradient's norm and 8 projections to 1e-9 of
  the gradient's norm.  Float64 against float64: the slack covers summation order.  Observed (docs/training_step_f64_errors.md):
  losses 0 to 3.3e-16, gradients at most 1.4e-14.  The reference builds Sinkhorn's log-marginals in float32 in every dtype;
  the twin rounds them alike for this comparison only (`reference_marginals`), which moves f_loss by 2.5e-9 relative.
* The admission cap: float32 twin against float64 twin, rel_ref <= 1e-4 in every tensor ('max': the margin rule as well),
  and no bar decided by the float32 residue of the superpoints' self-distance (training_step_cases.check_self_distance).
* The stored inputs satisfy the conditions of the cases.
* The yardstick rejects planted errors and passes the unplanted float32 gradients.
"""
import numpy as np
import pytest
import torch

import training_step_cases as cases
import training_step_f64 as ts

NAMES = list(cases.CASES)


@pytest.fixture(scope="module")
def twins():
    """Per case, computed once and left unchanged: the stored case, the state, and the twins' runs."""
    from gaussreg_amd.model import GeoTransformer
    out = {}
    for name in NAMES:
        cfg = cases.case_cfg(name)
        np.random.seed(0)                                    # (kernel points of a fresh KPConv: numpy's global RNG; replaced)
        state = cases.init_state(GeoTransformer(cfg).state_dict(), cfg)
        case, ref = cases.load_case(name)
        hp = cases.hyper(cfg)
        keep = {}
        out[name] = dict(cfg=cfg, hp=hp, state=state, case=case, ref=ref, keep=keep,
                         f64=ts.run(state, case, hp, torch.float64, keep=keep),
                         f32=[ts.run(state, c, hp, torch.float32) for c in cases.orderings(case)])   # three draws: the median counts
    return out


@pytest.mark.parametrize("name", NAMES)
def test_state_is_the_generators(twins, name):
    t = twins[name]
    assert np.array_equal(cases.state_checksums(t["state"]), t["ref"]["param_sums"])
    assert np.array_equal(t["state"]["transformer.embedding.embedding.div_term"].numpy(), t["ref"]["div_term"])
    params = [n for n in t["state"] if not n.endswith(("kernel_points", "div_term"))]
    assert sorted(params) == sorted(t["ref"]["grads"]) == sorted(t["f64"][1])
    assert sum(t["state"][n].numel() for n in params) > 1_400_000


@pytest.mark.parametrize("name", NAMES)
def test_twin_reproduces_the_references_float64_step(twins, name):
    t = twins[name]
    losses, grads, terms = ts.run(t["state"], t["case"], t["hp"], torch.float64, reference_marginals=True)
    for k, want in zip(("loss", "c_loss", "f_loss"), t["ref"]["losses"]):
        print(f"\nTRSTEP cpu {name} {k}: reference {want:.15f} twin {losses[k]:.15f} relative {abs(losses[k] - want) / want:.2e}")
        assert abs(losses[k] - want) <= 1e-12 * abs(want), k
    worst = (0.0, None)
    for n, want in t["ref"]["grads"].items():
        assert grads[n] is not None, n
        _, _, _, scale, _ = cases.relative_errors(n, grads[n], grads[n], grads[n], terms)
        err = float(np.abs(cases.summarise(n, grads[n].numpy()) - want).max()) / scale
        worst = max(worst, (err, n))
        assert err <= 1e-9, (n, err)
    print(f"\nTRSTEP cpu {name} twin against the reference's norms and projections: worst {worst[0]:.2e} of the norm ({worst[1]})")
    # the float32 marginals of the reference are worth this much (why the GPU test's truth does not round them):
    print(f"TRSTEP cpu {name} f_loss with float64 marginals: relative {abs(t['f64'][0]['f_loss'] - losses['f_loss']) / losses['f_loss']:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_admission_cap(twins, name):
    t = twins[name]
    g32 = [r[1] for r in t["f32"]]
    worst, which = cases.check_admission(t["f64"][1], g32, t["f64"][2])
    print(f"\nTRSTEP cpu {name} admission: worst rel_ref {worst:.3e} ({which}), cap {cases.CAP:g}")
    ratio, tensor = cases.check_self_distance(t["state"], t["case"], t["hp"], t["f64"][1], g32, t["f64"][2])
    print(f"TRSTEP cpu {name} admission: largest move of a bar with the exact self-distance {ratio:.2f}x ({tensor}), "
          f"limit {cases.SELF_DISTANCE_FACTOR:g}x")
    for k in ("c_loss", "f_loss"):
        print(f"TRSTEP cpu {name} {k}: float32 twin error {np.median([abs(r[0][k] - t['f64'][0][k]) for r in t['f32']]):.3e}")
    if name == "max":
        margin, err = cases.max_margin(t["state"], t["case"])
        print(f"TRSTEP cpu max: smallest float64 margin {margin:.3e}, fp32 error of the angular values {err:.3e}")
        assert max(np.asarray(t["case"]["lengths"])[-1]) <= 8


@pytest.mark.parametrize("name", NAMES)
def test_stored_inputs_satisfy_the_case_conditions(twins, name):
    t = twins[name]
    rec = cases.check_case(name, t["case"], t["hp"])
    rec["min_feature_distance"] = cases.check_feature_distances(t["case"], t["hp"], t["keep"])
    print(f"\nTRSTEP cpu {name} case: {rec}")
    # the stored clouds are the builder's, and the stored targets are a fresh RandomState's draw
    ref, src, T = cases.clouds(name)
    assert np.array_equal(t["case"]["points"][0], np.concatenate([ref, src])) and np.array_equal(t["case"]["transform"], T)
    assert np.array_equal(t["case"]["features"], cases.features(name, len(ref) + len(src)))
    from gaussreg_amd.matching import SuperPointTargetGenerator
    gen = SuperPointTargetGenerator(t["cfg"].coarse_matching.num_targets, t["cfg"].coarse_matching.overlap_threshold,
                                    generator=np.random.RandomState(cases.TARGET_SEED))
    ref_ci, src_ci, _ = gen(torch.from_numpy(t["case"]["gt_indices"]).long(), torch.from_numpy(t["case"]["gt_overlaps"]))
    assert np.array_equal(ref_ci.numpy(), t["case"]["ref_ci"]) and np.array_equal(src_ci.numpy(), t["case"]["src_ci"])
    dense = np.zeros_like(t["case"]["overlaps"])
    dense[t["case"]["gt_indices"][:, 0], t["case"]["gt_indices"][:, 1]] = t["case"]["gt_overlaps"]
    assert np.array_equal(dense, t["case"]["overlaps"])


def test_same_decisions_leaves_only_the_order_inside_a_patch_free(twins):
    case = twins["mean"]["case"]
    cases.same_decisions(case, case)
    ci = int(case["ref_ci"][0])
    k = int(case["ref_knn_masks"][ci].sum())
    assert k >= 2
    slots = [t for t, c in enumerate(case["ref_ci"]) if c == ci]
    swapped = {key: np.array(v, copy=True) if not isinstance(v, list) else v for key, v in case.items()}
    swapped["ref_knn_idx"][ci, [0, 1]] = case["ref_knn_idx"][ci, [1, 0]]           # two points of one patch change places,
    for t in slots:                                                                 # points and labels move with them
        swapped["ref_corr_knn_points"][t, [0, 1]] = case["ref_corr_knn_points"][t, [1, 0]]
        swapped["labels"][t, [0, 1]] = case["labels"][t, [1, 0]]
    assert not np.array_equal(swapped["ref_knn_idx"], case["ref_knn_idx"])
    cases.same_decisions(swapped, case)
    for key, edit in (("labels", lambda a: a.__setitem__((slots[0], 0), ~a[slots[0], 0])),          # a label row flipped
                      ("ref_knn_idx", lambda a: a.__setitem__((ci, 0), a[ci, 0] + 1 if a[ci, 0] + 1 not in a[ci] else a[ci, 0] + 2)),
                      ("overlaps", lambda a: a.__setitem__((0, 0), a[0, 0] + 1e-7 + 1e-3)),
                      ("src_ci", lambda a: a.__setitem__(0, a[1]))):
        wrong = dict(swapped)
        wrong[key] = np.array(swapped[key], copy=True)
        edit(wrong[key])
        with pytest.raises(AssertionError):
            cases.same_decisions(wrong, case)
    # a label that stays behind when its points move is a different decision
    stale = dict(swapped)
    stale["labels"] = case["labels"]
    if not np.array_equal(case["labels"][slots[0], 0], case["labels"][slots[0], 1]):
        with pytest.raises(AssertionError):
            cases.same_decisions(stale, case)


def test_yardstick_passes_the_float32_twin_and_rejects_planted_errors(twins):
    t = twins["mean"]
    l64, g64, terms = t["f64"]
    draws_l, draws_g = [r[0] for r in t["f32"]], [r[1] for r in t["f32"]]
    l32, g32 = draws_l[0], draws_g[0]               # "got": the float32 twin's first draw; the bar: the median of the three
    quiet = lambda *a: None
    # the orderings are one function: float64 moves by summation order only
    _, g64_shuffled, _ = ts.run(t["state"], cases.orderings(t["case"])[2], t["hp"], torch.float64)
    assert max(float((g64_shuffled[n] - g).norm()) / max(float(g.norm()), 1e-300) for n, g in g64.items()
               if float(g.abs().max()) > 1e-12) <= 1e-12
    for got_l, got_g in zip(draws_l, draws_g):
        rows = cases.compare("cpu unplanted", got_g, g64, draws_g, terms, emit=quiet)
        assert len(rows) == len(g64)
        cases.compare_losses("cpu unplanted", got_l, l64, draws_l, emit=quiet)
        cases.compare_golden("cpu unplanted", got_g, t["ref"]["grads"], g64, draws_g, terms, emit=quiet)

    def rejected(got, expect):
        with pytest.raises(AssertionError, match=expect):
            cases.compare("cpu planted", got, g64, draws_g, terms, emit=quiet)

    # one tensor scaled by 1.01
    name = "backbone.encoder3_2.KPConv.weights"
    rejected({**g32, name: g32[name] * 1.01}, name.replace(".", r"\.") + ": rel_hip")
    with pytest.raises(AssertionError, match="rel_hip|>"):
        cases.compare_golden("cpu planted", {**g32, name: g32[name] * 1.01}, t["ref"]["grads"], g64, draws_g, terms, emit=quiet)
    # the fine loss's contribution dropped from the backbone gradients (where the coarse loss reaches: decoder2 keeps its own)
    _, c_only, _ = ts.run(t["state"], t["case"], t["hp"], torch.float32, which="c_loss")
    assert c_only["backbone.decoder2.mlp.weight"] is None and c_only["optimal_transport.alpha"] is None
    dropped = {n: (c_only[n] if n.startswith("backbone.") and c_only[n] is not None else g) for n, g in g32.items()}
    rejected(dropped, r"backbone\.encoder1_1\.KPConv\.weights: rel_hip")
    # a tensor without a gradient, and a gradient where the loss reaches nothing
    rejected({**g32, name: None}, "received no gradient")
    with pytest.raises(AssertionError, match="has a gradient"):
        cases.compare("cpu planted", g32, c_only, c_only, terms, emit=quiet)
    # the glue: 1/sqrt(C) omitted, ref and src exchanged in the patch gather, the zero shadow row read from row 0
    for variant in ("no_scale", "swap_patches", "shadow_row0"):
        lv, gv, _ = ts.run(t["state"], t["case"], t["hp"], torch.float32, variant=variant)
        rejected(gv, "rel_hip")
        with pytest.raises(AssertionError):
            cases.compare_losses("cpu planted", lv, l64, draws_l, emit=quiet)
    # a loss off by 1e-5 of its value
    with pytest.raises(AssertionError):
        cases.compare_losses("cpu planted", {**l32, "c_loss": l64["c_loss"] * (1 + 1e-5)}, l64, draws_l, emit=quiet)
