"""CPU: the float64 statement of GS fusion (tests/gs_fusion_f64.py) pinned without a GPU -- its band matrices against
orthogonality, the band-1 closed form and the colour identity at fresh directions; its fields against oracle/fusion_np and
against the golden of the reference's own gaussian_fuse; the render statement that makes the GPU render check meaningful;
the reference arithmetic's orientation error that sets the GPU bar; and five doctored outputs that must be rejected."""
import functools
import math

import numpy as np
import pytest
import torch

import gs_fusion_cases as C
import gs_fusion_f64 as F
import raster_torch64 as rt
from gaussreg_amd import synthetic
from helpers import load_golden
from oracle import fusion_np

# fp32 level of the reference's quaternion path: about ten roundings of entries of size <= 1 in quaternion -> matrix,
# three products and two sums per entry of R32 . m, a square root and a division; 32 x 2^-24 bounds their sum with room
FP32_LEVEL = 32 * 2.0 ** -24
BG = [0.25, 0.5, 0.1]


@functools.lru_cache(maxsize=None)
def reference_fused(name, quaternions):
    tr = C.TRANSFORMS[name]
    rec = C.parity_cloud(quaternions)
    return rec, fusion_np.gaussian_fuse(C.far_cloud(), rec, tr["T"])


@pytest.mark.parametrize("name", list(C.TRANSFORMS))
def test_band_matrices_are_orthogonal_match_the_closed_form_and_keep_the_colour(name):
    R = C.TRANSFORMS[name]["R"]
    A = F.band_matrices(R)
    assert [a.shape for a in A] == [(3, 3), (5, 5), (7, 7)]
    for a in A:
        assert np.abs(a @ a.T - np.eye(a.shape[0])).max() <= 1e-12
    assert np.abs(A[0] - F.band1_closed_form(R)).max() <= 1e-12
    # fresh directions and coefficients: the colour seen from R d is the colour that was seen from d
    rng = np.random.default_rng(99)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.abs(d[:, None] - F.fit_directions()[None]).sum(2).min() > 1e-6    # none of them is a fitted direction
    for a, still, moved in zip(A, F.sh_rows(d), F.sh_rows(d @ R.T)):
        old = rng.normal(size=(a.shape[0], 40))
        assert np.abs(moved @ (a @ old) - still @ old).max() <= 1e-12
    if name == "general":   # the statement is not symmetric: the transposed matrices break it
        still, moved = F.sh_rows(d)[0], F.sh_rows(d @ R.T)[0]
        assert np.abs(moved @ A[0].T - still).max() > 0.1


def test_cases_reach_the_branches_they_are_meant_for():
    for name, tr in C.TRANSFORMS.items():
        A = tr["T"][:3, :3]
        scale = float((A @ A.T)[0, 0] ** 0.5)       # what the library derives from the matrix it is given
        assert (scale == 1.0) == (name in C.UNIT_SCALE) and (tr["s"] == 1.0) == (name in C.UNIT_SCALE), name
        assert abs(scale - tr["s"]) <= 1e-15 and np.abs(tr["R"] @ tr["R"].T - np.eye(3)).max() <= 1e-15
        assert abs(np.linalg.det(tr["R"]) - 1.0) <= 1e-15 and (tr["t"].any() or name == "identity")
    assert abs(1.0 + np.trace(C.TRANSFORMS["pi_skew"]["R"])) <= 1e-15 and np.trace(C.TRANSFORMS["zflip"]["R"]) == -1.0
    assert np.trace(C.TRANSFORMS["perm120"]["R"]) == 0.0    # all four qa tie at 1 for an identity quaternion
    assert abs(math.log(C.TRANSFORMS["tiny"]["s"]) - 1e-6) <= 1e-11
    for variant, lo, hi in (("generated", 0.5, 2.0), ("identity", 1.0, 1.0), ("norms", 1e-3, 1e3)):
        n = np.linalg.norm(C.parity_cloud(variant)[:, 58:62].astype(np.float64), axis=1)
        assert lo * (1 - 1e-6) <= n.min() and n.max() <= hi * (1 + 1e-6), variant
        assert variant == "identity" or (n.min() <= lo * 1.1 and n.max() >= hi * 0.9), variant
    rec = C.records_from_gaussians(50, 2)
    assert (np.abs(rec[:, 3:6]) >= 0.25).all()      # non-zero normals: the output must zero them
    # records_from_gaussians inverts gs_io.split_records
    from gaussreg_amd.gs_io import split_records
    g, d = synthetic.gaussians_c2(50, 2), split_records(rec)
    for k in ("means3D", "shs"):
        assert np.array_equal(d[k].numpy(), g[k]), k
    for k in ("opacities", "scales", "rotations"):
        assert np.abs(d[k].numpy().astype(np.float64) - g[k]).max() <= 4 * 2.0 ** -24, k


@pytest.mark.parametrize("quaternions", C.QUATERNIONS)
@pytest.mark.parametrize("name", list(C.TRANSFORMS))
def test_twin_agrees_with_reference_arithmetic(name, quaternions):
    """oracle/fusion_np passes the comparison the GPU has to pass: xyz, log-scales and SH within one fp32 rounding of the
    twin, the orientation matrices at the fp32 level.  The orientation error printed here is the reference arithmetic's
    own (docs/gs_fusion_f64_errors.md); four times it is the GPU's bar."""
    tr = C.TRANSFORMS[name]
    rec, fused = reference_fused(name, quaternions)
    err = C.reference_orientation_error(rec, tr)
    out = F.compare_fused(f"{name}/{quaternions}", fused, C.far_cloud(), rec, tr, FP32_LEVEL)
    print(f"{name}/{quaternions}: reference orientation error {err:.3e}; xyz {out['xyz']:.3f}, log-scales "
          f"{out['log_scales']:.3f}, f_rest {out['f_rest']:.3f} of the bar; min gap {out['min_gap']:.3g}")
    assert out["kept"] == (1, C.N_PARITY) and out["min_gap"] > 1e3
    assert out["orientation"] == err <= FP32_LEVEL


def test_twin_agrees_with_the_reference_golden():
    g = load_golden("gs_fusion.npz")
    T = g["transform"].astype(np.float64)
    s = np.linalg.det(T[:3, :3]) ** (1.0 / 3.0)
    tr = dict(s=float(s), R=T[:3, :3] / s, t=T[:3, 3], T=T)
    assert np.abs(tr["R"] @ tr["R"].T - np.eye(3)).max() <= 1e-12
    out = F.compare_fused("golden", g["fused"], g["rec1"], g["rec2"], tr, FP32_LEVEL)
    print("golden:", out)
    assert 0 < out["kept"][0] < g["rec1"].shape[0] and 0 < out["kept"][1] < g["rec2"].shape[0]


@pytest.mark.parametrize("name", list(C.TRANSFORMS))
def test_render_statement_moved_scene_equals_moved_camera(name):
    """The float64 rasterizer gives the same image for the statement's moved Gaussians seen from a camera and for the
    unmoved Gaussians seen from pose.similarity_camera.  Measured: 1.3e-6 ... 2.1e-6, and 2.0e-6 already at the
    identity transform: synthetic.camera stores its projmatrix rounded to fp32 (entries off by up to 6.6e-8 from
    viewmatrix times the perspective matrix), similarity_camera derives the moved one from the viewmatrix in float64,
    so the two cameras place a Gaussian some 1e-6 px apart.  With the fp32 projmatrix given to both renders the
    identity case agrees to 2.5e-9.  Bar: 1e-5, four to five times the measured figures."""
    W, H, P = 96, 72, 400
    tr = C.TRANSFORMS[name]
    rec = C.pull_back(C.records_from_gaussians(P, 5), tr)
    cam = synthetic.camera(W, H, R_c2w=synthetic.rot_yx(0.2, -0.1), C=(0.2, -0.1, -0.5))
    cam2 = F.moved_camera(cam, tr, W, H)
    moved = F.render_inputs(rec, tr)
    # the near-plane cull (z <= 0.2) acts on the unscaled depth of each frame: stay twice as far in both
    z_moved_scene, z_moved_camera = F.view_depths(cam, moved["means3D"].numpy()), F.view_depths(cam2, rec[:, 0:3])
    assert z_moved_scene.min() > 0.4 and z_moved_camera.min() > 0.4
    assert np.abs(z_moved_scene - tr["s"] * z_moved_camera).max() <= 1e-5
    a, radii = rt.render(rt.camera_dict(cam, W, H), BG, sh_degree=3, **moved)
    b, _ = rt.render(cam2, BG, sh_degree=3, **F.render_inputs(rec))
    diff = (a - b).abs().amax(0)
    lit = ((a - torch.tensor(BG, dtype=torch.float64)[:, None, None]).abs().amax(0) > 1e-3).double().mean().item()
    print(f"{name}: max |a - b| = {diff.max().item():.3e}; {int((radii > 0).sum())} of {P} visible; {lit:.2f} of the pixels lit")
    assert (radii > 0).sum().item() >= P // 2 and lit >= 0.1
    assert diff.max().item() <= 1e-5


# ------------------------------------------------------------------------------------------ the comparisons must bite
def _honest(name="general", quaternions="generated"):
    tr = C.TRANSFORMS[name]
    rec, fused = reference_fused(name, quaternions)
    return tr, rec, fused.copy()


def _doctor_bands_transposed(tr, rec, fused):
    A = [a.T for a in F.band_matrices(tr["R"])]
    fused[1:, 9:54] = F.transformed(rec, tr, bands=A)["f_rest"].astype(np.float32)


def _doctor_quaternion_conjugated(tr, rec, fused):
    fused[1:, 59:62] *= -1.0


def _doctor_log_scale_subtracted(tr, rec, fused):
    fused[1:, 55:58] = (rec[:, 55:58].astype(np.float64) - math.log(tr["s"])).astype(np.float32)


def _doctor_coefficient_major(tr, rec, fused):
    new = fused[1:, 9:54].reshape(-1, 3, 15)
    fused[1:, 9:54] = np.transpose(new, (0, 2, 1)).reshape(-1, 45)


DOCTORS = {"bands_transposed": _doctor_bands_transposed, "quaternion_conjugated": _doctor_quaternion_conjugated,
           "log_scale_subtracted": _doctor_log_scale_subtracted, "coefficient_major": _doctor_coefficient_major}


@pytest.mark.parametrize("doctor", list(DOCTORS))
def test_comparison_rejects_doctored_fields(doctor):
    tr, rec, fused = _honest()
    far = C.far_cloud()
    bar = 4.0 * C.reference_orientation_error(rec, tr)      # the GPU file's bar
    F.compare_fused("honest", fused, far, rec, tr, bar)
    DOCTORS[doctor](tr, rec, fused)
    with pytest.raises(AssertionError, match=doctor):
        F.compare_fused(doctor, fused, far, rec, tr, bar)


def test_comparison_rejects_a_row_that_should_have_been_dropped():
    tr = C.TRANSFORMS["general"]
    rec1, rec2 = C.overlapping_pair(63, 65, tr, 40)
    keep1, keep2, _, _ = F.selection(rec1, rec2, tr)
    assert 0 < keep2.sum() < 65 and 0 < keep1.sum() < 63
    fused = fusion_np.gaussian_fuse(rec1, rec2, tr["T"])
    bar = 4.0 * C.reference_orientation_error(rec2, tr)
    F.compare_fused("honest", fused, rec1, rec2, tr, bar)
    # one dropped vertex of cloud 2, honestly moved, slipped in at its place in input order
    extra = int(np.nonzero(~keep2)[0][0])
    k1 = int(keep1.sum())
    at = k1 + int(keep2[:extra].sum())
    all_moved = fusion_np.gaussian_fuse(C.far_cloud(), rec2, tr["T"])[1:]
    with pytest.raises(AssertionError, match="extra_row"):
        F.compare_fused("extra_row", np.insert(fused, at, all_moved[extra], axis=0), rec1, rec2, tr, bar)
    # ... and the same count with a dropped row in the place of a kept one
    swapped = fused.copy()
    swapped[at] = all_moved[extra]
    with pytest.raises(AssertionError, match="swapped_row"):
        F.compare_fused("swapped_row", swapped, rec1, rec2, tr, bar)


@pytest.mark.parametrize("name", ("general", "pi_skew"))
@pytest.mark.parametrize("n1,n2", C.SIZE_PAIRS)
def test_margin_filter_removes_at_most_one_percent(n1, n2, name):
    """The GPU selection test filters its inputs with this margin; the share it removes is recorded in the errors doc."""
    tr = C.TRANSFORMS[name]
    rec1, rec2 = C.overlapping_pair(n1, n2, tr, 40)
    f1, f2, removed = F.margin_filter(rec1, rec2, tr, C.KEEP_MARGIN)
    keep1, keep2, gap1, gap2 = F.selection(f1, f2, tr)
    print(f"{name} ({n1}, {n2}): removed {removed:.2e}; kept {int(keep1.sum())} + {int(keep2.sum())}; "
          f"min gap {min(gap1.min(), gap2.min()):.3g}")
    assert removed <= 0.01 and min(gap1.min(), gap2.min()) >= C.KEEP_MARGIN
    if (n1, n2) == (1, 1):
        assert removed == 0.0 and keep1.all() and keep2.all()
    want = fusion_np.gaussian_fuse(f1, f2, tr["T"])
    F.compare_fused(f"{name}/{n1}x{n2}", want, f1, f2, tr, FP32_LEVEL)
