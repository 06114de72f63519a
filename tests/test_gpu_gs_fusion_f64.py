"""GPU: gr_gs_fuse (gaussreg_amd/csrc/gs_fusion.hip through gs_io.gaussian_fuse_records) against the float64 statement
of fusion (tests/gs_fusion_f64.py, pinned on the CPU by tests/test_gs_fusion_f64_reference.py) on the cases of
tests/gs_fusion_cases.py, and the product check: the fused scene renders as the unmoved scene does from the moved camera.

Where every bar comes from (none is taken from the kernel's output):
  xyz, log-scales, f_rest, bit-equal fields   derivations in gs_fusion_f64.compare_transformed
  orientation                                 4 x the error of the reference arithmetic (oracle/fusion_np's fp32 quaternion
                                              path) on the same records and transform: the kernel runs the same fp32
                                              operation sequence and may differ only in the rounding of single operations
  keep rule                                   inputs filtered to a float64 gap of 1e-4, about 1000 x the fp32 noise of the
                                              reference's centres; then the row set and order are exact
  render                                      the project's forward rule (test_gpu_rasterizer_backward.compare_all): at
                                              most 1e-3 of the pixels differ by more than 1e-4
Measured figures: docs/gs_fusion_f64_errors.md."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gs_fusion_cases as C  # noqa: E402
import gs_fusion_f64 as F  # noqa: E402
import raster_torch64 as rt  # noqa: E402
from gaussreg_amd import synthetic  # noqa: E402
from gaussreg_amd.gs_io import gaussian_fuse_records, split_records  # noqa: E402
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402

pytestmark = pytest.mark.gpu
BG = [0.25, 0.5, 0.1]


def fuse(rec1, rec2, tr):
    return gaussian_fuse_records(rec1, rec2, tr["T"]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def parity_bar(name, quaternions):
    return 4.0 * C.reference_orientation_error(C.parity_cloud(quaternions), C.TRANSFORMS[name])


@pytest.mark.parametrize("quaternions", C.QUATERNIONS)
@pytest.mark.parametrize("name", list(C.TRANSFORMS))
def test_per_field_parity(name, quaternions):
    tr, rec, far = C.TRANSFORMS[name], C.parity_cloud(quaternions), C.far_cloud()
    bar = parity_bar(name, quaternions)
    got = fuse(far, rec, tr)
    out = F.compare_fused(f"{name}/{quaternions}", got, far, rec, tr, bar)
    print(f"{name}/{quaternions}: xyz {out['xyz']:.3f}, log-scales {out['log_scales']:.3f}, f_rest {out['f_rest']:.3f} of "
          f"the bar; orientation {out['orientation']:.3e} (bar {bar:.3e})")
    assert out["kept"] == (1, C.N_PARITY)


@pytest.mark.parametrize("name", ("general", "pi_skew"))
@pytest.mark.parametrize("n1,n2", C.SIZE_PAIRS)
def test_keep_rule_small_and_general(n1, n2, name):
    tr = C.TRANSFORMS[name]
    rec1, rec2 = C.overlapping_pair(n1, n2, tr, 40)
    rec1, rec2, removed = F.margin_filter(rec1, rec2, tr, C.KEEP_MARGIN)
    assert removed <= 0.01, f"the margin filter removed {removed:.3%} of the vertices"
    bar = 4.0 * C.reference_orientation_error(rec2, tr)
    got = fuse(rec1, rec2, tr)
    out = F.compare_fused(f"{name}/{n1}x{n2}", got, rec1, rec2, tr, bar)
    print(f"{name} ({n1}, {n2}): removed {removed:.2e}; kept {out['kept']}; min gap {out['min_gap']:.3g}; xyz "
          f"{out['xyz']:.3f}, f_rest {out['f_rest']:.3f} of the bar; orientation {out['orientation']:.3e} (bar {bar:.3e})")
    assert out["min_gap"] >= C.KEEP_MARGIN
    if (n1, n2) == (1, 1):
        assert removed == 0.0 and out["kept"] == (1, 1)
    else:
        assert out["kept"][1] < rec2.shape[0]       # the rule drops something: the clouds do overlap
    if n1 > 64:
        assert out["kept"][0] < rec1.shape[0]


def _settings(cam, W, H):
    d = torch.device("cuda")

    def f32(a):
        return torch.as_tensor(np.asarray(a, np.float32)).to(d)
    return GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], torch.tensor(BG, device=d), 1.0,
                                         f32(cam["viewmatrix"]), f32(cam["projmatrix"]), 3, f32(cam["campos"]), False, False)


def _hip_render(cam, W, H, rec):
    g = split_records(torch.as_tensor(rec).cuda())
    with torch.no_grad():
        img, radii = GaussianRasterizer(_settings(cam, W, H))(g["means3D"], None, g["opacities"], shs=g["shs"],
                                                              scales=g["scales"], rotations=g["rotations"])
    return img.double(), radii


@pytest.mark.parametrize("name", ("general", "pi_skew"))
def test_fused_scene_renders_as_the_moved_camera_sees_the_unmoved_one(name):
    W, H, P = 120, 88, 2500
    tr = C.TRANSFORMS[name]
    rec = C.pull_back(C.records_from_gaussians(P, 8), tr)
    cam = synthetic.camera(W, H, R_c2w=synthetic.rot_yx(0.2, -0.1), C=(0.2, -0.1, -0.5))
    cam2 = F.moved_camera(cam, tr, W, H)
    # the near-plane cull (z <= 0.2) acts on the unscaled depth of each frame: stay twice as far in both
    z_fused = F.view_depths(cam, F.transformed(rec, tr)["xyz"])
    z_moved = F.view_depths(cam2, rec[:, 0:3])
    assert z_fused.min() > 0.4 and z_moved.min() > 0.4
    assert np.abs(z_fused - tr["s"] * z_moved).max() <= 1e-5        # the same depths, up to the similarity scale
    # the reference: float64, the UNMOVED records from the moved camera -- no fusion arithmetic enters it
    ref, _ = rt.render(cam2, BG, chunk=2048, sh_degree=3, **F.render_inputs(rec, device="cuda"))
    lit = ((ref - torch.tensor(BG, dtype=torch.float64, device="cuda")[:, None, None]).abs().amax(0) > 1e-3).double().mean().item()
    assert lit >= 0.3, f"only {lit:.2f} of the pixels differ from the background"
    # (a) HIP fuse -> split_records -> HIP rasterizer from the original camera
    fused = fuse(C.far_cloud(), rec, tr)
    assert fused.shape == (P + 1, 62)
    img_a, radii = _hip_render(cam, W, H, fused[1:])        # row 0 is the far cloud
    assert (radii > 0).sum().item() >= P // 2
    # (b) HIP rasterizer on the unmoved records from the moved camera
    img_b, radii_b = _hip_render(cam2, W, H, rec)
    assert (radii_b > 0).sum().item() >= P // 2
    diff_a, diff_b = (img_a - ref).abs().amax(0), (img_b - ref).abs().amax(0)
    share_a, share_b = (diff_a > 1e-4).double().mean().item(), (diff_b > 1e-4).double().mean().item()
    print(f"{name}: {int((radii > 0).sum())} of {P} visible, {lit:.2f} of the pixels lit; fused: max {diff_a.max().item():.3e}, "
          f"{share_a:.2e} of the pixels over 1e-4; moved camera: max {diff_b.max().item():.3e}, {share_b:.2e} over 1e-4")
    assert share_a <= 1e-3, f"{name}: fused scene, {share_a:.3e} of the pixels differ by more than 1e-4"
    assert share_b <= 1e-3, f"{name}: moved camera, {share_b:.3e} of the pixels differ by more than 1e-4"


def test_empty_clouds():
    tr = C.TRANSFORMS["general"]
    rec = C.records_from_gaussians(70, 3)
    empty = np.zeros((0, 62), np.float32)
    for a, b in ((empty, rec), (rec, empty)):
        with pytest.raises(RuntimeError, match="both clouds must be non-empty"):
            gaussian_fuse_records(a, b, tr["T"])
    out = gaussian_fuse_records(empty, empty, tr["T"])
    assert tuple(out.shape) == (0, 62) and out.dtype == torch.float32 and out.is_cuda
    # the library still works after the refusals
    F.compare_fused("after refusal", fuse(C.far_cloud(), rec, tr), C.far_cloud(), rec, tr,
                    4.0 * C.reference_orientation_error(rec, tr))
