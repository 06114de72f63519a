"""Test helper (not collected): what GS fusion MEANS, in float64, written from the statement and not from the code.

Fusing moves cloud 2 by the similarity x -> s R x + t and keeps, of both clouds, the vertices closer to their own
cloud's centre.  For a moved Gaussian that means

  position      x' = s R x + t
  extent        log-scales + ln s
  orientation   R . R(q), compared as a MATRIX (R(q') of the normalised output quaternion): q and -q, and whichever of
                the four branches a matrix-to-quaternion routine takes, give the same matrix
  colour        the colour seen from the direction R d is the colour that was seen from d.  With Y_l the band-l row of
                the basis the rasterizer evaluates (tests/raster_torch64.sh_basis) that is Y_l(R d) . new = Y_l(d) . old
                for every d.  Band l spans a rotation-invariant space, so there is A_l with Y_l(R d) A_l = Y_l(d), and
                new = A_l old.  A_l is fitted here by float64 least squares over 256 seeded directions, solved for
                directly (no transpose or inverse is taken, no orthogonality assumed).
  unchanged     f_dc, opacity; the normals are written as zeros
  keep rule     |x - c_own| < |x - c_other| with c the float64 means of cloud 1 and of the moved cloud 2; `gap` is
                | |x - c_own| - |x - c_other| |, the margin of that decision

Nothing here is shared with gaussreg_amd/gs_io.py or oracle/fusion_np.py: the quaternion is applied to the basis vectors
as v + 2 w (u x v) + 2 u x (u x v), the band matrices come from the rasterizer twin's basis.

The compare_* functions return the per-field maximum errors and raise AssertionError naming the case.
"""
import math

import numpy as np
import torch

import raster_torch64 as rt

BANDS = ((0, 3), (3, 8), (8, 15))   # coefficient ranges of bands 1..3 inside one channel of f_rest
FIT_DIRECTIONS, FIT_SEED = 256, 2024
F64_NOISE = 1e-14                   # float64 rounding of a few operations on values of order one, with a wide margin
HALF_ULP = 2.0 ** -24               # one rounding to fp32: |error| <= 2^-24 |value|


# ------------------------------------------------------------------------------------------------ the statement
def rotation_of(q):
    """(n, 4) quaternions, real part first, any non-zero norm -> (n, 3, 3) float64 rotation matrices."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, u = q[:, 0:1], q[:, 1:4]
    cols = []
    for k in range(3):
        v = np.zeros_like(u)
        v[:, k] = 1.0
        uv = np.cross(u, v)
        cols.append(v + 2.0 * w * uv + 2.0 * np.cross(u, uv))
    return np.stack(cols, 2)   # column k is the image of e_k


def sh_rows(d):
    """(n, 3) unit directions -> the (n, 3), (n, 5), (n, 7) rows of bands 1..3 as the rasterizer reads them."""
    Y = rt.sh_basis(torch.as_tensor(np.asarray(d, np.float64)), 3).numpy()
    return Y[:, 1:4], Y[:, 4:9], Y[:, 9:16]


def fit_directions(n=FIT_DIRECTIONS, seed=FIT_SEED):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def band_matrices(R):
    """A_1 (3x3), A_2 (5x5), A_3 (7x7) with Y_l(R d) A_l = Y_l(d): new band = A_l @ old band."""
    d = fit_directions()
    moved = sh_rows(d @ np.asarray(R, np.float64).T)
    still = sh_rows(d)
    return tuple(np.linalg.lstsq(m, s, rcond=None)[0] for m, s in zip(moved, still))


def band1_closed_form(R):
    """Band 1 is C1 (-y, z, -x) = C1 P d: Y_1(R d) = Y_1(d) (P R P^T)^T, so A_1 = P R P^T."""
    P = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    return P @ np.asarray(R, np.float64) @ P.T


def transformed(rec, tr, bands=None):
    """The fields of the moved records, float64: xyz (n,3), log_scales (n,3), orientation (n,3,3), f_rest (n,45)
    channel-major, band_norm (n,45): for every coefficient the 2-norm of the OLD band it is computed from."""
    rec = np.asarray(rec, np.float32).astype(np.float64)
    n = rec.shape[0]
    A = band_matrices(tr["R"]) if bands is None else bands
    old = rec[:, 9:54].reshape(n, 3, 15)
    new, norm = np.empty_like(old), np.empty_like(old)
    for (lo, hi), a in zip(BANDS, A):
        new[:, :, lo:hi] = np.einsum("ji,nci->ncj", a, old[:, :, lo:hi])
        norm[:, :, lo:hi] = np.linalg.norm(old[:, :, lo:hi], axis=2, keepdims=True)
    return dict(xyz=tr["s"] * (rec[:, 0:3] @ tr["R"].T) + tr["t"], log_scales=rec[:, 55:58] + math.log(tr["s"]),
                orientation=tr["R"][None] @ rotation_of(rec[:, 58:62]), f_rest=new.reshape(n, 45),
                band_norm=norm.reshape(n, 45))


def selection(rec1, rec2, tr):
    """-> keep1, keep2 (bool), gap1, gap2 (float64): the keep rule on cloud 1 and on the moved cloud 2."""
    x1 = np.asarray(rec1, np.float32)[:, 0:3].astype(np.float64)
    x2 = tr["s"] * (np.asarray(rec2, np.float32)[:, 0:3].astype(np.float64) @ tr["R"].T) + tr["t"]
    c1, c2 = x1.mean(0), x2.mean(0)
    own1, other1 = np.linalg.norm(x1 - c1, axis=1), np.linalg.norm(x1 - c2, axis=1)
    own2, other2 = np.linalg.norm(x2 - c2, axis=1), np.linalg.norm(x2 - c1, axis=1)
    return own1 < other1, own2 < other2, np.abs(own1 - other1), np.abs(own2 - other2)


def margin_filter(rec1, rec2, tr, margin):
    """Take out of both inputs the vertices whose gap is below `margin`, until none is left (the centres move a
    little with every cut).  -> rec1, rec2, the share of the vertices removed."""
    n = rec1.shape[0] + rec2.shape[0]
    for _ in range(8):
        _, _, g1, g2 = selection(rec1, rec2, tr)
        if g1.min() >= margin and g2.min() >= margin:
            break
        rec1, rec2 = rec1[g1 >= margin], rec2[g2 >= margin]
    else:
        raise AssertionError("margin_filter did not settle")
    return rec1, rec2, 1.0 - (rec1.shape[0] + rec2.shape[0]) / n


# ------------------------------------------------------------------------------------------------ comparisons
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare_transformed(case, got, rec, tr, orientation_bar):
    """`got`: (n, 62) fp32 rows that claim to be `rec` moved by `tr`.  Bars (each is the bound of the rounding the
    statement allows, plus float64 noise of the comparison itself):
      xyz, log-scales   one rounding of the float64 value to fp32: 2^-24 |value|
      ... at s == 1.0   log-scales bit-equal to the input;  at the identity transform xyz bit-equal too
      normals           zero
      f_dc, opacity     bit-equal to the input
      f_rest            per coefficient 2^-23 ||old band||_2: a float64 sum over band-matrix entries rounded to fp32
                        (rows of an orthogonal matrix: 2^-24 ||old||_2 by Cauchy-Schwarz) and one rounding of the
                        result (2^-24 |new| <= 2^-24 ||old||_2)
      orientation       max entry of R(q') - R . R(q) at most `orientation_bar`, which the caller takes from the
                        reference arithmetic's own error
    -> dict of the maximum errors, in units of the bar for xyz / log_scales / f_rest (1.0 = the bar), absolute for the
    orientation."""
    got = np.asarray(got, np.float32)
    rec = np.asarray(rec, np.float32)
    assert got.shape == rec.shape, f"{case}: {got.shape} rows for {rec.shape} records"
    if rec.shape[0] == 0:
        return dict(xyz=0.0, log_scales=0.0, f_rest=0.0, orientation=0.0)
    want = transformed(rec, tr)
    g = got.astype(np.float64)
    out = {}

    def ratio(name, err, bar):
        r = err / bar
        worst = np.unravel_index(np.argmax(r), r.shape)
        out[name] = float(r[worst])
        assert r[worst] <= 1.0, (f"{case}: {name} of row {worst[0]}, column {worst[1]}: error {err[worst]:.3e} is "
                                 f"{r[worst]:.3g} x the bar {bar[worst]:.3e}")

    x = rec[:, 0:3].astype(np.float64)
    noise = F64_NOISE * (tr["s"] * np.abs(x).sum(1, keepdims=True) + np.abs(tr["t"]).max() + 1.0)
    ratio("xyz", np.abs(g[:, 0:3] - want["xyz"]), HALF_ULP * np.abs(want["xyz"]) + noise)
    ratio("log_scales", np.abs(g[:, 55:58] - want["log_scales"]), HALF_ULP * np.abs(want["log_scales"]) + F64_NOISE)
    if tr["s"] == 1.0:
        assert np.array_equal(_bits(got[:, 55:58]), _bits(rec[:, 55:58])), f"{case}: log-scales changed at scale 1.0"
        if np.array_equal(tr["R"], np.eye(3)) and not tr["t"].any():
            assert np.array_equal(_bits(got[:, 0:3]), _bits(rec[:, 0:3])), f"{case}: xyz changed by the identity"
    assert not got[:, 3:6].any(), f"{case}: non-zero normals"
    assert np.array_equal(_bits(got[:, 6:9]), _bits(rec[:, 6:9])), f"{case}: f_dc changed"
    assert np.array_equal(_bits(got[:, 54]), _bits(rec[:, 54])), f"{case}: opacity changed"
    ratio("f_rest", np.abs(g[:, 9:54] - want["f_rest"]), 2.0 * HALF_ULP * want["band_norm"] + F64_NOISE * (want["band_norm"] + 1e-30))
    assert np.isfinite(g[:, 58:62]).all() and (np.linalg.norm(g[:, 58:62], axis=1) > 0).all(), f"{case}: bad quaternion"
    e = np.abs(rotation_of(g[:, 58:62]) - want["orientation"]).max(axis=(1, 2))
    out["orientation"] = float(e.max())
    assert e.max() <= orientation_bar, (f"{case}: orientation of row {int(e.argmax())}: max entry error {e.max():.3e} "
                                        f"> bar {orientation_bar:.3e}")
    return out


def compare_fused(case, got, rec1, rec2, tr, orientation_bar):
    """`got`: the fused (m, 62) array.  The kept rows of cloud 1, bit for bit except for zeroed normals, then the kept
    rows of cloud 2, moved: both in input order.  -> compare_transformed's errors plus `kept` and `min_gap`."""
    got = np.asarray(got, np.float32)
    rec1, rec2 = np.asarray(rec1, np.float32), np.asarray(rec2, np.float32)
    keep1, keep2, gap1, gap2 = selection(rec1, rec2, tr)
    k1, k2 = int(keep1.sum()), int(keep2.sum())
    assert got.shape == (k1 + k2, 62), f"{case}: {got.shape} fused, the keep rule leaves {k1} + {k2} rows"
    want1 = rec1[keep1].copy()
    want1[:, 3:6] = 0.0
    same = (_bits(got[:k1]) == _bits(want1)).all(1)
    assert same.all(), f"{case}: cloud-1 row {int(np.argmin(same))} of the output is not the kept input row"
    out = compare_transformed(case, got[k1:], rec2[keep2], tr, orientation_bar)
    out["kept"] = (k1, k2)
    out["min_gap"] = float(min(gap1.min(), gap2.min()))
    return out


# ------------------------------------------------------------------------------------------------ rendering
def _covariances(orientation, log_scales):
    M = orientation * np.exp(log_scales)[:, None, :]
    S = M @ np.transpose(M, (0, 2, 1))
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def _render_inputs(xyz, log_scales, orientation, f_dc, f_rest, logit, device):
    n = xyz.shape[0]
    shs = np.concatenate([f_dc.reshape(n, 1, 3), np.transpose(f_rest.reshape(n, 3, 15), (0, 2, 1))], 1)
    t = dict(means3D=xyz, opacities=1.0 / (1.0 + np.exp(-logit.reshape(n, 1))), shs=shs,
             cov3D_precomp=_covariances(orientation, log_scales))
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=device) for k, v in t.items()}


def render_inputs(rec, tr=None, device="cpu"):
    """What tests/raster_torch64.render takes, float64, for the records as they are (tr None) or moved by `tr` (the
    statement's values, never rounded to fp32).  The orientation enters as a covariance, so no quaternion is formed."""
    r = np.asarray(rec, np.float32).astype(np.float64)
    if tr is None:
        return _render_inputs(r[:, 0:3], r[:, 55:58], rotation_of(r[:, 58:62]), r[:, 6:9], r[:, 9:54], r[:, 54], device)
    w = transformed(rec, tr)
    return _render_inputs(w["xyz"], w["log_scales"], w["orientation"], r[:, 6:9], w["f_rest"], r[:, 54], device)


def moved_camera(cam, tr, W, H):
    """The camera from which the UNMOVED scene looks as the moved scene looks from `cam` (pose.similarity_camera), as
    the float64 dict raster_torch64 reads."""
    from gaussreg_amd import pose
    vm = torch.as_tensor(np.asarray(cam["viewmatrix"], np.float64))
    pm = torch.as_tensor(np.asarray(cam["projmatrix"], np.float64))
    vm2, pm2, cp2, _ = pose.similarity_camera(vm, tr["s"], tr["R"], tr["t"], projmatrix=pm)
    return dict(W=W, H=H, image_width=W, image_height=H, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                viewmatrix=vm2.numpy(), projmatrix=pm2.numpy(), campos=cp2.numpy())


def view_depths(cam, xyz):
    """View-space z of the points `xyz` (n, 3) under the camera dict `cam` (matrices stored transposed)."""
    vm = np.asarray(cam["viewmatrix"], np.float64)
    return np.asarray(xyz, np.float64) @ vm[:3, 2] + vm[3, 2]
