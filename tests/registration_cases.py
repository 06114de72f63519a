"""Test helper (not collected): the named, seeded cases shared by tests/test_registration_f64_reference.py (CPU: the
float64 restatements against the reference, and the admission rule) and tests/test_gpu_registration_f64.py (the HIP
solvers against the restatements).

Every cloud is built in a unit frame (src in [0,1]^3, ref = s R (src + e) + t with |e_k| <= NOISE, so an inlier's residual
is at most sqrt(3) NOISE s), then both clouds are multiplied by `g` and moved by `off`; thresholds scale with s g.  The
inputs of a case are the float32 arrays: admission and expectations are computed from exactly those values.

Admission (float64 only, asserted on the CPU): no residual of a hypothesis that can still win (upper count >= the best
lower count), and of no refinement step, lies within the fp32 band of the threshold; the Horn eigen-gap of every fit
that reaches the output is above 1e-6.  SEED_REPLACED lists the cases whose first seed (the case's position in its
table) did not pass and was replaced -- at most one in ten.
"""
import numpy as np

import registration_f64 as F

NOISE = 0.01
OFFSET = (500.0, -300.0, 800.0)
GAP_MIN = 1e-6
# name -> seed used instead of the default.  All three had ONE hypothesis (of 499, 59 and 416 that can win) with one
# residual inside the band of the threshold.
SEED_REPLACED = {"ransac/offset": 1000, "ransac/n5_C2500_H10000": 1000, "ransac/outl0_norefine": 1001}


def rotation(kind, rng):
    if kind == "identity":
        return np.eye(3)
    if kind == "half_turn":                        # 180 degrees about a skew axis
        a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        return 2.0 * np.outer(a, a) - np.eye(3)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(1.1) * K + (1 - np.cos(1.1)) * K @ K


def cloud(kind, n, rng):
    p = rng.random((n, 3))
    if kind == "near_planar":
        p[:, 2] = 0.5 + 1e-3 * (p[:, 2] - 0.5)
    elif kind in ("planar", "planar_mirrored"):
        p[:, 2] = 0.0
    elif kind == "collinear":
        p = np.array([0.2, 0.1, 0.3]) + p[:, :1] * np.array([0.5, 0.7, -0.4])
    elif kind == "identical":
        p = np.tile(np.array([[0.3, 0.6, 0.2]]), (n, 1))
    return p


def planted_pair(geom, rot, n, scale, noise, rng, t=None):
    """-> src, ref in the unit frame (float64) and the planted 3x4 [sR | t]."""
    src = cloud(geom, n, rng)
    R = rotation(rot, rng)
    t = rng.uniform(-0.5, 0.5, 3) if t is None else np.asarray(t, np.float64)
    e = rng.uniform(-noise, noise, (n, 3))
    base = src.copy()
    if geom in ("near_planar", "planar", "planar_mirrored"):
        e[:, 2] = 0.0                              # the noise stays in the plane: the set keeps its thickness
    if geom == "planar_mirrored":
        base[:, 0] = 1.0 - base[:, 0]              # mirrored inside its plane: the best ORTHOGONAL map is a reflection
    if geom in ("collinear", "identical"):
        e[:] = 0.0
    ref = scale * (base + e) @ R.T + t
    return src, ref, np.concatenate([scale * R, t[:, None]], 1)


def to_frame(x, g, off):
    return (g * x + np.asarray(off, np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ RANSAC
def _r(name, geom="unit", rot="generic", g=1.0, off=(0, 0, 0), C=300, n=3, H=500, ws=1, refine=1, scale=1.8, outl=0.5,
       noise=NOISE, **kw):
    return dict(name=name, geom=geom, rot=rot, g=g, off=off, C=C, n=n, H=H, ws=ws, refine=refine,
                scale=scale if ws else 1.0, outl=outl, noise=noise, **kw)


RANSAC_CASES = [
    _r("unit"), _r("x100", g=100.0), _r("x0.01", g=0.01), _r("offset", off=OFFSET, outl=0.0, noise=1e-3),
    _r("rot_identity", rot="identity"), _r("rot_half_turn", rot="half_turn"),
    _r("near_planar", geom="near_planar", noise=1e-4), _r("planar_mirrored", geom="planar_mirrored", noise=1e-4),
    _r("n4_norefine", n=4, refine=0), _r("n5_C2500_H10000", n=5, C=2500, H=10000), _r("n8_H10000", n=8, H=10000),
    _r("rigid", ws=0), _r("rigid_half_turn_norefine", ws=0, rot="half_turn", refine=0),
    _r("scale0.05", scale=0.05), _r("scale20", scale=20.0), _r("outl0_norefine", outl=0.0, refine=0),
    _r("outl0.8_C2500_H10000", outl=0.8, C=2500, H=10000),
    # C_eq_n3_H64 and C_n_plus1_n3_H63 must stay: they are the only cases in which several hypotheses (12 and 4) draw the
    # winner's samples in the winner's order, i.e. the only ones where the lowest-index rule of the tie-break decides
    _r("C_eq_n3_H64", C=3, n=3, H=64, outl=0.0), _r("C_eq_n8_H65", C=8, n=8, H=65, outl=0.0),
    _r("C_n_plus1_n3_H63", C=4, n=3, H=63, outl=0.0), _r("C_n_plus1_n5_H64", C=6, n=5, H=64, outl=0.0),
    _r("C3073", C=3 * 1024 + 1), _r("H1", H=1, outl=0.0), _r("H63", H=63), _r("H64", H=64), _r("H65", H=65),
    _r("H131072_wide", H=131072), _r("tie_two_groups", tie=True, C=100),
]
for _i, _c in enumerate(RANSAC_CASES):
    _c["seed"] = SEED_REPLACED.get("ransac/" + _c["name"], 100 + _i)

RANSAC_DEGENERATE = [_r("collinear", geom="collinear", C=40, H=64, outl=0.0),
                     _r("identical", geom="identical", C=40, H=64, outl=0.0)]
for _i, _c in enumerate(RANSAC_DEGENERATE):
    _c["seed"] = 900 + _i


def build_ransac(c):
    """-> dict(src, ref (float32), thr, seed, planted) of one case."""
    rng = np.random.default_rng(c["seed"])
    C, s = c["C"], c["scale"]
    if c.get("tie"):
        # two disjoint consistent groups of equal size under different transforms; the second is the tighter one
        m = 40
        sa, ra, Ta = planted_pair("unit", "generic", m, s, c["noise"], rng, t=(0.4, -0.2, 0.1))
        sb, rb, Tb = planted_pair("unit", "half_turn", m, s, 0.4 * c["noise"], rng, t=(-2.0, 1.5, 3.0))
        so = rng.random((C - 2 * m, 3))
        ro = rng.uniform(-3.0, 3.0, (C - 2 * m, 3))
        src, ref, T = np.concatenate([sa, sb, so]), np.concatenate([ra, rb, ro]), Tb
        perm = rng.permutation(C)
        src, ref = src[perm], ref[perm]
    else:
        src, ref, T = planted_pair(c["geom"], c["rot"], C, s, c["noise"], rng)
        bad = rng.random(C) < c["outl"]
        lo, hi = ref.min(0), ref.max(0)
        ref[bad] = lo + rng.random((int(bad.sum()), 3)) * np.maximum(hi - lo, 0.2 * s)
    return {"src": to_frame(src, c["g"], c["off"]), "ref": to_frame(ref, c["g"], c["off"]),
            "thr": float(np.float32(0.05 * s * c["g"])), "seed": 7 + c["seed"], "planted": T}


def ransac_can_win(rep):
    """Indices of the hypotheses whose upper count reaches the best lower count."""
    if not rep["valid"].any():
        return np.zeros(0, np.int64)
    return np.nonzero(rep["valid"] & (rep["upper"] >= rep["lower"].max()))[0]


def ransac_admission(c, rep):
    """-> list of reasons why the case is NOT admitted (empty: admitted)."""
    why = []
    W = ransac_can_win(rep)
    if W.size == 0:
        return ["no valid hypothesis"]
    amb = W[rep["lower"][W] != rep["upper"][W]]
    if amb.size:
        why.append(f"{amb.size} of {W.size} hypotheses that can win have a residual within delta of the threshold")
    gaps = [F.horn_gap(rep["H"][h]) for h in W]
    if min(gaps) <= GAP_MIN:
        why.append(f"eigen-gap {min(gaps):.2e} of a hypothesis that can win")
    if c["refine"]:
        for h in W:
            rf = rep["refit"](h)
            if rf is None or F.horn_gap(rf["H"]) <= GAP_MIN:
                why.append(f"refit on hypothesis {h}: undefined or eigen-gap too small")
                break
    return why


# stack mode: pairs of 0, n - 1, n and 2500 rows
def build_ransac_stack(n=3, seed=321):
    rows, srcs, refs = [0, n - 1, n, 2500], [], []
    for i, C in enumerate(rows):
        if C == 0:
            continue
        b = build_ransac(dict(_r(f"stack{i}", C=C, n=n, outl=0.0 if C <= n else 0.5), seed=seed + i))
        srcs.append(b["src"]); refs.append(b["ref"])
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return {"src": np.concatenate(srcs), "ref": np.concatenate(refs), "off": off, "n": n, "H": 500, "seed": 11,
            "thr": float(np.float32(0.05 * 1.8))}


# ------------------------------------------------------------------------------------------------------------ LGR
def _l(name, geom="unit", rot="generic", g=1.0, off=(0, 0, 0), patches=None, thr=3, steps=5, weights="uniform",
       entry="register", noise=NOISE, **kw):
    # patches: list of (rows, group); group >= 0: planted transform of that group, -1: outlier patch
    if patches is None:
        patches = [(20, 0)] * 8 + [(12, -1)] * 4 + [(2, 0)] * 3
    return dict(name=name, geom=geom, rot=rot, g=g, off=off, patches=patches, thr=thr, steps=steps, weights=weights,
                entry=entry, noise=noise, **kw)


_TIE = [(10, -1), (20, 1), (20, 0), (20, 1), (20, 0), (8, -1)]      # groups 1 and 0: 40 rows each, group 1 comes first
_EDGE = [(6, 0)] + [(5, 1)] * 12 + [(9, -1)] * 3                    # threshold 6: one patch has exactly 6, twelve have 5
LGR_CASES = [
    _l("unit_equal", weights="equal"), _l("x100", g=100.0), _l("x0.01", g=0.01),
    _l("offset", off=OFFSET, patches=[(20, 0)] * 8 + [(2, 0)] * 3),
    _l("rot_identity", rot="identity"), _l("rot_half_turn", rot="half_turn"),
    _l("near_planar", geom="near_planar", noise=1e-4), _l("planar_mirrored", geom="planar_mirrored", noise=1e-4),
    _l("steps0", steps=0), _l("steps1", steps=1),
    _l("threshold_edge", patches=_EDGE, thr=6, groups=2),
    _l("global_branch", thr=10 ** 6, patches=[(20, 0)] * 8 + [(6, -1)]),
    _l("weights_span", weights="span"),
    _l("weights_tiny_global", weights="tiny", thr=10 ** 6, patches=[(20, 0)] * 8, t=(0.05, -0.04, 0.03)),
    _l("tie_first_index", patches=_TIE, groups=2),
    _l("verify_limit", entry="verify", limit=120, weights="span"),
    _l("seg_small", entry="seg", seg=[0, 15, 15, 22, 30], patches=([(20, 0)] * 8 + [(12, -1)] * 4 + [(2, 0)] * 3) * 2),
    _l("seg_wide_verify", entry="seg", seg=[0, 1100, 1100, 2200], patches=[(4, 0)] * 700 + [(4, -1)] * 400 + [(4, 0)] * 1100),
]
for _i, _c in enumerate(LGR_CASES):
    _c["seed"] = SEED_REPLACED.get("lgr/" + _c["name"], 500 + _i)

# Collinear and all-identical correspondences: the covariance has rank one or is zero, the rotation is not unique, so these
# are exempt from the gap rule and from the transform bound; the GPU test asserts what IS defined (a finite proper
# rigid transform whose residuals on the points are those of the float64 fit, the weighted centroid mapped as in the
# reference form).  Each set is sent once as patch hypotheses (threshold 3) and once through the global branch.
_DEG = [(10, 0)] * 4
LGR_DEGENERATE = [
    _l("collinear_patches", geom="collinear", patches=_DEG, noise=0.0, limit=25),
    _l("collinear_global", geom="collinear", patches=_DEG, noise=0.0, thr=10 ** 6, limit=25),
    _l("identical_patches", geom="identical", patches=_DEG, noise=0.0, limit=25),
    _l("identical_global", geom="identical", patches=_DEG, noise=0.0, thr=10 ** 6, limit=25),
]
for _i, _c in enumerate(LGR_DEGENERATE):
    _c["seed"] = 950 + _i


def build_lgr(c):
    """-> dict(ref, src (float32, C x 3), scores (float32), offsets (P + 1), radius, plus the case's parameters)."""
    rng = np.random.default_rng(c["seed"])
    ngroups = c.get("groups", 1)
    segs = c.get("seg") or [0, len(c["patches"])]
    srcs, refs = [], []
    for pa, pe in zip(segs[:-1], segs[1:]):          # every scene pair has its own planted transforms
        pl = [planted_pair(c["geom"], c["rot"] if k == 0 else "half_turn", 1, 1.0, 0.0, rng, t=c.get("t"))[2]
              for k in range(ngroups)]
        for rows, grp in c["patches"][pa:pe]:
            centre = cloud(c["geom"], 1, rng)
            p = cloud(c["geom"], rows, rng)
            p = centre + 0.5 * (p - p.mean(0)) if c["geom"] not in ("collinear", "identical") else p
            e = rng.uniform(-c["noise"], c["noise"], (rows, 3))
            q = p.copy()
            if c["geom"] in ("near_planar", "planar", "planar_mirrored"):
                e[:, 2] = 0.0
            if c["geom"] == "planar_mirrored":
                q[:, 0] = 1.0 - q[:, 0]
            if grp >= 0:
                r = (q + e) @ pl[grp][:, :3].T + pl[grp][:, 3]
            else:
                r = rng.uniform(-2.0, 3.0, (rows, 3))
            srcs.append(p); refs.append(r)
    src, ref = np.concatenate(srcs), np.concatenate(refs)
    C = src.shape[0]
    if c["weights"] == "equal":
        w = np.full(C, 0.7)
    elif c["weights"] == "span":
        w = 10.0 ** rng.uniform(-6.0, 0.0, C)
    elif c["weights"] == "tiny":
        w = rng.uniform(0.5, 1.5, C) * (1e-5 / C)    # sum w ~ eps of w / (sum w + eps)
    else:
        w = rng.uniform(0.3, 1.0, C)
    counts = np.array([r for r, _ in c["patches"]], np.int64)
    return {"src": to_frame(src, c["g"], c["off"]), "ref": to_frame(ref, c["g"], c["off"]), "scores": w.astype(np.float32),
            "offsets": np.concatenate([[0], np.cumsum(counts)]), "counts": counts,
            "radius": float(np.float32(0.1 * c["g"])), "thr": c["thr"], "steps": c["steps"], "seg": c.get("seg"),
            "limit": c.get("limit")}


def lgr_verify_set(b):
    """The verification set of correspondence_limit (local_global_registration.py:145-148): the `limit` largest scores, in
    descending order (the scores of such a case are distinct)."""
    if b["limit"] is None or b["scores"].shape[0] <= b["limit"]:
        return None
    sel = np.argsort(-b["scores"], kind="stable")[:b["limit"]]
    assert np.unique(b["scores"]).size == b["scores"].size
    return b["ref"][sel], b["src"][sel], b["scores"][sel]


def lgr_expected(b, renormalise=False):
    return F.local_to_global(b["ref"], b["src"], b["scores"], b["offsets"], b["radius"], b["thr"], b["steps"],
                             verify=lgr_verify_set(b), seg=b["seg"], renormalise=renormalise)


def lgr_admission(res):
    """-> list of reasons why one float64 result (one scene pair) is NOT admitted."""
    why = []
    if res["branch"] == "empty":
        return why
    if res["branch"] == "local":
        lower, upper = np.array(res["lower"]), np.array(res["upper"])
        W = np.nonzero(upper >= lower.max())[0]
        if (lower[W] != upper[W]).any():
            why.append("a hypothesis that can win has a residual within delta of the radius")
        if min(res["hyp_gap"][h] for h in W) <= GAP_MIN:
            why.append("eigen-gap of a hypothesis that can win")
    elif res["global_gap"] <= GAP_MIN:
        why.append("eigen-gap of the global fit")
    for k, st in enumerate(res["steps"]):
        if st["margin"].size and st["margin"].min() <= st["delta"]:
            why.append(f"step {k} ({st['what']}): a residual within delta of the radius")
    if min(res["step_gaps"]) <= GAP_MIN:
        why.append(f"eigen-gap {min(res['step_gaps']):.2e} of a refinement fit")
    return why
