"""Test helper (not collected): float64 restatements of the two solvers that turn correspondences into the final
transform, in plain NumPy and in the SVD form of the publications -- never the unit-quaternion form the kernels use.

  weighted_procrustes   geotransformer/modules/registration/procrustes.py:41-66
  local_to_global       geotransformer/modules/geotransformer/local_global_registration.py:135-193
  umeyama               Umeyama 1991, "Least-squares estimation of transformation parameters between two point patterns"
  ransac_replay         the published RANSAC loop with the sampler of include/gaussreg_hip.h (gr_ransac_sample_hash)

tests/test_registration_f64_reference.py pins the first two against the reference's own modules (1e-12) and the third
against planted similarities; the GPU tests compare gaussreg_amd/csrc/lgr.hip and ransac.hip with them.

The fp32 evaluation band of a residual.  Both kernels keep the transform in fp32 and evaluate
|ref - (T src)| per coordinate as three chained fp32 multiply-adds plus a subtraction.  Each of the twelve fp32
transform entries carries a relative error of eps32 / 2, each of the three chained operations adds eps32 / 2 of a partial
sum bounded by |T src|_max, and the subtraction adds eps32 / 2 of (|ref| + |T src|): per coordinate at most
(3 + 3 + 1) * eps32 / 2 * (max|ref| + max|T src|) = 3.5 eps32 * (...).  The norm over three coordinates multiplies by
sqrt(3), the squares and their two additions add 3 eps32 relative to a residual that is itself below the same magnitude,
and the comparison is made against thr * thr or through sqrtf (1 eps32 more): below 10 eps32 * (max|ref| + max|T src|).
The band used everywhere is 64 eps32 * (max|ref| + max|T src|): a factor of six above that, which also absorbs the
difference between the float64 transform and the kernel's (rounded from a fp64 Jacobi, not an SVD).
"""
import numpy as np

f64 = np.float64
EPS32 = float(np.finfo(np.float32).eps)


def residual_band(ref, src, T):
    """delta = 64 eps32 (max|ref| + max|T src|); T: (..., 3, 4) or (..., 4, 4), returns an array of shape (...)."""
    T = np.asarray(T, f64)
    ref, src = np.asarray(ref, f64), np.asarray(src, f64)
    if ref.shape[0] == 0:
        return np.zeros(T.shape[:-2])
    mapped = np.einsum("...rc,nc->...nr", T[..., :3, :3], src) + T[..., None, :3, 3]
    return 64.0 * EPS32 * (np.abs(ref).max() + np.abs(mapped).reshape(T.shape[:-2] + (-1,)).max(-1))


def residuals(ref, src, T):
    """|ref - (R src + t)| per correspondence, float64; T (..., 3|4, 4) -> (..., N)."""
    T = np.asarray(T, f64)
    mapped = np.einsum("...rc,nc->...nr", T[..., :3, :3], np.asarray(src, f64)) + T[..., None, :3, 3]
    return np.linalg.norm(np.asarray(ref, f64) - mapped, axis=-1)


def horn_gap(Hm):
    """(largest - second eigenvalue) / Frobenius norm of Horn's symmetric 4x4 matrix of the 3x3 covariance
    Hm[a][b] = sum src_a ref_b, in float64: how well the kernels' eigenvector is determined."""
    S = np.asarray(Hm, f64)
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    nrm = np.linalg.norm(N)
    if nrm == 0.0:
        return 0.0
    ev = np.linalg.eigvalsh(N)
    return float((ev[-1] - ev[-2]) / nrm)


# ---------------------------------------------------------------------------------------------- weighted Procrustes / LGR
def procrustes_parts(src, ref, w, eps=1e-5, renormalise=False):
    """procrustes.py:41-66, line by line -> dict(T 4x4, R, t, cs, cr, H).  `renormalise=True` is the VARIANT that divides
    by sum w exactly (not what the reference does): only the tiny-weight test uses it, as the thing NOT to match."""
    src, ref, w = np.asarray(src, f64), np.asarray(ref, f64), np.asarray(w, f64)
    w = np.where(w < 0.0, 0.0, w)                                     # :43  weight_thresh = 0
    w = w / (w.sum() + (0.0 if renormalise else eps))                 # :44
    w = w[:, None]                                                    # :45
    cs = (src * w).sum(0)                                             # :47  (not renormalised: shrinks when sum w ~ eps)
    cr = (ref * w).sum(0)                                             # :48
    sc, rc = src - cs, ref - cr                                       # :49-50
    Hm = sc.T @ (w * rc)                                              # :58
    U, _, Vt = np.linalg.svd(Hm)                                      # :59  H = U S V^T
    V = Vt.T
    D = np.eye(3)
    D[2, 2] = np.sign(np.linalg.det(V @ U.T))                         # :62
    R = V @ D @ U.T                                                   # :63
    t = cr - R @ cs                                                   # :65
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return {"T": T, "R": R, "t": t, "cs": cs, "cr": cr, "H": Hm}


def weighted_procrustes(src, ref, w, eps=1e-5):
    return procrustes_parts(src, ref, w, eps)["T"]


def _count_bands(ref, src, T, radius):
    """(exact count, lower, upper, delta, smallest |residual - radius|) of one transform."""
    res = residuals(ref, src, T)
    d = float(residual_band(ref, src, T))
    margin = float(np.abs(res - radius).min()) if res.size else np.inf
    return int((res < radius).sum()), int((res < radius - d).sum()), int((res < radius + d).sum()), d, margin


def _l2g_one(ref, src, sc, offs, radius, threshold, steps, verify, renormalise):
    ref, src, sc = np.asarray(ref, f64), np.asarray(src, f64), np.asarray(sc, f64)
    out = {"T": np.eye(4), "hyp_T": [], "hyp_patch": [], "counts": [], "lower": [], "upper": [], "hyp_margin": [],
           "hyp_gap": [], "best": -1, "steps": [], "last": None, "branch": "empty"}
    if ref.shape[0] == 0:
        return out                                                    # (the module leaves the identity for an empty pair)
    vref, vsrc, vsc = (ref, src, sc) if verify is None else [np.asarray(a, f64) for a in verify]
    fit = lambda s_, r_, w_: procrustes_parts(s_, r_, w_, renormalise=renormalise)

    def step(T, what):                                                # recompute_correspondence_scores :130-135
        res = residuals(vref, vsrc, T)
        mask = res < radius
        out["steps"].append({"what": what, "mask": mask, "margin": np.abs(res - radius),
                             "delta": float(residual_band(vref, vsrc, T))})
        return vsc * mask

    chunks = [(int(a), int(b)) for a, b in zip(offs[:-1], offs[1:]) if b - a >= threshold]   # :161-163
    if chunks:
        out["branch"] = "local"
        for p, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
            if b - a < threshold:
                continue
            h = fit(src[a:b], ref[a:b], sc[a:b])                      # :168-171 (zero padding adds zero-weight rows)
            c, lo, up, d, m = _count_bands(vref, vsrc, h["T"], radius)  # :172-176
            out["hyp_T"].append(h["T"]); out["hyp_patch"].append(p); out["counts"].append(c)
            out["lower"].append(lo); out["upper"].append(up); out["hyp_margin"].append(m - d)
            out["hyp_gap"].append(horn_gap(h["H"]))
        out["best"] = int(np.argmax(out["counts"]))                   # :177 first maximum
        cur = step(out["hyp_T"][out["best"]], "best hypothesis")      # :178
    else:
        out["branch"] = "global"
        g = fit(vsrc, vref, vsc)                                      # :181
        out["global_gap"] = horn_gap(g["H"])
        cur = step(g["T"], "global")                                  # :182-184
    last = fit(vsrc, vref, cur)                                       # :187
    gaps = [horn_gap(last["H"])]
    for _ in range(steps - 1):                                        # :188-192
        cur = step(last["T"], "refinement")
        last = fit(vsrc, vref, cur)
        gaps.append(horn_gap(last["H"]))
    out["T"], out["last"], out["step_gaps"] = last["T"], last, gaps
    return out


def local_to_global(ref_corr, src_corr, scores, patch_offsets, acceptance_radius, correspondence_threshold,
                    num_refinement_steps, verify=None, seg=None, renormalise=False):
    """local_global_registration.py:135-193 in float64.  patch_offsets (P + 1): first row of every patch (torch.nonzero
    order keeps a patch's rows together).  verify = (ref, src, scores) of the verification set (:145-148), default: all
    rows.  seg (nseg + 1 patch offsets): one independent problem per scene pair, a list of results is returned.
    A result holds the transform, every hypothesis with its exact / lower / upper inlier counts, the index of the winner
    among the hypotheses (`best`, `hyp_patch[best]` is its patch), and per refinement step the inlier mask with each
    residual's distance to the radius and the fp32 band."""
    offs = np.asarray(patch_offsets, np.int64)
    if seg is None:
        return _l2g_one(ref_corr, src_corr, scores, offs, acceptance_radius, correspondence_threshold,
                        num_refinement_steps, verify, renormalise)
    outs = []
    for pa, pe in zip(seg[:-1], seg[1:]):
        a, b = int(offs[pa]), int(offs[pe])
        outs.append(_l2g_one(ref_corr[a:b], src_corr[a:b], scores[a:b], offs[pa:pe + 1] - a, acceptance_radius,
                             correspondence_threshold, num_refinement_steps, None, renormalise))
    return outs


# ---------------------------------------------------------------------------------------------- Umeyama / RANSAC
def umeyama_batch(src, ref, with_scaling):
    """src, ref (B, n, 3) -> T (B, 3, 4) = [sR | t], scale (B,), valid (B,), plus R, cs, cr, H (for bounds and gaps).
    R = V diag(1, 1, det(V U^T)) U^T of H = sum (src - cs)(ref - cr)^T = U S V^T; s = tr(D S) / sum |src - cs|^2."""
    src, ref = np.asarray(src, f64), np.asarray(ref, f64)
    cs, cr = src.mean(1), ref.mean(1)
    sc, rc = src - cs[:, None], ref - cr[:, None]
    Hm = np.einsum("bna,bnc->bac", sc, rc)
    U, S, Vt = np.linalg.svd(Hm)
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, 1, 2)))
    D = np.ones_like(S)
    D[:, 2] = d
    R = np.einsum("bij,bj,bkj->bik", V, D, U)
    var = (sc * sc).sum((1, 2))
    valid = np.ones(src.shape[0], bool)
    scale = np.ones(src.shape[0])
    if with_scaling:
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = (D * S).sum(1) / var
        valid = (var > 1e-300) & np.isfinite(scale) & (scale > 0.0)
        scale = np.where(valid, scale, 1.0)
    t = cr - scale[:, None] * np.einsum("bij,bj->bi", R, cs)
    T = np.concatenate([scale[:, None, None] * R, t[:, :, None]], 2)
    return {"T": T, "scale": scale, "valid": valid, "R": R, "cs": cs, "cr": cr, "H": Hm}


def umeyama(src, ref, with_scaling):
    """-> (s, R, t) of one problem, or None where the similarity is undefined (no spread in src, or scale <= 0)."""
    u = umeyama_batch(np.asarray(src)[None], np.asarray(ref)[None], with_scaling)
    if not u["valid"][0]:
        return None
    return float(u["scale"][0]), u["R"][0], u["T"][0][:, 3]


def sample_hash(seed, h, k, attempt):
    """The sampler's counter hash (include/gaussreg_hip.h, gr_ransac_sample_hash) on uint32 arrays."""
    M = np.uint64(0xFFFFFFFF)
    u = lambda v: np.asarray(v, np.uint64) & M
    x = u(seed) ^ ((u(h) * np.uint64(0x9E3779B9)) & M) ^ ((u(k) * np.uint64(0x85EBCA6B)) & M) ^ \
        ((u(attempt) * np.uint64(0xC2B2AE35)) & M)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    return x


def ransac_samples(C, n, H, seed, hash_fn=None):
    """(H, n) indices: sample k of hypothesis h is hash(seed, h, k, attempt) % C, retried with attempt + 1 while it
    repeats an earlier sample of the same hypothesis and attempt <= 64 (the last try, attempt 65, is kept as it is)."""
    hash_fn = hash_fn or sample_hash
    hs = np.arange(H, dtype=np.uint64)
    idx = np.zeros((H, n), np.int64)
    for k in range(n):
        att = np.zeros(H, np.uint64)
        cur = (hash_fn(seed, hs, k, att) % np.uint64(C)).astype(np.int64)
        while True:
            dup = (idx[:, :k] == cur[:, None]).any(1) & (att <= 64)
            if not dup.any():
                break
            att[dup] += np.uint64(1)
            cur[dup] = (hash_fn(seed, hs[dup], k, att[dup]) % np.uint64(C)).astype(np.int64)
        idx[:, k] = cur
    return idx


def _score(ref, src, T, valid, thr, chunk):
    Hn = T.shape[0]
    cnt, lower, upper = np.full(Hn, -1, np.int64), np.full(Hn, -1, np.int64), np.full(Hn, -1, np.int64)
    sq, delta = np.zeros(Hn), np.zeros(Hn)
    for a in range(0, Hn, chunk):
        Tc = T[a:a + chunk]
        mapped = np.einsum("hrc,nc->hnr", Tc[:, :, :3], src) + Tc[:, None, :, 3]
        d = 64.0 * EPS32 * (np.abs(ref).max() + np.abs(mapped).max((1, 2)))
        res = np.linalg.norm(ref[None] - mapped, axis=2)
        inl = res < thr
        v = valid[a:a + chunk]
        cnt[a:a + chunk] = np.where(v, inl.sum(1), -1)
        lower[a:a + chunk] = np.where(v, (res < (thr - d)[:, None]).sum(1), -1)
        upper[a:a + chunk] = np.where(v, (res < (thr + d)[:, None]).sum(1), -1)
        sq[a:a + chunk] = np.where(v, (res * res * inl).sum(1), 0.0)
        delta[a:a + chunk] = d
    return cnt, lower, upper, sq, delta


def ransac_replay(src, ref, n, H, seed, thr, with_scaling, hash_fn=None, chunk=None):
    """Every hypothesis of gr_ransac_similarity in float64.  Returns a dict: idx (H, n), T (H, 3, 4), valid, scale, count
    (residual < thr), lower (< thr - delta), upper (< thr + delta), sqerr (sum of squared inlier residuals), delta, gap
    (Horn eigen-gap of every sample), best (most inliers, then smallest squared error, then lowest index; -1 when no
    hypothesis is valid) and refit(h): the same quantities for the fit on the inliers of hypothesis h."""
    src, ref = np.asarray(src, f64), np.asarray(ref, f64)
    C = src.shape[0]
    chunk = chunk or max(1, int(2e6 // max(C, 1)))
    idx = ransac_samples(C, n, H, seed, hash_fn)
    parts = {k: [] for k in ("T", "scale", "valid", "R", "cs", "cr", "H")}
    for a in range(0, H, 16384):
        u = umeyama_batch(src[idx[a:a + 16384]], ref[idx[a:a + 16384]], with_scaling)
        for k in parts:
            parts[k].append(u[k])
    u = {k: np.concatenate(v) for k, v in parts.items()}
    cnt, lower, upper, sq, delta = _score(ref, src, u["T"], u["valid"], thr, chunk)
    best = -1
    if u["valid"].any():
        top = np.nonzero(cnt == cnt.max())[0]
        best = int(top[np.argmin(sq[top])])                          # argmin keeps the first minimum: lowest index

    def refit(h):
        inl = residuals(ref, src, u["T"][h]) < thr
        r = umeyama_batch(src[inl][None], ref[inl][None], with_scaling) if inl.sum() >= 1 else None
        if r is None or not r["valid"][0]:
            return None
        c, lo, up, s2, d = _score(ref, src, r["T"], r["valid"], thr, 1)
        return {"T": r["T"][0], "scale": float(r["scale"][0]), "R": r["R"][0], "cs": r["cs"][0], "cr": r["cr"][0],
                "H": r["H"][0], "inliers": inl, "count": int(c[0]), "lower": int(lo[0]), "upper": int(up[0]),
                "sqerr": float(s2[0]), "delta": float(d[0])}

    return {"idx": idx, "T": u["T"], "valid": u["valid"], "scale": u["scale"], "R": u["R"], "cs": u["cs"], "cr": u["cr"],
            "H": u["H"], "count": cnt, "lower": lower, "upper": upper, "sqerr": sq, "delta": delta, "best": best,
            "refit": refit}


# ---------------------------------------------------------------------------------------------- the transform bound
def transform_bound(scale, R, cs, cr):
    """Both kernels form the result in fp64 and round once to fp32 (half an ulp); the fp64 path itself (raw-sum
    covariances, sixteen Jacobi sweeps) is allowed the rest of FOUR fp32 ulps: of the scale for the 3x3 block, of
    |cr| + s |R cs| (entry by entry) for the translation.  -> (3, 4) array of absolute bounds."""
    ulp = lambda v: np.spacing(np.abs(np.asarray(v, f64)).astype(np.float32)).astype(f64)
    b = np.empty((3, 4))
    b[:, :3] = 4.0 * ulp(scale)
    b[:, 3] = 4.0 * ulp(np.abs(cr) + scale * np.abs(R @ cs))
    return b


def bound_ratio(got, want34, scale, R, cs, cr):
    """max over the twelve entries of |got - want| / bound (must be <= 1)."""
    got = np.asarray(got, f64)[:3, :4]
    return float((np.abs(got - np.asarray(want34, f64)[:3, :4]) / transform_bound(scale, R, cs, cr)).max())
