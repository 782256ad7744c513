"""The planar-point rule of caelo_planar_points (include/caelo.h) restated literally in NumPy -- the reference's commented
per-pixel loop (SphericalRing.py:236-282) with np.cov, np.linalg.eig and argsort -- and the comparison rule the planar tests share.

Steps 1-5 are float32 decisions and are restated in the arithmetic the library pins (the 8-lane pairwise sum of the squared response
difference, every operation rounded on its own; the centre's norm summed left to right); they are vectorised over the image, which
changes no bit.  Steps 6-7 are the reference's own calls, one candidate at a time."""
import numpy as np

H0, H1, W0, W1 = 8, 56, 8, 1784          # AllPixelIndexes_WithoutWindowEdge (:64-68)
NET_H, NET_W = 64, 1792
PLANAR_MAX = (H1 - H0) * (W1 - W0)
NORMAL_BAR = 1.2e-7                      # 2 float32 ulps of 1: ~24 float64 roundings in the covariance, an eigenvector that moves by
                                         # |dC| / gap <= 3e-15 / 1e-4, and half an ulp for the cast to float32
UNDECIDED_GAP, UNDECIDED_NZ = 1e-4, 1e-9
OFFSETS = [(r, c) for r in range(-2, 3) for c in range(-2, 3)]   # window row-major


def min_diff(resp, occ):
    """-> (minDiff [64,1792] f32 over the occupied neighbours, inf where there is none; a NaN among them stays), neighbour count."""
    resp = np.asarray(resp, np.float32)[:NET_H, :NET_W]
    pad = np.zeros((NET_H + 4, NET_W + 4, 8), np.float32)
    pad[2:-2, 2:-2] = resp
    po = np.zeros((NET_H + 4, NET_W + 4), bool)
    po[2:-2, 2:-2] = occ[:NET_H, :NET_W]
    best = np.full((NET_H, NET_W), np.inf, np.float32)
    cnt = np.zeros((NET_H, NET_W), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r, c in OFFSETS:
            if (r, c) == (0, 0):
                continue
            q = pad[2 + r:2 + r + NET_H, 2 + c:2 + c + NET_W]
            o = po[2 + r:2 + r + NET_H, 2 + c:2 + c + NET_W]
            d = q - resp
            s = d * d
            t = ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) + ((s[..., 4] + s[..., 5]) + (s[..., 6] + s[..., 7]))
            best = np.where(o, np.minimum(best, np.sqrt(t)), best)       # np.minimum keeps a NaN
            cnt += o
    return best, cnt


def planar_points(ring, counter, resp):
    """-> dict(rows [m,6] f32, pixels [m,2] i32, cand [c,2] i32 the pixels that pass steps 1-5, eig [c,3] f64 ascending, absnz [c] f64,
    kept [c] bool).  A candidate whose covariance is not finite has NaN eigenvalues and is not kept."""
    ring = np.asarray(ring, np.float32)
    occ = np.asarray(counter) > 0                                         # :243 (the staged convention)
    md, cnt = min_diff(resp, occ)
    xyz = ring[:NET_H, :NET_W, 0:3]
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt((xyz[..., 0] * xyz[..., 0] + xyz[..., 1] * xyz[..., 1]) + xyz[..., 2] * xyz[..., 2])
        md64 = md.astype(np.float64)
        ok = occ[:NET_H, :NET_W] & (cnt >= 5)                             # :243, :250
        ok &= ~((md64 > 0.2) & (norm < np.float32(10.0)))                 # :259-262
        ok &= md64 < 0.4                                                  # :268
    ok[:H0] = False
    ok[H1:] = False
    ok[:, :W0] = False
    ok[:, W1:] = False
    cand = np.argwhere(ok).astype(np.int32)                               # row-major
    rows, pixels, eig, absnz, kept = [], [], [], [], []
    for y, x in cand:
        oneMask = np.array(occ[y - 2:y + 3, x - 2:x + 3], dtype=np.int32)
        oneMask[2, 2] = 0                                                 # :246-247
        oneWindow = ring[y - 2:y + 3, x - 2:x + 3, 0:3]                   # :269
        pts = oneWindow[oneMask > 0, :]                                   # :270
        with np.errstate(invalid="ignore", over="ignore"):
            covMat = np.cov(pts, rowvar=0)                                # :271
        if not np.isfinite(covMat).all():
            eig.append([np.nan] * 3); absnz.append(np.nan); kept.append(False)
            continue
        eigVals, eigVector = np.linalg.eig(covMat)                        # :272
        eigVals, eigVector = np.real(eigVals), np.real(eigVector)
        sortIdx = np.argsort(eigVals)                                     # :273
        vNorm = eigVector[:, sortIdx[0]]                                  # :274
        eig.append(eigVals[sortIdx]); absnz.append(abs(vNorm[2]))
        keep = bool(abs(vNorm[2]) > 0.9)                                  # :275
        kept.append(keep)
        if keep:
            if vNorm[2] < 0:
                vNorm = -vNorm                                            # the library's sign convention
            rows.append(np.r_[ring[y, x, 0:3], vNorm.astype(np.float32)].astype(np.float32))   # :276, :285
            pixels.append((y, x))
    return dict(rows=np.array(rows, np.float32).reshape(-1, 6), pixels=np.array(pixels, np.int32).reshape(-1, 2), cand=cand,
                eig=np.array(eig, np.float64).reshape(-1, 3), absnz=np.array(absnz, np.float64), kept=np.array(kept, bool), min_diff=md)


def undecided(ref):
    """Candidates that may fall either way: (l1 - l0) / l2 < 1e-4 (the smallest eigenvector is ill-conditioned), or |n_z| within 1e-9
    of 0.9.  A covariance that is not finite is decided: no row."""
    e, nz = ref["eig"], ref["absnz"]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (e[:, 1] - e[:, 0]) / e[:, 2]
    fin = np.isfinite(e).all(axis=1)
    return fin & (~(gap >= UNDECIDED_GAP) | (np.abs(nz - 0.9) < UNDECIDED_NZ))


def compare(ref, rows, pixels, max_undecided=None, label=""):
    """The comparison rule: outside the undecided set membership and pixel order are equal, points are equal byte for byte, normals
    lie within NORMAL_BAR.  max_undecided: the largest fraction of the candidates that may be undecided (frames: 0.005).
    -> (number of undecided candidates, the largest normal difference)."""
    rows, pixels = np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(pixels).reshape(-1, 2)
    und = undecided(ref)
    if max_undecided is not None:
        assert und.sum() <= max_undecided * max(len(und), 1), "%s: %d of %d candidates undecided" % (label, und.sum(), len(und))
    flat = lambda p: p[:, 0].astype(np.int64) * NET_W + p[:, 1]   # noqa: E731
    und_px = set(flat(ref["cand"][und]).tolist())
    cand_px = set(flat(ref["cand"]).tolist())
    got_flat = flat(pixels)
    assert set(got_flat.tolist()) <= cand_px, "%s: a row for a pixel that is no candidate" % label
    assert (np.diff(got_flat) > 0).all(), "%s: rows are not in row-major pixel order" % label
    gsel = np.array([p not in und_px for p in got_flat.tolist()], bool)
    want_flat = flat(ref["pixels"])
    wsel = np.array([p not in und_px for p in want_flat.tolist()], bool)
    assert np.array_equal(got_flat[gsel], want_flat[wsel]), "%s: membership differs outside the undecided set" % label
    g, w = rows[gsel], ref["rows"][wsel]
    assert g[:, 0:3].tobytes() == w[:, 0:3].tobytes(), "%s: points differ" % label
    assert (rows[:, 5] > 0).all(), "%s: a normal with n_z <= 0" % label
    worst = float(np.abs(g[:, 3:6].astype(np.float64) - w[:, 3:6].astype(np.float64)).max()) if len(g) else 0.0
    print("planar_errors %-28s candidates %6d kept %6d undecided %3d normal diff %.3e (bar %.1e)" % (label, len(und), len(w), und.sum(), worst, NORMAL_BAR))
    assert worst <= NORMAL_BAR, "%s: normals differ by %.3e" % (label, worst)
    return int(und.sum()), worst
