"""The SIFT3D key point definition (include/caelo.h) restated in float64 NumPy, the input conditions the GPU tests rest
on, and the scenes they use.  A test helper: nothing in the package imports it.

The restatement follows the device's arithmetic where the result depends on it: the masks come from the rounded
d2 = (dx*dx + dy*dy) + dz*dz against 9.0 * (sigma*sigma), every sum is np.cumsum(...)[-1] over the counting points in ascending index
-- NumPy's cumsum adds one element after the other, which is the device's order -- and the neighbourhood is
np.lexsort((index, d2))[:25].  Only exp is another implementation (np.exp against the device's float64 exp): the two agree to an ulp
or two, the responses and their differences to a few ulp of values of a few metres, and every decision taken from them is exact as
long as it is not closer to flipping than that -- which ``margins`` measures.
"""
import numpy as np

import iss_ref

DEFAULTS = dict(min_scale=0.5, n_octaves=4, n_scales_per_octave=8, min_contrast=0.1)   # PclKeyPts.py:55-58
K = 25


def _params(kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def scales(scale, n_scales_per_octave):
    """sigma[s] = scale * 2.0 ** ((s - 1) / n_scales_per_octave), s = 0 .. n_scales_per_octave + 2, float64."""
    return np.array([float(scale) * 2.0 ** ((s - 1) / int(n_scales_per_octave)) for s in range(int(n_scales_per_octave) + 3)], dtype=np.float64)


def centroids(pts, leaf):
    """pts [n,3] float32 -> [m,3] float32: per occupied cell (floor(double(p) / leaf) per component; cells in (cz, cy, cx) order, x
    fastest) the float64 sums of its points in ascending row, each divided by double(count) and rounded to float32."""
    P32 = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    if P32.shape[0] == 0:
        return P32
    P = P32.astype(np.float64)
    cell = np.floor(P / np.float64(leaf)).astype(np.int64)
    order = np.lexsort((np.arange(P.shape[0]), cell[:, 0], cell[:, 1], cell[:, 2]))   # the last key is the first criterion
    sc = cell[order]
    first = np.ones(P.shape[0], bool)
    first[1:] = (sc[1:] != sc[:-1]).any(axis=1)
    starts = np.r_[np.flatnonzero(first), P.shape[0]]
    out = np.zeros((starts.shape[0] - 1, 3), np.float32)
    for c in range(out.shape[0]):
        rows = order[starts[c]:starts[c + 1]]
        for a in range(3):
            out[c, a] = np.float32(np.cumsum(P[rows, a])[-1] / np.float64(rows.shape[0]))
    return out


def octave(pts, sigma, min_contrast):
    """One octave.  pts [n,3] float32, sigma [S] ascending -> dict: dog [n,S-1], knn [n,25] i32 in (d2, index) order (-1 behind the n
    points of a smaller cloud), d2_gap (the least d2[26th] - d2[25th] where the two differ; inf without a 26th), key_mask [n] i32 (bit s:
    (i, s) is a key), key_idx (the points with a non-zero mask, ascending)."""
    P = np.asarray(pts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    sigma = np.asarray(sigma, dtype=np.float64)
    n, S = P.shape[0], sigma.shape[0]
    D = S - 1
    z = P[:, 2]
    resp = np.zeros((n, S))
    knn = np.full((n, K), -1, np.int32)
    d2_gap = np.inf
    idx = np.arange(n)
    for i in range(n):
        _, d2 = iss_ref._d2(P, i)
        for s in range(S):
            s2 = sigma[s] * sigma[s]
            m = d2 <= np.float64(9.0) * s2
            w = np.exp((np.float64(-0.5) * d2[m]) / s2)
            resp[i, s] = np.cumsum(z[m] * w)[-1] / np.cumsum(w)[-1]
        near = np.lexsort((idx, d2))
        knn[i, :min(n, K)] = near[:K]
        if n > K and d2[near[K]] != d2[near[K - 1]]:
            d2_gap = min(d2_gap, d2[near[K]] - d2[near[K - 1]])
    dog = resp[:, 1:] - resp[:, :-1]
    mask = np.zeros(n, np.int32)
    mn = mx = None
    if n >= K:
        G = dog[knn]   # [n, 25, D]
        mn, mx = G.min(axis=1), G.max(axis=1)
        for s in range(1, D - 1):
            v = dog[:, s]
            low = (v == mn[:, s]) & (v < mn[:, s - 1]) & (v < mn[:, s + 1])
            high = (v == mx[:, s]) & (v > mx[:, s - 1]) & (v > mx[:, s + 1])
            mask |= ((np.abs(v) >= min_contrast) & (low | high)).astype(np.int32) << s
    return dict(P=P, sigma=sigma, min_contrast=float(min_contrast), dog=dog, knn=knn, d2_gap=float(d2_gap), key_mask=mask,
                key_idx=np.flatnonzero(mask).astype(np.int32))


def margins(r):
    """-> (contrast margin, value gap, d2 gap) of a result of ``octave``: the least ||dog| - min_contrast| over the levels 1 .. D-2; the
    least |v - u| over the contrast-passing v = dog[i][s] and every other value u that enters its rule (the 24 other neighbours at s,
    all 25 at s-1 and s+1); the least difference between the 25th and the 26th d2 where the index does not decide.  inf where there is
    nothing to decide."""
    dog, knn, mc = r["dog"], r["knn"], r["min_contrast"]
    n, D = dog.shape
    if n < K or D < 3:
        return np.inf, np.inf, r["d2_gap"]
    mid = dog[:, 1:D - 1]
    contrast = float(np.min(np.abs(np.abs(mid) - mc)))
    gap = np.inf
    for s in range(1, D - 1):
        for i in np.flatnonzero(np.abs(dog[:, s]) >= mc):
            v = dog[i, s]
            nb = knn[i]
            others = np.concatenate([dog[nb[nb != i], s], dog[nb, s - 1], dog[nb, s + 1]])
            gap = min(gap, float(np.min(np.abs(others - v))))
    return contrast, gap, r["d2_gap"]


def pyramid(pts, **kw):
    """pts [n,3] float32 -> dict: octaves (a list of dict(octave, scale, cloud [m,3] f32, result = ``octave`` of it)), stopped_at (the
    octave whose cloud fell under 25 points, or None), xyz [k,3] f32, scale [k] f64, octave [k] i32: the key points in the order
    octave, point index, scale index."""
    p = _params(kw)
    cloud = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    octs, xyz, sc, oc = [], [], [], []
    stopped_at = None
    for o in range(p["n_octaves"]):
        scale = p["min_scale"] * 2.0 ** o
        cloud = centroids(cloud, scale)
        if cloud.shape[0] < K:
            stopped_at = o
            break
        sg = scales(scale, p["n_scales_per_octave"])
        r = octave(cloud, sg, p["min_contrast"])
        octs.append(dict(octave=o, scale=scale, cloud=cloud, result=r))
        for i in r["key_idx"]:
            for s in range(sg.shape[0]):
                if (r["key_mask"][i] >> s) & 1:
                    xyz.append(cloud[i]); sc.append(sg[s]); oc.append(o)
    return dict(octaves=octs, stopped_at=stopped_at, xyz=np.array(xyz, np.float32).reshape(-1, 3), scale=np.array(sc, np.float64),
                octave=np.array(oc, np.int32), params=p)


# The scenes of the GPU parity test: (seed, n, parameters), iss_ref's scenes at the defaults and one at other parameters, where the
# number of scales (7) and of octaves (5) differ from the defaults' (11 and 4).
OTHER = dict(min_scale=0.25, n_octaves=5, n_scales_per_octave=4, min_contrast=0.05)
SCENES = [(9, 1500, {}), (2, 1500, {}), (3, 1025, {}), (4, 257, {}), (5, 600, {}), (1, 1500, {}), (3, 1025, OTHER)]


def scene_id(v):
    return "other" if v == OTHER else "defaults" if v == {} else None


_cache = {}


def reference(seed, n, kw):
    """``pyramid`` on ``iss_ref.scene(seed, n)``, computed once per process and shared (treat it as read-only)."""
    key = (seed, n, tuple(sorted(kw.items())))
    if key not in _cache:
        P = iss_ref.scene(seed, n)
        _cache[key] = (P, pyramid(P, **kw))
    return _cache[key]


def lattice():
    """125 points of a 5 x 5 x 5 lattice of pitch 1/4 m, shuffled: most distances tie, and every d2 is exact."""
    g = np.arange(5, dtype=np.float64) / 4.0
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(P[np.random.RandomState(5).permutation(125)], dtype=np.float32)


def two_points(far):
    """The origin and a point ``far`` metres above it: at sigma = 0.5 the second counts for the first iff far * far <= 2.25."""
    return np.array([[0.0, 0.0, 0.0], [0.0, 0.0, far]], dtype=np.float32)
