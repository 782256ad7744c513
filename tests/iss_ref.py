"""The ISS key point definition (include/caelo.h) restated in float64 NumPy, the two input conditions the GPU tests
rest on, and the scenes they use.  A test helper: nothing in the package imports it.

The restatement follows the device's arithmetic where the result depends on it: the neighbour mask comes from the rounded
d2 = (dx*dx + dy*dy) + dz*dz, and a scatter sum is np.cumsum(d_a * d_b)[-1] over the neighbours in ascending index -- NumPy's
cumsum adds one element after the other, which is the device's order, so the six sums are the device's bits.  Only the eigenvalues
come from another solver (np.linalg.eigvalsh against the kernel's cyclic Jacobi): they agree to a few ulp of ||C||, and every
decision taken from them is exact as long as it is not closer to its threshold than that -- which ``margins`` measures.
"""
import numpy as np

DEFAULTS = dict(salient_radius=2.0, non_max_radius=2.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)


def _params(kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _d2(P, i):
    """-> (d [n,3], d2 [n]) of every point against point i, as the device rounds them."""
    d = P - P[i]
    return d, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def iss(pts, **kw):
    """pts [n,3] float32 -> dict: n_neigh [n] i32 (at salient_radius), C [n,6] (xx, xy, xz, yy, yz, zz; 0 without enough neighbours),
    eig [n,3] = e1 >= e2 >= e3 (0 without enough neighbours), saliency [n], candidate [n] bool (saliency >= 0: the thresholds passed),
    n_neigh_nms [n], key_idx (ascending), and the parameters."""
    p = _params(kw)
    P = np.asarray(pts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = P.shape[0]
    rs2 = np.float64(p["salient_radius"]) * np.float64(p["salient_radius"])
    rn2 = np.float64(p["non_max_radius"]) * np.float64(p["non_max_radius"])
    n_neigh = np.zeros(n, np.int32)
    n_nms = np.zeros(n, np.int32)
    C = np.zeros((n, 6))
    eig = np.zeros((n, 3))
    sal = np.full(n, -1.0)
    nms_sets = []
    for i in range(n):
        d, d2 = _d2(P, i)
        nb = d2 < rs2
        n_neigh[i] = nb.sum()
        m = d2 < rn2
        n_nms[i] = m.sum()
        nms_sets.append(np.flatnonzero(m))
        if n_neigh[i] < p["min_neighbors"]:
            continue
        dn = d[nb]
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            C[i, k] = np.cumsum(dn[:, a] * dn[:, b])[-1]
        c = C[i]
        w = np.linalg.eigvalsh(np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]))
        e1, e2, e3 = w[2], w[1], w[0]
        eig[i] = e1, e2, e3
        with np.errstate(divide="ignore", invalid="ignore"):
            if e3 >= 0 and e2 / e1 < p["gamma_21"] and e3 / e2 < p["gamma_32"]:
                sal[i] = e3
    key = np.zeros(n, bool)
    for i in range(n):
        if sal[i] > 0 and n_nms[i] >= p["min_neighbors"] and not (sal[i] < sal[nms_sets[i]]).any():
            key[i] = True
    return dict(n_neigh=n_neigh, C=C, eig=eig, saliency=sal, candidate=sal >= 0, n_neigh_nms=n_nms, key_idx=np.flatnonzero(key).astype(np.int32),
                nms_sets=nms_sets, params=p)


def margins(r):
    """-> (minimum decision margin, minimum saliency gap) of a result of ``iss``.

    Margin: the smallest, over points with enough neighbours, of |e2 - g21 e1| / e1, |e3 - g32 e2| / e1 and e3 / e1 -- how far, in units
    of ||C||, the nearest threshold decision (and the sign of e3) is from flipping.  Gap: the smallest |s_i - s_j| / max(s) over pairs
    of candidates within non_max_radius of each other -- how far the nearest suppression decision is from flipping.  (inf when there is
    nothing to decide.)"""
    p = r["params"]
    ok = r["n_neigh"] >= p["min_neighbors"]
    e = r["eig"][ok]
    margin = np.inf
    if e.shape[0]:
        e1 = e[:, 0]
        margin = min(np.min(np.abs(e[:, 1] - p["gamma_21"] * e1) / e1), np.min(np.abs(e[:, 2] - p["gamma_32"] * e[:, 1]) / e1), np.min(e[:, 2] / e1))
    s = r["saliency"]
    gap = np.inf
    if r["candidate"].any():
        top = s.max()
        for i in np.flatnonzero(r["candidate"]):
            nb = r["nms_sets"][i]
            nb = nb[(nb != i) & r["candidate"][nb]]
            if nb.size:
                gap = min(gap, np.min(np.abs(s[nb] - s[i])) / top)
    return float(margin), float(gap)


def scene(seed, n):
    """n points of a small street scene inside 16 x 16 x 4 m: half on a noisy ground plane, a fifth on each of two noisy walls, the
    rest scattered uniformly; shuffled, rounded to 2^-10 m, float32."""
    rs = np.random.RandomState(seed)
    n_ground, n_wall = n // 2, n // 5
    n_free = n - n_ground - 2 * n_wall
    ground = np.c_[rs.uniform(0, 16, n_ground), rs.uniform(0, 16, n_ground), rs.normal(0.0, 0.03, n_ground)]
    wall_a = np.c_[rs.uniform(0, 16, n_wall), 15.5 + rs.normal(0.0, 0.03, n_wall), rs.uniform(0, 4, n_wall)]
    wall_b = np.c_[3.0 + rs.normal(0.0, 0.03, n_wall), rs.uniform(0, 16, n_wall), rs.uniform(0, 4, n_wall)]
    free = np.c_[rs.uniform(0, 16, n_free), rs.uniform(0, 16, n_free), rs.uniform(0, 4, n_free)]
    P = np.concatenate([ground, wall_a, wall_b, free])
    P = P[rs.permutation(P.shape[0])]
    return np.ascontiguousarray(np.round(P * 1024.0) / 1024.0, dtype=np.float32)


# the scenes of the GPU parity test: (seed, n, parameters).  n covers a partial last tile (1500), the chunk edge (1025), the tile edge
# (257) and a frame smaller than one chunk (600); the second parameter set puts the thresholds where they really cut.
# (Seed 1 at the defaults has two candidates 5.0e-8 of max(s) apart, under the bar below: seed 9 stands in for it.)
CUT = dict(salient_radius=1.0, non_max_radius=0.5, gamma_21=0.6, gamma_32=0.6)
SCENES = [(9, 1500, {}),(2, 1500, {}), (3, 1025, {}), (4, 257, {}), (5, 600, {}), (1, 1500, CUT), (3, 1025, CUT)]
CERTIFIED = 1e-7   # the least margin and gap a scene must have (tests/test_iss_host.py): an input condition, ~1e6 x the f64 error

_cache = {}


def reference(seed, n, kw):
    """``iss`` on ``scene(seed, n)``, computed once per process and shared (treat it as read-only)."""
    key = (seed, n, tuple(sorted(kw.items())))
    if key not in _cache:
        P = scene(seed, n)
        _cache[key] = (P, iss(P, **kw))
    return _cache[key]


def tie_cluster():
    """A 40-point cluster on multiples of 1/64 m and its copy 32 m away along x (80 points): every difference, product and sum is
    exact in float64, so point k and point k + 40 have bit-equal saliencies."""
    rs = np.random.RandomState(7)
    a = rs.randint(-64, 65, size=(40, 3)).astype(np.float64) / 64.0
    b = a + np.array([32.0, 0.0, 0.0])
    return np.ascontiguousarray(np.concatenate([a, b]), dtype=np.float32)


def strict_radius(inside):
    """A centre (row 0), three points well inside 2 m and a fifth at exactly 2.0 m (``inside`` False) or 2 - 1/64 m (True), all dyadic."""
    far = 2.0 - (1.0 / 64.0 if inside else 0.0)
    return np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0.25], [-0.25, 0.5, 0.5], [far, 0, 0]], dtype=np.float32)


def exact_plane():
    """200 dyadic points with z = 0 inside 8 x 8 m."""
    rs = np.random.RandomState(11)
    xy = rs.randint(0, 8 * 64, size=(200, 2)).astype(np.float64) / 64.0
    return np.ascontiguousarray(np.c_[xy, np.zeros(200)], dtype=np.float32)


MANY_FRAMES = 65537   # two more than one launch takes as its grid's y (65 535): the entry points slice the frames


def many_frames():
    """-> (pts [65 537, 4, 3] f32, n_pts [65 537] i32): frame f holds f % 5 points of a bent line, k = 0 .. 3 at
    (k, k^2 / 4, (k % 3) / 2) * (0.25 + (f % 7) / 8) + ((f % 64) / 4, 0, 0); the rows past n_pts are NaN.  At radius 1 the spacings give
    every neighbour count from 1 to 4."""
    f = np.arange(MANY_FRAMES)
    k = np.arange(4, dtype=np.float64)
    pts = np.stack([k, k * k / 4.0, (k % 3) / 2.0], axis=-1)[None] * (0.25 + (f % 7) / 8.0)[:, None, None]
    pts[:, :, 0] += ((f % 64) / 4.0)[:, None]
    n_pts = (f % 5).astype(np.int32)
    pts[k[None, :] >= n_pts[:, None]] = np.nan
    return np.ascontiguousarray(pts, dtype=np.float32), n_pts


def neighbour_counts(pts, n_pts, radius):
    """pts [F, ld, 3] f32, n_pts [F] -> [F, ld] i32: per point the points of its frame with d2 < radius * radius, as the device rounds
    them (itself included); 0 in the rows past n_pts."""
    P = pts.astype(np.float64)
    d = P[:, None, :, :] - P[:, :, None, :]   # [F, i, j, 3]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    inside = np.arange(pts.shape[1])[None, :] < np.asarray(n_pts)[:, None]
    with np.errstate(invalid="ignore"):
        near = (d2 < np.float64(radius) * np.float64(radius)) & inside[:, :, None] & inside[:, None, :]
    return near.sum(axis=2).astype(np.int32)
