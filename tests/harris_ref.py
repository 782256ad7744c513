"""The Harris3D key point definition (include/caelo.h) restated in float64 NumPy, the input conditions the GPU tests
rest on, and the scenes they use.  A test helper: nothing in the package imports it.

The restatement follows the device's arithmetic where the result depends on it: the neighbour mask comes from the rounded
d2 = (dx*dx + dy*dy) + dz*dz, every sum is np.cumsum(...)[-1] over the neighbours in ascending index (one element after the other, the
device's order), C_ab = S_ab - (S_a*S_b)/k and the response expression are evaluated in the stated operation order.  Only the
eigenvector comes from another solver (np.linalg.eigh against the kernel's cyclic Jacobi with accumulated rotations): two solvers
differ in the normal by a few ulp divided by the relative gap between the two smallest eigenvalues, which ``margins`` measures.
"""
import numpy as np

import iss_ref
from iss_ref import scene  # noqa: F401  (the scenes are the ISS tests' scenes: imported, not copied)

DEFAULTS = dict(radius=1.0, threshold=0.001)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _params(kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _seq(v):
    """The sum of v, one element after the other in ascending index, starting from 0.0."""
    return np.cumsum(v)[-1] if v.size else np.float64(0.0)


def normal_of(C6, p):
    """The unit eigenvector of the smallest eigenvalue of C (xx, xy, xz, yy, yz, zz), facing the origin from p -> (normal [3], w [3]
    ascending eigenvalues)."""
    c = C6
    w, v = np.linalg.eigh(np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]))
    x, y, z = v[:, 0]
    nrm = np.sqrt((x * x + y * y) + z * z)
    nv = np.array([x / nrm, y / nrm, z / nrm])
    if (nv[0] * p[0] + nv[1] * p[1]) + nv[2] * p[2] > 0:
        nv = -nv
    return nv, w


def response_of(N):
    """PCL's Harris expression on N (xx, xy, xz, yy, yz, zz), evaluated left to right as the definition states it."""
    xx, xy, xz, yy, yz, zz = N
    tr = (xx + yy) + zz
    if not tr != 0:
        return np.float64(0.0)
    det = (xx * yy) * zz + ((2.0 * xy) * xz) * yz
    det = det - (xz * xz) * yy
    det = det - (xy * xy) * zz
    det = det - (yz * yz) * xx
    return (0.04 + det) - (0.04 * tr) * tr


def harris(pts, **kw):
    """pts [n,3] float32 -> dict: n_neigh [n] i32, valid [n] bool (a normal exists: at least 3 neighbours), C [n,6], w [n,3] (ascending
    eigenvalues of C; 0 where invalid), normals [n,3] (0 where invalid), n_valid [n] (neighbours with a valid normal), N [n,6],
    response [n] (-1 where invalid), key_idx (ascending), nb_sets / valid_sets (per point: indices of the neighbours / of those with a
    valid normal), and the parameters."""
    p = _params(kw)
    P = np.asarray(pts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = P.shape[0]
    r2 = np.float64(p["radius"]) * np.float64(p["radius"])
    n_neigh = np.zeros(n, np.int32)
    valid = np.zeros(n, bool)
    C = np.zeros((n, 6))
    w = np.zeros((n, 3))
    normals = np.zeros((n, 3))
    nb_sets = []
    for i in range(n):
        d = P - P[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        nb = np.flatnonzero(d2 < r2)
        nb_sets.append(nb)
        k = nb.size
        n_neigh[i] = k
        if k < 3:
            continue
        valid[i] = True
        dn = d[nb]
        S = [_seq(dn[:, a]) for a in range(3)]
        for q, (a, b) in enumerate(PAIRS):
            C[i, q] = _seq(dn[:, a] * dn[:, b]) - (S[a] * S[b]) / np.float64(k)
        normals[i], w[i] = normal_of(C[i], P[i])
    n_valid = np.zeros(n, np.int32)
    N = np.zeros((n, 6))
    resp = np.full(n, -1.0)
    valid_sets = []
    for i in range(n):
        vs = nb_sets[i][valid[nb_sets[i]]]
        valid_sets.append(vs)
        if not valid[i]:
            continue
        n_valid[i] = vs.size
        nn = normals[vs]
        for q, (a, b) in enumerate(PAIRS):
            N[i, q] = _seq(nn[:, a] * nn[:, b]) / np.float64(vs.size)
        resp[i] = response_of(N[i])
    key = np.zeros(n, bool)
    for i in range(n):
        if valid[i] and resp[i] >= p["threshold"] and not (resp[i] < resp[valid_sets[i]]).any():
            key[i] = True
    return dict(n_neigh=n_neigh, valid=valid, C=C, w=w, normals=normals, n_valid=n_valid, N=N, response=resp,
                key_idx=np.flatnonzero(key).astype(np.int32), nb_sets=nb_sets, valid_sets=valid_sets, params=p, P=P)


def margins(r):
    """-> (normal gap, threshold margin, suppression gap) of a result of ``harris``, after asserting that ties are exact.

    Normal gap: the smallest (e2 - e3) / e1 over points with a valid normal -- the conditioning of the normal.  Threshold margin: the
    smallest |response - threshold| over those points.  Suppression gap: the smallest |response_i - response_j| over pairs where i is
    at or above the threshold, j is a neighbour of i with a valid normal, and the two points' valid-neighbour sets differ.  Pairs with
    IDENTICAL valid-neighbour sets are the same sums in the same order on both sides: their responses must be bit-equal (asserted
    here), so such ties are exact on any implementation of the definition and both points survive.  (inf when nothing is to decide.)"""
    p = r["params"]
    v = r["valid"]
    w = r["w"][v]
    normal_gap = float(np.min((w[:, 1] - w[:, 0]) / w[:, 2])) if w.shape[0] else np.inf
    resp = r["response"]
    thr_margin = float(np.min(np.abs(resp[v] - p["threshold"]))) if v.any() else np.inf
    gap = np.inf
    for i in np.flatnonzero(v & (resp >= p["threshold"])):
        si = r["valid_sets"][i]
        for j in si:
            if j == i:
                continue
            if np.array_equal(si, r["valid_sets"][j]):
                assert resp[i].tobytes() == resp[j].tobytes(), (i, j)
            else:
                gap = min(gap, abs(resp[i] - resp[j]))
    return normal_gap, thr_margin, float(gap)


# the scenes of the GPU parity test: (seed, n, parameters).  n covers a partial last tile (1500), the chunk edge (1025), the tile edge
# (257) and a frame smaller than one chunk (600); the last two put radius and threshold elsewhere.
WIDE_A = dict(radius=1.5, threshold=0.005)
WIDE_B = dict(radius=2.0, threshold=0.01)
SCENES = [(9, 1500, {}), (2, 1500, {}), (3, 1025, {}), (4, 257, {}), (5, 600, {}), (1, 1500, WIDE_A), (3, 1025, WIDE_B)]
# the least the three margins of a scene must be (tests/test_harris_host.py): input conditions, not kernel tolerances
NORMAL_GAP, THRESHOLD_MARGIN, SUPPRESSION_GAP = 1e-5, 1e-7, 1e-7


def scene_id(v):
    return "dflt" if v == {} else ("r%g" % v["radius"] if isinstance(v, dict) else str(v))


_cache = {}


def reference(seed, n, kw):
    """``harris`` on ``scene(seed, n)``, computed once per process and shared (treat it as read-only)."""
    key = (seed, n, tuple(sorted(kw.items())))
    if key not in _cache:
        P = iss_ref.scene(seed, n)
        _cache[key] = (P, harris(P, **kw))
    return _cache[key]


def strict_radius(inside):
    """A centre (row 0), two points well inside 1 m and a fourth at exactly 1.0 m (``inside`` False) or 1 - 1/64 m (True), all
    dyadic: the centre has 3 or 4 neighbours."""
    far = 1.0 - (1.0 / 64.0 if inside else 0.0)
    return np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0.125], [far, 0, 0]], dtype=np.float32)


def corner():
    """The corner of the three planes x = 0, y = 0, z = 0 at the origin (row 0), 13 dyadic points.  Two points that see each other lie
    in each other's plane, so every covariance has an exactly zero row and column and every normal is a unit vector exactly:
      rows 0-2    the origin and two points of z = 0: each sees only points of z = 0                        -> normal (0, 0, +-1)
      rows 3-5    three points on the y axis, rows 6-7 two helpers of x = 0 out of the origin's reach      -> normal (+-1, 0, 0)
      rows 8-10   three points on the x axis, rows 11-12 two helpers of y = 0 out of the origin's reach    -> normal (0, +-1, 0)
    No point of one group other than the origin is within 1 m of a point of another.  The origin sees rows 0-5 and 8-10: three normals
    of each kind, N = diag(3, 3, 3) / 9, response = (1/3)^3 to rounding."""
    return np.array([[0, 0, 0], [-0.75, -0.25, 0], [-0.25, -0.75, 0],
                     [0, 0.75, 0], [0, 0.8125, 0], [0, 0.875, 0], [0, 0.75, 0.75], [0, 0.75, -0.75],
                     [0.75, 0, 0], [0.8125, 0, 0], [0.875, 0, 0], [0.75, 0, 0.75], [0.75, 0, -0.75]], dtype=np.float32)


def collinear():
    """Three exactly collinear dyadic points within 1 m of each other: C has rank one, the normal is ill-defined."""
    return np.array([[1.0, 2.0, 0.5], [1.25, 2.25, 0.75], [1.5, 2.5, 1.0]], dtype=np.float32)
