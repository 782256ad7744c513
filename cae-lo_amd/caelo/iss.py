"""Host helpers of the ISS key point detector (csrc/iss.hip, Engine.iss_keypoints, detect_keypoints.py): the parameter checks of
the C ABI and the plumbing the reference wraps round its detector call (PclKeyPts.py:20-28, :33-46, :77-83).  Importable without a
GPU.  The detector itself runs on the device only; nothing here computes a key point.
"""
import math

import numpy as np

# PclKeyPts.py:42-46
DEFAULTS = dict(salient_radius=2.0, non_max_radius=2.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)
MAX_POINTS = 32768   # include/caelo.h CAELO_ISS_MAX_POINTS


def _finite(v):
    """Whether v is a number with a finite float value (caelo.harris checks its parameters with it too)."""
    try:
        return math.isfinite(float(v))
    except (TypeError, ValueError):
        return False


def _finite_positive(v):
    return _finite(v) and float(v) > 0.0


def check_params(**params):
    """The parameters of caelo_iss_keypoints with the defaults filled in -> dict.  ValueError for what the C ABI refuses: an unknown
    name, a radius or gamma that is not finite and positive, min_neighbors that is no integer >= 1."""
    unknown = sorted(set(params) - set(DEFAULTS))
    if unknown:
        raise ValueError("ISS parameters are %s (got %s)" % (", ".join(DEFAULTS), ", ".join(unknown)))
    p = dict(DEFAULTS)
    p.update(params)
    for name in ("salient_radius", "non_max_radius", "gamma_21", "gamma_32"):
        if not _finite_positive(p[name]):
            raise ValueError("ISS %s must be finite and positive (got %r)" % (name, p[name]))
        p[name] = float(p[name])
    m = p["min_neighbors"]
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) < 2 ** 31:
        raise ValueError("ISS min_neighbors must be an integer >= 1 (got %r)" % (m,))
    p["min_neighbors"] = int(m)
    return p


def voxel_downsample(pc, leaf):
    """pc [N, >=3] torch tensor (any device) -> the rows that are the FIRST point in scan order of their ``leaf``-sized cell
    (cell = floor(xyz / leaf)), still in scan order: real scan points, not centroids.  Stands in for the 0.2 m voxel grid behind the
    reference's ``np_0.20_20480_r90_sn`` files (PclKeyPts.py:77)."""
    import torch
    if not _finite_positive(leaf):
        raise ValueError("leaf must be finite and positive (got %r)" % (leaf,))
    if pc.dim() != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be [N, >= 3], got %s" % (tuple(pc.shape),))
    if pc.shape[0] == 0:
        return pc
    xyz = pc[:, 0:3].to(torch.float64)
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("voxel_downsample: the scan holds a non-finite coordinate")
    cell = torch.floor(xyz / float(leaf))
    cell = cell - cell.min(dim=0).values
    ext = cell.max(dim=0).values + 1
    if float(ext[0]) * float(ext[1]) * float(ext[2]) >= 2.0 ** 62:
        raise ValueError("voxel_downsample: %g-sized cells over this scan's extent do not fit a 64-bit key" % float(leaf))
    c = cell.to(torch.int64)
    e = ext.to(torch.int64)
    key = (c[:, 0] * e[1] + c[:, 1]) * e[2] + c[:, 2]
    order = torch.argsort(key, stable=True)   # stable: the first row of a run of equal keys is the cell's first point in scan order
    sk = key[order]
    first = torch.ones_like(sk, dtype=torch.bool)
    first[1:] = sk[1:] != sk[:-1]
    keep = torch.sort(order[first]).values
    return pc[keep]


def subsample(n, max_points, rng):
    """Indices of the points the detector sees: all n in order, or -- when n > max_points -- sorted
    ``rng.choice(n, max_points, replace=False)`` (PclKeyPts.py:81; sorted so that the points stay in scan order)."""
    n, max_points = int(n), int(max_points)
    if n <= max_points:
        return np.arange(n)
    return np.sort(rng.choice(n, max_points, replace=False))


def ensure_keypoint_number(kp, pc, k, rng):
    """Exactly k key points, the way PclKeyPts.py:20-28 gets them: kp [M,3] as it is when M == k; a random k of them when M > k; kp
    followed by k - M random points of pc [N,3] when M < k (``rng.choice(..., replace=False)`` in both cases: ValueError, as there,
    when pc holds fewer than k - M points)."""
    kp, pc, k = np.asarray(kp), np.asarray(pc), int(k)
    m = kp.shape[0]
    if m == k:
        return kp
    if m > k:
        return kp[rng.choice(m, k, replace=False), :]
    return np.concatenate((kp, pc[rng.choice(pc.shape[0], k - m, replace=False), :]), axis=0)
