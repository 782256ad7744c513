"""A literal NumPy restatement, in float64, of the loop-closure definitions of include/caelo.h (Scan Context descriptor, prepared
columns, column-shifted distance, causal top-k search): the yardstick of tests/test_loops_host.py and tests/test_loops_gpu.py.
No code of the library."""
import numpy as np

RINGS, SECTORS, BINS = 20, 60, 1200
R_MAX, RING_STEP = 80.0, 4.0
# |d - restatement| of a dense distance: the f32 fmaf chain over 1 200 products with sum |a b| <= n_s, divided by n_s, plus the
# roundings of the unit columns, the division and the subtraction
DIST_BAR = 1200 * 2.0 ** -24 + 8 * 2.0 ** -24


def bins_of(pts):
    """-> (keep [n] bool, ring [n] f64 r / 4, sector [n] f64 theta / 2 pi * 60) before the floor: what decides a point's bin."""
    p = np.asarray(pts)
    x, y, z = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)
    keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(x * x + y * y)
        th = np.arctan2(y, x)
        th = np.where(th < 0, th + 2 * np.pi, th)
        keep &= r < R_MAX
        return keep, r / RING_STEP, th / (2 * np.pi) * 60       # in this order: the quarter turns come out as 15, 30, 45 exactly


def scan_context(pts):
    """[n, 3 or 4] -> SC [20, 60] f32"""
    p = np.asarray(pts)
    keep, fr, fs = bins_of(p)
    ring = np.minimum(RINGS - 1, np.floor(fr[keep])).astype(np.int64)
    sector = np.minimum(SECTORS - 1, np.floor(fs[keep])).astype(np.int64)
    val = p[keep, 2].astype(np.float32) + np.float32(2.0)
    img = np.full((RINGS, SECTORS), -np.inf, dtype=np.float32)
    np.maximum.at(img, (ring, sector), val)
    img[np.isneginf(img)] = 0
    return img


def prepare(sc):
    """SC [20, 60] -> (u [1200] f64 with u[c * 20 + r], valid [60] bool)"""
    v = np.asarray(sc, dtype=np.float64)
    norm = np.sqrt((v * v).sum(axis=0))
    valid = norm > 0
    u = np.where(valid, v / np.where(valid, norm, 1.0), 0.0)
    return u.T.reshape(BINS).copy(), valid


def shift_distances(u, valid, min_cols=1):
    """u [N, 1200] f64, valid [N, 60] bool -> (d [N, N, 60] f64: query i, candidate j, shift s; +inf where n_s < min_cols, n [N, N, 60])"""
    n_frames = u.shape[0]
    cols = u.reshape(n_frames, SECTORS, RINGS)
    d = np.empty((n_frames, n_frames, SECTORS))
    cnt = np.empty((n_frames, n_frames, SECTORS), dtype=np.int64)
    vi = valid.astype(np.int64)
    for s in range(SECTORS):
        rolled = np.roll(cols, -s, axis=1).reshape(n_frames, BINS)      # column c <- column (c + s) mod 60
        num = u @ rolled.T
        cnt[:, :, s] = vi @ np.roll(vi, -s, axis=1).T
        with np.errstate(divide="ignore", invalid="ignore"):
            d[:, :, s] = np.where(cnt[:, :, s] >= max(min_cols, 1), 1.0 - num / cnt[:, :, s], np.inf)
    return d, cnt


def search(u, valid, min_gap=50, k=1, max_dist=None, min_cols=1):
    """-> dict(d [N, N] f64 best distance (+inf outside the candidates), shift [N, N] (-1), all [N, N, 60], cand / dist / shift_k [N, k])"""
    n_frames = u.shape[0]
    ds, _ = shift_distances(u, valid, min_cols)
    i, j = np.mgrid[0:n_frames, 0:n_frames]
    ds[~(j <= i - min_gap)] = np.inf
    d = ds.min(axis=2)
    shift = np.where(np.isfinite(d), ds.argmin(axis=2), -1)            # argmin: the lowest s among equals
    cand = np.full((n_frames, k), -1, dtype=np.int64)
    dist = np.full((n_frames, k), np.inf)
    shift_k = np.full((n_frames, k), -1, dtype=np.int64)
    for q in range(n_frames):
        ok = np.isfinite(d[q]) if max_dist is None else d[q] < max_dist
        order = [c for c in np.lexsort((np.arange(n_frames), d[q])) if ok[c]][:k]
        cand[q, :len(order)], dist[q, :len(order)], shift_k[q, :len(order)] = order, d[q, order], shift[q, order]
    return dict(d=d, shift=shift, all=ds, cand=cand, dist=dist, shift_k=shift_k)
