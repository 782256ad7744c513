"""The comparison protocol's registrar on the host side (csrc/adaptive.hip, include/caelo.h): the draw table, the
host twin of the kernel, and the chaining rule of the reference's trajectory writer (Scripts/GenerateTrajactory.m:203-237).

The script seeds every pair with the previous pair's motion.  That prior changes nothing but rounding (a least-squares rigid fit to
moved points is the fit to the unmoved points composed with the inverse move), except that a pair that FAILS inherits the previous
pair's motion: the pairs are registered independently and ``chain_relative`` applies the carry-over.
"""
import numpy as np

from . import _ffi

MAX_TRIALS, DRAWS = _ffi.ADAPTIVE_MAX_TRIALS, _ffi.ADAPTIVE_DRAWS
REGISTRARS = ("match", "comparison")   # run_sequence.py --registrar: Match.py's RANSAC4RT (default) | ransacfitRt.m


def draw_table(seed=0):
    """[10001, 3] f64: the uniform doubles of RandomState(seed) (caelo_host_random_sample), three per trial.  ransac.m resets its
    random stream at every call, so every pair of a run consumes the same table."""
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("draw seed %r outside [0, 2^32)" % (seed,))
    out = np.empty((DRAWS, 3), np.float64)
    _ffi.check(_ffi.load().caelo_host_random_sample(int(seed), out.size, out.ctypes.data))
    return out


def check_draws(draws):
    d = np.ascontiguousarray(draws, dtype=np.float64)
    if d.shape != (DRAWS, 3):
        raise ValueError("draws must be [%d, 3] float64, got %s" % (DRAWS, d.shape))
    return d


def check_pairs(x1, x2):
    """x1, x2 [n, 3] or the reference's [3, n] -> two contiguous [n, 3] f64 arrays, n <= 1024."""
    a, b = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 2 or 3 not in a.shape:
        raise ValueError("x1 and x2 must both be [n, 3] (or [3, n]), got %s and %s" % (a.shape, b.shape))
    if a.shape[1] != 3:   # (a [3, 3] input is read as [n, 3])
        a, b = a.T, b.T
    if a.shape[0] > 1024:
        raise ValueError("at most 1024 pairs, got %d" % a.shape[0])
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def host_ransac_adaptive(x1, x2, t, draws):
    """caelo_host_ransac_adaptive: the kernel's functions on the host (no device).  -> (record (_ffi.ADAPTIVE_DTYPE), mask [n] u8)."""
    a, b = check_pairs(x1, x2)
    d = check_draws(draws)
    res = np.zeros(1, _ffi.ADAPTIVE_DTYPE)
    mask = np.zeros(max(1, a.shape[0]), np.uint8)
    _ffi.check(_ffi.load().caelo_host_ransac_adaptive(a.ctypes.data, b.ctypes.data, a.shape[0], d.ctypes.data, float(t), res.ctypes.data, mask.ctypes.data))
    return res[0], mask[:a.shape[0]]


def fit_rows(records):
    """records [p] (_ffi.ADAPTIVE_DTYPE) -> ([p, 12] f64 (R | T), solved [p]): a pair is solved when the walk ended below the trial
    limit on at least three pairs AND its best trial kept at least three inliers -- every other pair returns the identity to the
    script, whose ``update o prev`` is then the previous pair's motion."""
    p = len(records)
    rel = np.concatenate([records["R"].reshape(p, 9), records["T"].reshape(p, 3)], axis=1)
    return rel, (records["status"] == 0) & (records["n_inliers"] >= 3)


def chain_relative(rel, solved):
    """GenerateTrajactory.m:224-237 over independent fits: relative_k = fit_k where pair k is solved, else relative_(k-1) (the identity
    before the first solved pair).  rel [p, 12] -> [p, 12] f64."""
    out = np.array(rel, dtype=np.float64).reshape(-1, 12)
    prev = np.r_[np.eye(3).ravel(), np.zeros(3)]
    for k in range(len(out)):
        if solved[k]:
            prev = out[k].copy()
        else:
            out[k] = prev
    return out
