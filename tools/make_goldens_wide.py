#!/opt/conda/bin/python3.9
"""Generate tests/golden/wide_desc.npz by IMPORTING THE REFERENCE: SolveRelativePose (Match.py:241-283) on descriptors that are not
the encoder's 60 columns -- 128 wide, the width of the USIP descriptors of the published comparison (GenerateTrajactory.m:193-203).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tools/make_goldens_wide.py

Same interpreter and stubs as tools/make_goldens_keysources.py.  The reference is touched under __main__ only: importing this
module (tests/test_wide_match_host.py reads PAIRS and make_pair from it) needs NumPy and nothing else.

Two synthetic pairs.  Frame 1's descriptors are frame 0's, permuted, plus noise; a share of them is replaced by fresh random
descriptors (their nearest neighbour is arbitrary: outlier correspondences).  Frame 1's key points are frame 0's under the inverse
of a known rigid motion, plus noise.  Pair "a" (K = 50, few outliers, little noise) is solved at the first residual threshold;
pair "b" (K = 256, noisy points) leaves too few inliers there and escalates.  The oracle is asserted against the reference on both,
so the test that reads the golden pins the engine to the reference itself.

The noisy pair is the larger one on purpose.  RANSAC4RT draws its four indices with replacement; a sample with a repeated index is
three points, its cross-covariance has rank 2, and the sign LAPACK gives the third singular vector decides between a rotation and
the reflection of Match.py:151-155 -- another NumPy build scores such a sample differently.  Among 50 noisy pairs one sample in
eight is of that kind and one of them can hold the largest count (seen: 17 inliers under one build, 1 under another); among 256 it
is one in forty, and the script asserts that the winning sample has four distinct indices.  tests/test_wide_match_host.py runs the
oracle on the golden's inputs under the test interpreter's NumPy and expects the golden's inlier sets.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "wide_desc.npz")
DIM = 128
# name: (K, outlier share, descriptor noise, key point noise [m], generator seed, RANSAC seed)
PAIRS = {"a": (50, 0.2, 0.05, 0.02, 11, 0), "b": (256, 0.3, 0.05, 0.50, 12, 1)}


def make_pair(K, outliers, desc_noise, pts_noise, seed):
    """-> key points 0 [K,3], descriptors 0 [K,DIM], key points 1, descriptors 1 (all f32), the permutation, R, T (p0 ~ R p1 + T)."""
    rs = np.random.RandomState(seed)
    p0 = rs.uniform(-40, 40, (K, 3)).astype(np.float32)
    p0[:, 2] *= 0.1
    f0 = rs.uniform(-1, 1, (K, DIM)).astype(np.float32)
    yaw = 0.05
    R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    T = np.array([[1.2], [-0.3], [0.05]])
    perm = rs.permutation(K)
    p1 = (np.dot(R.T, p0[perm].T.astype(np.float64) - T).T + rs.normal(0, pts_noise, (K, 3))).astype(np.float32)
    f1 = (f0[perm] + rs.normal(0, desc_noise, (K, DIM))).astype(np.float32)
    bad = rs.uniform(size=K) < outliers
    f1[bad] = rs.uniform(-1, 1, (int(bad.sum()), DIM)).astype(np.float32)
    return p0, f0, p1, f1, perm, R, T


def main():
    import contextlib
    import io
    import types
    import warnings
    if not hasattr(np, "bool"):
        np.bool = bool  # Match.py:179,193
    for n in ("mayavi", "mayavi.mlab"):
        sys.modules[n] = types.ModuleType(n)
    sys.modules["mayavi"].mlab = sys.modules["mayavi.mlab"]
    cp = types.ModuleType("cupy")  # every CuPy symbol used in SphericalRing.py:137-206 (imported by Match.py; not called here)
    for k in ("array", "zeros", "min", "sum", "squeeze", "int32", "float32"):
        setattr(cp, k, getattr(np, k))
    cp.bool = bool
    cp.asnumpy = np.asarray
    cp.argsort = lambda a: np.argsort(a, kind="stable")
    sys.modules["cupy"] = cp
    mpl = types.ModuleType("matplotlib"); mpl.pyplot = types.ModuleType("matplotlib.pyplot")
    sys.modules.setdefault("matplotlib", mpl); sys.modules.setdefault("matplotlib.pyplot", mpl.pyplot)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    warnings.filterwarnings("ignore")
    import Match as RefMatch
    import oracle as orc
    from scipy.spatial.distance import cdist

    g = {"dim": DIM}
    for name, (K, outliers, dn, pn, seed, rseed) in PAIRS.items():
        p0, f0, p1, f1, perm, Rg, Tg = make_pair(K, outliers, dn, pn, seed)
        W0, W1 = np.ones((K, 1), np.float32), np.ones((K, 1), np.float32)
        np.random.seed(rseed)        # RandomState(seed) is the stream of engine.ransac_draws(seed)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            R, T, ok, i0, i1, thr = RefMatch.SolveRelativePose(p0, f0, W0, p1, f1, W1)
        iters = int(buf.getvalue().split("cntItersRANSAC =")[1].split()[0])
        trace = []
        oR, oT, ook, oi0, oi1, othr = orc.SolveRelativePose(p0, f0, W0, p1, f1, W1, rng=np.random.RandomState(rseed), trace=trace)
        best = max((t for t in trace if t[2] == othr), key=lambda t: t[1])      # (max keeps the first of equal counts, like :199)
        assert len(set(best[0].tolist())) == 4, "the winning sample repeats an index: its score depends on the LAPACK build"
        assert ook == ok and othr == thr and np.array_equal(oi0, i0) and np.array_equal(oi1, i1)
        assert np.allclose(oR, R, atol=1e-6) and np.allclose(oT, T, atol=1e-5), "oracle pose != reference"
        pair_idx = np.argmin(cdist(f0, f1, metric="euclidean"), axis=0)   # Match.py:257-258
        assert np.array_equal(pair_idx, orc.match(f0, f1)[0])
        g.update({name + "_p0": p0, name + "_f0": f0, name + "_p1": p1, name + "_f1": f1, name + "_pair_idx": pair_idx.astype(np.int64),
                  name + "_R": np.asarray(R, np.float64), name + "_T": np.asarray(T, np.float64), name + "_ok": bool(ok),
                  name + "_thr": float(thr), name + "_iters": iters, name + "_idx0": np.asarray(i0, np.int32),
                  name + "_idx1": np.asarray(i1, np.int32), name + "_seed": rseed})
        print("pair %s: K=%d ok=%s thr=%.1f iters=%d inliers=%d, %d of %d matches follow the permutation, T=%s" % (
            name, K, ok, thr, iters, len(i0), int((pair_idx == perm).sum()), K, np.round(np.asarray(T).ravel(), 3)))
    assert g["a_ok"] and g["a_thr"] == 0.4, "pair a is meant to be solved at the first threshold"
    assert g["b_thr"] > 0.4, "pair b is meant to escalate"
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
