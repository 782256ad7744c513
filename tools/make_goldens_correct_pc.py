#!/usr/bin/env python3
"""Generate tests/golden/correct_pc.npz by IMPORTING THE REFERENCE: Transformations.CorrectPC (:28-39), the vertical-angle
calibration of the KITTI scans.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_correct_pc.py --reference <checkout of the reference>

Nothing of the reference is restated here: its CorrectPC runs on the points below for every angle, and the rotation matrices of a
256-point subset are recorded by wrapping its Quatern2RotMat while CorrectPC runs (the function looks the name up in its module at
call time).  Needs NumPy >= 2: the contract is the NEP 50 arithmetic (caelo/correct.py); the file records the NumPy version.

Points [4096,3] f32, mm-quantised like KITTI's .bin files, ranges out to 120 m on an HDL-64E-like elevation fan, plus the edge cases
the rotation axis p x z^ has: x = 0 only, y = 0 only, z = 0, negative z, signed zeros, twelve points on the z axis and the origin
(x = y = 0: the axis has norm 0 and the reference's result is NaN).  x^2 + y^2 is either exactly 0 or a normal float32 everywhere
(|x| or |y| >= 1 mm here; the contract asks for >= 2^-60), so flushing of denormals is never part of what the file pins.
"""
import argparse
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = [0.22, 0.205, -0.3, 0.0, 45.0]
N, N_SUB = 4096, 256


def make_points():
    rs = np.random.RandomState(20191103)
    n_special = 64
    n = N - n_special
    rng = np.exp(rs.uniform(np.log(1.5), np.log(120.0), n))
    az = rs.uniform(-np.pi, np.pi, n)
    el = np.deg2rad(rs.uniform(-24.8, 2.0, n))
    p = np.stack([rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el)], axis=1)
    p[:200, 2] = np.abs(p[:200, 2])                      # returns above the sensor too
    p[200:216] *= 120.0 / np.abs(p[200:216]).max(axis=1, keepdims=True)   # a coordinate at +-120 m
    p = (np.round(p * 1000.0) / 1000.0).astype(np.float32)
    assert (np.maximum(np.abs(p[:, 0]), np.abs(p[:, 1])) >= 1e-3).all()
    sp = np.zeros((n_special, 3), dtype=np.float32)
    k = 0

    def put(rows):
        nonlocal k
        rows = np.asarray(rows, dtype=np.float32)
        sp[k:k + len(rows)] = rows
        k += len(rows)
    put([[0.0, y, z] for y, z in ((3.217, -1.5), (-47.001, 0.25), (0.001, -0.001), (119.999, -1.733))])                           # x = 0 only
    put([[x, 0.0, z] for x, z in ((12.5, -1.7), (-80.003, 2.0), (0.001, 0.001), (-119.999, -1.733))])                           # y = 0 only
    put([[-0.0, 5.0, -1.0], [7.25, -0.0, -1.0], [0.0, -2.5, 0.0], [-3.0, 0.0, 0.0]])                                             # signed zeros, z = 0
    put([[10.0, -10.0, 0.0], [-0.001, 0.001, 0.0], [64.0, 32.0, 0.0], [1.0, 1.0, -0.0]])                                         # z = 0
    put([[0.0, 0.0, z] for z in (1.0, -1.0, 0.001, -0.001, 2.5, -1.733, 50.0, -30.0, 119.999, -119.999)])                        # the z axis
    put([[-0.0, 0.0, 1.5], [0.0, -0.0, -1.5]])                                                                                     # ... with signed zeros
    put([[0.0, 0.0, 0.0]])                                                                                                         # the origin
    fill = p[:n_special - k].copy()
    fill[:, 2] = -fill[:, 2]
    put(fill)
    assert k == n_special
    pts = np.concatenate([p, sp], axis=0)
    r2 = pts[:, 0].astype(np.float64) ** 2 + pts[:, 1].astype(np.float64) ** 2
    assert ((r2 == 0) | (r2 >= 2.0 ** -120)).all() and pts.shape == (N, 3) and pts.dtype == np.float32
    assert int((r2 == 0).sum()) >= 9
    return pts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="directory of the reference's Transformations.py")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "correct_pc.npz"))
    a = ap.parse_args()
    if not os.path.exists(os.path.join(a.reference, "Transformations.py")):
        ap.error("--reference must name the directory that holds the reference's Transformations.py")
    assert int(np.__version__.split(".")[0]) >= 2, "NumPy >= 2 (NEP 50 arithmetic) is the contract"
    sys.path.insert(0, a.reference)
    import Transformations as T

    pts = make_points()
    sub = np.r_[np.arange(0, N - 64, (N - 64) // (N_SUB - 64))[:N_SUB - 64], np.arange(N - 64, N)].astype(np.int32)
    assert sub.size == N_SUB and np.unique(sub).size == N_SUB
    out = np.empty((len(ANGLES), N, 3), dtype=np.float32)
    R = np.empty((len(ANGLES), N_SUB, 3, 3), dtype=np.float32)
    seen = []
    inner = T.Quatern2RotMat

    def recording(q):
        r = inner(q)
        seen.append(np.array(r, copy=True))
        return r
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the axis points divide 0 by 0
        for i, ang in enumerate(ANGLES):
            res = T.CorrectPC(pts, ang)
            assert res.dtype == np.float32 and res.shape == pts.shape
            out[i] = res
            T.Quatern2RotMat = recording
            try:
                del seen[:]
                res_sub = T.CorrectPC(np.ascontiguousarray(pts[sub]), ang)
            finally:
                T.Quatern2RotMat = inner
            assert len(seen) == N_SUB and all(r.dtype == np.float32 and r.shape == (3, 3) for r in seen)
            ok = ~np.isnan(res[sub])
            assert np.array_equal(np.isnan(res_sub), ~ok) and np.array_equal(res_sub.view(np.uint32)[ok], res[sub].view(np.uint32)[ok])
            R[i] = np.stack(seen)
    nan_rows = np.isnan(out).any(axis=2)
    axis = (pts[:, 0] == 0) & (pts[:, 1] == 0)
    assert (nan_rows == axis[None, :]).all(), "NaN exactly on the z axis, at every angle"
    np.savez_compressed(a.out, points=pts, angles=np.array(ANGLES, dtype=np.float64), out=out, R=R, R_index=sub,
                        numpy_version=np.array(np.__version__))
    print("wrote %s: %d points (%d on the z axis), %d angles, R of %d points, NumPy %s, %d bytes"
          % (a.out, N, int(axis.sum()), len(ANGLES), N_SUB, np.__version__, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
