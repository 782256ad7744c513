"""CPU: the host side of the Harris3D key point detector -- the NumPy restatement of the definition (tests/harris_ref.py) on cases
worked by hand, the input conditions of every scene the GPU tests use, the parameter checks, the workspace size, the refusals of the
C entry point and detect_keypoints.py's argument handling."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import harris_ref  # noqa: E402
import iss_ref  # noqa: E402
from caelo import harris, iss  # noqa: E402


def test_restatement_on_an_exact_plane():
    """z = 0 on dyadic points: the z row and column of every C are exactly zero, so every valid normal is (0, 0, +-1) exactly, every
    N is (0, 0, 0, 0, 0, 1), the response is exactly 0 and nothing is a key point."""
    P = iss_ref.exact_plane()
    r = harris_ref.harris(P)
    v = r["valid"]
    assert 150 < v.sum() <= 200 and np.array_equal(v, r["n_neigh"] >= 3)
    assert np.array_equal(np.abs(r["normals"][v]), np.tile([0.0, 0.0, 1.0], (v.sum(), 1)))
    assert (r["normals"][~v] == 0).all() and (r["response"][~v] == -1.0).all()
    assert (r["response"][v] == 0.0).all() and r["key_idx"].size == 0
    assert harris_ref.harris(P, threshold=0.0)["key_idx"].tolist() == np.flatnonzero(v).tolist()   # equal responses all survive


def test_restatement_at_the_corner_of_three_planes():
    """harris_ref.corner(): the origin sees three exact normals of each axis, N = diag(1/3, 1/3, 1/3), response (1/3)^3 to rounding;
    every other point sees normals of one kind, or of its own kind and the origin's z: an N of rank one or two, response 0."""
    P = harris_ref.corner()
    assert np.array_equal(P * 16, np.round(P * 16))
    r = harris_ref.harris(P)
    assert r["n_neigh"].tolist() == [9, 3, 3, 6, 6, 6, 4, 4, 6, 6, 6, 4, 4] and r["valid"].all()
    expect = np.zeros((13, 3))
    expect[0:3, 2] = 1
    expect[3:8, 0] = 1
    expect[8:13, 1] = 1
    assert np.array_equal(np.abs(r["normals"]), expect)
    assert r["n_valid"][0] == 9 and r["N"][0].tolist() == [3.0 / 9.0, 0.0, 0.0, 3.0 / 9.0, 0.0, 3.0 / 9.0]
    assert abs(r["response"][0] - 1.0 / 27.0) < 1e-16
    # rows 3-5 and 8-10 see the origin (normal z) among their own kind: two kinds of normals, a rank-two N, det = 0 to rounding
    assert np.abs(r["response"][1:]).max() < 1e-17
    assert r["key_idx"].tolist() == [0]
    assert harris_ref.harris(P, threshold=0.04)["key_idx"].size == 0   # 1/27 = 0.037 is below 0.04


def test_restatement_on_two_points_and_the_strict_radius():
    two = harris_ref.harris(np.float32([[0, 0, 0], [0.5, 0, 0]]))
    assert two["n_neigh"].tolist() == [2, 2] and not two["valid"].any() and (two["normals"] == 0).all()
    assert two["response"].tolist() == [-1.0, -1.0] and two["key_idx"].size == 0
    out, inside = harris_ref.harris(harris_ref.strict_radius(False)), harris_ref.harris(harris_ref.strict_radius(True))
    assert out["n_neigh"][0] == 3 and inside["n_neigh"][0] == 4          # exactly 1.0 m is outside, 1 - 1/64 m is inside
    assert out["n_neigh"][3] == 2 and not out["valid"][3] and out["response"][3] == -1.0
    assert inside["n_neigh"][3] == 3 and inside["valid"][3]


def test_the_orientation_faces_the_origin():
    P, r = harris_ref.reference(*harris_ref.SCENES[3])
    v = r["valid"]
    dot = (r["normals"] * r["P"]).sum(axis=1)
    assert (dot[v] <= 0).all() and np.abs(np.linalg.norm(r["normals"][v], axis=1) - 1).max() < 1e-15


@pytest.mark.parametrize("seed,n,kw", harris_ref.SCENES, ids=harris_ref.scene_id)
def test_gpu_scenes_are_certified(seed, n, kw):
    """Conditions on the INPUTS of tests/test_harris_gpu.py, not tolerances of the kernels: every normal is conditioned by a relative
    eigenvalue gap of at least 1e-5, no response is closer than 1e-7 to the threshold, and no two competing responses that are not
    the same sums are closer than 1e-7 (those that are the same sums are asserted bit-equal by ``margins``).  A scene that fails gets
    another seed, never another bar."""
    P, r = harris_ref.reference(seed, n, kw)
    normal_gap, thr_margin, gap = harris_ref.margins(r)
    v = r["valid"]
    above = int((r["response"][v] >= r["params"]["threshold"]).sum())
    print("scene %d n %d %s: normal gap %.3g, threshold margin %.3g, suppression gap %.3g, %d key points, %d of %d valid points at or "
          "above the threshold" % (seed, n, kw, normal_gap, thr_margin, gap, len(r["key_idx"]), above, int(v.sum())))
    assert P.shape == (n, 3) and P.dtype == np.float32
    assert normal_gap >= harris_ref.NORMAL_GAP
    assert thr_margin >= harris_ref.THRESHOLD_MARGIN
    assert gap >= harris_ref.SUPPRESSION_GAP
    assert len(r["key_idx"]) >= 5
    assert 0.02 * v.sum() <= above <= 0.5 * v.sum()   # the threshold really cuts
    assert (r["response"][v] >= -1e-15).all() and (r["response"][v] <= 1.0 / 27.0 + 1e-15).all()


def test_boundary_inputs_say_what_the_gpu_tests_assume():
    T = iss_ref.tie_cluster()
    r = harris_ref.harris(T)
    assert r["response"][:40].tobytes() == r["response"][40:].tobytes()   # exact differences, the same sums: bit-equal pairs
    k = r["key_idx"]
    assert np.array_equal(k[: len(k) // 2] + 40, k[len(k) // 2:])
    c = harris_ref.harris(harris_ref.collinear())
    assert c["valid"].all() and c["n_neigh"].tolist() == [3, 3, 3] and np.isfinite(c["normals"]).all()


def test_check_params_refusals_and_defaults():
    from caelo import _ffi
    assert harris.check_params() == harris.DEFAULTS == harris_ref.DEFAULTS == dict(radius=1.0, threshold=0.001)
    d = _ffi.HarrisParams(**harris.DEFAULTS)
    assert (d.radius, d.threshold) == (1.0, 0.001)
    assert harris.check_params(radius=2, threshold=0) == dict(radius=2.0, threshold=0.0)
    assert harris.MAX_POINTS == iss.MAX_POINTS == _ffi.ISS_MAX_POINTS
    assert harris.ensure_keypoint_number is iss.ensure_keypoint_number and harris.subsample is iss.subsample
    assert harris.voxel_downsample is iss.voxel_downsample
    for bad in (dict(radius=0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(radius="x"), dict(radius=None),
                dict(threshold=-1e-9), dict(threshold=float("inf")), dict(threshold=float("nan")), dict(threshold="x"),
                dict(salient_radius=2.0), dict(min_neighbors=5)):
        with pytest.raises(ValueError):
            harris.check_params(**bad)


def test_workspace_size_and_refusals_before_any_launch():
    """caelo_harris_ws_bytes is positive and non-decreasing in both arguments; caelo_harris_keypoints refuses bad arguments with
    CAELO_ERR_ARG before it touches the device (so this runs without one)."""
    import ctypes as C
    from caelo import _ffi
    lib = _ffi.load()
    assert C.sizeof(_ffi.HarrisParams) == 16
    lds, fs = (1, 2, 255, 256, 257, 1025, 16384, 32768), (1, 2, 3, 8, 100, 70000)
    for f in fs:
        sizes = [lib.caelo_harris_ws_bytes(f, ld) for ld in lds]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and all(s >= f * ld * 26 for s, ld in zip(sizes, lds))
    for ld in lds:
        sizes = [lib.caelo_harris_ws_bytes(f, ld) for f in fs]
        assert sizes == sorted(sizes)
    assert lib.caelo_harris_ws_bytes(0, 256) > 0 and lib.caelo_harris_ws_bytes(-1, 256) == 0 and lib.caelo_harris_ws_bytes(1, 0) == 0
    good = _ffi.HarrisParams(1.0, 0.001)
    fake = C.c_void_p(4096)   # never dereferenced: every call below is refused, or is the n_frames == 0 no-op
    enough = lib.caelo_harris_ws_bytes(1, 256)

    def call(prm=good, ld=256, n_frames=1, ctx=fake, pts=fake, n_pts=fake, response=fake, key_idx=fake, n_key=fake, ws=fake, ws_bytes=enough):
        return lib.caelo_harris_keypoints(ctx, pts, n_frames, ld, n_pts, C.byref(prm) if prm is not None else None, response, None, None,
                                          key_idx, n_key, ws, ws_bytes, None)
    assert call(n_frames=0) == 0
    for kw in (dict(ctx=None), dict(pts=None), dict(n_pts=None), dict(response=None), dict(key_idx=None), dict(n_key=None), dict(ws=None),
               dict(prm=None), dict(ld=0), dict(ld=-5), dict(ld=32769), dict(n_frames=-1), dict(ws_bytes=enough - 1), dict(ws_bytes=0),
               dict(prm=_ffi.HarrisParams(0.0, 0.001)), dict(prm=_ffi.HarrisParams(-1.0, 0.001)),
               dict(prm=_ffi.HarrisParams(float("inf"), 0.001)), dict(prm=_ffi.HarrisParams(float("nan"), 0.001)),
               dict(prm=_ffi.HarrisParams(1.0, -1e-9)), dict(prm=_ffi.HarrisParams(1.0, float("inf"))),
               dict(prm=_ffi.HarrisParams(1.0, float("nan")))):
        assert call(**kw) == -1 and lib.caelo_last_error(), kw


def test_detect_keypoints_arguments(tmp_path, monkeypatch):
    """Parse-time handling through main(argv): --method harris is a choice, the other detector's options are refused with a message that
    names them, bad values are refused -- all before any engine exists (caelo.engine.Engine is replaced by a trap)."""
    import detect_keypoints
    import caelo.engine

    def trap(*a, **k):
        raise AssertionError("an engine was created before the arguments were refused")
    monkeypatch.setattr(caelo.engine, "Engine", trap)
    scans, out = tmp_path / "velodyne", tmp_path / "out"
    scans.mkdir()
    base = ["--scans", str(scans), "--out", str(out)]

    def refused(argv, *words):
        import contextlib
        import io
        err = io.StringIO()
        with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(err):
            detect_keypoints.main(argv)
        assert e.value.code == 2
        for w in words:
            assert w in err.getvalue(), (w, err.getvalue())

    # accepted as far as the parse goes: the refusal is the empty directory, not the method or its options
    refused(["--method", "harris"] + base, "no .bin files")
    refused(["--method", "harris", "--radius", "1.5", "--threshold", "0.005"] + base, "no .bin files")
    refused(["--method", "iss", "--salient-radius", "1.0", "--min-neighbors", "4"] + base, "no .bin files")
    refused(["--method", "sift"] + base, "invalid choice")
    refused(["--method", "harris", "--salient-radius", "2.0"] + base, "--salient-radius", "--method iss")
    refused(["--method", "harris", "--gamma-21", "0.9", "--min-neighbors", "5"] + base, "--gamma-21", "--min-neighbors", "--method iss")
    refused(["--method", "harris", "--non-max-radius", "2.0"] + base, "--non-max-radius")
    refused(["--method", "harris", "--gamma-32", "0.9"] + base, "--gamma-32")
    refused(["--method", "iss", "--radius", "1.0"] + base, "--radius", "--method harris")
    refused(["--method", "iss", "--threshold", "0.001"] + base, "--threshold", "--method harris")
    refused(["--method", "harris", "--radius", "0"] + base, "radius must be finite and positive")
    refused(["--method", "harris", "--radius", "inf"] + base, "radius")
    refused(["--method", "harris", "--threshold", "-0.1"] + base, "threshold must be finite and not negative")
    refused(["--method", "harris", "--threshold", "nan"] + base, "threshold")
    refused(["--method", "iss", "--min-neighbors", "0"] + base, "min_neighbors")
    refused(["--method", "harris", "--max-points", "40000"] + base, "--max-points")
    assert not out.exists()
