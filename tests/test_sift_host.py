"""CPU: the host side of the SIFT3D key point detector -- the NumPy restatement of the definition (tests/sift_ref.py) on cases worked
by hand, the input conditions of every scene the GPU tests use, the parameter checks and the scales of an octave, the workspace size,
the refusals of the C entry points and detect_sift_keypoints.py's argument handling."""
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import iss_ref  # noqa: E402
import sift_ref  # noqa: E402
from caelo import iss, sift  # noqa: E402


def test_check_params_refusals_and_defaults():
    from caelo import _ffi
    assert sift.check_params() == sift.DEFAULTS == sift_ref.DEFAULTS == dict(min_scale=0.5, n_octaves=4, n_scales_per_octave=8, min_contrast=0.1)
    assert sift.check_params(min_scale=1, n_octaves=np.int64(8), n_scales_per_octave=16, min_contrast=0) == dict(
        min_scale=1.0, n_octaves=8, n_scales_per_octave=16, min_contrast=0.0)
    assert sift.K == sift_ref.K == _ffi.SIFT_K == 25 and sift.MAX_SCALES == _ffi.SIFT_MAX_SCALES == 19
    assert sift.MAX_POINTS == iss.MAX_POINTS and sift.ensure_keypoint_number is iss.ensure_keypoint_number and sift.subsample is iss.subsample
    for bad in (dict(min_scale=0), dict(min_scale=-0.5), dict(min_scale=float("inf")), dict(min_scale=float("nan")), dict(min_scale="x"),
                dict(min_scale=None), dict(min_scale=True), dict(n_octaves=0), dict(n_octaves=9), dict(n_octaves=2.0), dict(n_octaves=True),
                dict(n_scales_per_octave=0), dict(n_scales_per_octave=17), dict(n_scales_per_octave=4.0), dict(min_contrast=-1e-9),
                dict(min_contrast=float("inf")), dict(min_contrast=float("nan")), dict(min_contrast="x"), dict(radius=1.0),
                dict(salient_radius=2.0)):
        with pytest.raises(ValueError):
            sift.check_params(**bad)


def test_octave_scales():
    s = sift.octave_scales(0.5, 8)
    assert s.dtype == np.float64 and s.shape == (11,) and s[1] == 0.5 and s[9] == 1.0 and (np.diff(s) > 0).all()
    assert s.tobytes() == sift_ref.scales(0.5, 8).tobytes()
    assert s.tolist() == [0.5 * 2.0 ** ((k - 1) / 8) for k in range(11)]
    assert sift.octave_scales(2.0, 1).tolist() == [1.0, 2.0, 4.0, 8.0]
    assert sift.octave_scales(0.25, 16).shape == (19,)
    for bad in ((0.0, 8), (-1.0, 8), (float("nan"), 8), (0.5, 0), (0.5, 17), (0.5, 2.5)):
        with pytest.raises(ValueError):
            sift.octave_scales(*bad)
    assert sift.check_scales([0.5, 1, 2]).tolist() == [0.5, 1.0, 2.0]
    for bad in ([0.5, 1.0], list(range(1, 21)), [0.5, 0.5, 1.0], [1.0, 0.5, 2.0], [0.0, 1.0, 2.0], [0.5, 1.0, float("inf")],
                [0.5, float("nan"), 2.0], "abc"):
        with pytest.raises(ValueError):
            sift.check_scales(bad)


def test_restatement_of_a_two_point_response_and_the_radius():
    """The origin (z = 0) and a point 1.5 m above it, sigma = (0.25, 0.5, 1): at 0.5 the second point lies at exactly 3 sigma and counts
    (<=), so resp_1 of the origin is 1.5 w / (1 + w), w = exp(-4.5); at 0.25 it does not, resp_0 = 0.  1/64 m further it counts at
    neither, and dog[0][0] is exactly 0."""
    sg = np.array([0.25, 0.5, 1.0])
    on = sift_ref.octave(sift_ref.two_points(1.5), sg, 0.0)
    w = math.exp(-4.5)
    assert abs(on["dog"][0, 0] - 1.5 * w / (1.0 + w)) < 1e-16
    w2 = math.exp(-0.5 * 2.25 / 1.0)
    assert abs(on["dog"][0, 1] - (1.5 * w2 / (1.0 + w2) - 1.5 * w / (1.0 + w))) < 1e-16
    off = sift_ref.octave(sift_ref.two_points(1.5 + 1.0 / 64.0), sg, 0.0)
    assert off["dog"][0, 0] == 0.0 and off["dog"][1, 0] == 0.0 and off["dog"][0, 1] != 0.0
    assert on["knn"][0].tolist() == [0, 1] + [-1] * 23 and on["knn"][1].tolist() == [1, 0] + [-1] * 23 and on["key_idx"].size == 0


def test_restatement_of_the_centroids():
    """Cells of 0.5 m: (0.1, 0.1, 0.1) and (0.3, 0.4, 0.2) share the cell (0, 0, 0); the cells come out z-major, x fastest; a negative
    coordinate floors down."""
    P = np.float32([[0.6, 0.1, 0.1], [0.1, 0.1, 0.1], [0.1, 0.1, 0.6], [0.3, 0.4, 0.2], [0.1, 0.6, 0.1], [-0.1, 0.1, 0.1]])
    c = sift_ref.centroids(P, 0.5)
    d = P.astype(np.float64)
    expect = np.float32([d[5], (d[1] + d[3]) / 2.0, d[0], d[4], d[2]])
    assert c.dtype == np.float32 and c.tobytes() == expect.tobytes()
    assert sift_ref.centroids(np.zeros((0, 3), np.float32), 0.5).shape == (0, 3)


def test_restatement_on_an_exact_plane_and_on_the_tie_cluster():
    """z = 0: every response is 0 / den = 0 exactly, every dog the bits of 0.0, and at min_contrast 0 nothing is a key: v < mn[s +- 1]
    fails on equal values.  The cluster and its copy: bit-equal dog, the same neighbours relative to the cluster, the same masks."""
    r = sift_ref.octave(iss_ref.exact_plane(), sift_ref.scales(0.5, 8), 0.0)
    assert r["dog"].tobytes() == np.zeros((200, 10)).tobytes() and r["key_idx"].size == 0 and not r["key_mask"].any()
    T = iss_ref.tie_cluster()
    t = sift_ref.octave(T, sift_ref.scales(0.5, 8), 0.0)
    assert t["dog"][:40].tobytes() == t["dog"][40:].tobytes()
    assert np.array_equal(t["knn"][:40] + 40, t["knn"][40:]) and np.array_equal(t["key_mask"][:40], t["key_mask"][40:])
    L = sift_ref.octave(sift_ref.lattice(), [0.25, 0.5, 1.0], 0.0)
    assert (L["knn"] >= 0).all() and (L["knn"][:, 0] == np.arange(125)).all()


@pytest.mark.parametrize("seed,n,kw", sift_ref.SCENES, ids=sift_ref.scene_id)
def test_gpu_scenes_are_certified(seed, n, kw):
    """Conditions on the INPUTS of tests/test_sift_gpu.py, not tolerances of the kernels: in every octave that runs no |dog| is closer
    than 1e-7 to min_contrast, no contrast-passing value is closer than 1e-7 to another value that enters its rule, and the 25th and
    26th neighbour are 1e-7 apart in d2 wherever the index does not decide.  A scene that fails gets another seed, never another bar."""
    P, r = sift_ref.reference(seed, n, kw)
    p = r["params"]
    assert P.shape == (n, 3) and P.dtype == np.float32
    assert len(r["octaves"]) == p["n_octaves"] and r["stopped_at"] is None     # every octave of these scenes runs
    keys = []
    for o in r["octaves"]:
        contrast, gap, d2_gap = sift_ref.margins(o["result"])
        keys.append(len(o["result"]["key_idx"]))
        print("scene %d n %d %s octave %d: %d points, %d key points (%d keys); contrast margin %.3g, value gap %.3g, d2 gap %.3g"
              % (seed, n, kw, o["octave"], o["cloud"].shape[0], keys[-1], int(sum(bin(m).count("1") for m in o["result"]["key_mask"])),
                 contrast, gap, d2_gap))
        assert o["cloud"].shape[0] >= sift_ref.K
        assert contrast >= iss_ref.CERTIFIED and gap >= iss_ref.CERTIFIED and d2_gap >= iss_ref.CERTIFIED
    assert keys[0] >= 5 and keys[1] >= 5 and r["xyz"].shape[0] == r["scale"].shape[0] == r["octave"].shape[0] >= sum(keys)
    assert (np.diff(r["octave"]) >= 0).all()


def test_workspace_size_and_refusals_before_any_launch():
    """caelo_sift_ws_bytes is positive and non-decreasing in both arguments; caelo_sift_octave and caelo_voxel_centroids refuse bad
    arguments with CAELO_ERR_ARG before they touch the device (so this runs without one)."""
    import ctypes as C
    from caelo import _ffi
    lib = _ffi.load()
    assert C.sizeof(_ffi.SiftParams) == 16 + 8 * 19
    lds, fs = (1, 2, 255, 256, 257, 1025, 16384, 32768), (1, 2, 3, 8, 100, 70000)
    for f in fs:
        sizes = [lib.caelo_sift_ws_bytes(f, ld) for ld in lds]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and all(s >= f * ld * 101 for s, ld in zip(sizes, lds))
    for ld in lds:
        sizes = [lib.caelo_sift_ws_bytes(f, ld) for f in fs]
        assert sizes == sorted(sizes)
    assert lib.caelo_sift_ws_bytes(0, 256) > 0 and lib.caelo_sift_ws_bytes(-1, 256) == 0 and lib.caelo_sift_ws_bytes(1, 0) == 0

    def prm(sigma=(0.5, 1.0, 2.0), contrast=0.1, n=None):
        s = list(sigma) + [0.0] * (19 - len(sigma))
        return _ffi.SiftParams(len(sigma) if n is None else n, 0, contrast, (C.c_double * 19)(*s[:19]))
    good = prm()
    fake = C.c_void_p(4096)   # never dereferenced: every call below is refused, or is the n_frames == 0 no-op
    enough = lib.caelo_sift_ws_bytes(1, 256)

    def call(p=good, ld=256, n_frames=1, ctx=fake, pts=fake, n_pts=fake, dog=fake, mask=fake, key_idx=fake, n_key=fake, ws=fake, ws_bytes=enough):
        return lib.caelo_sift_octave(ctx, pts, n_frames, ld, n_pts, C.byref(p) if p is not None else None, dog, None, mask, key_idx, n_key,
                                     ws, ws_bytes, None)
    assert call(n_frames=0) == 0
    inf, nan = float("inf"), float("nan")
    for kw in (dict(ctx=None), dict(pts=None), dict(n_pts=None), dict(dog=None), dict(mask=None), dict(key_idx=None), dict(n_key=None),
               dict(ws=None), dict(p=None), dict(ld=0), dict(ld=-5), dict(ld=32769), dict(n_frames=-1), dict(ws_bytes=enough - 1),
               dict(ws_bytes=0), dict(p=prm((0.5, 1.0))), dict(p=prm((0.5, 1.0, 2.0), n=20)), dict(p=prm((0.5, 1.0, 2.0), n=-1)),
               dict(p=prm((1.0, 0.5, 2.0))), dict(p=prm((0.5, 0.5, 2.0))), dict(p=prm((0.0, 0.5, 2.0))), dict(p=prm((-1.0, 0.5, 2.0))),
               dict(p=prm((0.5, 1.0, inf))), dict(p=prm((0.5, nan, 2.0))), dict(p=prm(contrast=-1e-9)), dict(p=prm(contrast=inf)),
               dict(p=prm(contrast=nan))):
        assert call(**kw) == -1 and lib.caelo_last_error(), kw
    assert call(p=prm(tuple(0.5 * 1.1 ** k for k in range(19))), n_frames=0) == 0

    def cen(ctx=fake, pts=fake, n=10, order=fake, starts=fake, cells=3, out=fake):
        return lib.caelo_voxel_centroids(ctx, pts, n, order, starts, cells, out, None)
    assert cen(cells=0) == 0 and cen(n=0, cells=0) == 0
    for kw in (dict(ctx=None), dict(pts=None), dict(order=None), dict(starts=None), dict(out=None), dict(n=-1), dict(cells=-1),
               dict(cells=11), dict(n=2 ** 31, cells=1)):
        assert cen(**kw) == -1 and lib.caelo_last_error(), kw


def test_detect_sift_keypoints_arguments(tmp_path, monkeypatch):
    """Parse-time handling through detect_sift_keypoints.main(argv): sift is a method there, the default one, with its four options;
    each detector's options are refused under the others with a message that names them, bad values are refused -- all before any
    engine exists.  detect_keypoints.py's own command line is the one it had: sift and its options are unknown there."""
    import detect_keypoints
    import detect_sift_keypoints
    import caelo.engine

    def trap(*a, **k):
        raise AssertionError("an engine was created before the arguments were refused")
    monkeypatch.setattr(caelo.engine, "Engine", trap)
    scans, out = tmp_path / "velodyne", tmp_path / "out"
    scans.mkdir()
    base = ["--scans", str(scans), "--out", str(out)]

    def refused(argv, *words, main=detect_sift_keypoints.main):
        import contextlib
        import io
        err = io.StringIO()
        with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(err):
            main(argv)
        assert e.value.code == 2
        for w in words:
            assert w in err.getvalue(), (w, err.getvalue())

    # accepted as far as the parse goes: the refusal is the empty directory, not the method or its options
    refused(base, "no .bin files")
    refused(["--method", "sift"] + base, "no .bin files")
    refused(["--min-scale", "0.25", "--n-octaves", "5", "--n-scales-per-octave", "4", "--min-contrast", "0.05"] + base, "no .bin files")
    refused(["--method", "harris", "--radius", "1.5"] + base, "no .bin files")
    refused(["--method", "iss", "--min-neighbors", "4"] + base, "no .bin files")
    refused(["--method", "usip"] + base, "invalid choice")
    refused(["--radius", "1.0"] + base, "--radius", "--method harris", "--method sift")
    refused(["--salient-radius", "2.0", "--min-neighbors", "5"] + base, "--salient-radius", "--min-neighbors", "--method iss")
    refused(["--method", "iss", "--min-scale", "0.5"] + base, "--min-scale", "--method sift")
    refused(["--method", "harris", "--n-octaves", "4", "--min-contrast", "0.1"] + base, "--n-octaves", "--min-contrast", "--method sift")
    refused(["--method", "harris", "--n-scales-per-octave", "8"] + base, "--n-scales-per-octave")
    refused(["--min-scale", "0"] + base, "min_scale must be finite and positive")
    refused(["--n-octaves", "9"] + base, "n_octaves")
    refused(["--n-scales-per-octave", "17"] + base, "n_scales_per_octave")
    refused(["--min-contrast", "-0.1"] + base, "min_contrast must be finite and not negative")
    refused(["--min-contrast", "nan"] + base, "min_contrast")
    refused(["--max-points", "40000"] + base, "--max-points")
    # the other script: as it was
    refused(["--method", "sift"] + base, "invalid choice", main=detect_keypoints.main)
    refused(["--method", "iss", "--min-scale", "0.5"] + base, "unrecognized arguments", main=detect_keypoints.main)
    refused(base, "--method", main=detect_keypoints.main)
    assert not out.exists()
    import io
    import contextlib
    said = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stdout(said):
        detect_sift_keypoints.main(["--help"])
    assert "{iss,harris,sift}" in said.getvalue() and "--min-contrast" in said.getvalue()
    said = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stdout(said):
        detect_keypoints.main(["--help"])
    assert "{iss,harris}" in said.getvalue() and "detect_sift_keypoints.py" in said.getvalue() and "not built" not in said.getvalue()
