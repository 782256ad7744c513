"""CPU: the host side of the ISS key point detector -- the NumPy restatement of the definition (tests/iss_ref.py) on a case worked by
hand, the input conditions of every scene the GPU tests use, caelo.iss's plumbing against direct NumPy calls, the parameter checks
and the workspace size."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import iss_ref  # noqa: E402
from caelo import iss  # noqa: E402


def test_restatement_on_a_hand_checkable_case():
    """Seven points: the origin and (+-a, 0, 0), (0, +-b, 0), (0, 0, +-c) with a, b, c = 0.75, 0.5, 0.25.  Every point is within 2 m of
    every other.  For the origin C = diag(2 a^2, 2 b^2, 2 c^2) exactly, so e = (1.125, 0.5, 0.125), e2 / e1 = 0.444..., e3 / e2 =
    0.25 and the saliency is e3; with gamma_32 = 0.25 the strict test e3 / e2 < gamma_32 fails."""
    a, b, c = 0.75, 0.5, 0.25
    P = np.array([[0, 0, 0], [a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c], [0, 0, -c]], dtype=np.float32)
    r = iss_ref.iss(P)
    assert r["n_neigh"].tolist() == [7] * 7 and r["n_neigh_nms"].tolist() == [7] * 7
    assert r["C"][0].tolist() == [1.125, 0.0, 0.0, 0.5, 0.0, 0.125]
    assert r["eig"][0].tolist() == [1.125, 0.5, 0.125] and r["saliency"][0] == 0.125 and r["candidate"][0]
    # the point (a, 0, 0) sees d = (0, -a, -2a, (-a, +-b, 0) x 2, (-a, 0, +-c) x 2): C = (a^2 (1 + 4 + 4), 0, 0, 2 b^2, 0, 2 c^2)
    assert r["C"][1].tolist() == [9 * a * a, 0.0, 0.0, 0.5, 0.0, 0.125]
    assert not iss_ref.iss(P, gamma_32=0.25)["candidate"][0] and iss_ref.iss(P, gamma_32=0.2500001)["candidate"][0]
    assert iss_ref.iss(P, min_neighbors=8)["saliency"].tolist() == [-1.0] * 7
    assert iss_ref.iss(P, salient_radius=0.5)["n_neigh"].tolist() == [3, 1, 1, 1, 1, 2, 2]   # 0.5 m away is outside 0.5 m
    # seen from (0, +-b, 0) C = diag(2 a^2, 9 b^2, 2 c^2), from (0, 0, +-c) C = diag(2 a^2, 2 b^2, 9 c^2) = (1.125, 0.5, 0.5625)
    assert r["saliency"].tolist() == [0.125] * 5 + [0.5, 0.5]
    assert r["key_idx"].tolist() == [5, 6]   # equal saliencies both survive, everything else has a larger neighbour
    assert iss_ref.iss(P, non_max_radius=0.3)["key_idx"].size == 0   # at 0.3 m nobody has 5 neighbours
    assert iss_ref.iss(P, non_max_radius=0.3, min_neighbors=1)["key_idx"].tolist() == [1, 2, 3, 4, 5, 6]   # alone, or the larger of two


def test_hand_case_neighbour_counts_are_strict():
    """(1, 0, 0) and (-1, 0, 0) are exactly 2.0 m apart: each misses the other at radius 2 and sees the other five plus itself."""
    P = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.25], [0, 0, -0.25]], dtype=np.float32)
    assert iss_ref.iss(P)["n_neigh"].tolist() == [7, 6, 6, 7, 7, 7, 7]


@pytest.mark.parametrize("seed,n,kw", iss_ref.SCENES, ids=lambda v: "cut" if v == iss_ref.CUT else ("dflt" if v == {} else str(v)))
def test_gpu_scenes_are_certified(seed, n, kw):
    """A condition on the INPUTS of tests/test_iss_gpu.py, not a tolerance of the kernel: no threshold decision of the scene is closer
    than 1e-7 ||C|| to flipping and no two competing saliencies are closer than 1e-7 of the largest -- about six orders above what two
    float64 3 x 3 eigenvalue solvers differ by.  A scene that fails gets another seed, never another bar."""
    P, r = iss_ref.reference(seed, n, kw)
    margin, gap = iss_ref.margins(r)
    print("scene %d n %d %s: margin %.3g gap %.3g, %d key points, %d candidates of %d eligible"
          % (seed, n, kw, margin, gap, len(r["key_idx"]), int(r["candidate"].sum()), int((r["n_neigh"] >= r["params"]["min_neighbors"]).sum())))
    assert P.shape == (n, 3) and P.dtype == np.float32 and np.array_equal(P * 1024, np.round(P * 1024))
    assert margin >= iss_ref.CERTIFIED and gap >= iss_ref.CERTIFIED
    assert len(r["key_idx"]) >= 5
    if kw:   # the thresholds really cut: a good part of the eligible points fails them, a good part passes
        elig = int((r["n_neigh"] >= r["params"]["min_neighbors"]).sum())
        assert 0.25 * elig < int(r["candidate"].sum()) < 0.9 * elig


def test_boundary_inputs_say_what_the_gpu_tests_assume():
    assert iss_ref.iss(iss_ref.strict_radius(False))["n_neigh"][0] == 4 and iss_ref.iss(iss_ref.strict_radius(False))["saliency"][0] == -1.0
    assert iss_ref.iss(iss_ref.strict_radius(True))["n_neigh"][0] == 5
    T = iss_ref.tie_cluster()
    assert np.array_equal(T[40:] - T[:40], np.tile(np.float32([32, 0, 0]), (40, 1))) and np.array_equal(T * 64, np.round(T * 64))
    r = iss_ref.iss(T)
    assert np.array_equal(r["saliency"][:40], r["saliency"][40:])   # exact sums: bit-equal pairs
    assert r["key_idx"].tolist() == [12, 52]
    plane = iss_ref.iss(iss_ref.exact_plane())
    assert plane["saliency"].max() <= 0 and plane["key_idx"].size == 0 and (plane["n_neigh"] >= 5).all()


def test_subsample_and_ensure_keypoint_number_against_numpy():
    pc = np.random.RandomState(3).rand(500, 3).astype(np.float32)
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    assert np.array_equal(iss.subsample(500, 100, a), np.sort(b.choice(500, 100, replace=False)))
    assert np.array_equal(iss.subsample(500, 500, a), np.arange(500)) and np.array_equal(iss.subsample(0, 10, a), np.arange(0))
    assert a.randint(1 << 30) == b.randint(1 << 30)   # no draw when nothing is dropped
    kp = pc[:40]
    assert iss.ensure_keypoint_number(kp, pc, 40, a) is kp
    few = iss.ensure_keypoint_number(kp, pc, 64, a)
    assert np.array_equal(few, np.concatenate((kp, pc[b.choice(500, 24, replace=False)])))
    many = iss.ensure_keypoint_number(kp, pc, 16, a)
    assert np.array_equal(many, kp[b.choice(40, 16, replace=False)])
    none = iss.ensure_keypoint_number(np.zeros((0, 3), np.float32), pc, 8, a)
    assert np.array_equal(none, pc[b.choice(500, 8, replace=False)])
    with pytest.raises(ValueError):
        iss.ensure_keypoint_number(kp, pc[:10], 64, a)


def test_voxel_downsample_keeps_the_first_point_of_every_cell_in_scan_order():
    import torch
    rs = np.random.RandomState(9)
    pc = np.c_[rs.uniform(-3, 3, (4000, 3)), rs.rand(4000)].astype(np.float32)
    out = iss.voxel_downsample(torch.from_numpy(pc), 0.5).numpy()
    seen, keep = set(), []
    for i, p in enumerate(pc):
        c = tuple(np.floor(p[:3].astype(np.float64) / 0.5).astype(np.int64))
        if c not in seen:
            seen.add(c)
            keep.append(i)
    assert 100 < len(keep) < 4000 and np.array_equal(out, pc[keep])
    assert iss.voxel_downsample(torch.zeros((0, 3)), 0.2).shape == (0, 3)
    with pytest.raises(ValueError):
        iss.voxel_downsample(torch.from_numpy(pc), 0.0)
    bad = pc.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        iss.voxel_downsample(torch.from_numpy(bad), 0.2)


def test_check_params_refusals():
    assert iss.check_params() == iss.DEFAULTS == iss_ref.DEFAULTS
    assert iss.check_params(salient_radius=1, min_neighbors=np.int64(3)) == dict(iss.DEFAULTS, salient_radius=1.0, min_neighbors=3)
    for bad in (dict(salient_radius=0), dict(salient_radius=-1.0), dict(non_max_radius=float("inf")), dict(non_max_radius=float("nan")),
                dict(gamma_21=0.0), dict(gamma_32=float("nan")), dict(gamma_32="x"), dict(min_neighbors=0), dict(min_neighbors=2.5),
                dict(min_neighbors=True), dict(radius=1.0)):
        with pytest.raises(ValueError):
            iss.check_params(**bad)


def test_workspace_size_and_refusals_before_any_launch():
    """caelo_iss_ws_bytes is positive and non-decreasing in both arguments; caelo_iss_keypoints refuses bad arguments with
    CAELO_ERR_ARG before it touches the device (so this runs without one)."""
    import ctypes as C
    from caelo import _ffi
    lib = _ffi.load()
    assert _ffi.ISS_MAX_POINTS == iss.MAX_POINTS == 32768 and C.sizeof(_ffi.IssParams) == 40
    lds, fs = (1, 2, 255, 256, 257, 1025, 16384, 32768), (1, 2, 3, 8, 100, 70000)
    for f in fs:
        sizes = [lib.caelo_iss_ws_bytes(f, ld) for ld in lds]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and all(s >= f * ld for s, ld in zip(sizes, lds))
    for ld in lds:
        sizes = [lib.caelo_iss_ws_bytes(f, ld) for f in fs]
        assert sizes == sorted(sizes)
    good = _ffi.IssParams(2.0, 2.0, 0.975, 0.975, 5, 0)
    fake = C.c_void_p(4096)   # never dereferenced: every call below is refused, or is the n_frames == 0 no-op

    def call(prm=good, ld=256, n_frames=1, ctx=fake, pts=fake, ws=fake, ws_bytes=1 << 20):
        return lib.caelo_iss_keypoints(ctx, pts, n_frames, ld, fake, C.byref(prm) if prm is not None else None, fake, None, None, fake, fake,
                                       ws, ws_bytes, None)
    assert call(n_frames=0) == 0
    for kw in (dict(ctx=None), dict(pts=None), dict(ws=None), dict(prm=None), dict(ld=0), dict(ld=32769), dict(n_frames=-1), dict(ws_bytes=255),
               dict(prm=_ffi.IssParams(0.0, 2.0, 0.975, 0.975, 5, 0)), dict(prm=_ffi.IssParams(2.0, float("inf"), 0.975, 0.975, 5, 0)),
               dict(prm=_ffi.IssParams(2.0, 2.0, float("nan"), 0.975, 5, 0)), dict(prm=_ffi.IssParams(2.0, 2.0, 0.975, -0.5, 5, 0)),
               dict(prm=_ffi.IssParams(2.0, 2.0, 0.975, 0.975, 0, 0))):
        assert call(**kw) != 0 and lib.caelo_last_error(), kw
