"""The ring projection's pixel choice at its column and row edges, without a GPU.

tests/golden/ring_edges.npz (tools/make_goldens_ring_edges.py) holds points whose column, or row, hangs on the last bits of atan2, or
asin: the eight directions whose colf is an exact integer over the whole float32 range, a few hundred off-axis points within 8 ulp of
a column edge, and the sixteen float32 quotients nearest a row edge.  Here: the oracle on this machine gives the recorded pixels, ring
and counter (the canary for a C library other than the one the fixture was made with); tests/ring_ref.py, the per-point restatement,
gives the same; and the fixture is as sharp as it claims -- an atan2 that is one ulp off, either way, moves every off-axis probe
of the counted class.  tests/test_ring_edges_gpu.py puts the same points through k_project_points."""
import hashlib
import math
import os

import numpy as np
import pytest

import ring_ref as rr
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "ring_edges.npz")))


def test_oracle_reproduces_the_recorded_pixels_ring_and_counter(orc, fx):
    pts = fx["points"]
    ring, cnt = orc.ProjectPC2SphericalRing(pts)
    occ = np.flatnonzero(cnt.ravel())
    assert np.array_equal(occ, fx["ring_pixels"]) and np.array_equal(cnt.ravel()[occ], fx["ring_counts"])
    assert np.array_equal(ring.view(np.uint32), rr.expected_ring(pts, fx["ring_pixels"], fx["ring_winners"]).view(np.uint32))
    assert hashlib.sha256(ring.tobytes()).hexdigest() == str(fx["ring_sha256"])
    assert hashlib.sha256(cnt.tobytes()).hexdigest() == str(fx["counter_sha256"])
    # every point alone, behind three points of zero range: its own pixel, or none
    pc = np.zeros((4, 4), np.float32)
    for i, p in enumerate(pts):
        pc[3] = p
        hit = np.argwhere(orc.ProjectPC2SphericalRing(pc)[1])
        got = tuple(hit[0]) if len(hit) else (-1, -1)
        assert len(hit) <= 1 and got == tuple(fx["pixel"][i]), (i, p, got, fx["pixel"][i])
    for i, p in enumerate(fx["oob_points"]):        # column 1800: the reference's IndexError (SphericalRing.py:91)
        pc[3] = p
        with pytest.raises(IndexError):
            orc.ProjectPC2SphericalRing(pc)
        assert fx["oob_pixel"][i, 1] == rr.RING_W and 0 <= fx["oob_pixel"][i, 0] < rr.RING_H


def test_restatement_gives_the_same_pixels_per_point(orc, fx):
    pts = fx["points"]
    assert np.array_equal(rr.pixels(pts), fx["pixel"])
    ring, cnt = rr.project(pts)
    o_ring, o_cnt = orc.ProjectPC2SphericalRing(pts)
    assert np.array_equal(ring.view(np.uint32), o_ring.view(np.uint32)) and np.array_equal(cnt, o_cnt)
    assert np.array_equal(rr.pixels(fx["oob_points"]), fx["oob_pixel"])
    with pytest.raises(IndexError):
        rr.project(np.concatenate([pts[:3], fx["oob_points"][:1]]))
    # the host's atan2 is the correctly rounded one at every point, which the kernel's exact decision near an edge reproduces
    live = np.flatnonzero(rr.ranges(pts) != 0)
    assert fx["atan2_correctly_rounded"].all() and len(live) >= 1000
    for i in live:
        x, y = float(pts[i, 0]), float(pts[i, 1])
        assert float(np.arctan2(np.longdouble(y), np.longdouble(x))) == math.atan2(y, x), (i, x, y)
    # the recorded distances and moves are the restatement's
    _, cf, rf = rr.terms(pts)
    r = rr.ranges(pts)
    for i in np.flatnonzero(fx["edge"] >= 0):
        edge, ulp = rr.ulp_from_integer(cf[i])
        assert edge == fx["edge"][i] and ulp == fx["ulp"][i] and rr.flips_of_column(pts[i, 0], pts[i, 1]) == fx["flips"][i], i
    for i in np.flatnonzero(fx["kind"] == rr.ROW_PROBE):
        assert rr.ulp_from_integer(rf[i])[1] == fx["ulp"][i] and rr.flips_of_row(pts[i, 2] / r[i]) == fx["flips"][i] == 0, i


def test_counts_per_class(fx):
    kind, edge, ulp, pts, pixel = fx["kind"], fx["edge"], fx["ulp"], fx["points"], fx["pixel"]
    off, wide = kind == rr.OFF_AXIS, kind == rr.OFF_AXIS_EXTRA      # (the counts are asked of the first class alone: ring_ref.py)
    print("%d points: %d axis, %d diagonal, %d x = y = 0, %d off axis (%d exact, %d below, %d above) + %d that need two ulp, %d row probes, "
          "%d + %d in the group, %d of column 1800; %d trials, seed %d, %s" % (
              len(pts), (kind == rr.AXIS).sum(), (kind == rr.DIAGONAL).sum(), (kind == rr.ZERO_XY).sum(), off.sum(), (off & (ulp == 0)).sum(),
              (off & (ulp < 0)).sum(), (off & (ulp > 0)).sum(), wide.sum(), (kind == rr.ROW_PROBE).sum(), (kind == rr.GROUP_EDGE).sum(),
              (kind == rr.GROUP_ORDINARY).sum(), len(fx["oob_points"]), fx["trials"], fx["seed"], fx["libc"]))
    assert off.sum() >= 256 and (np.abs(ulp[off | wide]) <= 8).all() and fx["band_ulp"] == 8
    assert (off & (ulp == 0)).sum() >= 32 and (off & (ulp < 0)).sum() >= 32 and (off & (ulp > 0)).sum() >= 32
    assert len(set(zip(pts[off, 0] > 0, pts[off, 1] > 0))) == 4
    far = (off | wide) & (edge % 32 == 0) & (rr.ranges(pts) >= 10) & (pixel[:, 0] >= 0) & (pixel[:, 0] < 64)
    assert len(set(edge[far])) >= 16
    assert (kind == rr.ROW_PROBE).sum() == 16
    # the eight directions, each from the magnitudes that are dropped to inf
    axis = np.isin(kind, (rr.AXIS, rr.DIAGONAL))
    assert set(edge[axis & (edge >= 0)]) == {0, 225, 450, 675, 900, 1125, 1350, 1575}
    r = rr.ranges(pts)
    assert (axis & (r == 0)).sum() >= 8 * 4 and (axis & np.isinf(r)).sum() >= 8 * 2 and np.isinf(pts[axis, :2]).any(axis=1).sum() >= 3
    for e in (0, 225, 450, 675, 900, 1125, 1350, 1575):
        mags = np.abs(pts[axis & (edge == e), :2]).max(axis=1)
        assert mags.min() < 1e-21 and {1e-3, 1.0, 10.0, 80.0, 1e4} <= set(np.float64(mags).round(6)) and mags.max() >= 3e38, (e, mags)
    zeros = pts[axis & (pts[:, :2] == 0).any(axis=1)]
    assert np.signbit(zeros[:, :2][zeros[:, :2] == 0]).any() and not np.signbit(zeros[:, :2][zeros[:, :2] == 0]).all()
    zxy = pts[kind == rr.ZERO_XY]
    assert len(set(zip(np.signbit(zxy[:, 0]), np.signbit(zxy[:, 1])))) == 4 and (zxy[:, :2] == 0).all() and (pixel[kind == rr.ZERO_XY] == -1).all()
    # column 1800 is atan2(-0, x < 0)
    oob = fx["oob_points"]
    assert len(oob) >= 8 and (oob[:, 0] < 0).all() and (oob[:, 1] == 0).all() and np.signbit(oob[:, 1]).all()
    # intensities name the points; every column probe of an ordinary magnitude sits mid-row, on a pixel of its own
    assert np.array_equal(pts[:, 3], np.arange(1, len(pts) + 1, dtype=np.float32))
    _, _, rf = rr.terms(pts)
    mid = (off | wide | (axis & (r > 1e-4) & (r < 1e5))) & (pixel[:, 0] >= 0)
    assert ((rf[mid] % 1.0 >= 0.25) & (rf[mid] % 1.0 <= 0.75)).all()
    flat = pixel[mid, 0].astype(np.int64) * rr.RING_W + pixel[mid, 1]
    assert len(set(flat)) == len(flat) == mid.sum()
    # the same-pixel group: three pixels, the edge point first, in the middle, last among two ordinary points
    where = []
    for g in range(3):
        m = np.flatnonzero(fx["group"] == g)
        assert len(m) == 3 and (np.diff(m) == 1).all() and len(set(map(tuple, pixel[m]))) == 1 and (pixel[m, 0] >= 0).all()
        assert (kind[m] == rr.GROUP_EDGE).sum() == 1 and fx["flips"][m][kind[m] == rr.GROUP_EDGE][0] != 0
        assert fx["ring_counts"][fx["ring_pixels"] == pixel[m[0], 0].astype(np.int64) * rr.RING_W + pixel[m[0], 1]] == 3
        where.append(int(np.flatnonzero(kind[m] == rr.GROUP_EDGE)[0]))
    assert where == [0, 1, 2]


def test_fixture_is_sharp(fx):
    """Every off-axis probe flips under a move of atan2 by one ulp (the second class: by two), every x < 0 diagonal under + 1
    ulp; no row probe flips under +- 16 ulp of asin and the nearest any float32 quotient comes to a row edge is more than 1e4 ulp."""
    kind, pts, flips = fx["kind"], fx["points"], fx["flips"]
    for i in np.flatnonzero(kind == rr.OFF_AXIS):
        assert flips[i] & rr.ONE_ULP and rr.flips_of_column(pts[i, 0], pts[i, 1]) == flips[i], i
    for i in np.flatnonzero(kind == rr.OFF_AXIS_EXTRA):
        assert flips[i] and not flips[i] & rr.ONE_ULP and rr.flips_of_column(pts[i, 0], pts[i, 1]) == flips[i], i
    r = rr.ranges(pts)
    diag = np.flatnonzero((kind == rr.DIAGONAL) & (pts[:, 0] < 0) & (r > 0))
    assert len(diag) >= 2 * 8 and set(fx["edge"][diag]) == {225, 1575}
    for i in diag:
        assert flips[i] & 4, (i, pts[i])          # bit 2: + 1 ulp
    reach = tuple(range(-16, 0)) + tuple(range(1, 17))
    for i in np.flatnonzero(kind == rr.ROW_PROBE):
        assert rr.flips_of_row(pts[i, 2] / r[i], reach) == 0, i
    assert fx["row_margin_ulp"] >= 1e4 and fx["row_floats_walked"] >= 10 ** 8
    probes = np.flatnonzero(kind == rr.ROW_PROBE)
    _, _, rf = rr.terms(pts[probes])
    assert np.abs(rf - np.rint(rf)).min() == fx["row_margin_rows"] and (np.abs(rf - np.rint(rf)) < 1e-7).all()


def test_one_ulp_of_atan2_moves_more_than_half_of_the_off_axis_probes(fx):
    """What these tests are for: the restatement with an atan2 that is one ulp off no longer gives the recorded pixels.  A probe is
    the last double of its column, which an ulp up moves, or the first of the column before, which an ulp down moves, and a search finds
    about as many of one as of the other.  So no function that is off in ONE direction moves more than about half of the class: every
    probe moves under exactly one of the two, each direction moves at least a third, and an atan2 that is off by one ulp either way --
    the two taken together -- moves all of them, which is more than half.  Those that need two ulp move under exactly one of +- 2."""
    off, wide = fx["kind"] == rr.OFF_AXIS, fx["kind"] == rr.OFF_AXIS_EXTRA
    pts, want = fx["points"], fx["pixel"]
    moved = {k: (rr.pixels(pts, atan2=rr.moved(math.atan2, k)) != want).any(axis=1) for k in (1, -1, 2, -2)}
    print("moved by an atan2 that is off by k ulp: %r of %d off-axis probes, %r of the %d that need two" % (
        {k: int(m[off].sum()) for k, m in moved.items()}, off.sum(), {k: int(m[wide].sum()) for k, m in moved.items()}, wide.sum()))
    assert (moved[1] ^ moved[-1])[off].all() and (moved[2] ^ moved[-2])[off | wide].all() and not (moved[1] | moved[-1])[wide].any()
    assert 3 * moved[1][off].sum() >= off.sum() and 3 * moved[-1][off].sum() >= off.sum()
    assert (moved[1] | moved[-1])[off].sum() > off.sum() / 2
    diag = (fx["kind"] == rr.DIAGONAL) & (pts[:, 0] < 0) & (want[:, 0] >= 0)
    assert moved[1][diag].all() and diag.sum() >= 16
