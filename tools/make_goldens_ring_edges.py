#!/usr/bin/env python3
"""Writes tests/golden/ring_edges.npz: points that sit on, or within a few float64 ulp of, the edges of the spherical ring's pixels.

k_project_points (csrc/ring.hip) turns the device's f64 atan2 and asin into a column and a row; the oracle and the reference use the
host's C library.  A random scan never comes near enough to an edge to tell two libraries apart, so the points are made here:

  axis / diagonal   the eight directions whose colf = (pi - atan2(y, x)) / az_res is exactly 0, 225, ..., 1575 (and 1800: the
                    ``oob_points``), at magnitudes from the smallest denormal to inf, both signs of every zero; x = y = +-0.
  off axis          float32 (x, y) found by a directed search: an edge column c, a range of 3..80 m, x = f32(r cos A_c), y the float32
                    nearest x tan A_c, where A_c is the double at which the column steps from c to c - 1.  Kept: colf within 8 ulp of
                    c AND the column changes when atan2 is moved by one or two ulp either way (``flips``).  The class that is counted
                    holds the one-ulp probes, those that need two are a class of their own (tests/ring_ref.py: OFF_AXIS_EXTRA).
  row probes        the float32 quotients q = z / r nearest a row edge among ALL floats whose rowf lies in [-1, 70] (the walk's
                    minimum distance is recorded: no asin that deserves the name comes near it), each as a point whose float32
                    z / sqrtf(x x + y y + z z) is exactly that q (y != 0: each probe has a column of its own).
  same-pixel group  three pixels that an edge point shares with two ordinary ones, the edge point first, in the middle and last.

Every probe gets a z (column probes) or an azimuth (row probes) that puts it in the middle of the other coordinate and, where the
magnitudes allow it, on a pixel of its own; the intensity is the point's index + 1, so a ring pixel names the point that won it.
Recorded per point: the oracle's pixel, the signed ulp distance from the edge, the moves that flip it, and whether the host's atan2
is the correctly rounded one there (against the 80-bit ``np.longdouble`` arctan2).  Deterministic: a fixed seed, one generator per
chunk of the search, archive members without time stamps.  Needs NumPy and the oracle; about a minute on eight cores.

    python tools/make_goldens_ring_edges.py [--trials N] [--workers W] [--out PATH]
"""
import argparse
import hashlib
import io
import math
import multiprocessing
import os
import platform
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import ring_ref as rr  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "ring_edges.npz")
SEED = 20261020
TRIALS = 16 * 10 ** 9
CHUNK = 1 << 17
BAND_ULP = 8.0
F32 = rr.F32
INF = math.inf
NET_H, NET_W = 64, 1792


# ---- the directed search for off-axis points --------------------------------------------------------------------------------------
def edge_angle(c):
    """The largest double a with int((pi - a) / az_res) >= c: the next double up lies in column c - 1."""
    a = rr.PI - c * rr.AZ_RES
    while int((rr.PI - a) / rr.AZ_RES) < c:
        a = math.nextafter(a, -INF)
    while int((rr.PI - math.nextafter(a, INF)) / rr.AZ_RES) >= c:
        a = math.nextafter(a, INF)
    return a


def live_edges():
    """Edges where an ulp of atan2 can matter: not the eight exact directions, and not |atan2| < 1, where pi - a absorbs the ulp of a
    small a (columns 614..1186).  A third of the schedule goes to the edges of the eligibility map's 32-column blocks."""
    live = [c for c in range(1, rr.RING_W) if c % 225 and not 614 <= c <= 1186]
    blocks = [c for c in live if c % 32 == 0]
    sched = []
    for i, c in enumerate(live):
        sched.append(c)
        if i % 2:
            sched.append(blocks[(i // 2) % len(blocks)])
    return sched


def search_chunk(job):
    j, c = job
    th = edge_angle(c)
    ct, t = math.cos(th), math.tan(th)
    u = np.random.default_rng([SEED, j]).random(CHUNK)
    u *= 77.0 * ct
    u += 3.0 * ct
    x = u.astype(F32)
    xd = x.astype(np.float64)
    yt = xd * t
    y = yt.astype(F32)
    e = y.astype(np.float64)
    e -= yt            # the angle's distance from A_c, to first order: (y - x tan A) cos^2 A / x
    e *= ct * ct
    e /= xd
    near = np.flatnonzero(np.abs(e) <= 3.0 * (math.nextafter(th, INF) - th))
    return [(float(x[i]), float(y[i])) for i in near]


def search(trials, workers):
    sched = live_edges()
    jobs = [(j, sched[(j * 7919) % len(sched)]) for j in range(trials // CHUNK)]
    with multiprocessing.Pool(workers) as pool:
        found = [h for hits in pool.imap(search_chunk, jobs, chunksize=64) for h in hits]
    out, seen = [], set()
    for x, y in found:
        edge, ulp = rr.ulp_from_integer(rr.colf(x, y))
        if (x, y) in seen or abs(ulp) > BAND_ULP or not rr.flips_of_column(x, y):
            continue
        seen.add((x, y))
        out.append((x, y, edge))
    return out


# ---- the exhaustive walk of the row quotients -----------------------------------------------------------------------------------------
Q_TINY = 2.0 ** -14     # below it rowf stays within 0.009 of v_off = 58.296: no integer


def f32_bits(v):
    return int(np.array(v, F32).view(np.uint32))


def walk_chunk(span):
    lo, hi = span
    q = np.arange(lo, hi, dtype=np.uint32).view(F32).astype(np.float64)
    rowf = np.arcsin(q) / rr.V_RES + rr.V_OFF       # (vectorised asin: it only ranks; the kept values are recomputed with math.asin)
    d = np.abs(rowf - np.rint(rowf))
    d[(rowf < -1.0) | (rowf > 70.0)] = 1.0
    best = np.argsort(d, kind="stable")[:32]
    return [(float(d[i]), float(q[i])) for i in best], int(((rowf >= -1.0) & (rowf <= 70.0)).sum())


def walk_rows(workers):
    """-> (the 16 float32 q nearest a row edge, the walk's minimum distance in rows and in ulp of rowf, floats walked)."""
    q_lo = math.sin((-1.0 - rr.V_OFF) * rr.V_RES) * 1.001
    q_hi = math.sin((70.0 - rr.V_OFF) * rr.V_RES) * 1.001
    assert abs(Q_TINY / rr.V_RES) * 1.01 < min(rr.V_OFF - 58, 59 - rr.V_OFF)
    spans, step = [], 1 << 22
    for a, b in ((f32_bits(Q_TINY), f32_bits(q_hi)), (f32_bits(-Q_TINY), f32_bits(q_lo))):
        spans += [(s, min(s + step, b + 1)) for s in range(a, b + 1, step)]
    with multiprocessing.Pool(workers) as pool:
        res = pool.map(walk_chunk, spans)
    walked = sum(n for _, n in res)
    cand = sorted(set(q for hits, _ in res for _, q in hits))
    exact = sorted((abs(rr.rowf(q) - round(rr.rowf(q))), abs(rr.ulp_from_integer(rr.rowf(q))[1]), q) for q in cand if -1.0 <= rr.rowf(q) <= 70.0)
    return [q for _, _, q in exact[:16]], exact[0][0], exact[0][1], walked


# ---- placing points ---------------------------------------------------------------------------------------------------------------------
class Frame:
    def __init__(self):
        self.pts, self.kind, self.edge, self.group = [], [], [], []
        self.used, self.used_blocks = set(), set()

    def add(self, p, kind, edge=-1, group=-1):
        p = np.array(list(p[:3]) + [len(self.pts) + 1], F32)      # intensity = index + 1
        pix = tuple(int(v) for v in rr.pixels(p)[0])
        if pix[0] >= 0 and kind != rr.GROUP_ORDINARY and group < 0:
            self.used.add(pix)
        self.pts.append(p); self.kind.append(kind); self.edge.append(edge); self.group.append(group)
        return pix


def z_mid_row(x, y, row):
    """The float32 z that puts (x, y, z) in the middle of ring row ``row``."""
    beta = ((rr.RING_H - row) + 0.5 - rr.V_OFF) * rr.V_RES
    return F32(math.hypot(float(x), float(y)) * math.tan(beta))


def place_column_probe(fr, x, y, kind, edge, start, block_edge=False, rows=range(2, 63)):
    """(x, y) with a z in the middle of a row, on a pixel no probe has yet; a probe on the edge of a 32-column block also on a row where
    the two blocks it may fall into hold no other such probe."""
    rows = list(rows)
    for k in range(len(rows)):
        row = rows[(start + k) % len(rows)]
        p = np.array([x, y, z_mid_row(x, y, row), 0.0], F32)
        pix = tuple(int(v) for v in rr.pixels(p)[0])
        frac = rr.terms(p)[2][0] % 1.0
        if pix[0] != row or not 0.25 <= frac <= 0.75 or any((row, pix[1] + d) in fr.used for d in (-1, 0, 1)):
            continue            # (the pixels either side stay free too: a probe that moves is then alone where it lands)
        if block_edge:
            blocks = {(row, edge // 32), (row, edge // 32 - 1)}
            if blocks & fr.used_blocks:
                continue
            fr.used_blocks |= blocks
        return fr.add(p, kind, edge)
    raise RuntimeError("no free pixel for (%r, %r)" % (x, y))


DIRECTIONS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))     # colf 900, 675, 450, 225, 0 | 1800, 1575, 1350, 1125
DROPPED = (2.0 ** -149, 1e-40, 2.0 ** -126, 2.0 ** -75)      # x * x underflows to zero: r == 0
SMALLEST = (1.5 * 2.0 ** -75, 2.0 ** -74)                    # the smallest whose s is above zero (2^-149 and 2^-148 on an axis)
ORDINARY = (1e-3, 1.0, 10.0, 80.0, 1e4)
OVERFLOW = (2.0 ** 64, 3e38)                                  # x * x = inf: r = inf, q = 0, row 11


def signed_zeros(d, m):
    """The coordinate d * m; a zero coordinate in both signs."""
    return (0.0, -0.0) if d == 0 else (d * m,)


def axis_points(fr, oob):
    for di, (dx, dy) in enumerate(DIRECTIONS):
        kind = rr.DIAGONAL if dx and dy else rr.AXIS
        n = 0
        for m in DROPPED + SMALLEST + ORDINARY + OVERFLOW + (INF,):
            if m == INF and di not in (0, 1, 3, 4):      # inf itself: the +x and -x axes, a diagonal of either side
                continue
            for x in signed_zeros(dx, m):
                for y in signed_zeros(dy, m):
                    x32, y32 = float(F32(x)), float(F32(y))
                    wraps = x32 < 0 and y32 == 0 and math.copysign(1.0, y32) < 0          # atan2(-0, x < 0) = -pi: column 1800
                    if m in ORDINARY and not wraps:
                        place_column_probe(fr, x32, y32, kind, int(round(rr.colf(x32, y32))), 6 * di + n, rows=range(2, 66))
                        n += 1
                        continue
                    zs = (0.0,) if m not in OVERFLOW else (0.0, m)
                    for z in zs:
                        if wraps and m not in DROPPED:
                            oob.append(np.array([x32, y32, z if m not in ORDINARY else float(z_mid_row(x32, y32, 20 + n)), 0.0], F32))
                        else:
                            fr.add((x32, y32, z), kind, int(round(rr.colf(x32, y32))) if m not in DROPPED else -1)
    for x in (0.0, -0.0):           # r = |z|, q = +-1: the row is outside the image before the column (1800 for (-0, -0)) is used
        for y in (0.0, -0.0):
            for z in (5.0, -5.0):
                fr.add((x, y, z), rr.ZERO_XY)


def row_probe_point(q, col, rng):
    """A float32 point of column ``col`` (its middle) whose float32 z / sqrtf(x x + y y + z z) is exactly ``q``."""
    phi = rr.PI - (col + 0.5) * rr.AZ_RES
    rho = rng.uniform(8.0, 40.0, 1 << 15)
    p = np.zeros((len(rho), 4), F32)
    p[:, 0], p[:, 1] = rho * math.cos(phi), rho * math.sin(phi)
    planar = np.hypot(p[:, 0].astype(np.float64), p[:, 1].astype(np.float64))
    p[:, 2] = planar * (q / math.sqrt(1.0 - q * q))
    for step in (0, 1, -1, 2, -2):
        t = p.copy()
        for _ in range(abs(step)):
            t[:, 2] = np.nextafter(t[:, 2], F32(INF if step > 0 else -INF))
        hit = np.flatnonzero(t[:, 2] / rr.ranges(t) == F32(q))
        if len(hit):
            return t[hit[0]]
    raise RuntimeError("no point for q = %r" % q)


def npz_bytes(arrays):
    """An .npz without time stamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue(), zipfile.ZIP_DEFLATED, 9)
    return buf.getvalue()


def oracle_pixels(orc, pts):
    """The oracle's pixel per point, each projected alone (behind three r == 0 points the oracle drops): (-1, -1) dropped, column 1800
    where it raises."""
    out = np.full((len(pts), 2), -1, np.int64)
    pc = np.zeros((4, 4), F32)
    for i, p in enumerate(pts):
        pc[3] = p
        try:
            _, cnt = orc.ProjectPC2SphericalRing(pc)
        except IndexError:
            out[i] = rr.pixels(p)[0][0], rr.RING_W
            continue
        hit = np.argwhere(cnt)
        assert len(hit) <= 1
        if len(hit):
            out[i] = hit[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=TRIALS)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import oracle as orc
    orc.build()

    fr, oob = Frame(), []
    axis_points(fr, oob)

    found = search(a.trials, a.workers)
    for i, (x, y, edge) in enumerate(found):
        kind = rr.OFF_AXIS if rr.flips_of_column(x, y) & rr.ONE_ULP else rr.OFF_AXIS_EXTRA
        place_column_probe(fr, x, y, kind, edge, 7 * i, block_edge=edge % 32 == 0)

    qs, margin_rows, margin_ulp, walked = walk_rows(a.workers)
    rng = np.random.default_rng([SEED, 1 << 40])
    used_cols = set(c + d for _, c in fr.used for d in (-1, 0, 1))
    cols = [next(c for c in range(c0, c0 + 100) if c not in used_cols) for c0 in range(40, 1740, 107)]      # sixteen free columns
    for q, col in zip(qs, cols):
        pix = fr.add(row_probe_point(q, col, rng), rr.ROW_PROBE)
        assert pix[1] == col or pix[0] < 0, (q, col, pix)

    # the same-pixel group: an exact, a just-below and a just-above probe, each on a fresh row with two ordinary points of its pixel
    by_class = {}
    for x, y, edge in found:
        ulp = rr.ulp_from_integer(rr.colf(x, y))[1]
        by_class.setdefault(0 if ulp == 0 else (1 if ulp < 0 else 2), (x, y, edge))
    for g in range(3):
        x, y, edge = by_class[g]
        for row in range(30 + g, 60):
            e = np.array([x, y, z_mid_row(x, y, row), 0.0], F32)
            pix = tuple(int(v) for v in rr.pixels(e)[0])
            if pix[0] == row and not any((row, pix[1] + d) in fr.used for d in (-1, 0, 1)):
                break
        else:
            raise RuntimeError("no free pixel for group %d" % g)
        fr.used.add(pix)
        phi = rr.PI - (pix[1] + 0.5) * rr.AZ_RES
        members = [e]
        for rho in (7.0, 9.0):
            xo, yo = rho * math.cos(phi), rho * math.sin(phi)
            members.append(np.array([xo, yo, z_mid_row(F32(xo), F32(yo), row), 0.0], F32))
        order = ((0, 1, 2), (1, 0, 2), (1, 2, 0))[g]        # the edge point first, in the middle, last
        for k in order:
            got = fr.add(members[k], rr.GROUP_EDGE if k == 0 else rr.GROUP_ORDINARY, edge if k == 0 else -1, group=g)
            assert got == pix, (g, k, got, pix)

    pts = np.stack(fr.pts)
    oob = np.stack(oob)
    oob[:, 3] = len(pts) + 1 + np.arange(len(oob))
    kind, edge, group = np.array(fr.kind, np.int8), np.array(fr.edge, np.int16), np.array(fr.group, np.int8)
    r, cf, rf = rr.terms(pts)
    is_col = np.isin(kind, (rr.AXIS, rr.DIAGONAL, rr.OFF_AXIS, rr.OFF_AXIS_EXTRA, rr.GROUP_EDGE)) & (edge >= 0)
    ulp, flips = np.zeros(len(pts)), np.zeros(len(pts), np.uint8)
    cr = np.ones(len(pts), bool)
    for i in range(len(pts)):
        x, y = float(pts[i, 0]), float(pts[i, 1])
        if is_col[i]:
            ulp[i], flips[i] = rr.ulp_from_integer(cf[i])[1], rr.flips_of_column(x, y)
        elif kind[i] == rr.ROW_PROBE:
            ulp[i], flips[i] = rr.ulp_from_integer(rf[i])[1], rr.flips_of_row(pts[i, 2] / r[i])
        if r[i] != 0:
            cr[i] = float(np.arctan2(np.longdouble(y), np.longdouble(x))) == math.atan2(y, x)
    pixel = oracle_pixels(orc, pts)
    assert np.array_equal(pixel, rr.pixels(pts)), "the restatement and the oracle disagree"
    oob_pixel = oracle_pixels(orc, oob)
    assert (oob_pixel[:, 1] == rr.RING_W).all() and (oob_pixel[:, 0] >= 0).all()
    ring, cnt = orc.ProjectPC2SphericalRing(pts)
    occ = np.flatnonzero(cnt.ravel())
    winner = ring.reshape(-1, rr.RING_C)[occ, 3].astype(np.int64) - 1

    off = kind == rr.OFF_AXIS
    n_exact, n_below, n_above = int((off & (ulp == 0)).sum()), int((off & (ulp < 0)).sum()), int((off & (ulp > 0)).sum())
    quadrants = sorted(set((bool(p[0] > 0), bool(p[1] > 0)) for p in pts[off]))
    wide = kind == rr.OFF_AXIS_EXTRA
    far = (off | wide) & (r >= 10.5) & (pixel[:, 0] < NET_H)
    block_edges = sorted(set(int(c) for c in edge[far & (edge % 32 == 0)]))
    high = int((rr.pixels(pts[off], atan2=rr.moved(math.atan2, 1)) != pixel[off]).any(axis=1).sum())
    low = int((rr.pixels(pts[off], atan2=rr.moved(math.atan2, -1)) != pixel[off]).any(axis=1).sum())
    print("%d points (+ %d of column 1800): %d axis, %d diagonal, %d off axis (%d exact, %d below, %d above; %d / %d move when atan2 is an ulp "
          "high / low) + %d that need two ulp, %d block edges at >= 10 m, %d row probes, %d in the same-pixel group; %d occupied pixels; atan2 "
          "correctly rounded at %d of %d"
          % (len(pts), len(oob), (kind == rr.AXIS).sum(), (kind == rr.DIAGONAL).sum(), off.sum(), n_exact, n_below, n_above, high, low,
             wide.sum(), len(block_edges), (kind == rr.ROW_PROBE).sum(), (group >= 0).sum(), len(occ), cr[r != 0].sum(), (r != 0).sum()))
    print("row walk: %d floats, nearest %.3g rows = %.3g ulp of rowf" % (walked, margin_rows, margin_ulp))
    assert off.sum() >= 256 and min(n_exact, n_below, n_above) >= 32 and len(quadrants) == 4 and len(block_edges) >= 16, \
        "too few off-axis probes: raise --trials (never the band)"
    assert high + low == off.sum() and 3 * min(high, low) >= off.sum()      # either wrong atan2 moves its share, both together all
    assert (np.abs(ulp[off | wide]) <= BAND_ULP).all() and (flips[off] & rr.ONE_ULP != 0).all() and (flips[wide] != 0).all()
    assert (kind == rr.ROW_PROBE).sum() == 16

    data = npz_bytes(dict(
        points=pts, oob_points=oob, kind=kind, edge=edge, group=group, pixel=pixel.astype(np.int16), oob_pixel=oob_pixel.astype(np.int16),
        ulp=ulp, flips=flips, atan2_correctly_rounded=cr, ring_pixels=occ.astype(np.int32), ring_winners=winner.astype(np.int32),
        ring_counts=cnt.ravel()[occ].astype(np.int32), ring_sha256=np.array(hashlib.sha256(ring.tobytes()).hexdigest()),
        counter_sha256=np.array(hashlib.sha256(cnt.tobytes()).hexdigest()), row_margin_rows=np.float64(margin_rows),
        row_margin_ulp=np.float64(margin_ulp), row_floats_walked=np.int64(walked), seed=np.int64(SEED), trials=np.int64(a.trials),
        band_ulp=np.float64(BAND_ULP), libc=np.array(" ".join(platform.libc_ver()))))
    with open(a.out, "wb") as f:
        f.write(data)
    print("wrote %s: %d bytes, sha256 %s" % (a.out, len(data), hashlib.sha256(data).hexdigest()))


if __name__ == "__main__":
    main()
