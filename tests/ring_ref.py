"""ProjectPC2SphericalRing's pixel choice (SphericalRing.py:77-93; csrc/ring.hip: k_project_points) restated point by point, and the
handles the ring edge tests turn on it.

The float32 part -- the squares summed in order, the root, the quotient z / r -- is NumPy float32 arithmetic; everything behind it is
float64, as in the reference: ``col = int((pi - atan2(y, x)) / az_res)``, ``row = 69 - int(asin(z / r) / v_res + v_off)``.  The two
transcendentals are ``math.atan2`` and ``math.asin``, the C library's, one call per point: that is what the reference and the oracle
call, and NumPy's array loops are not the same functions on every CPU (where they are vectorised, about 7 % of ``np.arctan2`` results
differ from ``math.atan2`` in the last bit -- enough to move every probe of tests/golden/ring_edges.npz).  Both can be replaced, which
is how the tests ask what a function that is an ulp off would do.

tools/make_goldens_ring_edges.py builds the fixture with these functions; tests/test_ring_edges_host.py holds them against the oracle.
"""
import math

import numpy as np

F32 = np.float32
RING_H, RING_W, RING_C = 69, 1800, 5
PI = math.pi
D2R = PI / 180                                    # SphericalRing.py:28
AZ_RES = 0.20 * D2R                               # :35, :48
V_DOWN, V_UP = -24.8 * D2R, 2.0 * D2R             # :49-50
V_RES = (V_UP - V_DOWN) / (64 - 1)                # :51
V_OFF = -V_DOWN / V_RES                           # :52
ST_COL_OOB = 1                                    # include/caelo.h CAELO_ST_COL_OOB

# The fixture's point classes (``kind``).  OFF_AXIS, the class the fixture's counts are asked of: the column changes under ONE ulp of
# atan2 -- atan2 is the last double of its column, which an atan2 that is an ulp HIGH moves one column to the left, or the first double
# of the column before, which an atan2 that is an ulp LOW moves to the right; a search finds about as many of one as of the other, so
# either wrong function moves about half of the class and the two together all of it.  OFF_AXIS_EXTRA: the column only changes under
# two ulp (the doubles either side of those).
AXIS, DIAGONAL, ZERO_XY, OFF_AXIS, ROW_PROBE, GROUP_EDGE, GROUP_ORDINARY, OFF_AXIS_EXTRA = range(8)
ONE_ULP = 0b0110                                  # the bits of ``flips`` for the moves by -1 and +1 ulp
# bits of the fixture's ``flips``: the column (row probes: the row) changes when atan2 (asin) is moved by -2, -1, +1, +2 ulp
MOVES = (-2, -1, 1, 2)


def ranges(pc):
    """float32 [n]: LA.norm(PC[:, 0:3], axis=1) as NumPy computes it for float32 rows -- squares, summed in order, root (:77)."""
    p = np.asarray(pc, F32).reshape(-1, 4)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = p[:, 0] * p[:, 0]
        s = s + p[:, 1] * p[:, 1]
        s = s + p[:, 2] * p[:, 2]
        return np.sqrt(s)


def moved(fn, k):
    """``fn`` with every result moved by ``k`` ulp (k < 0: towards -inf)."""
    def f(*a):
        v = fn(*a)
        for _ in range(abs(k)):
            v = math.nextafter(v, math.inf if k > 0 else -math.inf)
        return v
    return f


def colf(x, y, atan2=math.atan2):
    return (PI - atan2(float(y), float(x))) / AZ_RES                                  # :86


def rowf(q, asin=math.asin):
    return asin(float(q)) / V_RES + V_OFF                                             # :88


def terms(pc, atan2=math.atan2, asin=math.asin):
    """-> (r float32 [n], colf float64 [n], rowf float64 [n]); NaN where r == 0 (the point is dropped, :78-80)."""
    p = np.asarray(pc, F32).reshape(-1, 4)
    r = ranges(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = p[:, 2] / r                                                                # :87, the float32 quotient
    cf, rf = np.full(len(p), np.nan), np.full(len(p), np.nan)
    for i in np.flatnonzero(r != 0):
        cf[i], rf[i] = colf(p[i, 0], p[i, 1], atan2), rowf(q[i], asin)
    return r, cf, rf


def pixels(pc, atan2=math.atan2, asin=math.asin):
    """int64 [n, 2]: the (row, col) every point is written to, (-1, -1) where the reference writes nothing (r == 0, or the row
    outside the image: :89 comes before the column is used).  A column of 1800 is returned as it is: IndexError at :91."""
    _, cf, rf = terms(pc, atan2, asin)
    out = np.full((len(cf), 2), -1, np.int64)
    for i in np.flatnonzero(cf == cf):
        row = RING_H - int(rf[i])
        if 0 <= row < RING_H:
            out[i] = row, int(cf[i])
    return out


def project(pc, atan2=math.atan2, asin=math.asin):
    """-> (Image_float [69, 1800, 5] f32, GridCounter [69, 1800] i32): the last point of a pixel in file order wins it (:91-93)."""
    p = np.asarray(pc, F32).reshape(-1, 4)
    ring, cnt = np.zeros((RING_H, RING_W, RING_C), F32), np.zeros((RING_H, RING_W), np.int32)
    r, pix = ranges(p), pixels(p, atan2, asin)
    for i in np.flatnonzero(pix[:, 0] >= 0):
        row, col = pix[i]
        if col >= RING_W:
            raise IndexError("index %d is out of bounds for axis 1 with size %d" % (col, RING_W))
        ring[row, col, 0:4], ring[row, col, 4] = p[i], r[i]
        cnt[row, col] += 1
    return ring, cnt


def ulp_from_integer(v):
    """(nearest integer, signed distance of ``v`` from it in units of the integer's float64 spacing)."""
    n = round(v)
    return n, (v - n) / float(np.spacing(np.float64(max(abs(n), 1))))


def flips_of_column(x, y):
    """Bit k: the column of (x, y) changes when atan2's result is moved by MOVES[k] ulp."""
    col = int(colf(x, y))
    return sum(1 << k for k, m in enumerate(MOVES) if int(colf(x, y, moved(math.atan2, m))) != col)


def flips_of_row(q, reach=(-2, -1, 1, 2)):
    """The same for the row of a float32 quotient ``q`` and asin."""
    row = int(rowf(q))
    return sum(1 << k for k, m in enumerate(reach) if int(rowf(q, moved(math.asin, m))) != row)


def expected_ring(points, winners_pix, winners_idx):
    """The ring image from the fixture's recorded winners: pixel ``winners_pix[j]`` (flat) holds point ``winners_idx[j]``."""
    p = np.asarray(points, F32)
    ring = np.zeros((RING_H * RING_W, RING_C), F32)
    ring[winners_pix, 0:4] = p[winners_idx]
    ring[winners_pix, 4] = ranges(p[winners_idx])
    return ring.reshape(RING_H, RING_W, RING_C)
