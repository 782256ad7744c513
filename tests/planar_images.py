"""Inputs of the planar-point tests (test_planar_host.py, test_planar_gpu.py): the crafted image, whose patches each place ONE decision
of the rule (include/caelo.h, caelo_planar_points) a clear factor from its threshold -- or on it, where the boundary is the point --,
the empty and the capacity image, and the host twin's call.  Patches lie at least 12 pixels apart, so no window sees two of them.

A patch is a set of occupied pixels around a centre pixel; pixel offset (dy, dx) carries the point origin + 0.3 (dx, dy, .) on the
patch's plane, 20 m or more from the sensor unless the patch says otherwise, so that the VisibleBottom quirk (:259-262) stays out of
the way of the other decisions."""
import ctypes as C

import numpy as np

import planar_ref as pr

F32 = np.float32
BLOCK = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]
SPREAD5 = [(-2, -2), (-2, 2), (2, -2), (2, 2), (0, -2)]        # five neighbours none of which sees five others
PREV = lambda v: np.nextafter(F32(v), F32(0))                  # noqa: E731
NEXT = lambda v: np.nextafter(F32(v), F32(1))                  # noqa: E731


class Image:
    def __init__(self, ring_c=3, height=64, width=1792):
        self.ring = np.zeros((height, width, ring_c), F32)
        self.counter = np.zeros((height, width), np.int32)
        self.resp = np.zeros((pr.NET_H, pr.NET_W, 8), F32)
        self.at = {}     # patch name -> centre pixel

    def put(self, y, x, xyz, resp=0.0, count=1):
        self.ring[y, x, 0:3] = xyz
        if self.ring.shape[2] == 5:
            self.ring[y, x, 3] = 0.5
            self.ring[y, x, 4] = np.sqrt(np.sum(np.asarray(xyz, np.float64) ** 2))
        self.counter[y, x] = count
        self.resp[y, x] = resp

    def patch(self, name, y, x, offsets=BLOCK, slope=(0.0, 0.0), origin=(20.0, 0.0, -1.7), resp=0.0, centre=True, centre_xyz=None, centre_resp=None):
        """z = origin_z + slope_x (X - origin_x) + slope_y (Y - origin_y) over the pixels centre + offsets."""
        self.at[name] = (y, x)
        for dy, dx in offsets:
            if (dy, dx) == (0, 0):
                continue
            X, Y = origin[0] + 0.3 * dx, origin[1] + 0.3 * dy
            self.put(y + dy, x + dx, (X, Y, origin[2] + slope[0] * 0.3 * dx + slope[1] * 0.3 * dy), resp, count=1 + (dy + dx) % 3)
        if centre:
            self.put(y, x, origin if centre_xyz is None else centre_xyz, resp if centre_resp is None else centre_resp)


def tilt(nz):
    """the slope of a plane whose unit normal has the z component nz (tilted about the y axis)"""
    return (float(np.sqrt(1.0 - nz * nz) / nz), 0.0)


def one_channel(v):
    """a response vector at float32 distance exactly v from the zero vector (sqrt(fl(v v)) == v in float32)"""
    r = np.zeros(8, F32)
    r[3] = v
    return r


def crafted(ring_c=3, height=64, width=1792):
    """-> (Image, expect): expect[name] = True / False / None -- whether the patch's CENTRE pixel is a planar point (None: undecided)."""
    im, ex = Image(ring_c, height, width), {}
    col = iter(range(40, 1700, 16))

    def add(name, keep, y=30, **kw):
        im.patch(name, y, next(col), **kw)
        ex[name] = keep
    add("flat", True)
    add("tilt_095", True, slope=tilt(0.95))
    add("tilt_085", False, slope=tilt(0.85))
    add("four_neighbours", False, offsets=SPREAD5[:4])
    add("five_neighbours", True, offsets=SPREAD5)
    # minDiff on PlanarThreshold: float32(0.4) is above 0.4 as a double (rejected), the float32 below it is not
    add("mindiff_04", False, centre_resp=one_channel(F32(0.4)))
    add("mindiff_04_below", True, centre_resp=one_channel(PREV(0.4)))
    add("mindiff_06", False, centre_resp=one_channel(F32(0.6)))
    # the quirk of :259-262: minDiff > 0.2 (float32(0.2) is, as a double) and |centre| < 10 skips the pixel; |(6, 8, 0)| is exactly 10
    for tag, v in (("below", PREV(0.2)), ("at", F32(0.2)), ("above", NEXT(0.2))):
        add("quirk_%s_norm10" % tag, True, origin=(6.0, 8.0, 0.0), centre_resp=one_channel(v))
        add("quirk_%s_near" % tag, tag == "below", origin=(3.0, 4.0, 0.0), centre_resp=one_channel(v))
    # with the centre in the covariance the smallest axis would lie in the plane
    add("centre_excluded", True, centre_xyz=(20.0, 0.0, 48.3))
    # the collinear window: two equal smallest eigenvalues -- undecided, the call still returns
    im.at["collinear"] = (30, next(col))
    ex["collinear"] = None
    y, x = im.at["collinear"]
    for k, (dy, dx) in enumerate([(0, 0)] + SPREAD5):
        im.put(y + dy, x + dx, (20.0 + 0.25 * k, 1.0 + 0.125 * k, -1.0))
    # a NaN response among the occupied neighbours; one on an unoccupied pixel is never looked at
    add("nan_neighbour", False)
    y, x = im.at["nan_neighbour"]
    im.resp[y + 1, x - 1, 5] = np.nan
    add("nan_unoccupied", True, offsets=[o for o in BLOCK if o != (1, 1)])
    y, x = im.at["nan_unoccupied"]
    im.resp[y + 1, x + 1, :] = np.nan
    add("inf_coordinate", False)
    y, x = im.at["inf_coordinate"]
    im.ring[y - 2, x + 2, 1] = np.inf
    # the edges of rows 8..55 and columns 8..1783: blocks whose centres lie ON them; their outer pixels 6, 7 / 56, 57 / 1784, 1785 are
    # read by the windows of the edge pixels and never emitted themselves
    for name, y, x in (("row_8", 8, 300), ("row_55", 55, 300), ("col_8", 30, 8), ("col_1783", 30, 1783), ("corner_lo", 8, 8), ("corner_hi", 55, 1783)):
        im.patch(name, y, x)
        ex[name] = True
    return im, ex


def capacity(ring_c=3, height=64, width=1792):
    """every pixel occupied, one response vector, the plane z = -1.7 exactly: all 48 x 1776 interior pixels are planar points with
    the normal (0, 0, 1) exactly (a zero row and column of the covariance keep their unit vector in the Jacobi)."""
    im = Image(ring_c, height, width)
    yy, xx = np.mgrid[0:height, 0:width]
    im.ring[..., 0] = (20.0 + 0.25 * xx).astype(F32)
    im.ring[..., 1] = (0.25 * yy).astype(F32)
    im.ring[..., 2] = F32(-1.75)
    im.counter[...] = 1 + (yy + xx) % 4
    im.resp[...] = np.linspace(-1, 1, 8, dtype=F32)
    return im


def frame(orc, models, scans, frame_no, scene_kind):
    """a synthetic mm-quantised scan as (ring [69,1800,5], counter, response of the oracle's RespondLayer)"""
    ring, cnt = orc.ProjectPC2SphericalRing(scans(frame_no, quantum=1e-3, scene_kind=scene_kind))
    resp = models[0].predict(ring[None, 0:64, 0:1792, 0:3])[0]
    return np.ascontiguousarray(ring, F32), np.ascontiguousarray(cnt, np.int32), np.ascontiguousarray(resp, F32)


def host_planar(ring, counter, resp, want_pixels=True, fill=None):
    """caelo_host_planar_points -> (rows [n,6], pixels [n,2], n, the whole output buffers)"""
    from caelo import _ffi
    lib = _ffi.load()
    ring, counter, resp = np.ascontiguousarray(ring, F32), np.ascontiguousarray(counter, np.int32), np.ascontiguousarray(resp, F32)
    planar = np.zeros((_ffi.PLANAR_MAX, 6), F32) if fill is None else np.full((_ffi.PLANAR_MAX, 6), fill, F32)
    pixels = np.full((_ffi.PLANAR_MAX, 2), -1, np.int32)
    n = np.full(1, -1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.caelo_host_planar_points(p(ring), ring.shape[1], ring.shape[2], p(counter), counter.shape[1], p(resp), p(planar),
                                      p(pixels) if want_pixels else None, p(n))
    assert rc == 0, lib.caelo_last_error()
    k = int(n[0])
    return planar[:k], pixels[:k], k, (planar, pixels)
