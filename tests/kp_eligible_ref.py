"""The key point eligibility map of the fused path (csrc/ring.hip: k_ring_fill writes it, k_respond_mfma and k_kp_score skip by it),
restated in NumPy, and the clouds its tests run on.

A pixel of the 64 x 1792 net area is *eligible* iff it is occupied and the float32 norm over the ring's first ``dist_c`` channels is
>= 10 (the range gate of SphericalRing.py:197-198: squares summed in channel order, a NaN fails, +inf passes).  The map holds one
bit per (row, 32-column block): some pixel of the block is eligible.  A response block (y, b) is *needed* iff a bit is set in rows
y - 2 .. y + 2 and blocks b - 1 .. b + 1 -- a superset of "within two columns of an eligible pixel"; a 4 x 64 score tile is live iff
one of its two blocks has a bit in one of its four rows.

The clouds are ``kp_images.cloud`` lattice clouds: one point per pixel, 5 m away (occupied, never eligible) except where a case
writes a range down.  tests/test_kp_eligible_host.py holds every case against the oracle, so the GPU tests cannot pass on a cloud
that missed its corner."""
import functools

import numpy as np

import kp_images as kpi

F32 = np.float32
NET_H, NET_W, BLK = kpi.NET_H, kpi.NET_W, 32
NBLK = NET_W // BLK
TILE_ROWS, TILE_COLS, ROW0, ROW1 = 4, 64, 8, 56      # k_kp_score's tiles over rows 8..55
RESP_ROW0, RESP_ROW1 = 6, 58                         # the response rows the fused path computes


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def ring_norm(ring, dist_c):
    """[H, W] float32: sqrt of the squares of channels 0 .. dist_c - 1, summed in channel order (SphericalRing.py:197)."""
    px = np.asarray(ring, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = px[..., 0] * px[..., 0]
        for c in range(1, dist_c):
            d2 = d2 + px[..., c] * px[..., c]
        return np.sqrt(d2)


def eligible(ring, cnt, dist_c):
    """bool [64, 1792] from the reference's ring image and grid counter."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(cnt)[:NET_H, :NET_W] > 0) & (ring_norm(np.asarray(ring)[:NET_H, :NET_W], dist_c) >= F32(10.0))


def map_bits(elig):
    """bool [64, 56]: some pixel of the block is eligible."""
    return elig.reshape(NET_H, NBLK, BLK).any(axis=2)


def map_words(elig):
    """The map as the device stores it: uint64 [64], bit b of word y."""
    bits = map_bits(elig)
    return (bits.astype(np.uint64) << np.arange(NBLK, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)


def bits_of_words(words):
    return ((np.asarray(words, np.uint64)[:, None] >> np.arange(NBLK, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def needed_blocks(bits):
    """bool [64, 56]: block (y, b) has a bit in rows y - 2 .. y + 2, blocks b - 1 .. b + 1."""
    rows = np.zeros_like(bits)
    for dy in range(-2, 3):
        lo, hi = max(0, dy), NET_H + min(0, dy)
        rows[lo - dy:hi - dy] |= bits[lo:hi]
    out = rows.copy()
    out[:, 1:] |= rows[:, :-1]
    out[:, :-1] |= rows[:, 1:]
    return out


def live_tiles(bits):
    """bool [12, 28]: the 4 x 64 score tiles of rows 8..55 that hold a bit."""
    return bits[ROW0:ROW1].reshape((ROW1 - ROW0) // TILE_ROWS, TILE_ROWS, NET_W // TILE_COLS, TILE_COLS // BLK).any(axis=(1, 3))


def window_blocks(centres):
    """-> (rows, blocks) index arrays of every pixel of the 5 x 5 windows of ``centres`` [n, 2] (all inside the image: rows 8..55,
    columns 8..1783)."""
    c = np.asarray(centres, np.int64).reshape(-1, 2)
    dy, dx = np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), indexing="ij")
    rows = (c[:, 0, None] + dy.ravel()[None, :]).ravel()
    cols = (c[:, 1, None] + dx.ravel()[None, :]).ravel()
    return rows, cols // BLK


# ---- clouds ------------------------------------------------------------------------------------------------------------------------
def _direction(row, col):
    theta = np.pi - (col + 0.5) * kpi.AZ_RES
    el = ((kpi.RING_H - row) + 0.5 - kpi.V_OFF) * kpi.V_RES
    return np.array([np.cos(el) * np.cos(theta), np.cos(el) * np.sin(theta), np.sin(el)])


def _point_norm(p, dist_c):
    """The ring pixel a point [.., 4] f32 becomes (x, y, z, intensity, range) and its gate norm."""
    p = np.asarray(p, F32)
    s = p[..., 0] * p[..., 0]
    s = s + p[..., 1] * p[..., 1]
    s = s + p[..., 2] * p[..., 2]
    return ring_norm(np.concatenate([p, np.sqrt(s)[..., None]], axis=-1), dist_c)


def tuned_point(row, col, dist_c, target, seed):
    """A point [4] f32 in the direction of pixel (row, col), intensity 0.5, whose gate norm over ``dist_c`` channels is exactly
    ``target`` (a float32 next to 10): 8192 copies of the solution, every coordinate jittered by a few 1e-6 of itself, the first that
    lands on it."""
    target = F32(target)
    rho0 = np.sqrt((float(target) ** 2 - 0.25) / 2.0) if dist_c == 5 else float(target)
    p = np.concatenate([rho0 * _direction(row, col), [0.5]])[None, :] * (1.0 + np.random.RandomState(seed).uniform(-4e-6, 4e-6, (8192, 4)))
    p = p.astype(F32)
    hit = np.nonzero(_point_norm(p, dist_c) == target)[0]
    assert len(hit), (row, col, dist_c, target)
    return p[hit[0]]


JUST_BELOW_10 = np.nextafter(F32(10.0), F32(0.0))
CORNERS = ((20, 320), (23, 383), (32, 671), (35, 704))     # corners of 32-column blocks (and of 64-column tiles) and of 4-row tiles
GATE_IN = ((8, 8), (55, 55), (8, 64), (55, 1783), (8, 1783), (55, 8))
GATE_OUT = ((7, 300), (56, 330), (20, 7), (24, 56), (28, 63), (32, 1784))
THRESHOLD = {   # name -> (row, col, channels the norm is tuned over, norm)
    "at_10_over_5": (20, 400, 5, F32(10.0)), "below_10_over_5": (20, 440, 5, JUST_BELOW_10),
    "at_10_over_3": (30, 400, 3, F32(10.0)), "below_10_over_3": (30, 440, 3, JUST_BELOW_10),
}
ONLY_5 = (20, 480)    # 8 m away: norm 11.3 over five channels (the range channel counts), 8 over xyz
INF_PIXEL = (11, 900)   # where the point (inf, 0, 0) lands: azimuth pi - atan2(0, inf) = pi, elevation asin(0 / inf) = 0
BESIDE_INF = (12, 902)  # an ordinary far pixel whose window reaches the responses computed from INF_PIXEL


def _cloud(centres=(), ranges=(), background=5.0, points=(), tail=()):
    """kp_images.cloud, then ``points`` ((row, col, point[4]) replaces that pixel's point) and ``tail`` (points appended in file
    order: the last point of a pixel wins it)."""
    centres = np.asarray(centres, np.int64).reshape(-1, 2)
    pc = kpi.cloud(centres, ranges, background, seed=7)
    if len(points):
        # undo the shuffle to address pixels: cloud() permutes the row-major pixel list with RandomState(7)
        perm = np.random.RandomState(7).permutation(len(pc))
        where = np.empty(len(pc), np.int64)
        where[perm] = np.arange(len(pc))
        for row, col, p in points:
            pc[where[row * NET_W + col]] = np.asarray(p, F32)
    if len(tail):
        pc = np.concatenate([pc, np.asarray(tail, F32).reshape(-1, 4)])
    pc = np.ascontiguousarray(pc, F32)
    pc.setflags(write=False)
    return pc


@functools.lru_cache(maxsize=None)
def cases():
    """name -> cloud [n, 4] f32 (read-only)."""
    rs = np.random.RandomState(20)
    out = {}
    out["corners"] = _cloud(CORNERS, [30.0, 34.0, 38.0, 42.0])
    for i, c in enumerate(CORNERS):
        out["corner_%d" % i] = _cloud([c], [30.0 + 4 * i])
    out["gates"] = _cloud(GATE_IN + GATE_OUT, rs.uniform(20.0, 50.0, len(GATE_IN) + len(GATE_OUT)))
    out["none"] = _cloud()
    lat = kpi.pick(1500, 3)
    out["all"] = _cloud(lat, rs.uniform(25.0, 60.0, len(lat)), background=20.0)
    pts = [(r, c, tuned_point(r, c, ch, v, 100 + i)) for i, (r, c, ch, v) in enumerate(THRESHOLD.values())]
    out["threshold"] = _cloud([ONLY_5] + list(CORNERS[:2]), [8.0, 30.0, 34.0], points=pts)
    out["inf"] = _cloud(list(CORNERS) + [BESIDE_INF], [30.0, 34.0, 38.0, 42.0, 25.0], tail=[[np.inf, 0.0, 0.0, 0.5]])
    out["nan"] = _cloud(CORNERS, [30.0, 34.0, 38.0, 42.0], tail=[[np.nan, 1.0, 1.0, 0.5]])
    lat = kpi.lattice()
    left, right = lat[lat[:, 1] < 800], lat[lat[:, 1] > 1000]
    out["left"] = _cloud(left[rs.permutation(len(left))[:300]], rs.uniform(12.0, 60.0, 300))
    out["right"] = _cloud(right[rs.permutation(len(right))[:300]], rs.uniform(12.0, 60.0, 300))
    rows, cols = np.meshgrid(np.arange(32), np.arange(NET_W), indexing="ij")
    upper = np.stack([rows.ravel(), cols.ravel()], axis=1)
    out["upper_half"] = _cloud(upper, 20.0 + 10.0 * np.sin(cols.ravel() / 7.0) * np.cos(rows.ravel() / 3.0))
    return out


PIPELINE_ORDER = ("none", "all", "upper_half", "corner_1", "corners", "gates", "threshold", "left")
ORACLE_FREE = ("nan",)     # the reference raises on a NaN coordinate (int(nan)): no oracle result
