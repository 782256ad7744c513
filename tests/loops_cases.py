"""Inputs shared by tests/test_loops_host.py and tests/test_loops_gpu.py: the host twins behind NumPy arrays, the crafted and generated
clouds of the descriptor tests and the sparse images of the search tests.  Everything is made once and left unchanged."""
import ctypes as C
import functools

import numpy as np

import loops_ref as lr


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _lib():
    from caelo import _ffi
    return _ffi.load()


def host_scan_context(pts, n_pts, fill=0.0):
    """pts [F, ld, C] f32, n_pts [F] -> (sc [F,20,60] f32, u [F,1200] f32, valid [F] u64) from caelo_host_scan_context"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    n_pts = np.ascontiguousarray(n_pts, dtype=np.int32)
    f, ld, c = pts.shape
    sc = np.full((f, lr.RINGS, lr.SECTORS), fill, np.float32)
    u = np.full((f, lr.BINS), fill, np.float32)
    valid = np.zeros(f, np.uint64)
    rc = _lib().caelo_host_scan_context(_p(pts), ld, c, _p(n_pts), f, _p(sc), _p(u), _p(valid))
    assert rc == 0, _lib().caelo_last_error()
    return sc, u, valid


def host_loop_search(u, valid, min_gap=50, k=1, max_dist=None, min_cols=1, queries=None, dense=False):
    """-> (cand [Nq,k] i32, dist [Nq,k] f32, shift [Nq,k] i32[, dense dist [Nq,N] f32, dense shift [Nq,N] i8]) from caelo_host_loop_search"""
    u = np.ascontiguousarray(u, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.uint64)
    n = u.shape[0]
    q0, q1 = (0, n) if queries is None else queries
    nq = q1 - q0
    cand, dist, shift = np.full((nq, k), -7, np.int32), np.full((nq, k), -7, np.float32), np.full((nq, k), -7, np.int32)
    dd = np.full((nq, n), -7, np.float32) if dense else None
    ds = np.full((nq, n), -7, np.int8) if dense else None
    rc = _lib().caelo_host_loop_search(_p(u), _p(valid), n, q0, q1, min_gap, k, np.inf if max_dist is None else max_dist, min_cols,
                                       _p(cand), _p(dist), _p(shift), _p(dd), _p(ds))
    assert rc == 0, _lib().caelo_last_error()
    return (cand, dist, shift, dd, ds) if dense else (cand, dist, shift)


def valid_bits(valid):
    """[N] u64 -> [N, 60] bool"""
    return ((np.asarray(valid, dtype=np.uint64)[:, None] >> np.arange(lr.SECTORS, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def pack(clouds, ld=None, cols=None):
    """a list of [n_i, C] clouds -> (pts [F, ld, C] f32 padded with NaN rows that must never be read as points, n_pts [F] i32)"""
    cols = cols or clouds[0].shape[1]
    ld = ld or max(1, max(len(c) for c in clouds))
    pts = np.full((len(clouds), ld, cols), np.nan, np.float32)
    pts[:, :, 2] = 1e6          # a padding row read by mistake would be dropped (NaN) -- or show as a huge height if only z were read
    for f, c in enumerate(clouds):
        pts[f, :len(c)] = c
    return pts, np.array([len(c) for c in clouds], np.int32)


# ---- descriptor clouds ------------------------------------------------------------------------------------------------------------------
F32_BELOW_80 = np.nextafter(np.float32(80.0), np.float32(0.0))
# (x, y, z) -> (ring, sector) or None when the point is skipped; z values are distinct so that a bin names its point
CRAFTED = [
    # the four axes, where atan2 is exact: theta = 0, pi / 2, pi, -pi / 2 (+ 2 pi) open sectors 0, 15, 30, 45; r = 4 opens ring 1
    ((4.0, 0.0, 0.125), (1, 0)), ((0.0, 4.0, 0.25), (1, 15)), ((-4.0, 0.0, 0.375), (1, 30)), ((0.0, -4.0, 0.5), (1, 45)),
    # ring edges r = 8, 12, ..., 76 on the +x axis (sqrt is exact): each opens its ring
] + [((4.0 * k, 0.0, 0.01 * k), (k, 0)) for k in range(2, 20)] + [
    # just inside the edges: the float32 below 4 stays in ring 0, the float32 below 80 is ring 19, 80 itself is out
    ((0.0, float(np.nextafter(np.float32(4.0), np.float32(0.0))), 0.625), (0, 15)),
    ((0.0, float(F32_BELOW_80), 0.75), (19, 15)), ((80.0, 0.0, 9.0), None), ((0.0, -80.0, 9.0), None), ((60.0, 60.0, 9.0), None),
    # the last sector: just below the +x axis
    ((10.0, -1e-3, 0.875), (2, 59)),
    # below -2: the bin keeps its negative value; exactly -2 gives 0, like an empty bin
    ((21.0, 21.0, -3.5), (7, 7)), ((-21.0, 21.0, -2.0), (7, 22)),
    # duplicates in a bin: the maximum, whichever comes first
    ((-30.0, -30.0, 1.0), (10, 37)), ((-30.5, -30.0, 1.5), (10, 37)), ((-30.0, -30.5, -1.0), (10, 37)),
    # the origin: r = 0, atan2(0, 0) = 0
    ((0.0, 0.0, 2.5), (0, 0)),
    # non-finite coordinates are skipped, whichever column holds them
    ((np.nan, 1.0, 9.0), None), ((1.0, np.inf, 9.0), None), ((1.0, 1.0, np.nan), None), ((-np.inf, 1.0, 9.0), None), ((1.0, 1.0, -np.inf), None),
]


def crafted_cloud(cols):
    pts = np.zeros((len(CRAFTED), cols), np.float32)
    pts[:, 0:3] = np.array([p for p, _ in CRAFTED], np.float32)
    if cols == 4:
        pts[:, 3] = 77.0            # intensity is ignored
    return pts


def crafted_expected():
    """-> SC [20, 60] f32 the crafted cloud must give, written out by hand from the table"""
    img = np.full((lr.RINGS, lr.SECTORS), -np.inf, np.float32)
    for (x, y, z), at in CRAFTED:
        if at is not None:
            img[at] = max(img[at], np.float32(z) + np.float32(2.0))
    img[np.isneginf(img)] = 0
    return img


def random_cloud(n, seed, cols=4, r_max=95.0):
    """n points, a tenth of them beyond 80 m; no kept point lies within 1e-9 (in bin units) of a ring or sector edge, nor within 1e-9 m of r = 80"""
    rs = np.random.RandomState(seed)
    r, th = rs.uniform(0.3, r_max, n), rs.uniform(-np.pi, np.pi, n)
    pts = np.zeros((n, cols), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = r * np.cos(th), r * np.sin(th), rs.uniform(-4.0, 3.0, n)
    if cols == 4:
        pts[:, 3] = rs.uniform(0, 1, n)
    keep, fr, fs = lr.bins_of(pts)
    assert np.abs(fr - np.round(fr))[keep].min() > 1e-9 and np.abs(fs - np.round(fs))[keep].min() > 1e-9
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    assert np.abs(np.sqrt(x * x + y * y) - 80.0).min() > 1e-9
    return pts


@functools.lru_cache(maxsize=None)
def descriptor_batches():
    """-> {name: (pts [F, ld, C], n_pts [F])}: everything the descriptor tests run, for the host twin and for the device alike"""
    out = {}
    for cols in (3, 4):
        out["crafted c=%d" % cols] = pack([crafted_cloud(cols)])
        out["counts c=%d" % cols] = pack([random_cloud(n, 10 + n, cols) for n in (1, 255, 256, 257)])
    out["one empty of three"] = pack([random_cloud(300, 1), np.zeros((0, 4), np.float32), random_cloud(5000, 2)])   # more than one workgroup
    out["ld beyond n"] = pack([random_cloud(700, 3, 3)], ld=1000)
    return out


# ---- search images --------------------------------------------------------------------------------------------------------------------
def cloud_of_image(img):
    """SC [20, 60] -> a cloud with one point at the centre of every non-zero bin whose height gives back the bin's value"""
    ring, sector = np.nonzero(img)
    r, th = 4.0 * ring + 2.0, (sector + 0.5) * (2 * np.pi / lr.SECTORS)
    pts = np.zeros((len(ring), 3), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = r * np.cos(th), r * np.sin(th), img[ring, sector].astype(np.float32) - np.float32(2.0)
    return pts


def random_images(n, seed):
    """n sparse images: 5 - 40 % empty columns each, a third of the other bins empty, heights in (-1, 3) without zero -- multiples of
    1 / 256, so that a point's z = height - 2 gives the height back exactly"""
    rs = np.random.RandomState(seed)
    imgs = (rs.randint(51, 768, (n, lr.RINGS, lr.SECTORS)) / 256.0).astype(np.float32)
    neg = rs.uniform(size=imgs.shape) < 0.15
    imgs[neg] = -(rs.randint(1, 256, int(neg.sum())) / 256.0).astype(np.float32)
    imgs[rs.uniform(size=imgs.shape) < 0.33] = 0
    for f in range(n):
        empty = rs.permutation(lr.SECTORS)[:rs.randint(3, 25)]
        imgs[f][:, empty] = 0
    return imgs


def prepared(imgs):
    """images [N, 20, 60] -> (u [N,1200] f32, valid [N] u64) through the host twin, and the restatement's (u [N,1200] f64, valid [N,60] bool)"""
    pts, n_pts = pack([cloud_of_image(i) for i in imgs])
    sc, u, valid = host_scan_context(pts, n_pts)
    assert sc.tobytes() == np.ascontiguousarray(imgs, np.float32).tobytes()
    ref = [lr.prepare(i) for i in imgs]
    return u, valid, np.array([r[0] for r in ref]), np.array([r[1] for r in ref])


PLANTED = [(40, 5, 7), (52, 11, 59), (69, 30, 33), (61, 61 - 3, 1)]   # (i, j, s): frame i is frame j seen s sectors on, slightly perturbed


@functools.lru_cache(maxsize=None)
def search_images():
    """N = 70 random sparse images with the planted pairs -> (imgs, u f32, valid u64, u64 f64, valid bool)"""
    imgs = random_images(70, 7)
    rs = np.random.RandomState(8)
    for i, j, s in PLANTED:
        imgs[i] = np.roll(imgs[j], -s, axis=1)             # SC_i[c] = SC_j[c + s]
        imgs[i] = np.where(imgs[i] != 0, imgs[i] + (rs.randint(-5, 6, imgs[i].shape) / 256.0).astype(np.float32), 0)
    return (imgs,) + prepared(imgs)


# ---- search cases: what both the host twin (against the restatement) and the device (against the host twin) run --------------------------
def _small(n, seed):
    return prepared(random_images(n, seed))


@functools.lru_cache(maxsize=None)
def search_cases():
    """-> {name: (u f32, valid u64, u f64, valid bool, keyword arguments)}"""
    out = {}
    base = search_images()[1:]
    out["70 frames k=8"] = base + (dict(min_gap=3, k=8),)
    out["70 frames k=1"] = base + (dict(min_gap=3, k=1),)
    out["70 frames min_cols=40"] = base + (dict(min_gap=3, k=2, min_cols=40),)
    out["70 frames max_dist"] = base + (dict(min_gap=3, k=8, max_dist=0.5),)
    out["one frame"] = _small(1, 20) + (dict(min_gap=1, k=1),)
    out["N = min_gap"] = _small(5, 21) + (dict(min_gap=5, k=2),)
    out["N = min_gap + 1"] = _small(6, 22) + (dict(min_gap=5, k=2),)
    out["17 frames"] = _small(17, 23) + (dict(min_gap=1, k=3),)
    out["33 frames"] = _small(33, 24) + (dict(min_gap=1, k=8),)
    out["fewer than k"] = _small(6, 25) + (dict(min_gap=1, k=8),)
    imgs = random_images(9, 26)
    imgs[3] = 0                                             # an all-empty frame, as a candidate and as a query
    out["an empty frame"] = prepared(imgs) + (dict(min_gap=1, k=8),)
    return out


def identical_frames():
    """five times the same image: every candidate is equally far, the lower j wins"""
    return prepared(np.repeat(random_images(1, 27), 5, axis=0))


def period_30():
    """frame 0 repeats after 30 columns, frame 1 is frame 0 seen 40 sectors on: shifts 10 and 40 are equally good, 10 wins"""
    img = random_images(1, 28)[0]
    img[:, 30:] = img[:, :30]
    return prepared(np.stack([img, np.roll(img, -40, axis=1)]))
