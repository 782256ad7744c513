"""Designed inputs for the key point selection (csrc/ring.hip: k_kp_score -> k_kp_hist -> k_kp_gather -> k_kp_emit and the
single-workgroup fallback), and the plain statement of what it must select.

A *lattice image* holds its candidates on isolated centre pixels: every pixel is occupied and far enough (ring norm 20), the response
is zero except for one value at each centre, and no centre's 5 x 5 window holds another centre.  A centre's score is then
sqrt(v * v) in float32 -- which is v itself (a correctly rounded square root undoes a correctly rounded square when nothing
overflows) -- and every other pixel scores 0, so a test chooses the candidate count M, every score and every tie by writing them
down.  ``expected_selection`` is SphericalRing.py:192-218 on such a list: threshold in float64, stable ascending order, [-1025:-1].

A *cloud* does the same through the fused path: one point per pixel of the 64 x 1792 net area, 5 m away except at the centres, so
that only centres pass the 10 m gate; with ``clamp_respond_weights`` every centre's score is exactly 1.0.

``staged_cases`` / ``fused_recipes`` name every recipe the GPU tests use; tests/test_keypoint_select_host.py holds each of them
against the oracle and against the bins it claims to hit, so the GPU tests cannot pass on an input that missed its branch."""
import collections
import functools
import zlib

import numpy as np

NET_H, NET_W = 64, 1792
RING_H, RING_W = 69, 1800
KP_BIN_BASE, KP_BINS, SEL_N, KEEP = 0x3E00, 2048, 2048, 1025
STATE_NONE, STATE_LISTED, STATE_FALLBACK = 0, 1, 2      # cand_count[KP_CC_STATE]
BIN_0P2 = 0x4C                                           # float32(0.2) = 0x3E4CCCCD: the lowest bin a candidate can have
F32 = np.float32


# ---- lattice ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice():
    """[9392, 2] centre pixels (row, col): rows 8, 11 .. 53, columns 8, 11 .. 1781 without 53 <= col <= 66 (clear of the 56..63
    column quirk of SphericalRing.py:166-167 and of every window that touches it)."""
    rows = np.arange(8, 56, 3)
    cols = np.arange(8, 1784, 3)
    cols = cols[(cols < 53) | (cols > 66)]
    out = np.stack(np.meshgrid(rows, cols, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int64)
    out.setflags(write=False)
    return out


def pick(m, seed, rows_from=8):
    """m lattice centres in a seeded random order (``rows_from``: only rows >= that)."""
    lat = lattice()
    lat = lat[lat[:, 0] >= rows_from]
    assert m <= len(lat)
    return lat[np.random.RandomState(seed).permutation(len(lat))[:m]]


def _ring_base(h, w, channels):
    """Every pixel (12, 16, flat index * 2^-30, 0, 0): the float32 norm is exactly 20 (the third square vanishes against 400) and the
    xyz of every pixel is its own, so a key point row names its pixel."""
    ring = np.zeros((h, w, channels), F32)
    ring[..., 0] = 12.0
    ring[..., 1] = 16.0
    ring[..., 2] = (np.arange(h * w, dtype=np.float64).reshape(h, w) * 2.0 ** -30).astype(F32)
    return ring


def lattice_images(values, centres, ring_channels=5, chan=0):
    """-> (ring, counter, resp): ring [69,1800,5] + counter [69,1800] (demo mode) or ring [64,1792,3] + counter [64,1792] (batch
    mode), all occupied, norm 20; resp [64,1792,8] zero but for resp[r, c, chan] = values[i] at centre i."""
    assert ring_channels in (5, 3)
    h, w = (RING_H, RING_W) if ring_channels == 5 else (NET_H, NET_W)
    ring = _ring_base(h, w, ring_channels)
    counter = np.ones((h, w), np.int32)
    resp = np.zeros((NET_H, NET_W, 8), F32)
    centres = np.asarray(centres, np.int64).reshape(-1, 2)
    resp[centres[:, 0], centres[:, 1], chan] = np.asarray(values, F32)
    return ring, counter, resp


def scores_of(values):
    """The score of a centre that holds ``values[i]`` in one channel among zero neighbours, in NumPy float32."""
    v = np.asarray(values, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(v * v)


def kp_bin(scores):
    """ring.hip's kp_bin: clamp((float32 bits >> 16) - 0x3E00, 0, 2047)."""
    bits = np.ascontiguousarray(scores, F32).view(np.uint32).astype(np.int64)
    return np.clip((bits >> 16) - KP_BIN_BASE, 0, KP_BINS - 1)


def expected_selection(centres, scores, range_ok=None):
    """SphericalRing.py:192-218 on a candidate list -> key pixels [K, 2] (row, col): keep float64(score) > 0.2 (a NaN fails), sort
    ascending by (score, row * 1792 + col) -- the stable argsort of the flattened map --, take [-1025:-1]."""
    centres = np.asarray(centres, np.int64).reshape(-1, 2)
    scores = np.asarray(scores, F32)
    keep = scores.astype(np.float64) > 0.2
    if range_ok is not None:
        keep &= np.asarray(range_ok, bool)
    c, s = centres[keep], scores[keep]
    order = np.lexsort((c[:, 0] * NET_W + c[:, 1], s))
    return c[order][-KEEP:-1]


Design = collections.namedtuple("Design", "M K cut_bin nsel state nsel_word")


def design(scores):
    """What the selection kernels must find in a candidate list: M candidates, K = min(max(M, 1) - 1, 1024) key points and, for
    M > 1025, the bin of the 1025th largest key, the number of keys from that bin upwards and the branch that follows (listed while
    nsel <= 2048, else the fallback, which never counts the list: nsel_word 0)."""
    s = np.asarray(scores, F32)
    s = s[s.astype(np.float64) > 0.2]
    m = len(s)
    k = min(max(m, 1) - 1, 1024)
    if m <= KEEP:
        return Design(m, k, None, 0, STATE_NONE, 0)
    b = np.sort(kp_bin(s))[::-1]
    cut = int(b[KEEP - 1])
    nsel = int((b >= cut).sum())
    state = STATE_LISTED if nsel <= SEL_N else STATE_FALLBACK
    return Design(m, k, cut, nsel, state, nsel if state == STATE_LISTED else 0)


def oracle_keypoints(orc, ring, cnt, resp):
    """The oracle's orc_keypoints without GetKeyPtsByAE's `K > 50` assert -> (key points [K,3], key pixels [K,2], score map)."""
    import ctypes as C
    ring, cnt, resp = (np.ascontiguousarray(a, t) for a, t in ((ring, F32), (cnt, np.int32), (resp, F32)))
    kpix = np.zeros((1024, 2), np.int64)
    kpts = np.zeros((1024, 3), F32)
    score = np.zeros((NET_H, NET_W), F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    k = orc.lib().orc_keypoints(p(ring), C.c_int(ring.shape[1]), C.c_int(ring.shape[2]), p(cnt), C.c_int(cnt.shape[1]), p(resp),
                                p(kpix), p(kpts), p(score))
    return kpts[:k].copy(), kpix[:k].copy(), score


# ---- score lists ----------------------------------------------------------------------------------------------------------------------
def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def distinct(rs, n, lo, hi, log=False):
    """n float32 values in [lo, hi) with pairwise different scores, in random order."""
    u = rs.uniform(np.log(lo), np.log(hi), 2 * n + 64) if log else rs.uniform(lo, hi, 2 * n + 64)
    v = (np.exp(u) if log else u).astype(F32)
    s = scores_of(v)
    v = v[(s >= F32(lo)) & (s < F32(hi))]
    _, first = np.unique(scores_of(v), return_index=True)
    v = v[rs.permutation(first)]
    assert len(v) >= n
    return v[:n]


def in_bin(rs, n, b):
    """n float32 values with pairwise different scores, all in histogram bin b (0 < b < 2047: 65536 floats wide)."""
    low = rs.choice(65536, n, replace=False).astype(np.uint32)
    v = (np.uint32((KP_BIN_BASE + b) << 16) + low).view(F32)
    assert (kp_bin(scores_of(v)) == b).all() and len(np.unique(scores_of(v))) == n
    return v


Case = collections.namedtuple("Case", "name values centres scores claim")
COUNTS = (0, 1, 2, 51, 52, 1024, 1025, 1026, 1027, 3000, 9000)
TIES = (1026, 2047, 2048, 2049, 5000)
BIN_2P5 = 0x4020 - KP_BIN_BASE   # 544: float32(2.5) = 0x40200000
V8160 = F32(8160.0)              # 0x45FF0000: the first score of bin 2047, which every larger score shares
BELOW_8160 = np.nextafter(V8160, F32(0))


def _case(name, values, claim=None, scores=None):
    values = np.asarray(values, F32)
    rs = _rs(name + "/centres")
    centres = pick(len(values), rs.randint(1 << 30))
    return Case(name, values, centres, scores_of(values) if scores is None else np.asarray(scores, F32), dict(claim or {}))


def _build_cases():
    cases = []
    # ---- counts: distinct random scores in (0.25, 64)
    for m in COUNTS:
        rs = _rs("count%d" % m)
        cases.append(_case("count_%d" % m, distinct(rs, m, 0.25, 64.0) if m else np.zeros(0, F32), dict(M=m, K=min(max(m, 1) - 1, 1024))))
    # ---- ties against the list capacity: the order is by flat index alone
    for m in TIES:
        cases.append(_case("ties_%d" % m, np.full(m, 2.5, F32),
                           dict(M=m, cut_bin=BIN_2P5, nsel=m, state=STATE_LISTED if m <= SEL_N else STATE_FALLBACK)))
    for nsel in (2048, 2049):   # 1 000 distinct scores above a bin of equal keys that brings nsel to exactly 2048 / 2049
        rs = _rs("nsel%d" % nsel)
        v = np.concatenate([distinct(rs, 1000, 4.0, 64.0), np.full(nsel - 1000, 2.5, F32), distinct(rs, 300, 0.25, 2.0)])
        cases.append(_case("nsel_%d" % nsel, v, dict(M=nsel + 300, cut_bin=BIN_2P5, nsel=nsel,
                                                     state=STATE_LISTED if nsel <= SEL_N else STATE_FALLBACK)))
    # ---- cut bin parity: bins 512 = [2.0, 2.015625) and 513 = [2.015625, 2.03125) belong to one thread (t = 256)
    rs = _rs("parity")
    cases.append(_case("cut_odd_513", np.concatenate([distinct(rs, 900, 4.0, 64.0), in_bin(rs, 400, 513), distinct(rs, 300, 0.25, 2.0)]),
                       dict(M=1600, cut_bin=513, nsel=1300, state=STATE_LISTED)))
    cases.append(_case("cut_even_512", np.concatenate([distinct(rs, 800, 4.0, 64.0), in_bin(rs, 100, 513), in_bin(rs, 400, 512),
                                                       distinct(rs, 300, 0.25, 2.0)]),
                       dict(M=1600, cut_bin=512, nsel=1300, state=STATE_LISTED)))
    cases.append(_case("cut_even_512_partner_holds_1024", np.concatenate([in_bin(rs, 1024, 513), in_bin(rs, 400, 512), distinct(rs, 300, 0.25, 2.0)]),
                       dict(M=1724, cut_bin=512, nsel=1424, state=STATE_LISTED)))
    cases.append(_case("cut_odd_513_holds_1025", np.concatenate([in_bin(rs, 1025, 513), in_bin(rs, 400, 512), distinct(rs, 300, 0.25, 2.0)]),
                       dict(M=1725, cut_bin=513, nsel=1025, state=STATE_LISTED)))
    # ---- the last bin: `thresh` is only a lower bound there, the rank / radix step orders what the bins cannot.  (A float32 score is
    #      sqrt of a finite float32 sum, so it ends at 1.8e19, inside the [8160, 3e38] of bin 2047.)
    rs = _rs("last")
    cases.append(_case("last_bin_listed", np.concatenate([distinct(rs, 1500, 8160.0, 1.8e19, log=True), distinct(rs, 500, 0.25, 64.0)]),
                       dict(M=2000, cut_bin=2047, nsel=1500, state=STATE_LISTED)))
    cases.append(_case("last_bin_fallback", np.concatenate([distinct(rs, 2100, 8160.0, 1.8e19, log=True), distinct(rs, 500, 0.25, 64.0)]),
                       dict(M=2600, cut_bin=2047, nsel=2100, state=STATE_FALLBACK)))
    low = np.concatenate([[BELOW_8160], in_bin(rs, 199, 2046), distinct(rs, 300, 64.0, 4000.0)])   # bin 2046 = [8128, 8160)
    for n_top, cut, nsel in ((1024, 2046, 1224), (1025, 2047, 1025)):   # the 1025th largest: nextafter below 8160.0 / 8160.0 itself
        top = distinct(rs, n_top - 1, 8161.0, 1.0e6, log=True)
        cases.append(_case("edge_8160_top%d" % n_top, np.concatenate([[V8160], top, low]),
                           dict(M=n_top + 500, cut_bin=cut, nsel=nsel, state=STATE_LISTED)))
    # ---- the 0.2 threshold is compared in float64: float32(0.2) = 0.2000000029... is a candidate, its lower neighbour is not
    t = F32(0.2)
    three = np.array([t, np.nextafter(t, F32(0)), np.nextafter(t, F32(1))], F32)
    rs = _rs("threshold")
    cases.append(_case("threshold_among_1100", np.concatenate([three, distinct(rs, 1100, 0.25, 64.0)]), dict(M=1102)))
    cases.append(_case("threshold_cut_in_bin_0x4c", np.concatenate([three, distinct(rs, 1024, 0.25, 64.0)]),
                       dict(M=1026, cut_bin=BIN_0P2, nsel=1026, state=STATE_LISTED)))
    # ---- +inf in a pixel's own response: inf - inf = NaN in the reference's self term, the pixel is no candidate
    for n_inf in (1, 3):
        rs = _rs("inf%d" % n_inf)
        v = np.concatenate([np.full(n_inf, np.inf, F32), distinct(rs, 1100, 0.25, 64.0)])
        s = scores_of(v)
        s[:n_inf] = np.nan
        cases.append(_case("inf_at_self_%d" % n_inf, v, dict(M=1100), scores=s))
    return collections.OrderedDict((c.name, c) for c in cases)


@functools.lru_cache(maxsize=None)
def staged_cases():
    """name -> Case(values, centres, scores, claim): every lattice recipe of tests/test_keypoint_select_gpu.py part A."""
    return _build_cases()


# ---- gates: hand-placed probes on top of a lattice of 120 ordinary candidates -----------------------------------------------------------
Probe = collections.namedtuple("Probe", "name row col candidate score")


def pairwise8(v):
    """float32 norm of eight equal differences v in NumPy's pairwise order."""
    s = F32(v) * F32(v)
    return np.sqrt(((s + s) + (s + s)) + ((s + s) + (s + s)))


def ring_norm(px):
    """SphericalRing.py:197: float32 squares, summed in channel order."""
    px = np.asarray(px, F32)
    d2 = px[0] * px[0]
    for c in range(1, len(px)):
        d2 = d2 + px[c] * px[c]
    return np.sqrt(d2)


def gate_images(ring_channels):
    """-> (ring, counter, resp, probes, base): 120 ordinary lattice candidates (``base`` = (centres, scores), scores in (1, 2)) and
    one probe per gate, each with its own score in [3, 5) and the statement whether it is a candidate:
      occupancy   exactly 4 / exactly 5 occupied neighbours (:186), an unoccupied centre (:163)
      range       ring norm just below 10 / exactly 10.0 over the ring's channels (:197-198; with 5 channels intensity and range count)
      borders     rows 7 / 8 / 55 / 56, columns 7 / 8 / 55 / 56 / 63 / 64 / 1783 / 1784 (:163-167 with its 56..63 quirk, :210-213)
      channels    a value in channel 5 only, and the same value in all 8 channels."""
    rs = _rs("gates")
    lat = lattice()
    inner = lat[(lat[:, 0] >= 17) & (lat[:, 0] <= 44) & (lat[:, 1] >= 200) & (lat[:, 1] <= 1600)]
    bc = inner[rs.permutation(len(inner))[:120]]
    bv = distinct(rs, 120, 1.0, 2.0)
    ring, counter, resp = lattice_images(bv, bc, ring_channels)
    probes = []

    def put(name, row, col, candidate, chans=(0,), occupied=None, px=None, unoccupied=False):
        v = F32(3.0 + len(probes) / 16.0)
        resp[row, col, list(chans)] = v
        if occupied is not None:   # only these neighbours of the 5 x 5 window stay occupied
            counter[row - 2:row + 3, col - 2:col + 3] = 0
            counter[row, col] = 1
            for dy, dx in occupied:
                counter[row + dy, col + dx] = 1
        if unoccupied:
            counter[row, col] = 0
        if px is not None:
            ring[row, col, :] = np.asarray(px, F32)
            assert (ring_norm(ring[row, col]) >= F32(10.0)) == candidate
        probes.append(Probe(name, row, col, candidate, pairwise8(v) if len(chans) == 8 else scores_of(v)))

    nb = [(-2, -2), (-1, 1), (0, 2), (2, 0), (1, -2)]
    put("occupied_4", 11, 100, False, occupied=nb[:4])
    put("occupied_5", 11, 120, True, occupied=nb)
    put("unoccupied_centre", 11, 140, False, unoccupied=True)
    just_below = np.nextafter(F32(10.0), F32(0))
    zeros = [0.0] * (ring_channels - 1)
    put("norm_just_below_10", 11, 160, False, px=[just_below] + zeros)
    put("norm_exactly_10", 11, 180, True, px=[10.0] + zeros)
    put("norm_6_8_0", 11, 200, True, px=[6.0, 8.0, 0.0] + zeros[2:])
    if ring_channels == 5:   # xyz alone (norm 6) would fail: the intensity and the range channel make the 10
        put("norm_with_range_channel", 11, 220, True, px=[6.0, 0.0, 0.0, 0.0, 8.0])
        put("norm_with_intensity_channel", 11, 240, True, px=[0.0, 6.0, 0.0, 8.0, 0.0])
        put("norm_with_range_channel_short", 11, 260, False, px=[6.0, 0.0, 0.0, 0.0, 7.99])
    else:
        put("norm_xyz_6", 11, 220, False, px=[6.0, 0.0, 0.0])
    for row, col, ok in ((7, 300, False), (8, 310, True), (55, 320, True), (56, 330, False)):
        put("row_%d" % row, row, col, ok)
    for k, (col, ok) in enumerate(((7, False), (8, True), (55, True), (56, False), (63, False), (64, True), (1783, True), (1784, False))):
        put("col_%d" % col, 12 + 6 * (k % 2) + 12 * (k // 4), col, ok)     # neighbours in column, never in one window
    put("channel_5_only", 50, 400, True, chans=(5,))
    put("all_8_channels", 50, 420, True, chans=tuple(range(8)))
    return ring, counter, resp, probes, (bc, scores_of(bv))


def gate_expected(probes, base):
    """expected_selection over the base candidates and the probes that are candidates."""
    ok = [p for p in probes if p.candidate]
    centres = np.concatenate([base[0], np.array([(p.row, p.col) for p in ok], np.int64).reshape(-1, 2)])
    scores = np.concatenate([base[1], np.array([p.score for p in ok], F32)])
    return expected_selection(centres, scores)


# ---- clouds for the fused path -----------------------------------------------------------------------------------------------------------
AZ_RES = 0.20 * np.pi / 180.0                                    # SphericalRing.py:35,:48
V_DOWN, V_UP = -24.8 * np.pi / 180.0, 2.0 * np.pi / 180.0         # :49-50
V_RES = (V_UP - V_DOWN) / 63.0                                    # :51
V_OFF = -V_DOWN / V_RES                                           # :52


def cloud(centres, ranges, background=5.0, seed=7):
    """-> [64 * 1792, 4] f32: one point per pixel of the 64 x 1792 net area at the pixel's centre direction (the inverse of
    ProjectPC2SphericalRing: theta = pi - (col + 0.5) az_res, elevation = ((69 - row) + 0.5 - v_off) v_res), ``background`` metres away,
    ``ranges[i]`` metres at centre i, intensity 0.5, rows shuffled by a fixed seed."""
    rng = np.full((NET_H, NET_W), float(background), np.float64)
    centres = np.asarray(centres, np.int64).reshape(-1, 2)
    rng[centres[:, 0], centres[:, 1]] = np.asarray(ranges, np.float64)
    row, col = np.meshgrid(np.arange(NET_H), np.arange(NET_W), indexing="ij")
    theta = np.pi - (col + 0.5) * AZ_RES
    el = ((RING_H - row) + 0.5 - V_OFF) * V_RES
    pc = np.stack([rng * np.cos(el) * np.cos(theta), rng * np.cos(el) * np.sin(theta), rng * np.sin(el), np.full_like(rng, 0.5)], axis=-1)
    pc = pc.reshape(-1, 4).astype(F32)
    return np.ascontiguousarray(pc[np.random.RandomState(seed).permutation(len(pc))])


def clamp_respond_weights():
    """Response weights (Keras shapes) whose channel 0 is clamp(-z - 2, 0, 1) and whose other channels are 0: two hidden units
    relu(-z - 2) and relu(-z - 3) on the centre tap, subtracted.  On ``cloud`` with centres in rows >= 30 and ranges in [40, 60] that is
    exactly 1.0 at a centre (z <= -5.5) and 0.0 on the background (z >= -2): exact score ties through the fused path."""
    w1, b1 = np.zeros((3, 3, 3, 32), F32), np.zeros(32, F32)
    w2, b2 = np.zeros((1, 1, 32, 8), F32), np.zeros(8, F32)
    w1[1, 1, 2, 0], b1[0] = -1.0, -2.0
    w1[1, 1, 2, 1], b1[1] = -1.0, -3.0
    w2[0, 0, 0, 0], w2[0, 0, 1, 0] = 1.0, -1.0
    return [w1, b1, w2, b2]


SHIPPED_M = (0, 1, 2, 51, 52, 1024, 1025, 1026, 3000)
CLAMP_M = (0, 1, 52, 1025, 1026, 2048, 2049, 3000)
CLAMP_ROWS_FROM = 30


@functools.lru_cache(maxsize=None)
def fused_cloud(kind, m):
    """kind "shipped": m centres anywhere on the lattice, ranges ~ U(12, 60) (under the shipped response weights the candidates are
    exactly the centres: the background fails the 10 m gate); kind "clamp": m centres in rows >= 30, ranges ~ U(40, 60), for
    ``clamp_respond_weights`` (every score 1.0).  -> (cloud, centres), read-only."""
    rs = _rs("cloud/%s/%d" % (kind, m))
    if kind == "shipped":
        centres, ranges = pick(m, rs.randint(1 << 30)), rs.uniform(12.0, 60.0, m)
    else:
        centres, ranges = pick(m, rs.randint(1 << 30), rows_from=CLAMP_ROWS_FROM), rs.uniform(40.0, 60.0, m)
    pc = cloud(centres, ranges)
    pc.setflags(write=False)
    centres.setflags(write=False)
    return pc, centres


def fused_recipes():
    return [("shipped", m) for m in SHIPPED_M] + [("clamp", m) for m in CLAMP_M]
