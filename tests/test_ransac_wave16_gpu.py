"""The RANSAC hypothesis kernels at sixteen and at four hypotheses per wavefront (csrc/ransac.hip, wave_hypotheses<CERT, PW>), and
k_respond_mfma at 88 registers (csrc/ring.hip).  DESIGN.md 5.2c.

Lane l of a wavefront derives trial0 + (l & (PW - 1)); PW / 4 scoring passes of four poses each.  At sixteen, 64 trials per workgroup --
500 does not divide by 64, the last workgroup holds 52 and its last wavefront 4; at four, the last wavefront of the last workgroup holds
none.  A call of fewer than four pairs runs four per wavefront (the shortest launch), a call of four or more sixteen (a quarter of the
wavefronts): the single calls below (Engine.match_pose, match_pose_exact, ransac) pin the former, the table of all seven sets through
caelo_register_pairs (a set per slice of the table) the latter, and the two leave the same records and results.

Crafted pair sets of N in {5, 63, 64, 65, 1000, 1024} key points: seeded descriptors that match one to one, a known rigid motion on about
two thirds of the pairs (so that about a fifth of the 4-samples are all inliers and reach leastInliers) and outliers on the rest; one set
whose first level fails.  In every set trial 7 and trial 498 (the tail wavefront) sample three collinear pairs (rank 2: two candidate
poses) and trial 11 four collinear ones (rank 1: no bound).

Per set, computed once (fixture `run`) and never written: the certificate record, the host half's result, the device's own finish, and on
the host the exact inlier count of every hypothesis by the host half's SolveRT (caelo_host_solve_rt) and Match.py:190-194 in NumPy.
tests/golden/ransac_wave16_parent.npz holds hi / idx / hi_up / idx_up of the same sets as the kernels wrote them before either form
existed (four hypotheses per wavefront, each derived by sixteen lanes): every hypothesis is still the same instruction sequence on the
same operands, so the records are equal.

The response layer against the oracle's orc_respond, bit for bit, on the clouds of tests/kp_eligible_ref.py -- every pixel eligible, none,
one eligible pixel at each corner case of the map, the gate rows and columns: the staged caelo_respond (no map: all 64 rows and 56 blocks,
so rows 0 and 63 with their halo rows outside the image and blocks 0 and 55 with their halo columns), and the fused path on the blocks
the map selects, untouched elsewhere.  A map is written by k_ring_fill only and its bits lie in the rule's rows 8..55, so a single bit
in row 0 or 63 cannot be made; the staged call is what reaches those rows.  (These clouds put a point in every pixel of row 0: the
kernel used to read 0 for the pixel left of a block in image row 0 -- its offset is negative before the block's column is added, and
negative meant "no element" -- which real scans, empty up there, never showed.  DESIGN.md 5.2c.)"""
import os

import numpy as np
import pytest
import torch

import kp_eligible_ref as ker
import kp_images as kpi
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = (5, 63, 64, 65, 1000, 1024)
CASES = tuple("n%d" % n for n in SIZES) + ("fail",)
TRIALS = 500
T_RANK2, T_RANK1, T_RANK2_TAIL = 7, 11, 498
FIELDS = ("R", "T", "R_ransac", "T_ransac", "threshold", "success", "iterations", "n_inliers", "n_pairs")
# a motion that is exact in float32 on coordinates that are multiples of 1/1024: a quarter turn about z and a dyadic shift, so that
# the collinear triple is collinear in both frames to the last bit
R_GT = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
T_GT = np.array([2.0, -1.0, 0.5], np.float32)


def _q(x):
    return (np.round(np.asarray(x, np.float64) * 1024.0) / 1024.0).astype(np.float32)


def make_case(name):
    """-> dict(N, rows_a, rows_b [1024,64] f32, draws [6000] f64).  Frame b's key point i matches frame a's perm[i]."""
    fail = name == "fail"
    N = 1000 if fail else int(name[1:])
    rng = np.random.RandomState(7100 + (N if not fail else 4))
    half = 4.0 if fail else 25.0
    pb = _q(rng.uniform(-half, half, (N, 3)) * np.array([1, 1, 0.2]))
    pb[0:3] = np.array([1.0, 2.0, 0.5], np.float32) + np.arange(3, dtype=np.float32)[:, None] * np.array([0.5, 0.25, 0.125], np.float32)
    pa = pb @ R_GT.T + T_GT   # exact
    inl = rng.random_sample(N) < (0.62 if fail else 0.67)
    inl[0:3] = True
    if N == 5:
        # five pairs, four draws with replacement: four samples in five repeat a pair, and on such a rank-deficient sample the kernels'
        # float64 fit and the reference's float32 SVD may pick different candidate poses.  All five are consistent and the draws' seed
        # makes trial 0 a sample of four distinct, non-coplanar pairs: it counts 5 = N in either arithmetic and nothing later can exceed it
        inl[:] = True
    if fail:
        # every consistent pair is off by 0.62 .. 0.75 m in a random direction: none within 0.4 m of any pose that fits four of them
        # well, most within 0.8 m
        d = rng.standard_normal((N, 3))
        d *= (rng.uniform(0.62, 0.75, N) / np.linalg.norm(d, axis=1))[:, None]
    else:
        d = rng.standard_normal((N, 3)) * 0.005
    d[0:3] = 0.0
    pa = np.where(inl[:, None], _q(pa + d), _q(rng.uniform(-half, half, (N, 3)) * np.array([1, 1, 0.2])))
    perm = rng.permutation(N)
    desc_b = rng.standard_normal((N, 60)).astype(np.float32)
    rows_a = np.zeros((1024, 64), np.float32)
    rows_b = np.zeros((1024, 64), np.float32)
    rows_b[:N, 0:60], rows_b[:N, 60:63], rows_b[:N, 63] = desc_b, pb, 1.0
    rows_a[perm, 0:60] = desc_b + rng.standard_normal((N, 60)).astype(np.float32) * 1e-3
    rows_a[perm, 60:63] = pa
    rows_a[:N, 63] = 1.0
    draws = np.random.RandomState(7216 if N == 5 else 7200 + N + (1 if fail else 0)).random_sample(6000)
    far = min(N - 1, 9)
    for lvl in range(3):   # the crafted samples, in every level's draws
        for t, s in ((T_RANK2, (0, 1, 2, far)), (T_RANK1, (0, 1, 2, 1)), (T_RANK2_TAIL, (2, 0, far, 1))):
            draws[lvl * 2000 + 4 * t: lvl * 2000 + 4 * t + 4] = (np.array(s) + 0.5) / N
    return dict(N=N, rows_a=rows_a, rows_b=rows_b, draws=draws, perm=perm)


def host_counts(P0, P1, draws, level):
    """The exact inlier count of every hypothesis of one level, as the reference evaluates it (Match.py:182-194), and its inlier sets."""
    from caelo import hostexact
    N = P0.shape[0]
    thr = np.float64(0.4 * (1 << level))
    counts = np.zeros(TRIALS, np.int64)
    sets = np.zeros((TRIALS, N), bool)
    for t in range(TRIALS):
        idx = np.array(draws[level * 2000 + 4 * t: level * 2000 + 4 * t + 4] * N, dtype=np.int32)
        R, T, _ = hostexact.solve_rt(P0[idx], P1[idx])
        dists = np.linalg.norm(P0 - (np.dot(R, P1.T) + T).T, axis=1)
        sets[t] = dists < thr
        counts[t] = int(sets[t].sum())
    return counts, sets


def replay(counts_by_level, N):
    """Match.py:166-169,:181-214 over the counts -> (level, iterations, success, best trial of that level or -1)."""
    least, min_success = min(100, int(0.2 * N)), 0.25 * N
    for level in range(3):
        c, cur, best, it, ok = counts_by_level(level), 0, -1, 0, False
        while it < 100 or (it < TRIALS and cur < min_success):
            if c[it] >= least:
                if c[it] > cur:
                    cur, best = int(c[it]), it
                ok = True
            it += 1
        if ok or level == 2:
            return level, it, ok, best


@pytest.fixture(scope="module")
def run(engine):
    """name -> everything the tests below look at, computed once per set."""
    from caelo import _ffi, hostexact
    from caelo.engine import FrameFeatures
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        c = make_case(name)
        dev, N = engine.device, c["N"]
        faults0, violations0 = engine.lane_faults(), engine.bound_violations()   # (process-wide counters: other tests raise them on purpose)
        nk = torch.tensor([N], dtype=torch.int32, device=dev)
        fa = FrameFeatures(torch.from_numpy(c["rows_a"]).to(dev), None, nk, None, None)
        fb = FrameFeatures(torch.from_numpy(c["rows_b"]).to(dev), None, nk.clone(), None, None)
        rand = torch.from_numpy(c["draws"]).to(dev)
        exact, exact_mask, idx = engine.match_pose_exact(fa, fb, rand, c["draws"])
        cert = engine.new_cert(1)   # the record itself: the staged calls match_pose_exact makes
        engine.ransac(fa.key_pts, fb.key_pts, idx, rand, fb.n_key, cert=cert[0])
        rec = np.frombuffer(cert.cpu().numpy().tobytes(), dtype=_ffi.CERT_DTYPE)[0]
        r, m, idx2 = engine.match_pose(fa, fb, rand)
        own = np.frombuffer(r.cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE)[0]
        pair_idx = idx.cpu().numpy()
        assert np.array_equal(pair_idx[:N], c["perm"]) and torch.equal(idx, idx2), "the crafted descriptors match one to one"
        P0 = np.ascontiguousarray(c["rows_a"][pair_idx[:N], 60:63])
        P1 = np.ascontiguousarray(c["rows_b"][:N, 60:63])
        levels = {}
        out = dict(c, P0=P0, P1=P1, rec=rec, exact=exact, exact_mask=np.asarray(exact_mask), own=own, own_mask=m.cpu().numpy(),
                   level=lambda l: levels.setdefault(l, host_counts(P0, P1, c["draws"], l)),
                   exhaustive=hostexact.ransac(P0, P1, c["draws"]), faults=engine.lane_faults() - faults0, violations=engine.bound_violations() - violations0)
        cache[name] = out
        return out
    return get


@pytest.fixture(scope="module")
def parent_records():
    return np.load(os.path.join(GOLDEN, "ransac_wave16_parent.npz"))


@pytest.mark.parametrize("name", CASES)
def test_record_pins_the_lane_to_trial_mapping(run, name):
    """idx[t] = int32(rnd[t] * N) for every trial, the tail workgroup's 52 included; nothing is written past trial 499."""
    c = run(name)
    want = (c["draws"][:4 * TRIALS].reshape(TRIALS, 4) * c["N"]).astype(np.int32)
    assert np.array_equal(c["rec"]["idx"][:TRIALS], want)
    assert not c["rec"]["idx"][TRIALS:].any() and not c["rec"]["hi"][TRIALS:].any()
    assert c["rec"]["n_pairs"] == c["N"] and c["rec"]["magic"] == __import__("caelo")._ffi.CERT_MAGIC
    assert c["faults"] == 0


@pytest.mark.parametrize("name", CASES)
def test_bounds_cover_the_exact_counts(run, name):
    """hi[t] >= the host's exact count of hypothesis t, for all 500; rank 1 has no bound; the host half met no violation."""
    c = run(name)
    counts, _ = c["level"](0)
    hi = c["rec"]["hi"][:TRIALS]
    print("%s: %d of 500 exact counts reach leastInliers, max %d, hi - count in [%d, %d]" % (
        name, int((counts >= min(100, int(0.2 * c["N"]))).sum()), counts.max(), (hi - counts).min(), (hi - counts).max()))
    assert (hi >= counts).all(), "trials %s" % np.flatnonzero(hi < counts)[:8]
    assert hi[T_RANK1] == c["N"]
    assert (hi <= c["N"]).all()
    assert c["violations"] == 0 and c["faults"] == 0


@pytest.mark.parametrize("name", CASES)
def test_records_are_the_four_per_wavefront_kernels_bits(run, parent_records, name):
    c = run(name)
    for f in ("hi", "idx", "levels_up", "hi_up", "idx_up"):
        assert np.array_equal(c["rec"][f], parent_records["%s_%s" % (name, f)]), f


@pytest.mark.parametrize("name", CASES)
def test_exact_result_equals_the_exhaustive_host_ransac(run, name):
    c = run(name)
    want, want_mask, _ = c["exhaustive"]
    for f in FIELDS:
        assert np.array_equal(c["exact"][f], want[f]) and c["exact"][f].tobytes() == want[f].tobytes(), f
    assert np.array_equal(c["exact_mask"][:c["N"]].astype(bool), want_mask) and not c["exact_mask"][c["N"]:].any()
    assert c["violations"] == 0 and c["faults"] == 0


@pytest.mark.parametrize("name", CASES)
def test_device_finish_equals_the_replay_over_exact_counts(run, name):
    """No set is skipped: with the seeds above no exact count sits on leastInliers or brings the running maximum onto 0.25 N (asserted
    here on the host's counts), so the kernels' float64 fits must decide every level like the reference."""
    c = run(name)
    N = c["N"]
    least = min(100, int(0.2 * N))
    level, it, ok, best = replay(lambda l: c["level"](l)[0], N)
    for l in range(level + 1):   # (a failed level is read to its end, the deciding one up to its last iteration)
        counts = c["level"](l)[0][:it if l == level else TRIALS]
        assert not np.isin(counts, (least - 1, least)).any() or least <= 1, "a count on leastInliers: choose another seed"
        pm = np.maximum.accumulate(np.where(counts >= least, counts, 0))
        assert not ((pm >= 0.25 * N - 1) & (pm < 0.25 * N + 1)).any(), "a running maximum on 0.25 N: choose another seed"
    own = c["own"]
    assert (int(own["success"]) != 0) == ok and int(own["iterations"]) == it and int(own["n_pairs"]) == N
    assert float(own["threshold"]) == np.float32(0.4 * (1 << level))
    assert int(own["best_trial"]) == (level * TRIALS + best if best >= 0 else -1)
    inl = c["level"](level)[1][best] if best >= 0 else np.zeros(N, bool)
    assert np.array_equal(c["own_mask"][:N].astype(bool), inl) and int(own["n_inliers"]) == int(inl.sum())
    assert not c["own_mask"][N:].any()


def test_failing_first_level_leaves_the_upper_levels_bounds(run):
    """All 500 counts of the 0.4 m level below leastInliers, 0.8 m accepts: levels_up = 1 and idx_up / hi_up hold for both upper levels
    as idx / hi do for the first."""
    c = run("fail")
    N, rec = c["N"], c["rec"]
    c0, _ = c["level"](0)
    c1, _ = c["level"](1)
    assert c0.max() < 100 and (c1 >= 100).any()
    assert int(rec["levels_up"]) == 1 and float(c["exact"]["threshold"]) == np.float32(0.8) and int(c["exact"]["success"]) == 1
    for l in (1, 2):
        want = (c["draws"][l * 2000: l * 2000 + 4 * TRIALS].reshape(TRIALS, 4) * N).astype(np.int32)
        assert np.array_equal(rec["idx_up"][l - 1][:TRIALS], want)
        counts, _ = c["level"](l)
        hi = rec["hi_up"][l - 1][:TRIALS]
        assert (hi >= counts).all() and (hi <= N).all() and hi[T_RANK1] == N
        assert not rec["idx_up"][l - 1][TRIALS:].any() and not rec["hi_up"][l - 1][TRIALS:].any()
    assert c["violations"] == 0 and c["faults"] == 0


@pytest.mark.parametrize("name", ["n5", "n64", "n1000", "fail"])
def test_rank_deficient_samples(run, name):
    """Three collinear pairs and a fourth (rank 2): the bound is the larger of the two candidate poses' -- at least the count of either
    pose of the quarter turn and of its mirror image through the sample's plane, counted here in float64 with a millimetre to spare; four
    collinear pairs (rank 1): N."""
    c = run(name)
    N, P0, P1 = c["N"], c["P0"].astype(np.float64), c["P1"].astype(np.float64)
    hi = c["rec"]["hi"]
    assert hi[T_RANK1] == N
    for t in (T_RANK2, T_RANK2_TAIL):
        idx = c["rec"]["idx"][t]
        a, b = P0[idx] - P0[idx].mean(0), P1[idx] - P1[idx].mean(0)
        U, S, Vt = np.linalg.svd(b.T @ a)
        assert S[2] <= 1e-9 * S[0] < S[1], "the crafted sample has rank 2"
        for sgn in (1.0, -1.0):
            R = Vt.T @ np.diag([1.0, 1.0, sgn]) @ U.T
            T = P0[idx].mean(0) - R @ P1[idx].mean(0)
            n = int((np.linalg.norm(P0 - (P1 @ R.T + T), axis=1) < 0.4 - 1e-3).sum())
            assert hi[t] >= n, (t, sgn, int(hi[t]), n)



def test_table_of_seven_scores_sixteen_per_wavefront(engine, run, parent_records):
    """All seven sets as ONE table (caelo_register_pairs: a set per slice, sixteen hypotheses per wavefront) leave the records, the
    kernels' own results and the masks of the seven single calls (four per wavefront)."""
    from caelo import _ffi
    cs = [run(name) for name in CASES]
    dev, P = engine.device, len(CASES)
    faults0 = engine.lane_faults()
    rows = torch.from_numpy(np.stack([r for c in cs for r in (c["rows_a"], c["rows_b"])])).to(dev)
    nk = torch.tensor([c["N"] for c in cs for _ in (0, 1)], dtype=torch.int32, device=dev)
    pairs = torch.tensor([(2 * i, 2 * i + 1) for i in range(P)], dtype=torch.int32, device=dev)
    rand = torch.from_numpy(np.stack([c["draws"] for c in cs])).to(dev)
    ws = engine._ws("register_pairs", int(engine.lib.caelo_register_pairs_ws_bytes(P)))

    def call(cert, res, mask):
        idx = engine.zeros((P, 1024), torch.int64)
        p = lambda t: None if t is None else t.data_ptr()
        _ffi.check(engine.lib.caelo_register_pairs(engine.ctx, rows.data_ptr(), rows.shape[0], nk.data_ptr(), pairs.data_ptr(), P, rand.data_ptr(),
                                                   idx.data_ptr(), p(res), p(mask), p(cert), ws.data_ptr(), engine.stream))
        torch.cuda.synchronize()
        return idx.cpu().numpy()

    cert = engine.new_cert(P)
    idx = call(cert, None, None)
    recs = np.frombuffer(cert.cpu().numpy().tobytes(), dtype=_ffi.CERT_DTYPE)
    for i, (name, c) in enumerate(zip(CASES, cs)):
        assert np.array_equal(idx[i, :c["N"]], c["perm"])
        for f in ("n_pairs", "hi", "idx", "levels_up", "hi_up", "idx_up", "p0", "p1"):
            assert np.array_equal(recs[i][f], c["rec"][f]), (name, f)
        for f in ("hi", "idx", "levels_up", "hi_up", "idx_up"):
            assert np.array_equal(recs[i][f], parent_records["%s_%s" % (name, f)]), (name, f)
    res = engine.zeros((P, _ffi.POSE_DTYPE.itemsize), torch.uint8)
    mask = engine.zeros((P, 1024), torch.uint8)
    call(None, res, mask)
    own = np.frombuffer(res.cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE)
    for i, (name, c) in enumerate(zip(CASES, cs)):
        for f in FIELDS + ("best_trial",):
            assert own[i][f].tobytes() == c["own"][f].tobytes(), (name, f)
        assert np.array_equal(mask[i].cpu().numpy()[:c["N"]], c["own_mask"][:c["N"]]), name
    assert engine.lane_faults() == faults0


# ---- k_respond_mfma ------------------------------------------------------------------------------------------------------------------
RING_BYTES = (kpi.RING_H * kpi.RING_W * 5 * 4 + 255) // 256 * 256
RESP_BYTES = kpi.NET_H * kpi.NET_W * 8 * 4
NAN_PATTERN = 0x7FC00BAD     # a quiet NaN no kernel produces


def _fused_response(engine, pc):
    """The fused path's response image after one extract over a workspace filled with NAN_PATTERN, and the map it went by."""
    ws = engine._ws("extract", int(engine.lib.caelo_extract_ws_bytes()))
    off = int(engine.lib.caelo_extract_ws_kp_eligible_offset()) + 512 + RING_BYTES   # (pinned by tests/test_kp_eligible_gpu.py)
    ws[off:off + RESP_BYTES].view(torch.int32).fill_(NAN_PATTERN)
    engine.extract(pc)
    words = engine.extract_kp_eligible()
    return ws[off:off + RESP_BYTES].clone().view(torch.int32).view(kpi.NET_H, kpi.NET_W, 8).cpu().numpy(), words


@pytest.mark.parametrize("name", ["all", "none", "corner_0", "corner_1", "corner_2", "corner_3", "gates"])
def test_response_blocks_equal_the_oracle(engine, orc, models, name):
    pc = ker.cases()[name]
    faults0 = engine.lane_faults()
    o_ring, _ = orc.ProjectPC2SphericalRing(pc)
    want = models[0].predict(o_ring[None, 0:64, 0:1792, 0:3])[0].view(np.int32)
    pc_d = torch.from_numpy(np.array(pc)).to(engine.device)
    ring, _, _ = engine.project(pc_d)
    staged = engine.respond(ring).cpu().numpy().view(np.int32)
    bad = np.argwhere(staged != want)
    assert len(bad) == 0, "caelo_respond: %d elements, rows %s, columns %s" % (len(bad), np.unique(bad[:, 0])[:8], np.unique(bad[:, 1])[:8])
    got, words = _fused_response(engine, pc_d)
    need = ker.needed_blocks(ker.bits_of_words(words))
    need[:ker.RESP_ROW0] = False
    need[ker.RESP_ROW1:] = False
    px = np.repeat(need, ker.BLK, axis=1)
    print("%s: %d map bits, %d blocks computed" % (name, int(ker.bits_of_words(words).sum()), int(need.sum())))
    assert need.sum() == {"all": (ker.RESP_ROW1 - ker.RESP_ROW0) * (kpi.NET_W // ker.BLK), "none": 0}.get(name, need.sum())
    assert name in ("all", "none") or 0 < need.sum() < 200
    assert np.array_equal(got[px], want[px]) and (got[~px] == NAN_PATTERN).all()
    assert engine.lane_faults() == faults0
