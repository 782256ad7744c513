"""Descriptors 65 .. 256 wide (csrc/match_screen_wide.inc): the f16 screen over several K = 64 blocks gives the float64 argmin of
cdist bit for bit -- against the oracle's match on every block edge, on small and large magnitudes, on ties, with the screen (not
the exact re-scan) doing the work; pair tables and the command line on descriptors of the caller's (caelo_register_pairs_desc)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

DIMS = [65, 66, 126, 127, 128, 129, 190, 191, 192, 254, 255, 256]   # both sides of every block edge and of the norm slots' move
REL_TOL = 1e-4   # poses against the reference's goldens, as tests/test_gpu_parity.py asks of every pose
FIELDS = ("R", "T", "R_ransac", "T_ransac", "threshold", "success", "iterations", "n_inliers", "n_pairs")

# the window of match_screen_wide.inc, in float64: e_ij = C(nb) (2 |a|^2 + |b|^2) + A (|a|_1 + 1 + 2 |b|_1)
MS_A = 2.0 ** -24


def nb_of(dim):
    return (dim + 2 + 63) // 64


def window_c(nb):
    return (1.5 / 1.24) * (4 * 2.0 ** -22 + 192 * nb * 2.0 ** -24)


def survivors(a, b):
    """Rows per column that the screen can keep: the device's s is within e of the true s = |a|^2 - 2 <a, b>, so a row it keeps
    (s_dev - e <= min(s_dev + e)) satisfies s - 2 e <= min(s + 2 e) on true values.  NumPy float64."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    c = window_c(nb_of(a.shape[1]))
    s = (a * a).sum(1)[:, None] - 2.0 * a @ b.T
    e = (2 * c * (a * a).sum(1) + MS_A * (np.abs(a).sum(1) + 1))[:, None] + (c * (b * b).sum(1) + 2 * MS_A * np.abs(b).sum(1))[None, :]
    return ((s - 2 * e) <= (s + 2 * e).min(axis=0)[None, :]).sum(axis=0)


def dev(engine, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)


def strided(engine, x):
    """x [k, dim] as a row-strided device view whose leading dimension is no multiple of 4 (the scalar load path)."""
    k, dim = x.shape
    ld = dim + (1 if (dim + 1) % 4 else 2)
    buf = torch.full((k, ld), float("nan"), dtype=torch.float32, device=engine.device)
    buf[:, :dim] = dev(engine, x)
    v = buf[:, :dim]
    assert v.stride(0) % 4 != 0 and v.stride(1) == 1
    return v


def match_stats(engine, a, b, **kw):
    """Engine.match with the workspace's statistics words around it: (pair_idx, columns re-scanned exactly, columns decided among 2..8)."""
    kmax, dim = max(a.shape[0], b.shape[0]), a.shape[1]
    ws = engine._ws("match%d_%d" % (kmax, dim), int(engine.lib.caelo_match_ws_bytes_dim(kmax, dim)))
    ws[:256].zero_()
    idx = engine.match(a, b, **kw).cpu().numpy()
    torch.cuda.synchronize()
    st = ws[:8].view(torch.int32).cpu().numpy()
    return idx, int(st[0]), int(st[1])


@pytest.mark.parametrize("dim", DIMS)
def test_width_and_shape_sweep_vs_oracle(engine, orc, dim):
    rs = np.random.RandomState(1000 + dim)
    shapes = [(1, 1), (17, 33), (129, 65)] + ([(1024, 1024)] if dim in (128, 256) else [])
    for k0, k1 in shapes:
        a = rs.uniform(-1, 1, (k0, dim)).astype(np.float32)
        b = rs.uniform(-1, 1, (k1, dim)).astype(np.float32)
        if k0 > 40:
            b[5] = a[3]; b[6] = (a[7] + a[9]) * 0.5
        want = orc.match(a, b)[0]
        for view in (dev, strided):
            idx = engine.match(view(engine, a), view(engine, b)).cpu().numpy()
            assert np.array_equal(idx, want), (dim, k0, k1, view.__name__, np.nonzero(idx != want)[0][:8])
        # device counts below the capacities: rows and columns past them are not read (NaN) and not written
        n0, n1 = max(1, k0 - k0 // 3), max(1, k1 - k1 // 4)
        an, bn = a.copy(), b.copy()
        an[n0:], bn[n1:] = np.nan, np.nan
        t0 = torch.tensor([n0], dtype=torch.int32, device=engine.device); t1 = torch.tensor([n1], dtype=torch.int32, device=engine.device)
        idx = engine.match(dev(engine, an), dev(engine, bn), t0, t1).cpu().numpy()
        assert np.array_equal(idx[:n1], orc.match(a[:n0], b[:n1])[0]) and not idx[n1:].any(), (dim, k0, k1, n0, n1)
        # no frame-0 descriptor at all: index 0, as for the narrow widths
        z = torch.zeros(1, dtype=torch.int32, device=engine.device)
        idx = engine.match(dev(engine, a), dev(engine, b), z, None).cpu().numpy()
        assert not idx.any()
    assert engine.lane_faults() == 0


@pytest.mark.parametrize("dim", [128, 192, 256])
def test_a_later_block_decides(engine, orc, dim):
    """Frame-0 rows equal everywhere but in channel dim - 1 (the last block that holds descriptor channels).  The common part is
    small, so the rows' gaps in d^2 (3.4e-3) are well above four times the window (2.5e-4 at 256): the SCREEN must single out the row --
    the counters say that it did -- and a kernel that drops or mis-indexes a block sees equal rows and cannot."""
    rs = np.random.RandomState(dim)
    k0, k1 = 32, 40
    base = (rs.uniform(-1, 1, dim) * 0.05).astype(np.float32)
    a = np.tile(base, (k0, 1))
    a[:, dim - 1] = rs.permutation(k0).astype(np.float32) / 16.0 - 1.0
    pick = rs.randint(0, k0, k1)
    b = a[pick].copy()
    b[:, :64] += (rs.uniform(-1, 1, (k1, 64)) * 0.01).astype(np.float32)
    b[:, dim - 1] += np.float32(0.004)
    assert (survivors(a, b) == 1).all()
    idx, rescanned, decided = match_stats(engine, dev(engine, a), dev(engine, b))
    assert np.array_equal(idx, pick) and np.array_equal(idx, orc.match(a, b)[0])
    assert rescanned == 0 and decided == 0


@pytest.mark.parametrize("dim", [128, 256])
def test_scales(engine, orc, dim):
    """1e-3: the low halves of the splits are f16 subnormals (the MS_A part of the window); 1; and 20, which puts |x|^2 above
    MS_NORM_MAX = 3e4 at 256 channels (256 x 400 / 3 = 3.4e4): the exact scan -- for every row, and for a single row and column."""
    rs = np.random.RandomState(33 + dim)
    for scale, k0, k1 in [(1e-3, 200, 96), (1.0, 200, 96), (20.0, 130, 40), (45.0, 130, 40)]:
        a = (rs.uniform(-1, 1, (k0, dim)) * scale).astype(np.float32)
        b = (rs.uniform(-1, 1, (k1, dim)) * scale).astype(np.float32)
        b[1] = a[k0 - 1]                       # the last real row is the exact answer of a column: pad rows must not shadow it
        b[2] = (a[4] + a[11]) * 0.5            # a near tie
        idx = engine.match(dev(engine, a), dev(engine, b)).cpu().numpy()
        want = orc.match(a, b)[0]
        assert idx.max() < k0 and np.array_equal(idx, want), (scale, dim, np.nonzero(idx != want)[0][:8])
    a = rs.uniform(-1, 1, (300, dim)).astype(np.float32); b = rs.uniform(-1, 1, (100, dim)).astype(np.float32)
    b2 = b.copy(); b2[3] *= 500.0              # one column out of range: that column alone is re-scanned
    idx, rescanned, _ = match_stats(engine, dev(engine, a), dev(engine, b2))
    assert np.array_equal(idx, orc.match(a, b2)[0]) and rescanned == 1
    a[17] *= 1e3                               # one row out of range: every column of the pair
    idx, rescanned, _ = match_stats(engine, dev(engine, a), dev(engine, b2))
    assert np.array_equal(idx, orc.match(a, b2)[0]) and rescanned == 100


@pytest.mark.parametrize("dim", [128, 255])
def test_ties_and_near_ties(engine, orc, dim):
    rs = np.random.RandomState(77 + dim)
    a = rs.uniform(-1, 1, (700, dim)).astype(np.float32); b = rs.uniform(-1, 1, (90, dim)).astype(np.float32)
    a[350] = a[3]; b[5] = a[3]                                   # a row twice: the first index wins
    a[np.arange(100, 120) * 3] = a[640]; b[40] = a[640]          # 20 times: more than the candidate list holds, the column is re-scanned
    a[21] = a[9]; a[21, 70] = np.nextafter(a[9, 70], np.float32(2)); b[8] = a[21]    # one f32 ulp apart in one channel: float64 decides,
    a[30] = a[12]; a[30, dim - 1] = np.nextafter(a[12, dim - 1], np.float32(2)); b[9] = a[12]   # whichever of the two comes first
    sv = survivors(a, b)
    idx, rescanned, decided = match_stats(engine, dev(engine, a), dev(engine, b))
    want = orc.match(a, b)[0]
    assert np.array_equal(idx, want)
    assert idx[5] == 3 and idx[40] == 300 and idx[8] == 21 and idx[9] == 12
    # column 40 is re-scanned (equal rows get equal s: all twenty survive), and so is at most every other column whose nearest row is
    # one of the twenty; columns 5, 8 and 9 are decided between two rows in float64
    assert sv[40] > 8 and 1 <= rescanned <= int((sv > 8).sum()) and decided >= 3


def test_the_screen_does_the_work(engine, orc):
    """(1024, 1024, 128), uniform [-1, 1]: no column may be re-scanned exactly.  The input makes that a MUST: on the CPU, with the
    window of the source header doubled (see `survivors`), no column keeps more than eight rows.  A test on pair_idx alone would
    pass with a broken screen and a working re-scan."""
    rs = np.random.RandomState(5)
    a = rs.uniform(-1, 1, (1024, 128)).astype(np.float32); b = rs.uniform(-1, 1, (1024, 128)).astype(np.float32)
    sv = survivors(a, b)
    assert sv.min() >= 1 and sv.max() <= 8
    idx, rescanned, decided = match_stats(engine, dev(engine, a), dev(engine, b))
    print("wide screen, 1024 x 1024 x 128: %d columns re-scanned, %d decided among 2..8 rows (CPU bound on the latter: %d)" % (rescanned, decided, int((sv > 1).sum())))
    assert np.array_equal(idx, orc.match(a, b)[0])
    assert rescanned == 0 and decided <= int((sv > 1).sum())


# ---- pair tables ------------------------------------------------------------------------------------------------------------------
N_FRAMES = 5
TABLE = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (4, 0), (2, 2), (0, 2), (3, 1), (1, 4), (0, 0), (2, 4)]   # 12 pairs: two slices


@pytest.fixture(scope="module")
def frames(engine, scans):
    """Five synthetic frames' rows and counts, the draws of the 12 pairs, and 128-d descriptors derived from the 60-d ones (tiled
    twice plus eight channels, perturbed).  Shared and never written."""
    from caelo.engine import ransac_draws
    ff = [engine.extract(dev(engine, scans(f))) for f in range(N_FRAMES)]
    rows = torch.stack([f.rows for f in ff]).contiguous()
    n_key = torch.cat([f.n_key.reshape(1) for f in ff]).to(torch.int32).contiguous()
    draws = np.stack([ransac_draws(900 + q) for q in range(len(TABLE))])
    g = torch.Generator(device="cpu").manual_seed(3)
    d60 = rows[:, :, 0:60]
    noise = (torch.rand((N_FRAMES, 1024, 128), generator=g) * 0.02 - 0.01).to(engine.device)
    d128 = (torch.cat([d60, d60, d60[:, :, :8]], dim=2) + noise).contiguous()
    torch.cuda.synchronize()
    return dict(rows=rows, n_key=n_key, draws=draws, d128=d128)


def _same_records(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), "%s: field %s differs" % (what, f)


@pytest.mark.parametrize("certify", [True, False])
def test_table_on_the_rows_own_descriptors(engine, frames, certify):
    want = engine.register_pairs(frames["rows"], frames["n_key"], TABLE, frames["draws"], certify=certify)
    for desc in (frames["rows"][:, :, 0:60].contiguous(), frames["rows"][:, :, 0:60]):   # a copy, and the column slice itself (ld 64)
        got = engine.register_pairs(frames["rows"], frames["n_key"], TABLE, frames["draws"], certify=certify, desc=desc)
        assert torch.equal(got.pair_idx, want.pair_idx) and np.array_equal(got.masks, want.masks)
        _same_records(got.results, want.results, "desc = the rows' columns 0:60")
    assert engine.lane_faults() == 0


@pytest.mark.parametrize("certify", [True, False])
def test_table_on_128_channels_equals_the_staged_calls(engine, frames, certify):
    from caelo import _ffi
    rows, nk, d = frames["rows"], frames["n_key"], frames["d128"]
    got = engine.register_pairs(rows, nk, TABLE, frames["draws"], certify=certify, desc=d)
    idx = got.pair_idx.cpu().numpy()
    for q, (a, b) in enumerate(TABLE):
        rand = dev(engine, frames["draws"][q])
        x = engine.match(d[a], d[b], nk[a:a + 1], nk[b:b + 1])
        if certify:
            cert = engine.new_cert(1)
            engine.ransac(rows[a][:, 60:63], rows[b][:, 60:63], x, rand, nk[b:b + 1], cert=cert[0])
            res, masks, _, status = engine.certify(cert, [frames["draws"][q]])
            assert status[0] == 0
            r, m = res[0], masks[0]
        else:
            r, m = engine.ransac(rows[a][:, 60:63], rows[b][:, 60:63], x, rand, nk[b:b + 1])
            r, m = np.frombuffer(r.cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE)[0], m.cpu().numpy()
        kb = int(nk[b].item())
        assert np.array_equal(idx[q][:kb], x.cpu().numpy()[:kb]), "pair %d (%d, %d): pair_idx" % (q, a, b)
        assert np.array_equal(got.masks[q][:kb], np.asarray(m)[:kb]), "pair %d (%d, %d): inlier mask" % (q, a, b)
        _same_records(got.results[q], r, "pair %d (%d, %d)" % (q, a, b))
    with pytest.raises((ValueError, _ffi.CaeloError)):
        engine.register_pairs(rows, nk, TABLE, frames["draws"], certify=certify, desc=torch.zeros((N_FRAMES, 1024, 257), device=engine.device))


# ---- the reference's own SolveRelativePose on 128-d descriptors (tools/make_goldens_wide.py) ---------------------------------------
def test_relative_pose_vs_reference_golden_128(engine):
    from caelo import api
    g = np.load(os.path.join(GOLDEN, "wide_desc.npz"))
    assert g["a_thr"] == 0.4 and g["b_thr"] > 0.4        # one pair solved at the first threshold, one escalated
    for name in ("a", "b"):
        s = int(g[name + "_seed"])
        idx = engine.match(dev(engine, g[name + "_f0"]), dev(engine, g[name + "_f1"])).cpu().numpy()
        assert np.array_equal(idx, g[name + "_pair_idx"])                    # reference cdist + argmin
        rng = np.random.RandomState(s)
        R, T, ok, i0, i1, thr = api.SolveRelativePose(g[name + "_p0"], g[name + "_f0"], None, g[name + "_p1"], g[name + "_f1"], None, rng=rng)
        assert ok == bool(g[name + "_ok"]) and thr == float(g[name + "_thr"])
        assert np.array_equal(i0, g[name + "_idx0"]) and np.array_equal(i1, g[name + "_idx1"])  # inlier sets, bit-exact
        assert np.abs(R - g[name + "_R"]).max() <= REL_TOL
        assert np.abs(T - g[name + "_T"]).max() <= REL_TOL * max(1.0, np.abs(g[name + "_T"]).max())
        # the RNG stream advanced exactly as the reference's loop would have (4 draws per iteration; an escalated pair ran the
        # 500 trials of every level it left behind)
        levels_left = int(round(np.log2(float(g[name + "_thr"]) / 0.4)))
        ref = np.random.RandomState(s)
        ref.random_sample(4 * (500 * levels_left + int(g[name + "_iters"])))
        assert rng.random_sample() == ref.random_sample()
    with pytest.raises(ValueError, match="256"):
        api.SolveRelativePose(g["a_p0"], np.zeros((256, 257), np.float32), None, g["a_p1"], np.zeros((256, 257), np.float32), None)


# ---- run_sequence.py --desc-dir ---------------------------------------------------------------------------------------------------
RS = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")
N_SEQ, SEED = 12, 4300


def _run(args):
    r = subprocess.run([sys.executable, RS] + [str(a) for a in args], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


@pytest.fixture(scope="module")
def seq_files(engine, scans, tmp_path_factory):
    """12 synthetic frames' key points and 60-d features as Features/*.bin.mat, the same features as 60-d descriptor files, and 128-d
    descriptors made of them (tiled, perturbed) as descriptor files; written once."""
    from caelo import keysources
    d = tmp_path_factory.mktemp("descdir")
    rs = np.random.RandomState(6)
    out = dict(dir=d, kp=[], f60=[], f128=[])
    for f in range(N_SEQ):
        ff = engine.extract(dev(engine, scans(f)))
        k = int(ff.n_key.item())
        rows = ff.rows[:k].cpu().numpy()
        kp, f60 = rows[:, 60:63].copy(), rows[:, 0:60].copy()
        f128 = (np.concatenate([f60, f60, f60[:, :8]], axis=1) + rs.uniform(-0.01, 0.01, (k, 128))).astype(np.float32)
        keysources.save_features(str(d / "seq" / "velodyne" / ("%06d.bin" % f)), kp, f60)
        keysources.write_descriptors(keysources.desc_path(str(d / "d60"), f), f60)
        keysources.write_descriptors(keysources.desc_path(str(d / "d128"), f), f128)
        out["kp"].append(kp); out["f60"].append(f60); out["f128"].append(f128)
    return out


def test_cli_60_channels_as_descriptor_files(seq_files, tmp_path):
    """The engine's own features once as --features-from rows (the pipeline's pair stage) and once as --desc-dir files of width 60
    (the pair table on descriptors): the same pose and matchability files, steps 1 and 5."""
    d = seq_files["dir"]
    common = ["--frame-steps", "1,5", "--seed-base", SEED]
    _run(["--synthetic", N_SEQ, "--trajectory", "line", "--features-from", d / "seq" / "Features", "--matchability", tmp_path / "a" / "m.mat",
          "--out", tmp_path / "a" / "00.txt"] + common)
    _run(["--desc-dir", d / "d60", "--desc-dim", 60, "--features-from", d / "seq" / "Features", "--matchability", tmp_path / "b" / "m.mat",
          "--out", tmp_path / "b" / "00.txt", "--chunk", 5] + common)      # (chunks of 5: pairs of both steps cross them)
    rd = lambda p: open(str(p), "rb").read()
    for name in ("00.txt", "5_00.txt"):
        assert rd(tmp_path / "a" / name) == rd(tmp_path / "b" / name) and len(rd(tmp_path / "a" / name)) > 0
    for name in ("m.mat", "5_m.mat"):   # (a MAT-file opens with 128 bytes of header whose text carries the time of writing)
        assert rd(tmp_path / "a" / name)[128:] == rd(tmp_path / "b" / name)[128:] and len(rd(tmp_path / "b" / name)) > 128


def test_cli_128_channels(engine, seq_files, tmp_path):
    """--desc-dim 128 writes the pose file that api.SolveRelativePoses(..., desc=) and stageio.chain_poses give."""
    from caelo import api, stageio
    d = seq_files["dir"]
    _run(["--desc-dir", d / "d128", "--desc-dim", 128, "--features-from", d / "seq" / "Features", "--seed-base", SEED, "--out", tmp_path / "c" / "00.txt"])
    rows = np.zeros((N_SEQ, 1024, 64), np.float32); desc = np.zeros((N_SEQ, 1024, 128), np.float32)
    for f in range(N_SEQ):
        k = len(seq_files["kp"][f])
        rows[f, :k, 60:63], rows[f, :k, 63], desc[f, :k] = seq_files["kp"][f], 1.0, seq_files["f128"][f]
    res = api.SolveRelativePoses(rows, [(i - 1, i) for i in range(1, N_SEQ)], [SEED + i - 1 for i in range(1, N_SEQ)], desc=desc)
    rel = np.stack([np.r_[R.reshape(9), T.reshape(3)] for R, T, _, _, _, _ in res]).astype(np.float32)
    stageio.write_poses(str(tmp_path / "want.txt"), stageio.chain_poses(rel, None))
    assert open(str(tmp_path / "c" / "00.txt"), "rb").read() == open(str(tmp_path / "want.txt"), "rb").read()
    assert sum(ok for _, _, ok, _, _, _ in res) >= N_SEQ - 3      # (the perturbed descriptors still register the sequence)
