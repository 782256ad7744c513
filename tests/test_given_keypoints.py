"""Key point sources other than the detector (PoseEstimation.py:26-66): CAELO_EXTRACT_GIVEN_KEYPTS (the caller's key points through
the fused extract and the pipeline), CAELO_EXTRACT_GIVEN_ROWS (the caller's rows, pair stage only), CAELO_ST_BAD_KEYPTS, the readers
of caelo.keysources and run_sequence.py --keypts-source / --features-from.  tests/golden/keysources.npz comes from the reference's
own EulerAngle2RotateMat, GetPatchesList and SolveRelativePose (tools/make_goldens_keysources.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
VIS = (99.84, 99.84, 14.72)


def _header_defines():
    src = open(os.path.join(REPO, "include", "caelo.h")).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"#define\s+(CAELO_\w+)\s+([0-9.]+)", src)}


def _golden():
    return np.load(os.path.join(GOLDEN, "keysources.npz"))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_bits_header_ffi_engine():
    from caelo import _ffi, engine
    d = _header_defines()
    assert int(d["CAELO_EXTRACT_GIVEN_KEYPTS"]) == 8 == _ffi.EXTRACT_GIVEN_KEYPTS
    assert int(d["CAELO_EXTRACT_GIVEN_ROWS"]) == 16 == _ffi.EXTRACT_GIVEN_ROWS
    assert int(d["CAELO_ST_BAD_KEYPTS"]) == 128 == _ffi.ST_BAD_KEYPTS == engine.ST_BAD_KEYPTS
    assert float(d["CAELO_GIVEN_KEYPTS_RANGE"]) == _ffi.GIVEN_KEYPTS_RANGE >= 10000.0
    assert int(d["CAELO_ABI_VERSION"]) == 6
    others = [int(d[k]) for k in d if k.startswith("CAELO_ST_") and k != "CAELO_ST_BAD_KEYPTS"]
    assert 128 not in others and all(o & 128 == 0 for o in others)
    assert engine.extract_mode(given_keypts=True) == 8 and engine.extract_mode(exact_patches=True, given_keypts=True) == 12
    assert engine.extract_mode(given_rows=True) == 16
    with pytest.raises(ValueError, match="given key points"):
        engine.raise_status(engine.ST_BAD_KEYPTS)


def test_accepted_range_covers_the_voxel_packing():
    """Within CAELO_GIVEN_KEYPTS_RANGE every key voxel and ball-cube brick index of every scale is below 2^20 (caelo_pack3's field):
    no far point aliases onto a brick of the grid."""
    from caelo import _ffi
    r = _ffi.GIVEN_KEYPTS_RANGE
    for vs in (0.02, 0.16, 0.64):
        hi = int((r + max(VIS)) / vs)
        assert (hi + 13) >> 3 < (1 << 20) and hi < (1 << 24)


def test_r90_and_usip_rotation_equal_the_golden():
    from caelo import keysources
    g = _golden()
    assert np.array_equal(keysources.R90.view(np.uint64), g["r90_bits"])
    for f in g["frames"]:
        raw = g["usip_raw_%d" % f]
        assert np.array_equal(np.dot(keysources.R90, raw.T).T, g["usip_rot64_%d" % f])
        assert np.array_equal(raw.astype(np.float64), raw)


def test_readers(tmp_path):
    from caelo import keysources
    g = _golden()
    f = int(g["frames"][0])
    raw = g["usip_raw_%d" % f]
    keysources.write_usip(keysources.keypts_path(tmp_path / "usip", f), raw)
    got64 = keysources.read_usip_f64(keysources.keypts_path(tmp_path / "usip", f))
    assert got64.dtype == np.float64 and np.array_equal(got64, g["usip_rot64_%d" % f])
    got = keysources.load_keypts("usip", str(tmp_path / "usip"), f)
    assert got.dtype == np.float32 and np.array_equal(got, g["usip_rot32_%d" % f])
    pts = g["featnet_pts_%d" % f]
    desc = np.random.RandomState(3).rand(pts.shape[0], 32).astype(np.float32)
    p = keysources.write_3dfeatnet(keysources.keypts_path(tmp_path / "fn", 7), pts, desc)
    assert os.path.getsize(p) == pts.shape[0] * 35 * 4
    a = np.fromfile(p, dtype=np.float32).reshape([-1, 35])   # PoseEstimation.py:34-35
    assert np.array_equal(keysources.load_keypts("3dfeatnet", str(tmp_path / "fn"), 7), a[:, 0:3])
    kp, d = keysources.read_3dfeatnet(p, descriptors=True)
    assert np.array_equal(d, desc) and kp.flags["C_CONTIGUOUS"]
    rows = keysources.rows_from_features(kp, d)
    assert rows.shape == (pts.shape[0], 64) and not rows[:, 32:60].any() and (rows[:, 63] == 1).all()
    assert np.array_equal(rows[:, 60:63], kp) and np.array_equal(rows[:, 0:32], d)
    # Features/*.mat through stageio
    raw_file = str(tmp_path / "seq" / "velodyne" / "000003.bin")
    keysources.save_features(raw_file, kp, d)
    k2, d2, w2 = keysources.load_features(raw_file)
    assert np.array_equal(k2, kp) and np.array_equal(d2, d) and w2.shape == (kp.shape[0], 1)
    k3, d3, _ = keysources.load_features_dir(str(tmp_path / "seq" / "Features"), 3)
    assert np.array_equal(k3, kp) and np.array_equal(d3, d)


def test_oversize_and_missing_files_are_clear_errors(tmp_path):
    from caelo import keysources
    keysources.write_usip(keysources.keypts_path(tmp_path, 0), np.zeros((1025, 3), np.float32))
    keysources.write_3dfeatnet(keysources.keypts_path(tmp_path / "f", 0), np.zeros((1025, 3), np.float32))
    keysources.write_usip(keysources.keypts_path(tmp_path, 1), np.zeros((1024, 3), np.float32))
    with pytest.raises(ValueError, match="staged API"):
        keysources.load_keypts("usip", str(tmp_path), 0)
    with pytest.raises(ValueError, match="staged API"):
        keysources.load_keypts("3dfeatnet", str(tmp_path / "f"), 0)
    with pytest.raises(ValueError, match="staged API"):
        keysources.rows_from_features(np.zeros((1025, 3)), np.zeros((1025, 32)))
    assert keysources.load_keypts("usip", str(tmp_path), 1).shape == (1024, 3)
    with pytest.raises(FileNotFoundError, match="000002.bin"):
        keysources.load_keypts("usip", str(tmp_path), 2)
    with pytest.raises(FileNotFoundError):
        keysources.load_features_dir(str(tmp_path / "Features"), 0)
    with pytest.raises(ValueError):
        keysources.load_keypts("iss", str(tmp_path), 1)


def test_run_sequence_rejects_the_native_loader_with_key_point_files(tmp_path):
    script = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")
    for extra in (["--keypts-source", "usip", "--keypts-dir", str(tmp_path)], ["--features-from", str(tmp_path)]):
        r = subprocess.run([sys.executable, script, "--scans", str(tmp_path), "--out", str(tmp_path / "p.txt")] + extra,
                           capture_output=True, timeout=300)
        assert r.returncode == 2 and b"native scan loader" in r.stderr and b"add --python-loader" in r.stderr
    r = subprocess.run([sys.executable, script, "--synthetic", "4", "--keypts-source", "usip"], capture_output=True, timeout=300)
    assert r.returncode == 2 and b"--keypts-dir" in r.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU
def _pc(engine, scans, f, **kw):
    import torch
    return torch.from_numpy(scans(f, **kw)).to(engine.device)


def _bits_of(orc, pts, vox):
    return np.stack([orc.patches_bits(pts, vox[s], s)[0] for s in range(3)], axis=1)   # [K, 3, 64]


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True])
def test_detector_points_fed_back_give_the_same_results(engine, scans, exact):
    import torch
    from caelo.engine import Pipeline, ransac_draws
    frames = [(f, {}) for f in range(5)] + [(23, {"quantum": 1e-3, "scene_kind": "clutter"}), (24, {"quantum": 1e-3, "scene_kind": "clutter"})]
    pcs = [_pc(engine, scans, f, **kw) for f, kw in frames]
    det = [engine.extract(pc, exact_patches=exact) for pc in pcs]
    kps = []
    for pc, d in zip(pcs, det):
        k = int(d.n_key.item())
        kps.append(d.key_pts[:k].clone())
        g = engine.extract(pc, exact_patches=exact, key_pts=kps[-1])
        torch.cuda.synchronize()
        assert int(g.status[0].item()) == int(d.status[0].item()) == 0 and int(g.n_key.item()) == k
        assert torch.equal(g.rows[:k], d.rows[:k]) and torch.equal(g.rows[:, 0:60], d.rows[:, 0:60])
        assert torch.equal(g.rows[:, 63], d.rows[:, 63]) and torch.equal(g.flags[:k], d.flags[:k])
        assert (g.key_pixels == -1).all()
    rnd = [torch.from_numpy(ransac_draws(40 + i)).to(engine.device) for i in range(len(pcs))]
    dn = [ransac_draws(40 + i) for i in range(len(pcs))]
    a = Pipeline(engine, 4, 3).run(pcs, rnd, certify=True, rands_host=dn, exact_patches=exact)
    b = Pipeline(engine, 4, 3).run(pcs, rnd, certify=True, rands_host=dn, exact_patches=exact, keypts=kps)
    torch.cuda.synchronize()
    n = len(pcs)
    assert torch.equal(a.pair_idx[:n], b.pair_idx[:n]) and torch.equal(a.rows[:, :, 0:60], b.rows[:, :, 0:60])
    assert torch.equal(a.result[:n], b.result[:n]) and torch.equal(a.inlier_mask[:n], b.inlier_mask[:n])
    assert np.array_equal(a.exact[0][:n], b.exact[0][:n]) and np.array_equal(a.exact[1][:n], b.exact[1][:n])
    assert (a.exact[3][1:n] == 0).all()
    assert engine.lane_faults() == 0


def _off_points(det_pts, seed):
    """Detector points + seeded offsets, points beyond every face of the voxel grid (both sides, near and far), duplicates: 1024."""
    rs = np.random.RandomState(seed)
    out = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            for d in (0.3, 2.0, 9.0, 60.0):
                p = det_pts[rs.randint(det_pts.shape[0])].astype(np.float64).copy()
                p[a] = sgn * (VIS[a] + d)
                out.append(p)
    out += [[-16000.0, 3.0, -1.0], [16000.0, 16000.0, -16000.0], [-99.85, -99.85, -14.73], [0.0, 0.0, 0.0]]
    off = det_pts[rs.randint(det_pts.shape[0], size=600)] + rs.normal(0, 0.4, (600, 3))
    pts = np.concatenate([det_pts[:300], np.array(out), off]).astype(np.float32)
    pts = np.concatenate([pts, pts[rs.randint(pts.shape[0], size=1024 - pts.shape[0])]])   # duplicates fill up to 1024
    return pts[rs.permutation(1024)]


@pytest.mark.gpu
def test_off_scan_and_off_grid_points_against_the_oracle(engine, scans, orc, models):
    import torch
    enc = orc.PatchEncoder(models[1].w)
    for f, kw in ((2, {}), (23, {"quantum": 1e-3, "scene_kind": "clutter"})):
        pc_h = scans(f, **kw)
        pc = torch.from_numpy(pc_h).to(engine.device)
        det = engine.extract(pc)
        det_pts = det.key_pts[:int(det.n_key.item())].cpu().numpy()
        pts = _off_points(det_pts, 11 + f)
        vox = orc.Voxelization(pc_h[:, 0:3])[6:9]
        ref_bits = _bits_of(orc, pts, vox)
        for K in (1, 4, 50, 51, 1023, 1024):
            g = engine.extract(pc, exact_patches=True, key_pts=pts[:K])
            mine = engine.encode(torch.from_numpy(ref_bits[:K].view(np.int64)).to(engine.device).contiguous(), group=3)
            torch.cuda.synchronize()
            assert int(g.status[0].item()) == 0 and int(g.n_key.item()) == K
            assert np.array_equal(g.rows[:K, 60:63].cpu().numpy(), pts[:K])              # the caller's xyz bits
            assert torch.equal(g.rows[:K, 0:60], mine), (f, K)                            # the patches are the oracle's, bit for bit
            want = np.c_[tuple(enc.predict_bits(ref_bits[:K, s]) for s in range(3))]
            got = g.rows[:K, 0:60].cpu().numpy()
            assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), (f, K)
            v = g.rows[:, 63].cpu().numpy()
            assert (v[:K] == 1).all() and (v[K:] == 0).all()
        far = [i for i in range(1024) if np.abs(pts[i]).max() > 1000]
        assert far and not ref_bits[far].any()                                            # far away: empty at every scale


@pytest.mark.gpu
def test_bad_key_points_set_the_status_bit_and_raise(engine, scans):
    import torch
    from caelo import api, engine as E
    pc_h = scans(0)
    pc = torch.from_numpy(pc_h).to(engine.device)
    good = engine.extract(pc)
    base = good.key_pts[:100].cpu().numpy()
    nan = base.copy(); nan[7, 1] = np.nan
    inf = base.copy(); inf[3, 2] = np.inf
    far = base.copy(); far[50, 0] = -16384.5
    cases = [("K=0", np.zeros((0, 3), np.float32)), ("K=1025", np.zeros((1025, 3), np.float32)), ("nan", nan), ("inf", inf),
             ("range", far)]
    for name, pts in cases:
        g = engine.extract(pc, key_pts=pts)
        st = int(g.status[0].item())
        assert st & E.ST_BAD_KEYPTS, name
        if name.startswith("K="):
            assert int(g.n_key.item()) == 0 and (g.rows[:, 63] == 0).all()
        with pytest.raises(ValueError, match="given key points"):
            E.raise_status(st)
    # a coordinate on the bound is accepted
    edge = base.copy(); edge[0] = (16384.0, -16384.0, 16384.0)
    assert int(engine.extract(pc, key_pts=edge).status[0].item()) == 0
    for name, pts in cases[2:]:
        with pytest.raises(ValueError, match="given key points"):
            api.GetFeaturesAtKeyPts(pc_h, pts)
    with pytest.raises(ValueError, match="staged API"):
        api.GetFeaturesAtKeyPts(pc_h, np.zeros((1025, 3), np.float32))
    kp, feats = api.GetFeaturesAtKeyPts(pc_h[:, 0:3], base)
    assert kp is base and feats.shape == (100, 60) and feats.dtype == np.float32
    assert np.array_equal(feats, engine.extract(pc, exact_patches=True, key_pts=base).rows[:100, 0:60].cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [3, 4])
def test_pipeline_mixing_sources_equals_single_calls(engine, scans, batch):
    import torch
    from caelo.engine import FrameFeatures, Pipeline, ransac_draws
    kinds = ["det", "det", "kp", "kp", "rows", "det", "kp", "rows", "rows", "det", "kp", "det", "rows"]
    n = len(kinds)
    pcs = [_pc(engine, scans, i % 6) for i in range(n)]
    rs = np.random.RandomState(5)
    keypts, rows = [None] * n, [None] * n
    single = []
    for i, kd in enumerate(kinds):
        d = engine.extract(pcs[i])
        k = int(d.n_key.item())
        if kd == "kp":
            K = [1024, 60, 700, 5][i % 4]
            base = d.key_pts[:k].cpu().numpy()
            keypts[i] = (base[rs.randint(k, size=K)] + rs.normal(0, 0.2, (K, 3))).astype(np.float32)
            d = engine.extract(pcs[i], key_pts=keypts[i])
        elif kd == "rows":
            K = [k, 40, 900][i % 3] if k >= 900 else k
            rows[i] = d.rows[:K].clone()
            full = torch.zeros_like(d.rows)
            full[:K] = rows[i]
            d = FrameFeatures(full, None, torch.tensor([K], dtype=torch.int32, device=engine.device), None, None)
        single.append(d)
    rnd = [torch.from_numpy(ransac_draws(90 + i)).to(engine.device) for i in range(n)]
    out = Pipeline(engine, batch, 3).run([None if kd == "rows" else pcs[i] for i, kd in enumerate(kinds)], rnd, keypts=keypts,
                                         rows_given=rows)
    torch.cuda.synchronize()
    for i in range(n):
        k = int(single[i].n_key.item())
        assert int(out.n_key[i].item()) == k, i
        assert torch.equal(out.rows[i, :k], single[i].rows[:k]) and torch.equal(out.rows[i, :, 0:60], single[i].rows[:, 0:60]), i
        if kinds[i] != "rows":
            assert int(out.status[i, 0].item()) == 0
        if i > 0:
            res, mask, idx = engine.match_pose(single[i - 1], single[i], rnd[i])
            assert torch.equal(out.result[i], res) and torch.equal(out.pair_idx[i], idx) and torch.equal(out.inlier_mask[i], mask), i
    assert engine.lane_faults() == 0


@pytest.mark.gpu
def test_rows_given_with_32d_descriptors(engine):
    import torch
    from scipy.spatial.distance import cdist
    from caelo import api, keysources
    from caelo.engine import Pipeline, ransac_draws
    rs = np.random.RandomState(21)
    k0, k1 = 310, 287
    p0 = rs.uniform(-30, 30, (k0, 3)).astype(np.float32)
    d0 = rs.rand(k0, 32).astype(np.float32)
    sel = rs.randint(k0, size=k1)
    ang = 0.05
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    p1 = ((p0[sel] - [0.8, 0.1, 0.0]) @ R + rs.normal(0, 0.02, (k1, 3))).astype(np.float32)
    d1 = (d0[sel] + rs.normal(0, 0.05, (k1, 32))).astype(np.float32)
    d1[::7] = rs.rand(len(d1[::7]), 32)                                     # outliers
    r0, r1 = keysources.rows_from_features(p0, d0), keysources.rows_from_features(p1, d1)
    seed = 77
    draws = ransac_draws(seed)
    out = Pipeline(engine, 2, 2).run([None, None], [torch.from_numpy(ransac_draws(1)).to(engine.device),
                                                    torch.from_numpy(draws).to(engine.device)],
                                     rows_given=[r0, r1], certify=True, rands_host=[ransac_draws(1), draws])
    torch.cuda.synchronize()
    idx = out.pair_idx[1, :k1].cpu().numpy()
    assert np.array_equal(idx, np.argmin(cdist(d0, d1, metric="euclidean"), axis=0))   # Match.py:257-258, float64
    Rr, Tr, ok, i0, i1, thr = api.SolveRelativePose(p0, d0, None, p1, d1, None, rng=np.random.RandomState(seed))
    res = out.exact[0][1]
    assert out.exact[3][1] == 0 and ok and bool(res["success"])
    assert np.array_equal(np.array(res["R"], np.float32).reshape(3, 3), Rr) and np.array_equal(np.array(res["T"], np.float32).reshape(3, 1), Tr)
    m = out.exact[1][1, :k1].astype(bool)
    assert np.array_equal(np.nonzero(m)[0], i1) and np.array_equal(idx[m], i0)
    assert (out.key_pixels[:2] == -1).all() and not out.status[:2].any() and not out.flags[:2].any()


@pytest.mark.gpu
def test_keysources_golden_end_to_end(engine, scans):
    """tests/golden/keysources.npz: the reference's GetPatchesList + GetFeaturesFromPatches + SolveRelativePose on USIP (float32
    after R90) and 3DFeatNet key points of two synthetic scans, reproduced through the fused path and the certified pipeline."""
    import torch
    from caelo import api, synth
    from caelo.engine import Pipeline, ransac_draws
    g = _golden()
    f0, f1 = (int(f) for f in g["frames"])
    pcs = [torch.from_numpy(synth.make_scan(f)).to(engine.device) for f in (f0, f1)]
    for f, pc in zip((f0, f1), pcs):
        assert synth.cloud_sha256(pc.cpu().numpy()) == str(g["cloud_sha256_%d" % f])
    seed = int(g["seed_base"]) + f0
    draws = ransac_draws(seed)
    for name in ("usip", "featnet"):
        pts = [g["%s_%d" % ("usip_rot32" if name == "usip" else "featnet_pts", f)] for f in (f0, f1)]
        for f, pc, p in zip((f0, f1), pcs, pts):
            ff = engine.extract(pc, exact_patches=True, key_pts=p)
            want = engine.encode(torch.from_numpy(g["%s_bits_%d" % (name, f)].view(np.int64)).to(engine.device).contiguous(), group=3)
            torch.cuda.synchronize()
            assert int(ff.status[0].item()) == 0
            assert torch.equal(ff.rows[:p.shape[0], 0:60], want), (name, f)              # patches exact
            assert np.abs(ff.rows[:p.shape[0], 0:60].cpu().numpy() - g["%s_features_%d" % (name, f)]).max() <= 1e-4
        out = Pipeline(engine, 2, 2).run(pcs, [torch.from_numpy(ransac_draws(1)).to(engine.device), torch.from_numpy(draws).to(engine.device)],
                                         keypts=pts, exact_patches=True, certify=True, rands_host=[ransac_draws(1), draws])
        torch.cuda.synchronize()
        k1 = pts[1].shape[0]
        res, m = out.exact[0][1], out.exact[1][1, :k1].astype(bool)
        idx = out.pair_idx[1, :k1].cpu().numpy()
        assert out.exact[3][1] == 0
        assert np.array_equal(idx, g["%s_pair_idx" % name])
        assert np.array_equal(np.nonzero(m)[0], g["%s_inliers1" % name]) and np.array_equal(idx[m], g["%s_inliers0" % name])
        # R* / T*: the refit over the same inlier set goes through this host's BLAS, the golden's through the build
        # container's: equal within float32 rounding here, bit for bit against the staged API on this host
        R, T = np.array(res["R"], np.float32).reshape(3, 3), np.array(res["T"], np.float32)
        assert np.abs(R - g["%s_R" % name]).max() <= 1e-6 and np.abs(T - g["%s_T" % name]).max() <= 1e-5 * max(1.0, np.abs(g["%s_T" % name]).max())
        ff = [engine.extract(pc, exact_patches=True, key_pts=p) for pc, p in zip(pcs, pts)]
        Rs, Ts, ok, i0, i1, _ = api.SolveRelativePose(pts[0], ff[0].rows[:pts[0].shape[0], 0:60].cpu().numpy(), None, pts[1],
                                                      ff[1].rows[:k1, 0:60].cpu().numpy(), None, rng=np.random.RandomState(seed))
        assert ok == bool(g["%s_success" % name]) and np.array_equal(i1, g["%s_inliers1" % name])
        assert np.array_equal(R, Rs) and np.array_equal(T, Ts.ravel())


@pytest.mark.gpu
def test_run_sequence_key_point_files_equal_the_staged_loop(engine, tmp_path):
    """run_sequence.py --keypts-source usip / 3dfeatnet (files written here) against a loop over the staged API -- Voxelization,
    GetPatchesList, GetFeaturesFromPatches, SolveRelativePose with the same per-pair seeds -- chained and written the same way."""
    from caelo import api, keysources, stageio, synth
    from caelo.engine import ENCODER_H5
    n, base = 6, 1000
    rs = np.random.RandomState(8)
    scans_ = [synth.make_scan(i, quantum=None, scene_kind="boxes", trajectory="circuit") for i in range(n)]
    pts = {}
    for i, pc in enumerate(scans_):
        k = 250 + 40 * i
        p = (pc[rs.choice(pc.shape[0], k, replace=False), 0:3] + rs.normal(0, 0.05, (k, 3))).astype(np.float32)
        keysources.write_usip(keysources.keypts_path(tmp_path / "usip", i), (keysources.R90.T @ p.T).T)
        keysources.write_3dfeatnet(keysources.keypts_path(tmp_path / "fn", i), p)
    enc = api.load_model(ENCODER_H5)
    script = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")
    for src, d in (("usip", "usip"), ("3dfeatnet", "fn")):
        out = str(tmp_path / ("%s.txt" % src))
        r = subprocess.run([sys.executable, script, "--synthetic", str(n), "--keypts-source", src, "--keypts-dir", str(tmp_path / d),
                            "--seed-base", str(base), "--batch", "4", "--chunk", "4", "--out", out], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        rel = []
        feats = []
        for i in range(n):
            kp = keysources.load_keypts(src, str(tmp_path / d), i)
            vox = api.Voxelization(scans_[i])[6:9]
            _, plist = api.GetPatchesList(kp, *vox)
            feats.append((kp, api.GetFeaturesFromPatches(enc, plist)))
            if i:
                (a, fa), (b, fb) = feats[i - 1], feats[i]
                R, T, ok, _, _, _ = api.SolveRelativePose(a, fa, None, b, fb, None, rng=np.random.RandomState(base + i - 1))
                rel.append(np.r_[np.asarray(R, np.float32).ravel(), np.asarray(T, np.float32).ravel()])
        want = str(tmp_path / ("%s_staged.txt" % src))
        stageio.write_poses(want, stageio.chain_poses(np.array(rel, np.float32), None))
        assert open(out, "rb").read() == open(want, "rb").read(), src
