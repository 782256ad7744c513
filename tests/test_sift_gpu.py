"""SIFT3D key points on the device (caelo_sift_octave, caelo_voxel_centroids, csrc/sift.hip; Engine.sift_octave / voxel_centroids /
sift_keypoints) against the float64 NumPy restatement of the definition (tests/sift_ref.py) on scenes whose decisions
tests/test_sift_host.py certifies; the tile, chunk, scale-count, radius, tie and degenerate boundaries; the pyramid's stop; padded and
ragged batches against single calls; determinism; api.KeyPtsBySIFT; detect_sift_keypoints.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import iss_ref  # noqa: E402
import sift_ref  # noqa: E402

pytestmark = pytest.mark.gpu
# The dog bar: a tenth of the certified decision margins (1e-7), which is what makes every decision of a certified scene exact.
DOG_ATOL = 1e-8
S11 = sift_ref.scales(0.5, 8)


@pytest.fixture(scope="module")
def eng():
    from caelo.engine import Engine
    return Engine(respond_h5=None, encoder_h5=None)


def run(eng, P, n_pts=None, sigma=S11, min_contrast=0.1):
    r = eng.sift_octave(torch.from_numpy(np.ascontiguousarray(P)).to(eng.device), n_pts=n_pts, sigma=sigma, min_contrast=min_contrast, knn=True)
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def keys_of(d):
    """The key point list of a single-cloud result, after checking its shape: n_key indices ascending, -1 behind them, and exactly the
    rows with a non-zero mask."""
    k = int(d["n_key"])
    idx = d["key_idx"]
    assert (idx[k:] == -1).all() and (np.diff(idx[:k]) > 0).all() and (k == 0 or (idx[0] >= 0 and idx[k - 1] < idx.shape[0]))
    assert np.array_equal(idx[:k], np.flatnonzero(d["key_mask"]))
    return idx[:k]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_octave(d, ref, what):
    """One single-cloud device result against ``sift_ref.octave``: knn, masks and keys exact, dog within the bar -> the worst dog difference."""
    err = float(np.abs(d["dog"] - ref["dog"]).max()) if ref["dog"].size else 0.0
    print("%s: %d points, %d scales, %d key points, worst dog difference %.3g" % (what, ref["dog"].shape[0], ref["dog"].shape[1] + 1, len(ref["key_idx"]), err))
    assert d["dog"].shape == ref["dog"].shape and err <= DOG_ATOL
    assert np.array_equal(d["knn"], ref["knn"])
    assert np.array_equal(d["key_mask"], ref["key_mask"])
    assert int(d["n_key"]) == len(ref["key_idx"]) and np.array_equal(keys_of(d), ref["key_idx"])
    return err


@pytest.mark.parametrize("seed,n,kw", sift_ref.SCENES, ids=sift_ref.scene_id)
def test_parity_with_the_restatement(eng, seed, n, kw):
    P, ref = sift_ref.reference(seed, n, kw)
    r, octs = eng.sift_keypoints(torch.from_numpy(P).to(eng.device), details=True, **kw)
    assert len(octs) == len(ref["octaves"])
    worst = 0.0
    for o, ro in zip(octs, ref["octaves"]):
        assert o["octave"] == ro["octave"] and o["scale"] == ro["scale"] and o["frames"] == [0]
        cloud = o["clouds"][0].cpu().numpy()
        assert cloud.shape == ro["cloud"].shape and same_bits(cloud, ro["cloud"])          # the centroids: bit-equal
        assert same_bits(o["sigma"], ro["result"]["sigma"])
        d = {k: getattr(o["result"], k)[0].cpu().numpy() for k in o["result"]._fields}
        worst = max(worst, check_octave(d, ro["result"], "scene %d n %d %s octave %d" % (seed, n, kw, o["octave"])))
    print("scene %d n %d %s: worst dog difference over the octaves %.3g" % (seed, n, kw, worst))
    k = int(r.n_key.item())
    assert k == ref["xyz"].shape[0] and r.xyz.shape == (k, 3) and r.scale.shape == (k,) and r.octave.shape == (k,)
    assert same_bits(r.xyz.cpu().numpy(), ref["xyz"]) and same_bits(r.scale.cpu().numpy(), ref["scale"])
    assert same_bits(r.octave.cpu().numpy(), ref["octave"])


@pytest.mark.parametrize("n_scales", [3, 19])
@pytest.mark.parametrize("seed,n", [(9, 1500), (3, 1025), (4, 257), (5, 600)])
def test_one_octave_at_the_edges_of_the_walk(eng, seed, n, n_scales):
    """The entry point alone, scales handed in, on the raw scenes: a partial last tile (1500), one point past a chunk (1025), one past
    a tile (257), less than a chunk (600), with the fewest and the most scales it takes.  The masks are compared where the restatement
    certifies them, which it does for all eight (an input condition, asserted)."""
    P = iss_ref.scene(seed, n)
    sigma = np.array([0.5, 0.75, 1.25]) if n_scales == 3 else 0.3 * 2.0 ** (np.arange(19) / 12.0)
    ref = sift_ref.octave(P, sigma, 0.02)
    d = run(eng, P, sigma=sigma, min_contrast=0.02)
    err = float(np.abs(d["dog"] - ref["dog"]).max())
    contrast, gap, d2_gap = sift_ref.margins(ref)
    print("scene %d n %d S %d: worst dog difference %.3g; margins %.3g %.3g %.3g; %d key points" % (seed, n, n_scales, err, contrast, gap, d2_gap, len(ref["key_idx"])))
    assert d["dog"].shape == (n, n_scales - 1) and err <= DOG_ATOL
    assert np.array_equal(d["knn"], ref["knn"])
    if n_scales == 3:
        assert not d["key_mask"].any() and int(d["n_key"]) == 0   # D = 2: there is no level between two others
    else:
        assert min(contrast, gap) >= iss_ref.CERTIFIED
        assert np.array_equal(d["key_mask"], ref["key_mask"]) and np.array_equal(keys_of(d), ref["key_idx"]) and len(ref["key_idx"]) > 0


@pytest.mark.parametrize("n", [1, 24, 25])
def test_fewer_points_than_and_exactly_25(eng, n):
    """Under 25 points nothing is a key and dog is still written; with exactly 25 every point's neighbourhood is the whole cloud, and
    three points are keys (the scene shrunk to 4 x 4 x 1 m, exactly, so that everybody is within reach of everybody)."""
    P = (iss_ref.scene(6, 25) * np.float32(0.25))[:n]
    ref = sift_ref.octave(P, S11, 0.0)
    d = run(eng, P, min_contrast=0.0)
    assert np.abs(d["dog"] - ref["dog"]).max() <= DOG_ATOL and np.array_equal(d["knn"], ref["knn"])
    if n < 25:
        assert int(d["n_key"]) == 0 and (d["key_idx"] == -1).all() and not d["key_mask"].any()
        assert (d["knn"][:, :n] >= 0).all() and (d["knn"][:, n:] == -1).all()
        assert n == 1 or d["dog"].any()
    else:
        assert (np.sort(d["knn"], axis=1) == np.arange(25)[None, :]).all() and (d["knn"][:, 0] == np.arange(25)).all()
        assert min(sift_ref.margins(ref)[:2]) >= iss_ref.CERTIFIED     # an input condition
        assert np.array_equal(d["key_mask"], ref["key_mask"]) and keys_of(d).tolist() == [5, 10, 22]


def test_the_radius_is_not_strict(eng):
    """sigma = (0.25, 0.5, 1): a point at exactly 1.5 m = 3 sigma_1 counts at sigma_1 (<=), so dog[0][0] = resp_1 - resp_0 =
    1.5 w / (1 + w) with w = exp(-4.5); at 1.5 + 1/64 m it does not, and dog[0][0] is the bits of 0.0."""
    sg = np.array([0.25, 0.5, 1.0])
    w = math.exp(-4.5)
    on = run(eng, sift_ref.two_points(1.5), sigma=sg, min_contrast=0.0)
    off = run(eng, sift_ref.two_points(1.5 + 1.0 / 64.0), sigma=sg, min_contrast=0.0)
    assert abs(on["dog"][0, 0] - 1.5 * w / (1.0 + w)) < 1e-15 and abs(on["dog"][1, 0] - (1.5 / (1.0 + w) - 1.5)) < 1e-15
    assert same_bits(off["dog"][:, 0], np.zeros(2)) and off["dog"][0, 1] != 0.0
    for d, far in ((on, 1.5), (off, 1.5 + 1.0 / 64.0)):
        ref = sift_ref.octave(sift_ref.two_points(far), sg, 0.0)
        assert np.abs(d["dog"] - ref["dog"]).max() <= 1e-15 and np.array_equal(d["knn"], ref["knn"]) and int(d["n_key"]) == 0
        assert np.array_equal(d["dog"] == 0.0, ref["dog"] == 0.0)


def test_distance_ties_go_to_the_lower_index(eng):
    """A shuffled 5 x 5 x 5 lattice of pitch 1/4 m: every d2 is exact, most tie, and the 25th neighbour is decided by the index."""
    P = sift_ref.lattice()
    ref = sift_ref.octave(P, [0.25, 0.5, 1.0], 0.0)
    d = run(eng, P, sigma=[0.25, 0.5, 1.0], min_contrast=0.0)
    Pd = P.astype(np.float64)
    d2 = ((Pd[:, None, :] - Pd[None, :, :]) ** 2).sum(axis=2)
    tied = sum(1 for i in range(125) if np.sort(d2[i])[24] == np.sort(d2[i])[25])
    assert tied > 100 and np.array_equal(d["knn"], ref["knn"]) and (d["knn"][:, 0] == np.arange(125)).all()
    assert np.abs(d["dog"] - ref["dog"]).max() <= DOG_ATOL


def test_an_exact_plane_and_the_tie_cluster(eng):
    """z = 0: every dog is the bits of 0.0 and, at min_contrast 0, nothing is a key -- v < mn[s +- 1] fails on equal values.  The
    cluster and its copy 32 m away: dog, the neighbours relative to the cluster, and the masks of point k and k + 40 are bit-equal."""
    P = iss_ref.exact_plane()
    d = run(eng, P, min_contrast=0.0)
    assert same_bits(d["dog"], np.zeros((200, 10))) and int(d["n_key"]) == 0 and not d["key_mask"].any() and (d["key_idx"] == -1).all()
    assert np.array_equal(d["knn"], sift_ref.octave(P, S11, 0.0)["knn"])
    T = iss_ref.tie_cluster()
    t = run(eng, T, min_contrast=0.0)
    ref = sift_ref.octave(T, S11, 0.0)
    assert same_bits(t["dog"][:40], t["dog"][40:]) and np.array_equal(t["knn"][:40] + 40, t["knn"][40:])
    assert np.array_equal(t["key_mask"][:40], t["key_mask"][40:]) and np.array_equal(t["knn"], ref["knn"])
    assert np.abs(t["dog"] - ref["dog"]).max() <= DOG_ATOL
    keys_of(t)


def test_the_pyramid_stops_under_25_points(eng):
    """n_octaves = 6 on the 257-point scene: octave 3 still holds 32 points, octave 4 does not reach 25, and nothing runs from there."""
    P = iss_ref.scene(4, 257)
    ref = sift_ref.pyramid(P, n_octaves=6)
    assert ref["stopped_at"] == 4 and len(ref["octaves"]) == 4
    r, octs = eng.sift_keypoints(torch.from_numpy(P).to(eng.device), details=True, n_octaves=6)
    assert [o["octave"] for o in octs] == [0, 1, 2, 3]
    assert [int(o["clouds"][0].shape[0]) for o in octs] == [o["cloud"].shape[0] for o in ref["octaves"]]
    assert same_bits(r.xyz.cpu().numpy(), ref["xyz"]) and same_bits(r.octave.cpu().numpy(), ref["octave"])
    assert same_bits(r.xyz.cpu().numpy(), sift_ref.reference(4, 257, {})[1]["xyz"])     # the same as four octaves
    few = eng.sift_keypoints(torch.from_numpy(P[:24]).to(eng.device))
    assert int(few.n_key.item()) == 0 and few.xyz.shape == (0, 3)


def check_frames(eng, batch, frames):
    for f, p in enumerate(frames):
        n = p.shape[0]
        assert not batch["dog"][f, n:].any() and (batch["knn"][f, n:] == -1).all() and not batch["key_mask"][f, n:].any()
        if n == 0:
            continue
        one = run(eng, p)
        nk = int(one["n_key"])
        assert int(batch["n_key"][f]) == nk and nk > 0
        assert same_bits(batch["key_idx"][f, :nk], one["key_idx"][:nk]) and (batch["key_idx"][f, nk:] == -1).all()
        for k in ("dog", "knn", "key_mask"):
            assert same_bits(np.ascontiguousarray(batch[k][f, :n]), one[k]), (f, k)


def test_a_padded_batch_equals_single_calls_and_repeats_itself(eng):
    """Three frames of 1500, 0 and 257 points in ld = 1536, the padding rows NaN: every frame's results are the single-cloud call's
    bits, the empty frame has no key points, a second call returns the same bytes, and the pyramid over the batch gives each frame the
    rows of its own call."""
    frames = [iss_ref.scene(9, 1500), np.zeros((0, 3), np.float32), iss_ref.scene(4, 257)]
    counts = [1500, 0, 257]
    pts = np.full((3, 1536, 3), np.nan, np.float32)
    for f, p in enumerate(frames):
        pts[f, :counts[f]] = p
    batch = run(eng, pts, n_pts=counts)
    again = run(eng, pts, n_pts=torch.tensor(counts, dtype=torch.int32, device=eng.device))
    for k in batch:
        assert same_bits(batch[k], again[k]), k
    assert batch["n_key"].tolist()[1] == 0 and (batch["key_idx"][1] == -1).all()
    check_frames(eng, batch, frames)
    r = eng.sift_keypoints(torch.from_numpy(pts).to(eng.device), n_pts=counts)
    assert r.n_key.tolist()[1] == 0
    for f, (seed, n) in ((0, (9, 1500)), (2, (4, 257))):
        ref = sift_ref.reference(seed, n, {})[1]
        k = int(r.n_key[f].item())
        assert k == ref["xyz"].shape[0] and same_bits(r.xyz[f, :k].cpu().numpy(), ref["xyz"])
        assert same_bits(r.scale[f, :k].cpu().numpy(), ref["scale"]) and same_bits(r.octave[f, :k].cpu().numpy(), ref["octave"])
        assert not r.xyz[f, k:].any() and (r.octave[f, k:] == -1).all()


def test_a_batch_of_frames_with_different_point_counts(eng):
    """600, 1025 and 257 points under ld = 1025, the padding rows a finite point inside the scene: bit for bit the single calls."""
    frames = [iss_ref.scene(5, 600), iss_ref.scene(3, 1025), iss_ref.scene(4, 257)]
    pts = np.full((3, 1025, 3), 8.0, np.float32)   # inside the scene: a padding row that reached a decision would change it
    for f, p in enumerate(frames):
        pts[f, :p.shape[0]] = p
    check_frames(eng, run(eng, pts, n_pts=[600, 1025, 257]), frames)


def test_more_frames_than_one_launch_takes(eng):
    """65 537 frames of 0 .. 4 points under ld = 4: the entry point slices them at 65 535.  dog is the bits of two calls on the frames
    before and from the cut and of the single-cloud calls at both ends of both slices; no frame reaches 25 points, so nothing is a key."""
    pts, n_pts = iss_ref.many_frames()
    cut = 65535
    whole = run(eng, pts, n_pts=n_pts)
    head, tail = run(eng, pts[:cut], n_pts=n_pts[:cut]), run(eng, pts[cut:], n_pts=n_pts[cut:])
    for k in whole:
        assert same_bits(whole[k], np.concatenate([head[k], tail[k]])), k
    assert not whole["n_key"].any() and (whole["key_idx"] == -1).all() and not whole["key_mask"].any()
    assert whole["dog"][3].any() and whole["dog"][cut - 1].any()
    for f in (0, cut - 1, cut, cut + 1):
        n = int(n_pts[f])
        one = run(eng, pts[f, :n])
        assert same_bits(np.ascontiguousarray(whole["dog"][f, :n]), one["dog"]) and not whole["dog"][f, n:].any()
        assert same_bits(np.ascontiguousarray(whole["knn"][f, :n]), one["knn"]) and (whole["knn"][f, n:] == -1).all()
    ref = sift_ref.octave(pts[cut - 1, :int(n_pts[cut - 1])], S11, 0.1)
    assert int(n_pts[cut - 1]) == 4 and np.abs(whole["dog"][cut - 1] - ref["dog"]).max() <= DOG_ATOL


def test_refusals_leave_the_context_usable(eng):
    P, ref = sift_ref.reference(4, 257, {})
    dev = torch.from_numpy(P).to(eng.device)
    bad = P.copy()
    bad[100, 2] = np.nan
    with pytest.raises(ValueError):
        run(eng, bad)
    run(eng, bad, n_pts=[100])   # the NaN sits past n_pts: not the frame's
    with pytest.raises(ValueError):
        eng.sift_keypoints(torch.from_numpy(bad).to(eng.device))
    with pytest.raises(ValueError):
        eng.sift_octave(torch.zeros((32769, 3), device=eng.device), sigma=S11)
    for sigma in (S11[::-1].copy(), [0.5, 1.0], np.linspace(0.5, 2.0, 20), [0.5, 0.5, 1.0], [0.0, 0.5, 1.0], None):
        with pytest.raises(ValueError):
            eng.sift_octave(dev, sigma=sigma)
    with pytest.raises(ValueError):
        run(eng, P, min_contrast=-0.1)
    for kw in (dict(min_contrast=-0.1), dict(salient_radius=2.0), dict(n_octaves=0), dict(n_scales_per_octave=17), dict(min_scale=0.0)):
        with pytest.raises(ValueError):
            eng.sift_keypoints(dev, **kw)
    with pytest.raises(ValueError):
        eng.sift_octave(dev[None], n_pts=[258], sigma=S11)
    with pytest.raises(ValueError):
        eng.voxel_centroids(dev, 0.0)
    assert eng.sift_octave(dev, sigma=S11).knn is None
    r = eng.sift_keypoints(dev)
    assert same_bits(r.xyz.cpu().numpy(), ref["xyz"]) and same_bits(r.scale.cpu().numpy(), ref["scale"])


def test_voxel_centroids_alone(eng):
    """The raw scenes at three leaves, a leaf that is no power of two among them, and the empty cloud: the restatement's bits."""
    for (seed, n), leaf in (((9, 1500), 0.5), ((3, 1025), 0.3), ((4, 257), 2.0)):
        P = iss_ref.scene(seed, n)
        c = eng.voxel_centroids(torch.from_numpy(P).to(eng.device), leaf).cpu().numpy()
        assert same_bits(c, sift_ref.centroids(P, leaf)) and 0 < c.shape[0] < n
    assert eng.voxel_centroids(torch.zeros((0, 3), device=eng.device), 0.5).shape == (0, 3)


def test_api_key_points_equal_the_engine_call(engine):
    from caelo import api
    P, ref = sift_ref.reference(5, 600, {})
    r = engine.sift_keypoints(torch.from_numpy(P).to(engine.device))
    assert same_bits(r.xyz.cpu().numpy(), ref["xyz"])
    pc4 = np.c_[P, np.ones(len(P), np.float32)].astype(np.float32)
    kp = api.KeyPtsBySIFT(pc4)
    assert isinstance(kp, np.ndarray) and kp.dtype == np.float32 and same_bits(kp, ref["xyz"])
    on_dev = api.KeyPtsBySIFT(torch.from_numpy(P).to(engine.device), min_scale=0.25, n_octaves=2, n_scales_per_octave=4, min_contrast=0.05)
    r2 = engine.sift_keypoints(torch.from_numpy(P).to(engine.device), min_scale=0.25, n_octaves=2, n_scales_per_octave=4, min_contrast=0.05)
    assert on_dev.is_cuda and int(r2.n_key.item()) > 0 and same_bits(on_dev.cpu().numpy(), r2.xyz.cpu().numpy())
    with pytest.raises(ValueError):
        api.KeyPtsBySIFT(P[:, :2])


def test_detect_sift_keypoints_end_to_end(eng, scans, tmp_path, capsys):
    """Three small synthetic scans -> detect_sift_keypoints.main -> files that keysources.read_3dfeatnet reads as [256,3];
    their leading rows are Engine.sift_keypoints' xyz rows on the same thinned cloud, the rest are points of that cloud; a second run
    with the same seed writes the same bytes; --radius is refused."""
    import detect_keypoints
    import detect_sift_keypoints
    from caelo import keysources
    scans_dir, out_dir, out_again = tmp_path / "velodyne", tmp_path / "sift", tmp_path / "sift_again"
    scans_dir.mkdir()
    frames = (0, 1, 2)
    clouds = [scans(f, n_az=500, quantum=1e-3) for f in frames]
    for f, s in zip(frames, clouds):
        s.tofile(str(scans_dir / ("%06d.bin" % f)))
    argv = ["--scans", str(scans_dir), "--keypoints", "256", "--max-points", "4096", "--seed", "3", "--batch", "2"]
    detect_sift_keypoints.main(argv + ["--out", str(out_dir)])
    said = capsys.readouterr().out
    assert "SIFT3D found" in said and "ISS" not in said and "Harris" not in said
    detect_sift_keypoints.main(["--method", "sift"] + argv + ["--out", str(out_again)])
    with pytest.raises(SystemExit):
        detect_sift_keypoints.main(argv + ["--radius", "1.0", "--out", str(tmp_path / "refused")])
    assert not (tmp_path / "refused").exists()
    for f, s in zip(frames, clouds):
        path = keysources.keypts_path(str(out_dir), f)
        assert open(path, "rb").read() == open(keysources.keypts_path(str(out_again), f), "rb").read()
        kp = keysources.read_3dfeatnet(path)
        assert kp.shape == (256, 3) and kp.dtype == np.float32
        pc, _ = detect_keypoints.prepare(eng, s, f, 0.2, 4096, 3)
        assert 256 < pc.shape[0] <= 4096
        r = eng.sift_keypoints(pc)
        m = int(r.n_key.item())
        cloud = pc.cpu().numpy()
        assert m > 0
        if m <= 256:
            assert same_bits(kp[:m], r.xyz.cpu().numpy())
            assert {tuple(p) for p in kp[m:]} <= {tuple(p) for p in cloud}
        else:
            assert {tuple(p) for p in kp} <= {tuple(p) for p in r.xyz.cpu().numpy()}
