"""ISS key points on the device (caelo_iss_keypoints, csrc/iss.hip) against the float64 NumPy restatement of the definition
(tests/iss_ref.py) on scenes whose decisions tests/test_iss_host.py certifies to be at least 1e-7 away from flipping; the tile, chunk,
radius, tie and degenerate boundaries; a padded batch against single calls; determinism; refusals; and detect_keypoints.py end to end."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import iss_ref  # noqa: E402

pytestmark = pytest.mark.gpu
EIG_RTOL = 1e-13   # per eigenvalue, in units of e1: two symmetric 3 x 3 solvers each err by a few ulp of ||C|| (2.2e-16): ~100 x that


@pytest.fixture(scope="module")
def eng():
    from caelo.engine import Engine
    return Engine(respond_h5=None, encoder_h5=None)


def run(eng, P, n_pts=None, **kw):
    r = eng.iss_keypoints(torch.from_numpy(np.ascontiguousarray(P)).to(eng.device), n_pts=n_pts, eig=True, **kw)
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def keys_of(d):
    """The key point list of a single-cloud result, after checking its shape: n_key indices ascending, -1 behind them."""
    k = int(d["n_key"])
    idx = d["key_idx"]
    assert (idx[k:] == -1).all() and (np.diff(idx[:k]) > 0).all() and (k == 0 or (idx[0] >= 0 and idx[k - 1] < idx.shape[0]))
    return idx[:k]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("seed,n,kw", iss_ref.SCENES, ids=lambda v: "cut" if v == iss_ref.CUT else ("dflt" if v == {} else str(v)))
def test_parity_with_the_restatement(eng, seed, n, kw):
    P, ref = iss_ref.reference(seed, n, kw)
    d = run(eng, P, **kw)
    assert np.array_equal(d["n_neigh"], ref["n_neigh"])
    e1 = np.maximum(ref["eig"][:, 0:1], np.finfo(np.float64).tiny)
    err = float((np.abs(d["eig"] - ref["eig"]) / e1).max())
    print("scene %d n %d: worst eigenvalue difference %.3g e1" % (seed, n, err))
    assert err <= EIG_RTOL
    assert (d["eig"][ref["n_neigh"] < ref["params"]["min_neighbors"]] == 0).all()
    cand = d["saliency"] >= 0
    assert np.array_equal(cand, ref["candidate"])
    assert (d["saliency"][~cand] == -1.0).all() and np.array_equal(d["saliency"][cand], d["eig"][cand, 2])
    assert int(d["n_key"]) == len(ref["key_idx"])
    assert np.array_equal(keys_of(d), ref["key_idx"])


@pytest.mark.parametrize("n", [1, 4, 5])
def test_fewer_points_than_and_exactly_min_neighbors(eng, n):
    """Points 1/8 m apart on a bent line: with n < 5 nobody has min_neighbors neighbours; with n = 5 everybody has exactly 5."""
    P = np.float32([[k / 8.0, (k * k) / 64.0, (k % 3) / 16.0] for k in range(n)])
    ref = iss_ref.iss(P)
    d = run(eng, P)
    assert d["n_neigh"].tolist() == [n] * n and np.array_equal(d["n_neigh"], ref["n_neigh"])
    if n < 5:
        assert (d["saliency"] == -1.0).all() and not d["eig"].any() and int(d["n_key"]) == 0 and (d["key_idx"] == -1).all()
    else:
        assert np.array_equal(d["saliency"] >= 0, ref["candidate"]) and ref["candidate"].any()
        assert np.abs(d["eig"] - ref["eig"]).max() <= EIG_RTOL * ref["eig"].max()
        assert np.array_equal(keys_of(d), ref["key_idx"])


def test_the_radius_is_strict(eng):
    out = run(eng, iss_ref.strict_radius(False))
    assert out["n_neigh"][0] == 4 and out["saliency"][0] == -1.0 and not out["eig"][0].any()
    inside = run(eng, iss_ref.strict_radius(True))
    assert inside["n_neigh"][0] == 5 and inside["eig"][0, 0] > 0
    for d, b in ((out, False), (inside, True)):
        assert np.array_equal(d["n_neigh"], iss_ref.iss(iss_ref.strict_radius(b))["n_neigh"])


def test_equal_saliencies_both_survive(eng):
    """The cluster and its copy 32 m away: all sums are exact, so the saliencies are bit-equal pairwise and the key points come in
    mirrored pairs, index k and k + 40 (the restatement gives 12 and 52 for this cluster).  The two halves are out of each other's
    reach, so the second case puts two equal saliencies into ONE neighbourhood: the hand case of tests/test_iss_host.py, whose points
    5 and 6 see each other, have saliency 0.5 both, and both survive."""
    T = iss_ref.tie_cluster()
    d = run(eng, T)
    assert same_bits(d["saliency"][:40], d["saliency"][40:]) and same_bits(d["eig"][:40], d["eig"][40:])
    k = keys_of(d)
    assert k.tolist() == [12, 52] and np.array_equal(k[: len(k) // 2] + 40, k[len(k) // 2:])
    a, b, c = 0.75, 0.5, 0.25
    P = np.float32([[0, 0, 0], [a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c], [0, 0, -c]])
    h = run(eng, P)
    assert h["saliency"].tolist() == [0.125] * 5 + [0.5, 0.5] and keys_of(h).tolist() == [5, 6]   # neighbours with equal saliency
    assert h["eig"][0].tolist() == [1.125, 0.5, 0.125]   # a diagonal C is its own eigenvalues, exactly


def test_an_exact_plane_has_no_key_points(eng):
    """z = 0 on dyadic points: the z row and column of every C are exactly zero and stay an exactly zero eigenvalue."""
    d = run(eng, iss_ref.exact_plane())
    assert (d["n_neigh"] >= 5).all() and (d["eig"][:, 2] == 0).all() and (d["eig"][:, 1] > 0).all()
    assert d["saliency"].max() <= 0 and int(d["n_key"]) == 0 and (d["key_idx"] == -1).all()


def test_a_padded_batch_equals_single_calls_and_repeats_itself(eng):
    """Three frames of 1500, 0 and 257 points in ld = 1536, the padding rows NaN: every frame's results are the single-cloud call's
    bits, the empty frame has no key points, and a second call returns the same bytes."""
    frames = [iss_ref.reference(*iss_ref.SCENES[0])[0], np.zeros((0, 3), np.float32), iss_ref.reference(*iss_ref.SCENES[3])[0]]
    counts = [f.shape[0] for f in frames]
    assert counts == [1500, 0, 257]
    pts = np.full((3, 1536, 3), np.nan, np.float32)
    for f, p in enumerate(frames):
        pts[f, :counts[f]] = p
    batch = run(eng, pts, n_pts=counts)
    again = run(eng, pts, n_pts=torch.tensor(counts, dtype=torch.int32, device=eng.device))
    for k in batch:
        assert same_bits(batch[k], again[k]), k
    assert batch["n_key"].tolist()[1] == 0 and (batch["key_idx"][1] == -1).all()
    for f, p in enumerate(frames):
        n = counts[f]
        assert (batch["saliency"][f, n:] == -1.0).all() and not batch["eig"][f, n:].any() and not batch["n_neigh"][f, n:].any()
        if n == 0:
            continue
        one = run(eng, p)
        nk = int(one["n_key"])
        assert int(batch["n_key"][f]) == nk and nk > 0
        assert same_bits(batch["key_idx"][f, :nk], one["key_idx"][:nk]) and (batch["key_idx"][f, nk:] == -1).all()
        for k in ("saliency", "eig", "n_neigh"):
            assert same_bits(np.ascontiguousarray(batch[k][f, :n]), one[k]), (f, k)


def test_more_frames_than_one_launch_takes(eng):
    """65 537 frames of 0 .. 4 points under ld = 4: the entry point slices them at 65 535.  Every output is the bits of two calls on
    the frames before and from the cut, the frames at both ends of both slices are their single-cloud calls, and the neighbour counts
    are NumPy's over all frames."""
    kw = dict(salient_radius=1.0, non_max_radius=1.0, min_neighbors=3)
    pts, n_pts = iss_ref.many_frames()
    cut = 65535
    assert pts.shape == (cut + 2, 4, 3)
    whole = run(eng, pts, n_pts=n_pts, **kw)
    head, tail = run(eng, pts[:cut], n_pts=n_pts[:cut], **kw), run(eng, pts[cut:], n_pts=n_pts[cut:], **kw)
    for k in whole:
        assert same_bits(whole[k], np.concatenate([head[k], tail[k]])), k
    assert np.array_equal(whole["n_neigh"], iss_ref.neighbour_counts(pts, n_pts, 1.0))
    assert whole["n_key"].sum() > 0 and whole["n_neigh"][cut + 1].tolist() == [1, 0, 0, 0]
    for f in (0, cut - 1, cut, cut + 1):
        n = int(n_pts[f])
        one = run(eng, pts[f, :n], **kw)
        nk = int(one["n_key"])
        assert int(whole["n_key"][f]) == nk and same_bits(whole["key_idx"][f, :nk], one["key_idx"][:nk]) and (whole["key_idx"][f, nk:] == -1).all()
        for k in ("saliency", "eig", "n_neigh"):
            assert same_bits(np.ascontiguousarray(whole[k][f, :n]), one[k]), (f, k)


def test_refusals_leave_the_context_usable(eng):
    P = iss_ref.reference(*iss_ref.SCENES[3])[0]
    bad = P.copy()
    bad[100, 2] = np.nan
    with pytest.raises(ValueError):
        run(eng, bad)
    run(eng, bad, n_pts=[100])   # the NaN sits past n_pts: not the frame's
    with pytest.raises(ValueError):
        eng.iss_keypoints(torch.zeros((32769, 3), device=eng.device))
    with pytest.raises(ValueError):
        run(eng, P, salient_radius=0.0)
    with pytest.raises(ValueError):
        run(eng, P, min_neighbors=0)
    with pytest.raises(ValueError):
        run(eng, P[None], n_pts=[258])
    ref = iss_ref.reference(*iss_ref.SCENES[3])[1]
    assert np.array_equal(keys_of(run(eng, P)), ref["key_idx"])


def test_detect_keypoints_end_to_end(eng, engine, scans, tmp_path):
    """Three synthetic scans -> detect_keypoints.main -> files that keysources.read_3dfeatnet reads as [1024,3]; their leading rows are
    Engine.iss_keypoints on the same thinned cloud, the rest are points of that cloud, and Engine.extract takes them as key points."""
    sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
    import detect_keypoints
    from caelo import keysources
    scans_dir, out_dir = tmp_path / "velodyne", tmp_path / "iss"
    scans_dir.mkdir()
    frames = (0, 1, 2)
    clouds = [scans(f, quantum=1e-3) for f in frames]
    for f, s in zip(frames, clouds):
        s.tofile(str(scans_dir / ("%06d.bin" % f)))
    detect_keypoints.main(["--method", "iss", "--scans", str(scans_dir), "--out", str(out_dir), "--keypoints", "1024", "--seed", "3",
                           "--batch", "2"])
    for f, s in zip(frames, clouds):
        kp = keysources.read_3dfeatnet(keysources.keypts_path(str(out_dir), f))
        assert kp.shape == (1024, 3) and kp.dtype == np.float32
        pc, _ = detect_keypoints.prepare(eng, s, f, 0.2, 16384, 3)
        assert 1024 < pc.shape[0] <= 16384
        r = eng.iss_keypoints(pc)
        m = int(r.n_key.item())
        cloud = pc.cpu().numpy()
        assert 0 < m <= 1024 and np.array_equal(kp[:m], cloud[r.key_idx[:m].cpu().numpy()])
        assert {tuple(p) for p in kp[m:]} <= {tuple(p) for p in cloud}
        ff = engine.extract(torch.from_numpy(s).to(engine.device), key_pts=torch.from_numpy(kp).to(engine.device))
        assert int(ff.n_key.item()) == 1024 and int(ff.status[0].item()) == 0
        assert (ff.rows[:1024, 63].cpu().numpy() == 1.0).all()
    xyz_dir = tmp_path / "xyz"
    detect_keypoints.main(["--method", "iss", "--scans", str(scans_dir), "--out", str(xyz_dir), "--layout", "xyz", "--no-ensure", "--seed", "3"])
    raw = np.fromfile(keysources.keypts_path(str(xyz_dir), 0), dtype=np.float32).reshape(-1, 3)
    first = keysources.read_3dfeatnet(keysources.keypts_path(str(out_dir), 0))
    assert 0 < raw.shape[0] <= 1024 and np.array_equal(raw, first[:raw.shape[0]])
