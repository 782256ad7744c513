"""Harris3D key points on the device (caelo_harris_keypoints, csrc/harris.hip) against the float64 NumPy restatement of the definition
(tests/harris_ref.py) on scenes whose normals and decisions tests/test_harris_host.py certifies; the tile, chunk, radius, tie and
degenerate boundaries; padded and ragged batches against single calls; determinism; api.KeyPtsByHarris; detect_keypoints.py."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import harris_ref  # noqa: E402
import iss_ref  # noqa: E402

pytestmark = pytest.mark.gpu
# The response bar: a tenth of the certified decision margins (1e-7), which is what makes every decision of a certified scene exact.
RESPONSE_ATOL = 1e-8
# The normal bar: two symmetric 3 x 3 solvers each err by a few ulp of ||C|| (2.2e-16) in the matrix; the eigenvector of the smallest
# eigenvalue moves by that over the relative gap to the next one, certified >= 1e-5: 50 ulp / 1e-5 = 1.1e-9, and ~10 x that.
NORMAL_ATOL = 1e-8
SIGN_FREE = 1e-6    # |n . p| < SIGN_FREE |p|: the orientation test is within rounding of zero, the sign is compared freely
SIGN_FREE_SHARE = 0.01


@pytest.fixture(scope="module")
def eng():
    from caelo.engine import Engine
    return Engine(respond_h5=None, encoder_h5=None)


def run(eng, P, n_pts=None, **kw):
    r = eng.harris_keypoints(torch.from_numpy(np.ascontiguousarray(P)).to(eng.device), n_pts=n_pts, normals=True, **kw)
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def keys_of(d):
    """The key point list of a single-cloud result, after checking its shape: n_key indices ascending, -1 behind them."""
    k = int(d["n_key"])
    idx = d["key_idx"]
    assert (idx[k:] == -1).all() and (np.diff(idx[:k]) > 0).all() and (k == 0 or (idx[0] >= 0 and idx[k - 1] < idx.shape[0]))
    return idx[:k]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def valid_of(d):
    """The valid mask as the device reports it: a response of -1 and a zero normal together, or neither."""
    inv = d["response"] == -1.0
    assert np.array_equal(inv, ~d["normals"].any(axis=-1))
    return ~inv


@pytest.mark.parametrize("seed,n,kw", harris_ref.SCENES, ids=harris_ref.scene_id)
def test_parity_with_the_restatement(eng, seed, n, kw):
    P, ref = harris_ref.reference(seed, n, kw)
    d = run(eng, P, **kw)
    assert np.array_equal(d["n_neigh"], ref["n_neigh"])
    v = ref["valid"]
    assert np.array_equal(valid_of(d), v)
    # normals: compared after orientation; where n . p is within rounding of zero the two solvers may land on either side
    pn = np.linalg.norm(ref["P"], axis=1)
    free = v & (np.abs((ref["normals"] * ref["P"]).sum(axis=1)) < SIGN_FREE * pn)
    diff = np.abs(d["normals"] - ref["normals"]).max(axis=1)
    flipped = np.abs(d["normals"] + ref["normals"]).max(axis=1)
    diff[free] = np.minimum(diff, flipped)[free]
    n_err = float(diff.max())
    r_err = float(np.abs(d["response"] - ref["response"]).max())
    print("scene %d n %d %s: worst normal difference %.3g, worst response difference %.3g, %d of %d points compared up to sign"
          % (seed, n, kw, n_err, r_err, int(free.sum()), int(v.sum())))
    assert free.sum() <= SIGN_FREE_SHARE * n
    assert n_err <= NORMAL_ATOL
    assert np.abs(np.linalg.norm(d["normals"][v], axis=1) - 1.0).max() <= 1e-15
    assert ((d["normals"] * ref["P"]).sum(axis=1)[v & ~free] <= 0).all()
    assert r_err <= RESPONSE_ATOL
    assert int(d["n_key"]) == len(ref["key_idx"])
    assert np.array_equal(keys_of(d), ref["key_idx"])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fewer_points_than_and_exactly_three(eng, n):
    """Points 1/8 m apart on a bent line: with n < 3 nobody has a normal; with n = 3 everybody has exactly 3 neighbours."""
    P = np.float32([[k / 8.0, (k * k) / 64.0, (k % 3) / 16.0] for k in range(n)])
    ref = harris_ref.harris(P)
    d = run(eng, P)
    assert d["n_neigh"].tolist() == [n] * n and np.array_equal(d["n_neigh"], ref["n_neigh"])
    if n < 3:
        assert (d["response"] == -1.0).all() and not d["normals"].any() and int(d["n_key"]) == 0 and (d["key_idx"] == -1).all()
    else:
        assert valid_of(d).all() and np.abs(np.linalg.norm(d["normals"], axis=1) - 1.0).max() <= 1e-15
        # three points span a plane: every normal is the plane's, every N has rank one, the response is 0 to rounding
        assert np.abs(np.abs(d["normals"]) - np.abs(ref["normals"])).max() <= NORMAL_ATOL
        assert np.abs(d["response"] - ref["response"]).max() <= RESPONSE_ATOL and int(d["n_key"]) == 0


def test_the_radius_is_strict(eng):
    out = run(eng, harris_ref.strict_radius(False))
    assert out["n_neigh"].tolist() == [3, 4, 3, 2] and out["response"][3] == -1.0 and not out["normals"][3].any()
    inside = run(eng, harris_ref.strict_radius(True))
    assert inside["n_neigh"][0] == 4 and inside["n_neigh"][3] == 3 and inside["response"][3] != -1.0
    for d, b in ((out, False), (inside, True)):
        ref = harris_ref.harris(harris_ref.strict_radius(b))
        assert np.array_equal(d["n_neigh"], ref["n_neigh"]) and np.array_equal(valid_of(d), ref["valid"])


def test_an_exact_plane_has_exact_normals_and_no_key_points(eng):
    """z = 0 on dyadic points: the z row and column of every C are exactly zero and keep their unit vector exactly; the points lie at
    x, y >= 0, z = 0, so n . p = 0 and the normal stays (0, 0, +1).  Every response is the bits of 0.0."""
    P = iss_ref.exact_plane()
    ref = harris_ref.harris(P)
    d = run(eng, P)
    v = valid_of(d)
    assert np.array_equal(v, ref["valid"]) and v.sum() > 150 and np.array_equal(d["n_neigh"], ref["n_neigh"])
    assert same_bits(d["normals"][v], np.tile([0.0, 0.0, 1.0], (int(v.sum()), 1)))
    assert same_bits(d["response"][v], np.zeros(int(v.sum())))
    assert int(d["n_key"]) == 0 and (d["key_idx"] == -1).all()
    corner = run(eng, harris_ref.corner())
    assert np.array_equal(np.abs(corner["normals"]), np.abs(harris_ref.harris(harris_ref.corner())["normals"]))   # exact unit vectors
    assert abs(corner["response"][0] - 1.0 / 27.0) < 1e-16 and keys_of(corner).tolist() == [0]


def test_three_collinear_points(eng):
    """C has rank one: the normal is any unit vector across the line, so only this is held: finite, unit length, the same bits
    twice, and no key point unless the restatement's response agrees."""
    P = harris_ref.collinear()
    a, b = run(eng, P), run(eng, P)
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert a["n_neigh"].tolist() == [3, 3, 3] and np.isfinite(a["normals"]).all() and np.isfinite(a["response"]).all()
    assert np.abs(np.linalg.norm(a["normals"], axis=1) - 1.0).max() <= 1e-15
    ref = harris_ref.harris(P)
    for i in keys_of(a):
        assert abs(a["response"][i] - ref["response"][i]) <= RESPONSE_ATOL and ref["response"][i] >= ref["params"]["threshold"]


def test_equal_responses_both_survive(eng):
    """The cluster and its copy 32 m away: all differences and sums are exact, so the covariances, the normals up to sign, and the
    responses are bit-equal pairwise, and point k is a key point iff point k + 40 is.  On the exact plane at threshold 0 every valid
    point has response 0.0, neighbours included, and all of them survive."""
    T = iss_ref.tie_cluster()
    d = run(eng, T)
    assert same_bits(d["response"][:40], d["response"][40:]) and same_bits(d["n_neigh"][:40], d["n_neigh"][40:])
    assert same_bits(np.abs(d["normals"][:40]), np.abs(d["normals"][40:]))
    is_key = np.zeros(80, bool)
    is_key[keys_of(d)] = True
    assert np.array_equal(is_key[:40], is_key[40:])
    ref = harris_ref.harris(T)
    assert np.array_equal(d["n_neigh"], ref["n_neigh"]) and np.array_equal(valid_of(d), ref["valid"])
    plane = run(eng, iss_ref.exact_plane(), threshold=0.0)
    assert np.array_equal(keys_of(plane), np.flatnonzero(valid_of(plane)))


def test_a_padded_batch_equals_single_calls_and_repeats_itself(eng):
    """Three frames of 1500, 0 and 257 points in ld = 1536, the padding rows NaN: every frame's results are the single-cloud call's
    bits, the empty frame has no key points, and a second call returns the same bytes."""
    frames = [harris_ref.reference(*harris_ref.SCENES[0])[0], np.zeros((0, 3), np.float32), harris_ref.reference(*harris_ref.SCENES[3])[0]]
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
    check_frames(eng, batch, frames)


def check_frames(eng, batch, frames):
    for f, p in enumerate(frames):
        n = p.shape[0]
        assert (batch["response"][f, n:] == -1.0).all() and not batch["normals"][f, n:].any() and not batch["n_neigh"][f, n:].any()
        if n == 0:
            continue
        one = run(eng, p)
        nk = int(one["n_key"])
        assert int(batch["n_key"][f]) == nk and nk > 0
        assert same_bits(batch["key_idx"][f, :nk], one["key_idx"][:nk]) and (batch["key_idx"][f, nk:] == -1).all()
        for k in ("response", "normals", "n_neigh"):
            assert same_bits(np.ascontiguousarray(batch[k][f, :n]), one[k]), (f, k)


def test_a_batch_of_frames_with_different_point_counts(eng):
    """600, 1025 and 257 points under ld = 1025 (the last frame ends inside the first chunk, the second one point into the second),
    the padding rows a far-away finite point: bit for bit the single calls."""
    frames = [harris_ref.reference(*harris_ref.SCENES[4])[0], harris_ref.reference(*harris_ref.SCENES[2])[0], harris_ref.reference(*harris_ref.SCENES[3])[0]]
    assert [f.shape[0] for f in frames] == [600, 1025, 257]
    pts = np.full((3, 1025, 3), 8.0, np.float32)   # inside the scene: a padding row that reached a decision would change it
    for f, p in enumerate(frames):
        pts[f, :p.shape[0]] = p
    check_frames(eng, run(eng, pts, n_pts=[600, 1025, 257]), frames)


def test_more_frames_than_one_launch_takes(eng):
    """65 537 frames of 0 .. 4 points under ld = 4: the entry point slices them at 65 535.  Every output is the bits of two calls on
    the frames before and from the cut, the frames at both ends of both slices are their single-cloud calls, and the neighbour counts
    are NumPy's over all frames."""
    kw = dict(radius=1.0, threshold=0.0)
    pts, n_pts = iss_ref.many_frames()
    cut = 65535
    assert pts.shape == (cut + 2, 4, 3)
    whole = run(eng, pts, n_pts=n_pts, **kw)
    head, tail = run(eng, pts[:cut], n_pts=n_pts[:cut], **kw), run(eng, pts[cut:], n_pts=n_pts[cut:], **kw)
    for k in whole:
        assert same_bits(whole[k], np.concatenate([head[k], tail[k]])), k
    counts = iss_ref.neighbour_counts(pts, n_pts, 1.0)
    assert np.array_equal(whole["n_neigh"], counts) and np.array_equal(valid_of(whole), counts >= 3)
    assert whole["n_key"].sum() > 0 and whole["n_neigh"][cut + 1].tolist() == [1, 0, 0, 0]
    for f in (0, cut - 1, cut, cut + 1):
        n = int(n_pts[f])
        one = run(eng, pts[f, :n], **kw)
        nk = int(one["n_key"])
        assert int(whole["n_key"][f]) == nk and same_bits(whole["key_idx"][f, :nk], one["key_idx"][:nk]) and (whole["key_idx"][f, nk:] == -1).all()
        for k in ("response", "normals", "n_neigh"):
            assert same_bits(np.ascontiguousarray(whole[k][f, :n]), one[k]), (f, k)


def test_refusals_leave_the_context_usable(eng):
    P = harris_ref.reference(*harris_ref.SCENES[3])[0]
    bad = P.copy()
    bad[100, 2] = np.nan
    with pytest.raises(ValueError):
        run(eng, bad)
    run(eng, bad, n_pts=[100])   # the NaN sits past n_pts: not the frame's
    with pytest.raises(ValueError):
        eng.harris_keypoints(torch.zeros((32769, 3), device=eng.device))
    with pytest.raises(ValueError):
        run(eng, P, radius=0.0)
    with pytest.raises(ValueError):
        run(eng, P, threshold=-1.0)
    with pytest.raises(ValueError):
        run(eng, P, salient_radius=2.0)
    with pytest.raises(ValueError):
        run(eng, P[None], n_pts=[258])
    assert eng.harris_keypoints(torch.from_numpy(P).to(eng.device)).normals is None
    ref = harris_ref.reference(*harris_ref.SCENES[3])[1]
    assert np.array_equal(keys_of(run(eng, P)), ref["key_idx"])


def test_api_key_points_equal_the_engine_call(engine):
    from caelo import api
    P, ref = harris_ref.reference(*harris_ref.SCENES[4])
    r = engine.harris_keypoints(torch.from_numpy(P).to(engine.device))
    k = r.key_idx[:int(r.n_key.item())].cpu().numpy()
    assert np.array_equal(k, ref["key_idx"])
    pc4 = np.c_[P, np.ones(len(P), np.float32)].astype(np.float32)
    kp = api.KeyPtsByHarris(pc4)
    assert isinstance(kp, np.ndarray) and kp.dtype == np.float32 and np.array_equal(kp, P[k])
    on_dev = api.KeyPtsByHarris(torch.from_numpy(P).to(engine.device), radius=1.5, threshold=0.005)
    r2 = engine.harris_keypoints(torch.from_numpy(P).to(engine.device), radius=1.5, threshold=0.005)
    assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), P[r2.key_idx[:int(r2.n_key.item())].cpu().numpy()])
    with pytest.raises(ValueError):
        api.KeyPtsByHarris(P[:, :2])


def test_detect_keypoints_end_to_end(eng, scans, tmp_path, capsys):
    """Three small synthetic scans -> detect_keypoints.main --method harris -> files that keysources.read_3dfeatnet reads as [256,3];
    their leading rows are Engine.harris_keypoints on the same thinned cloud, the rest are points of that cloud; a second run with
    the same seed writes the same rows."""
    import detect_keypoints
    from caelo import keysources
    scans_dir, out_dir, out_again = tmp_path / "velodyne", tmp_path / "harris", tmp_path / "harris_again"
    scans_dir.mkdir()
    frames = (0, 1, 2)
    clouds = [scans(f, n_az=500, quantum=1e-3) for f in frames]
    for f, s in zip(frames, clouds):
        s.tofile(str(scans_dir / ("%06d.bin" % f)))
    argv = ["--method", "harris", "--scans", str(scans_dir), "--keypoints", "256", "--max-points", "4096", "--seed", "3", "--batch", "2"]
    detect_keypoints.main(argv + ["--out", str(out_dir)])
    said = capsys.readouterr().out
    assert "Harris3D found" in said and "ISS" not in said
    detect_keypoints.main(argv + ["--out", str(out_again)])
    for f, s in zip(frames, clouds):
        kp = keysources.read_3dfeatnet(keysources.keypts_path(str(out_dir), f))
        assert kp.shape == (256, 3) and kp.dtype == np.float32
        assert same_bits(kp, keysources.read_3dfeatnet(keysources.keypts_path(str(out_again), f)))
        pc, _ = detect_keypoints.prepare(eng, s, f, 0.2, 4096, 3)
        assert 256 < pc.shape[0] <= 4096
        r = eng.harris_keypoints(pc)
        m = int(r.n_key.item())
        cloud = pc.cpu().numpy()
        assert m > 0
        if m <= 256:
            assert np.array_equal(kp[:m], cloud[r.key_idx[:m].cpu().numpy()])
            assert {tuple(p) for p in kp[m:]} <= {tuple(p) for p in cloud}
        else:
            assert {tuple(p) for p in kp} <= {tuple(p) for p in cloud[r.key_idx[:m].cpu().numpy()]}
