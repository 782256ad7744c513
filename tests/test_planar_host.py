"""caelo_host_planar_points -- the per-pixel rule of caelo_planar_points compiled for the host (csrc/planar.hip) --
against what the reference's own lines returned (tests/golden/planar_pts.npz, written by tools/make_goldens_planar.py), against the
NumPy restatement tests/planar_ref.py on the crafted image and on two synthetic frames, the entry points' refusals, and
refine_sequence.py --planar-pts ring on an engine that stands in for the device.  CPU only.

Every comparison goes through planar_ref.compare: outside the undecided candidates ((l1 - l0) / l2 < 1e-4, or |n_z| within 1e-9 of
0.9) membership and order are equal, points are equal byte for byte, float32 normals lie within 1.2e-7; on a frame at most 0.5 % of
the candidates may be undecided.  Measured on this suite's inputs (profiles/planar_errors.txt): the float32 normals are equal on the frames and differ by at most 8.9e-16
on the crafted image; 2 of 10 606 and 13 of 6 124 candidates of the two frames are undecided."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planar_images as pi
import planar_ref as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planar_pts.npz")


def _has(pixels, at):
    return bool((np.asarray(pixels) == np.array(at)).all(axis=1).any())


def test_golden_cases_against_the_references_lines():
    """The image the reference's un-commented loop ran on: its PlanarPts (LAPACK's sign turned to n_z > 0), its per-pixel minDiff, and
    what each patch was built to decide."""
    g = dict(np.load(GOLDEN))
    im = pi.Image()
    y, x = g["pix"][:, 0].astype(int), g["pix"][:, 1].astype(int)
    im.ring[y, x, 0:3], im.counter[y, x], im.resp[y, x] = g["xyz"], g["cnt"], g["resp"]
    want = g["planar_reference"].copy()
    down = want[:, 5] < 0
    want[down, 3:6] = -want[down, 3:6]
    assert want.shape[0] == g["pixels"].shape[0] > 300 and int(g["n_key_reference"]) > 50
    ref = dict(rows=want, pixels=g["pixels"], cand=g["cand"], eig=g["eig"], absnz=g["absnz"])
    rows, pixels, n, _ = pi.host_planar(im.ring, im.counter, im.resp)
    pr.compare(ref, rows, pixels, label="golden")
    md, _ = pr.min_diff(im.resp, im.counter > 0)
    assert np.array_equal(md[g["cand"][:, 0], g["cand"][:, 1]], g["min_diff_reference"][[np.flatnonzero((g["pix"] == c).all(axis=1))[0] for c in g["cand"]]])
    und = {tuple(p) for p in g["cand"][pr.undecided(ref)].tolist()}
    for name, at, expect in zip(g["patch_names"], g["patch_at"], g["patch_expect"]):
        if expect >= 0:
            assert tuple(at) not in und and _has(pixels, at) == bool(expect), name
    assert {"flat", "tilt_085", "mindiff_04", "quirk_at_near", "centre_excluded", "row_8", "col_1783"} <= set(g["patch_names"].tolist())


@pytest.mark.parametrize("ring_c,height,width", [(3, 64, 1792), (5, 69, 1800)])
def test_crafted_image(ring_c, height, width):
    """Every decision of the rule on its own patch (tests/planar_images.py), batch mode (3 channels, 64 x 1792) and demo mode (5
    channels, 69 x 1800): the host twin against the restatement, and each patch's centre against what the patch was built for."""
    im, expect = pi.crafted(ring_c, height, width)
    ref = pr.planar_points(im.ring, im.counter, im.resp)
    rows, pixels, n, _ = pi.host_planar(im.ring, im.counter, im.resp)
    pr.compare(ref, rows, pixels, label="crafted c=%d" % ring_c)
    und = {tuple(p) for p in ref["cand"][pr.undecided(ref)].tolist()}
    for name, want in expect.items():
        if want is None:
            assert im.at[name] in und, name            # the collinear window: either way, and the call returned
        else:
            assert im.at[name] not in und and _has(pixels, im.at[name]) == want, name
    # rows 7 and 56, columns 7 and 1784 hold occupied pixels with full windows and are never emitted
    assert im.counter[7, 300] > 0 and im.counter[56, 300] > 0 and im.counter[30, 7] > 0 and im.counter[30, 1784] > 0
    assert pixels[:, 0].min() == 8 and pixels[:, 0].max() == 55 and pixels[:, 1].min() == 8 and pixels[:, 1].max() == 1783
    # what the centres of the threshold patches were given
    md = ref["min_diff"]
    assert md[im.at["mindiff_04"]] == np.float32(0.4) and md[im.at["mindiff_04_below"]] == np.nextafter(np.float32(0.4), np.float32(0))
    assert md[im.at["quirk_at_near"]] == np.float32(0.2) and np.isnan(md[im.at["nan_neighbour"]]) and md[im.at["nan_unoccupied"]] == 0
    y, x = im.at["quirk_at_norm10"]
    assert np.sqrt(np.sum(im.ring[y, x, 0:3] ** 2, dtype=np.float32)) == np.float32(10.0)
    # the tilted planes' normals are the planes': |n_z| = 0.95 kept, 0.85 not
    k = np.flatnonzero((pixels == np.array(im.at["tilt_095"])).all(axis=1))[0]
    assert abs(rows[k, 5] - 0.95) < 1e-5 and rows[k, 3] < 0
    k = np.flatnonzero((ref["cand"] == np.array(im.at["tilt_085"])).all(axis=1))[0]
    assert abs(ref["absnz"][k] - 0.85) < 1e-5
    # including the centre would flip :275 for the centre_excluded patch
    y, x = im.at["centre_excluded"]
    w = im.ring[y - 2:y + 3, x - 2:x + 3, 0:3].reshape(-1, 3).astype(np.float64)
    vals, vecs = np.linalg.eigh(np.cov(w, rowvar=0))
    assert abs(vecs[2, 0]) < 0.1
    # pixels = None is accepted and changes nothing
    rows2, _, n2, _ = pi.host_planar(im.ring, im.counter, im.resp, want_pixels=False)
    assert n2 == n and rows2.tobytes() == rows.tobytes()


def test_empty_and_capacity_images():
    im = pi.Image()
    rows, pixels, n, (planar, _) = pi.host_planar(im.ring, im.counter, im.resp, fill=7.0)
    assert n == 0 and (planar == 7.0).all()                                   # nothing is written
    im = pi.capacity()
    rows, pixels, n, _ = pi.host_planar(im.ring, im.counter, im.resp)
    assert n == pr.PLANAR_MAX == 48 * 1776
    yy, xx = np.mgrid[8:56, 8:1784]
    assert np.array_equal(pixels, np.c_[yy.ravel(), xx.ravel()])              # row-major
    assert rows[:, 0:3].tobytes() == im.ring[8:56, 8:1784, 0:3].tobytes()
    assert np.array_equal(rows[:, 3:6], np.tile(np.array([0, 0, 1], np.float32), (n, 1)))   # a zero row and column: the unit vector, exactly


@pytest.fixture(scope="module")
def frames(orc, models, scans):
    return {kind: pi.frame(orc, models, scans, 0, kind) for kind in ("boxes", "clutter")}


@pytest.mark.parametrize("kind", ["boxes", "clutter"])
def test_synthetic_frames_against_the_restatement(frames, kind):
    """Two full mm-quantised frames, response from the oracle's RespondLayer: thousands of candidates and planar points."""
    ring, cnt, resp = frames[kind]
    ref = pr.planar_points(ring, cnt, resp)
    rows, pixels, n, _ = pi.host_planar(ring, cnt, resp)
    assert len(ref["cand"]) > 3000 and len(ref["rows"]) > 2000                # the subsample of MyICP.py:135-140 is exercised
    pr.compare(ref, rows, pixels, max_undecided=0.005, label="frame 0 %s" % kind)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from caelo import _ffi
    lib = _ffi.load()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "caelo.h")).read()
    for name in ("caelo_planar_ws_bytes", "caelo_planar_points", "caelo_host_planar_points"):
        assert hasattr(lib, name) and name + "(" in header
    assert "#define CAELO_PLANAR_MAX (48 * 1776)" in header and _ffi.PLANAR_MAX == 48 * 1776
    assert lib.caelo_abi_version() == _ffi.ABI_VERSION
    assert lib.caelo_planar_ws_bytes() >= 48 * 1792 * 24 + 48 * 28 * 8 and lib.caelo_planar_ws_bytes() % 16 == 0
    buf = np.zeros(4096, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert buf.ctypes.data % 16 == 0

    def host(text, ring=p, ring_w=1792, ring_c=3, counter=p, cnt_w=1792, resp=p, planar=p, n=p):
        assert lib.caelo_host_planar_points(ring, ring_w, ring_c, counter, cnt_w, resp, planar, None, n) == -1
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()

    def device(text, ctx=p, ring=p, ring_w=1792, ring_c=5, counter=p, cnt_w=1800, resp=p, ws=p, planar=p, n=p):
        # (no context exists here: every pointer is a host buffer that is never read)
        assert lib.caelo_planar_points(ctx, ring, ring_w, ring_c, counter, cnt_w, resp, ws, planar, None, n, None) == -1
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()
    for refuse in (host, device):
        for name in ("ring", "counter", "resp", "planar", "n"):
            refuse("null argument", **{name: None})
        refuse("bad ring shape", ring_w=1791)
        refuse("bad ring shape", cnt_w=1791)
        for c in (0, 2, 4, 6):
            refuse("bad ring shape", ring_c=c)
    device("null argument", ctx=None)
    device("null argument", ws=None)
    device("16-byte aligned", ws=C.c_void_p(buf.ctypes.data + 8))


def test_get_key_pts_by_ae_keeps_its_default():
    """api.GetKeyPtsByAE(..., planar=False): the third value is the reference's empty PlanarPts unless asked otherwise."""
    from caelo import api
    sig = inspect.signature(api.GetKeyPtsByAE)
    assert list(sig.parameters) == ["SphericalRing", "GridCounter", "RespondImg", "planar"] and sig.parameters["planar"].default is False
    assert list(inspect.signature(api.GetPlanarPts).parameters) == ["SphericalRing", "GridCounter", "RespondImg"]


# ---- refine_sequence.py --planar-pts ring on an engine that stands in for the device ------------------------------------------------------
class _Result:
    def __init__(self, R, T, ok):
        self.R_star, self.T_star, self.success = np.asarray(R, np.float64).ravel().tolist(), np.asarray(T, np.float64).ravel().tolist(), int(ok)


class _HostEngine:
    """The stages refine_sequence.py's KeyPts._make calls, on the oracle and the host twin; Engine.icp records what reaches it and
    answers with the identity."""
    device = "cpu"

    def __init__(self, orc, models, planar_rows=None):
        self.orc, self.models, self.calls, self.planar_rows = orc, models, [], planar_rows

    def project(self, pc):
        import torch
        ring, cnt = self.orc.ProjectPC2SphericalRing(pc.numpy())
        return torch.from_numpy(ring), torch.from_numpy(cnt), torch.zeros(1, dtype=torch.int32)

    def respond(self, ring):
        import torch
        return torch.from_numpy(self.models[0].predict(ring.numpy()[None, 0:64, 0:1792, 0:3])[0])

    def keypoints(self, ring, cnt, resp, status=None):
        import torch
        kpts, kpix, _ = self.orc.GetKeyPtsByAE(ring.numpy(), cnt.numpy(), resp.numpy())
        return torch.from_numpy(kpts), torch.from_numpy(kpix), torch.tensor([len(kpix)], dtype=torch.int32), status

    def planar_points(self, ring, cnt, resp):
        import torch
        _, _, n, (planar, pixels) = pi.host_planar(ring.numpy(), cnt.numpy(), resp.numpy())
        if self.planar_rows is not None:
            n = min(n, self.planar_rows)
        return torch.from_numpy(planar), torch.from_numpy(pixels), torch.tensor([n], dtype=torch.int32)

    def extend_keypts(self, ring, cnt, kpix):
        import torch
        ext = self.orc.ExtendKeyPtsInShpericalRing(ring.numpy(), cnt.numpy(), kpix.numpy())
        return torch.from_numpy(ext), torch.tensor([len(ext)], dtype=torch.int32)

    def icp(self, pc0, pc1, planar0=None, planar1=None, nn="brute", **kw):
        self.calls.append(dict(kw, nn=nn, m0=None if planar0 is None else planar0.shape[0], m1=None if planar1 is None else planar1.shape[0],
                               unit=None if planar0 is None else float(np.abs(np.linalg.norm(planar0.numpy()[:, 3:6], axis=1) - 1).max())))
        return _Result(np.eye(3), np.zeros(3), True)

    @staticmethod
    def icp_result(res):
        return res


@pytest.fixture()
def tool(orc, models, scans, tmp_path, monkeypatch):
    """-> (directory, engine, arguments): four poses 0.3 m apart, the host engine behind refine_sequence.py, and two scans that serve
    every frame (the test is about the plumbing)."""
    import caelo.engine
    from caelo import synth
    two = [scans(f, quantum=1e-3) for f in (0, 1)]
    eng = _HostEngine(orc, models)
    monkeypatch.setattr(caelo.engine, "default_engine", lambda: eng)
    monkeypatch.setattr(synth, "make_scan", lambda frame, **kw: two[frame % 2])
    poses = np.tile(np.eye(3, 4).reshape(12), (4, 1))
    poses[:, 3] = 0.3 * np.arange(4)
    np.savetxt(str(tmp_path / "00.txt"), poses)
    return tmp_path, eng, ["--poses", str(tmp_path / "00.txt"), "--mode", "consecutive", "--out", str(tmp_path / "out.txt")]


def test_tool_planar_pts_ring_reaches_the_icp_with_planar_sets(tool):
    """--synthetic --icp pt2plane --planar-pts ring: accepted; every registration gets both frames' planar points (unit normals, more
    than 2 000 of frame 1's cut to 2 000), and --save-keypts writes a frame's as its PlanarPts."""
    import refine_sequence
    from caelo import synth
    from scipy import io
    tmp, eng, common = tool
    kp = str(tmp / "seq" / "KeyPts")
    r = refine_sequence.run(common + ["--synthetic", "--icp", "pt2plane", "--planar-pts", "ring", "--save-keypts", kp])
    assert len(eng.calls) == len(r["tried"]) == 2
    for c in eng.calls:
        assert c["m0"] > 2000 and c["m1"] == 2000 and c["unit"] < 1e-6 and c["min_pairs"] == 200 and c["fail_only_first"] == 1
    m = io.loadmat(os.path.join(kp, "000001.bin.mat"))
    assert m["PlanarPts"].dtype == np.float32 and m["PlanarPts"].shape == (eng.calls[1]["m0"], 6) and m["ExtendedKeyPts"].shape[1] == 3
    ring, cnt = eng.orc.ProjectPC2SphericalRing(synth.make_scan(1))
    rows, _, _, _ = pi.host_planar(ring, cnt, eng.models[0].predict(ring[None, 0:64, 0:1792, 0:3])[0])
    assert m["PlanarPts"].tobytes() == rows.tobytes()
    # without --icp pt2plane the planar points are made and saved all the same, and the point-to-point call ignores them
    del eng.calls[:]
    refine_sequence.run(common + ["--synthetic", "--planar-pts", "ring"])
    assert len(eng.calls) == 2 and all(c["m0"] is None for c in eng.calls)


def test_tool_refuses_a_frame_without_planar_points(tool):
    import refine_sequence
    tmp, eng, common = tool
    eng.planar_rows = 0
    with pytest.raises(SystemExit) as e:
        refine_sequence.run(common + ["--synthetic", "--icp", "pt2plane", "--planar-pts", "ring"])
    assert "frame 0 has no planar points" in str(e.value) and eng.calls == []


def test_tool_planar_pts_argument_errors(tool, capsys):
    import refine_sequence
    tmp, eng, common = tool

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            refine_sequence.run(argv)
        assert e.value.code == 2 and eng.calls == []
        return capsys.readouterr().err
    keypts = common + ["--keypts-dir", str(tmp / "KeyPts")]
    assert "--keypts-dir files carry their own" in refused(keypts + ["--planar-pts", "ring"])
    assert "--keypts-dir files carry their own" in refused(keypts + ["--planar-pts", "ring", "--icp", "pt2plane"])
    assert "invalid choice" in refused(common + ["--synthetic", "--planar-pts", "pca"])
    # without the flag the refusal is the one it was
    err = refused(common + ["--synthetic", "--icp", "pt2plane"])
    assert "RefinePoses.py:291-294" in err and "give --keypts-dir files that hold PlanarPts, or use --icp pt2pt" in err
