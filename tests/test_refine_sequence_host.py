"""The sequence logic of caelo.refine (FixJumpPoses, GetTransferPairIdx, LongestPair, RefineOdometry, CloseLoopPipeline) against what
the reference's RefinePoses.py did on the same inputs (tests/golden/refine_sequence.npz, written by tools/make_goldens_refine.py).
CPU only: the registration is the scripted stand-in of tests/refine_cases.py, or the oracle's ICP.

Decisions are compared with ==: de-jumped frames, every pair tried and its code, the failed list, DebugInfo's frame columns, the
second pass's pairs.  The golden keeps every planted jump a factor 2 away from FixJumpPoses' thresholds (asserted below on the
recorded differences), and every registration of the real-ICP run changes the relative pose by less than half of the 10 degree /
5 m rejection (asserted too), so no case depends on rounding.  Poses and DebugInfo values are float64 3 x 3 algebra under another
NumPy / BLAS than the golden's: BARS holds, per case, four times the largest absolute difference measured
(profiles/refine_errors.txt)."""
import os

import numpy as np
import pytest

import refine_cases as rc
from caelo import refine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_sequence.npz")
# case -> bars on |poses - golden| and |DebugInfo values - golden|, absolute: 4 x the figures of profiles/refine_errors.txt; where the
# figure is 0 the float32 table has to be equal
BARS = {
    "dejump": (3.56e-14, 5.33e-15),              # (its second figure: GetDiffRels' float64 outputs)
    "keyframes_gt": (1.14e-13, 4.26e-14),
    "keyframes_nogt": (1.43e-13, 0.0),
    "consecutive_gt": (7.11e-15, 6.56e-15),
    "consecutive_nogt": (3.13e-13, 0.0),
    "real_icp": (2.10e-05, 2.59e-05),            # the oracle's ICP against MyICP.ICP: float32 SolveRT, as in profiles/icp_loop_errors.txt
}
WORST = {}


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (case, kind), v in sorted(WORST.items()):
        print("refine_errors %-17s %-6s worst %.3e  bar %.3e" % (case, kind, v, BARS[case][("poses", "debug").index(kind)]))


def _within(case, kind, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (case, kind, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    WORST[(case, kind)] = max(WORST.get((case, kind), 0.0), err)
    bar = BARS[case][("poses", "debug").index(kind)]
    assert err <= bar, "%s %s: %.3e above %.3e" % (case, kind, err, bar)


def _pairs(g, seq):
    cnt = g["inl_%d_count" % seq]
    off = np.r_[0, np.cumsum(cnt)]
    a, b = g["inl_%d_idx0" % seq], g["inl_%d_idx1" % seq]
    return lambda f0, f1: (a[off[f0]:off[f0 + 1]], b[off[f0]:off[f0 + 1]])


def _rows(t):
    return [tuple(int(v) for v in r) for r in np.asarray(t).reshape(-1, np.asarray(t).shape[-1] if np.asarray(t).ndim == 2 else 1)]


def test_transfer_pair_idx(g):
    for k in range(int(g["transfer_n"])):
        got = np.array(refine.GetTransferPairIdx(g["transfer_%d_a" % k], g["transfer_%d_b" % k]), dtype=np.int64).reshape(-1, 2)
        assert np.array_equal(got, g["transfer_%d_out" % k]), k
    assert refine.GetTransferPairIdx(np.array([5, 5]), np.array([7, 5, 5])) == [[0, 1], [1, 1]]   # the FIRST position of a repeated value


def test_diff_rels(g):
    out = refine.GetDiffRels(g["dejump_both_in"])
    for got, name in zip(out, ("relRs", "relTs", "relEulers", "diffEulers", "diffTs")):
        assert got.dtype == np.float64
        _within("dejump", "debug", got, g["diffrels_" + name])
    # the differences are taken between absolute values (Transformations.py:85-86): a relative yaw that flips sign is no jump
    poses = g["gt_0"].copy()
    relRs, relTs, relEulers, dE, dT = refine.GetDiffRels(poses)
    assert np.allclose(dE, np.linalg.norm(np.abs(relEulers[1:]) - np.abs(relEulers[:-1]), axis=1), rtol=0, atol=0)
    assert np.allclose(dT, np.linalg.norm(np.abs(relTs[1:]) - np.abs(relTs[:-1]), axis=1), rtol=0, atol=0)


@pytest.mark.parametrize("name", rc.DEJUMP)
def test_fix_jump_poses(g, name):
    seen = g["dejump_%s_seen" % name]
    flagged = (seen[:, 0] > 2.0) | (seen[:, 1] > 0.5)
    clear = (seen[:, 0] > 4.0) | (seen[:, 1] > 1.0) | ((seen[:, 0] < 1.0) & (seen[:, 1] < 0.25))
    assert clear.all() and int(flagged.sum()) == len(g["dejump_%s_fixed" % name])   # the golden's own margin: a factor 2 everywhere
    poses, fixed = refine.FixJumpPoses(g["dejump_%s_in" % name])
    assert fixed == g["dejump_%s_fixed" % name].tolist()
    _within("dejump", "poses", poses, g["dejump_%s_out" % name])
    n = poses.shape[0]
    want = {"rotation": 1, "translation": 1, "both": 1, "frame_2": 1, "frame_n_2": 1, "two_in_a_row": 2, "none": 0}[name]
    assert len(fixed) == want and all(2 <= f <= n - 2 for f in fixed)
    if name == "frame_2":
        assert fixed == [2]
    if name == "frame_n_2":
        assert fixed == [n - 2]
    if name == "two_in_a_row":
        assert fixed[1] == fixed[0] + 1


@pytest.mark.parametrize("name", sorted(rc.WALKS))
def test_walks_with_scripted_registration(g, name):
    seq, iOption, with_gt, start = rc.WALKS[name]
    gt, est, codes = g["gt_%d" % seq], g["est_%d" % seq], g["codes_%d" % seq]
    assert np.array_equal(codes, rc.code_table(gt.shape[0]))
    calls = []
    core = rc.scripted_core(codes, gt, refine.ForwardUpdatePoses, refine.GetRelRtBetween2Poses, refine.GetRtFromOnePose, calls)
    log = []
    poses, info, failed, tried = refine.RefineOdometry(est, iOption, core, pairs=_pairs(g, seq) if iOption == 1 else None, gt=gt if with_gt else None,
                                                       iStartFrame=start, log=log.append)
    assert tried == _rows(g["walk_%s_tried" % name])
    assert [tuple(int(v) for v in f) for f in failed] == _rows(g["walk_%s_failed" % name])
    assert all(t == 1.0 for _, _, t in calls) and len(log) == len(tried)
    want = g["walk_%s_debug" % name]
    assert info.dtype == np.float32 and info.shape == want.shape and info.shape[1] == (7 if with_gt else 4)
    assert np.array_equal(info[:, 0:2], want[:, 0:2])
    _within(name, "debug", info[:, 2:], want[:, 2:])
    _within(name, "poses", poses, g["walk_%s_poses" % name])
    assert tried[0][0] == start and all(f1 <= gt.shape[0] - 2 + 1 for _, f1, _ in tried)
    n_first = len(calls)
    poses2, second = refine.CloseLoopPipeline(poses, info, core)
    assert second == _rows(g["walk_%s_second" % name]) and all(t == 0.5 for _, _, t in calls[n_first:])
    _within(name, "poses", poses2, g["walk_%s_second_poses" % name])
    if info.shape[0] <= 7:
        assert second == [] and np.array_equal(poses2, poses)
    else:
        kf = info[:, 0].astype(np.int32)
        assert [(a, b) for a, b, _ in second] == [(int(kf[k]), int(kf[k + 2])) for k in range(0, len(kf) - 7, 2)]


def test_walk_coverage(g):
    """What the golden was built to hold: every code on long and on one-frame pairs, a chain cut at nMaxTransferFrames = 20, the retry
    of the same start frame with one frame after -1 and after 0, and a second pass that registers something."""
    tried = _rows(g["walk_keyframes_gt_tried"]) + _rows(g["walk_keyframes_nogt_tried"])
    assert {(min(b - a, 2), c) for a, b, c in tried} == {(s, c) for s in (1, 2) for c in (-1, 0, 1)}
    assert max(b - a for a, b, _ in tried) == 20
    for code in (-1, 0):
        assert any(c == code and b - a > 1 and tried[i + 1][0] == a and tried[i + 1][1] == a + 1 for i, (a, b, c) in enumerate(tried[:-1]))
    assert len(g["walk_consecutive_nogt_second"]) >= 2
    assert (g["inl_1_count"] == 0).sum() == 1   # the empty pair file
    a, cnt = g["inl_2_idx0"], g["inl_2_count"]
    off = np.r_[0, np.cumsum(cnt)]
    assert any(len(np.unique(a[off[i]:off[i + 1]])) < cnt[i] for i in range(len(cnt)))   # duplicated inliersIdx0 entries


def test_close_loop_with_few_key_frames(g):
    """7 key frames or fewer: unchanged, nothing registered.  Below 3 the reference raises IndexError (RefinePoses.py:490-491); here
    the poses come back unchanged as well."""
    poses = g["est_0"]

    def core(*a):
        raise AssertionError("nothing may be registered")
    for rows in (0, 1, 2, 3, 7):
        info = np.zeros((rows, 4), np.float32)
        info[:, 0] = np.arange(rows)
        out, tried = refine.CloseLoopPipeline(poses, info if rows else np.array([], dtype=np.float32), core)
        assert tried == [] and np.array_equal(out, poses)


def test_real_icp_walk_with_the_oracles_icp(g, orc):
    """RefinementCore as it is, the registration of RefinePoses.py:295 (ICP with its defaults, the oracle's restatement here,
    MyICP.ICP in the golden), key frames by inlier transfer on 14 frames of a 400-point static world."""
    gt, est, Tr, clouds = g["gt_0"], g["est_0"], g["tr_0"], g["clouds_0"]
    assert Tr.dtype == np.float32 and clouds.dtype == np.float32
    empty = np.zeros((0, 6), np.float32)
    core = refine.make_core(lambda f: (clouds[f], empty), Tr, refine.pt2pt_adapter(lambda a, b: orc.ICP(a, b)))
    poses, info, failed, tried = refine.RefineOdometry(est, 1, core, pairs=_pairs(g, 0), gt=gt)
    assert tried == _rows(g["real_tried"]) and failed == [] and len(g["real_failed"]) == 0
    assert np.array_equal(info[:, 0:2], g["real_debug"][:, 0:2])
    # the golden's own margin: every registration moved the relative pose by less than half of what RefinementCore rejects
    m = g["real_margins"]
    assert m.shape == (len(tried), 2) and (m[:, 0] < 5.0).all() and (m[:, 1] < 2.5).all() and all(c == 1 for _, _, c in tried)
    _within("real_icp", "poses", poses, g["real_poses"])
    _within("real_icp", "debug", info[:, 2:], g["real_debug"][:, 2:])
    assert info[:, 6].mean() < 0.5 * info[:, 4].mean()   # the refinement refines
    poses2, second = refine.CloseLoopPipeline(poses, info, core)
    assert second == _rows(g["real_second"])
    _within("real_icp", "poses", poses2, g["real_second_poses"])


# ---- refine_sequence.py: what it refuses before it touches a device -----------------------------------------------------------------------
def _tool(argv, capsys):
    import refine_sequence
    with pytest.raises(SystemExit) as e:
        refine_sequence.run(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_tool_refuses_pt2plane_without_planar_points(g, tmp_path, capsys):
    """--icp pt2plane is RefinePoses.py:291-294, which fails on the reference's own artefacts: refused with --scans, and with --keypts-dir
    files whose PlanarPts are empty or missing, with a message that names the reference lines."""
    from scipy import io
    poses = str(tmp_path / "00.txt")
    np.savetxt(poses, g["est_0"])
    common = ["--poses", poses, "--inliers-dir", str(tmp_path / "InliersIdx"), "--out", str(tmp_path / "out.txt"), "--icp", "pt2plane"]
    err = _tool(common + ["--scans", str(tmp_path)], capsys)
    assert "RefinePoses.py:291-294" in err and "SphericalRing.py:219,285" in err and "MyICP.py:94" in err
    kp = tmp_path / "KeyPts"
    kp.mkdir()
    for f in range(g["est_0"].shape[0]):
        planar = np.zeros((0, 3), np.float32) if f == 5 else np.ones((7, 6), np.float32)
        if f != 9:
            io.savemat(str(kp / ("%06d.bin.mat" % f)), {"KeyPts": np.zeros((4, 3), np.float32), "ExtendedKeyPts": np.zeros((9, 3), np.float32), "PlanarPts": planar})
    err = _tool(common + ["--keypts-dir", str(kp)], capsys)
    assert "RefinePoses.py:291-294" in err and "[5, 9]" in err
    assert not (tmp_path / "out.txt").exists()


def test_tool_argument_checks(g, tmp_path, capsys):
    poses = str(tmp_path / "00.txt")
    np.savetxt(poses, g["est_0"])
    out = ["--poses", poses, "--out", str(tmp_path / "out.txt")]
    assert "exactly one of" in _tool(out + ["--inliers-dir", "x"], capsys)
    assert "exactly one of" in _tool(out + ["--inliers-dir", "x", "--synthetic", "--keypts-dir", "k"], capsys)
    assert "--inliers-dir" in _tool(out + ["--synthetic"], capsys)
    assert "--calib-angle" in _tool(out + ["--inliers-dir", "x", "--keypts-dir", "k", "--calib-angle", "0.22"], capsys)
    assert "invalid choice" in _tool(out + ["--inliers-dir", "x", "--synthetic", "--nn", "tree"], capsys)


# ---- the two C entry points without a device --------------------------------------------------------------------------------------------
def test_icp_grid_entry_points_without_a_device():
    """caelo_icp_grid_ws_layout: offsets in order, multiples of 256, behind caelo_icp's own workspace, growing with n0 and m0, the refusals;
    caelo_icp_grid: what it refuses before it touches a device (no context exists here: every pointer is a host buffer never read)."""
    import ctypes as C
    from caelo import _ffi
    lib = _ffi.load()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "caelo.h")).read()
    for name in ("caelo_icp_grid", "caelo_icp_grid_ws_layout"):
        assert hasattr(lib, name) and name + "(" in header
    assert lib.caelo_abi_version() == _ffi.ABI_VERSION

    def layout(n0, n1, m0, m1):
        out = (C.c_int64 * 8)()
        assert lib.caelo_icp_grid_ws_layout(n0, n1, m0, m1, C.cast(out, C.c_void_p)) == 0
        return [int(v) for v in out]
    for n0, n1, m0, m1 in ((1, 1, 0, 0), (1300, 600, 0, 0), (1300, 600, 450, 390), (173056, 173056, 2000, 2000)):
        lay = layout(n0, n1, m0, m1)
        assert all(v % 256 == 0 for v in lay) and lay[0] >= lib.caelo_icp_loop_ws_bytes(n1, m1)
        assert all(lay[i] < lay[i + 1] for i in (0, 1, 3, 4, 6)) and lay[2] <= lay[3] and lay[5] <= lay[6]
        assert lay[3] - lay[2] >= 16 * n0 and lay[6] - lay[5] >= 16 * m0             # the (x, y, z, index) tables
        assert lay[1] - lay[0] >= 4 * ((1 << 22) + 1) and lay[4] - lay[3] >= 4 * ((1 << 18) + 1)   # cell starts: 2^22 / 2^18 cells + 1
    assert layout(2000, 600, 0, 0)[7] > layout(1300, 600, 0, 0)[7] and layout(1300, 600, 900, 390)[7] > layout(1300, 600, 450, 390)[7]
    out = (C.c_int64 * 8)()
    for bad in ((0, 1, 0, 0), (1, 0, 0, 0), (1, 1, -1, 0), (1, 1, 0, -1), (1 << 30, 1, 0, 0)):
        assert lib.caelo_icp_grid_ws_layout(*bad, C.cast(out, C.c_void_p)) == -1 and lib.caelo_last_error()
    assert lib.caelo_icp_grid_ws_layout(1, 1, 0, 0, None) == -1

    buf = np.zeros(4096, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert buf.ctypes.data % 16 == 0

    def refused(text, ctx=p, pc0=p, n0=8, n1=8, planar0=None, m0=0, ws=p, **over):
        kw = dict(threshold0=0.5, threshold1=5.0, decay0=0.9, decay1=0.9, small_shift=0.05, ep=0.001, max_iter=50, min_iter=19, min_pairs=100,
                  fail_only_first=0, use_planar=0, reserved=0)
        kw.update(over)
        prm = _ffi.IcpParams(**kw)
        assert lib.caelo_icp_grid(ctx, pc0, n0, p, n1, planar0, m0, p, 4, C.byref(prm), p, ws, None) == -1
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()
    refused("null argument", ctx=None)
    refused("null argument", pc0=None)
    refused("null argument", ws=None)
    refused("16-byte aligned", ws=C.c_void_p(buf.ctypes.data + 8))
    refused("bad shape", n0=0)
    refused("bad shape", n1=1 << 30)
    refused("planar points", use_planar=1)
    refused("max_iter", max_iter=0)
    for decay in (0.0, -0.5, 1.0 + 2.0 ** -40, float("nan")):
        refused("decay", decay0=decay)
        refused("decay", decay1=decay, use_planar=1, planar0=p, m0=4)
    refused("thresholds", threshold0=0.0)
    refused("thresholds", threshold0=float("inf"))
    refused("thresholds", threshold1=float("nan"), use_planar=1, planar0=p, m0=4)


# ---- refine_sequence.py on an engine that stands in for the device: its sources, options and what goes to which file ----------------------
class _Result:
    def __init__(self, R, T, ok):
        self.R_star, self.T_star, self.success = np.asarray(R, np.float64).ravel().tolist(), np.asarray(T, np.float64).ravel().tolist(), int(ok)


class _HostEngine:
    """Engine.icp / icp_result on the oracle's loops; host tensors."""
    device = "cpu"

    def __init__(self, orc):
        self.orc, self.calls = orc, []

    def icp(self, pc0, pc1, planar0=None, planar1=None, nn="brute", **kw):
        self.calls.append(dict(kw, nn=nn, planar=planar0 is not None, n0=pc0.shape[0], m1=None if planar1 is None else planar1.shape[0]))
        if planar0 is None:
            return _Result(*self.orc.ICP(pc0.numpy(), pc1.numpy(), maxIterTimes=kw["max_iter"], minIterTimes=kw["min_iter"], inlierThreshold=kw["threshold0"],
                                         smallShiftThreshold=kw["small_shift"], decay_rate=kw["decay0"], ep=kw["ep"]))
        return _Result(*self.orc.ICP_Pt2PtAndPt2Plane(pc0.numpy(), pc1.numpy(), planar0.numpy(), planar1.numpy(), maxIterTimes=kw["max_iter"],
                                                      minIterTimes=kw["min_iter"], inlierThreshold0=kw["threshold0"], decay_rate0=kw["decay0"],
                                                      inlierThreshold1=kw["threshold1"], decay_rate1=kw["decay1"], smallShiftThreshold=kw["small_shift"], ep=kw["ep"]))

    @staticmethod
    def icp_result(res):
        return res


@pytest.fixture()
def tool_tree(g, orc, tmp_path, monkeypatch):
    """Sequence 0 of the golden as files: poses, ground truth, calib_.txt, InliersIdx, KeyPts (400 extended points; planar = every
    fourth of them with the normal (0, 0, 1), 2 100 for frame 3) -- and refine_sequence.py's engine replaced by the host stand-in."""
    from scipy import io
    from caelo import stageio
    import caelo.engine
    eng = _HostEngine(orc)
    monkeypatch.setattr(caelo.engine, "default_engine", lambda: eng)
    n = g["est_0"].shape[0]
    np.savetxt(str(tmp_path / "est.txt"), g["est_0"])
    np.savetxt(str(tmp_path / "gt.txt"), g["gt_0"])
    calib = np.zeros((5, 12))
    calib[4] = g["tr_0"].astype(np.float64).reshape(12)
    np.savetxt(str(tmp_path / "calib_.txt"), calib, fmt="%.17g")
    pairs = _pairs(g, 0)
    (tmp_path / "KeyPts").mkdir()
    for f in range(n):
        if f < n - 1:
            stageio.save_inliers(str(tmp_path), f, f + 1, *pairs(f, f + 1))
        ext = g["clouds_0"][f]
        planar = np.c_[np.tile(ext[::4], (21, 1))[:2100] if f == 3 else ext[::4], np.zeros((2100 if f == 3 else 100, 2)), np.ones((2100 if f == 3 else 100, 1))]
        io.savemat(str(tmp_path / "KeyPts" / ("%06d.bin.mat" % f)), {"KeyPts": ext[:8], "ExtendedKeyPts": ext, "PlanarPts": planar.astype(np.float32)})
    common = ["--poses", str(tmp_path / "est.txt"), "--calib", str(tmp_path / "calib_.txt"), "--inliers-dir", str(tmp_path / "InliersIdx"),
              "--keypts-dir", str(tmp_path / "KeyPts")]
    return tmp_path, common, eng


def test_tool_key_frames_from_keypts_files_with_ground_truth(g, tool_tree, capsys):
    """--keypts-dir, --gt, --debug-info: the golden's real-ICP walk through the tool (the oracle's ICP behind Engine.icp), the printed
    lines, the DebugInfo.mat layout of RefinePoses.py:583-584 and the mean errors of :668-692."""
    import refine_sequence
    from scipy import io
    tmp, common, eng = tool_tree
    r = refine_sequence.run(common + ["--gt", str(tmp / "gt.txt"), "--out", str(tmp / "o" / "00.txt"), "--debug-info", str(tmp / "o" / "DebugInfo.mat"), "--nn", "brute"])
    assert r["tried"] == _rows(g["real_tried"]) and r["failed"] == [] and r["fixed"] == [] and r["second"] == []
    _within("real_icp", "poses", np.loadtxt(str(tmp / "o" / "00.txt")), g["real_poses"])
    info = io.loadmat(str(tmp / "o" / "DebugInfo.mat"))["aDebugInfo"]
    assert info.dtype == np.float32 and info.shape == g["real_debug"].shape and np.array_equal(info[:, 0:2], g["real_debug"][:, 0:2])
    _within("real_icp", "debug", info[:, 2:], g["real_debug"][:, 2:])
    assert all(c["nn"] == "brute" and not c["planar"] and c["threshold0"] == 0.5 and c["min_pairs"] == 100 for c in eng.calls)   # :295: ICP's defaults
    out = capsys.readouterr().out
    assert out.count("refine success, frame length =") == len(r["tried"])
    errs = {l.split()[0]: (float(l.split("=")[1].split()[0]), float(l.split("=")[2].split()[0])) for l in out.splitlines() if "mean sum|error Euler|" in l}
    from caelo import evaluate
    for label, poses in (("odometry", g["est_0"]), ("refined", r["poses"])):   # (per consecutive pair: only key frames were registered)
        _, _, e, t = evaluate.GetErrorRTs(g["gt_0"], poses, g["tr_0"])
        assert errs[label] == (float("%.6f" % np.mean(np.sum(np.abs(e), axis=1))), float("%.6f" % np.mean(np.linalg.norm(t, axis=1))))


def test_tool_second_pass_outputs(g, tool_tree):
    """--mode consecutive (12 key frames) with --second-pass: three more registrations at threshold 0.5 -- which pt2pt ignores, like
    RefinePoses.py:295 --; with --second-pass-out the refined poses go to --out and the second pass's to that file, without it the
    second pass's go to --out; --dejumped-out holds FixJumpPoses' poses."""
    import refine_sequence
    tmp, common, eng = tool_tree
    np.savetxt(common[1], g["dejump_translation_in"])
    base = common + ["--mode", "consecutive", "--dejump", "--dejumped-out", str(tmp / "a" / "poses__.txt")]
    first = refine_sequence.run(base + ["--out", str(tmp / "a" / "00.txt")])
    assert first["fixed"] == g["dejump_translation_fixed"].tolist() and first["second"] == []
    _within("dejump", "poses", np.loadtxt(str(tmp / "a" / "poses__.txt")), g["dejump_translation_out"])
    n_first = len(eng.calls)
    assert len(first["tried"]) == n_first == 12 and all(c["nn"] == "grid" for c in eng.calls)       # the tool's default search
    both = refine_sequence.run(base + ["--second-pass", "--out", str(tmp / "b" / "00.txt"), "--second-pass-out", str(tmp / "b" / "second.txt")])
    kf = both["debug"][:, 0].astype(int)
    assert [t[:2] for t in both["second"]] == [(kf[k], kf[k + 2]) for k in range(0, len(kf) - 7, 2)] and len(both["second"]) == 3
    one = refine_sequence.run(base + ["--second-pass", "--out", str(tmp / "c" / "00.txt")])
    read = lambda *p: open(os.path.join(str(tmp), *p), "rb").read()   # noqa: E731
    assert read("b", "00.txt") == read("a", "00.txt") != read("b", "second.txt") == read("c", "00.txt")
    assert np.array_equal(np.loadtxt(str(tmp / "c" / "00.txt")), one["poses"]) and not os.path.exists(str(tmp / "c" / "second.txt"))


def test_tool_pt2plane_with_planar_points(g, tool_tree):
    """--icp pt2plane accepted: RefinementCore's arguments of RefinePoses.py:291-294 reach the engine with both planar sets, frame 3's
    2 100 planar points are cut to 2 000 by RandomState(seed_base + k) of the k-th registration."""
    import refine_sequence
    tmp, common, eng = tool_tree
    r = refine_sequence.run(common + ["--mode", "consecutive", "--icp", "pt2plane", "--seed-base", "77", "--nn", "brute", "--out", str(tmp / "p" / "00.txt")])
    assert len(eng.calls) == len(r["tried"]) == 12 and all(t[2] == 1 for t in r["tried"])
    for k, c in enumerate(eng.calls):
        assert c["planar"] and (c["threshold0"], c["threshold1"], c["decay0"], c["decay1"], c["small_shift"], c["ep"]) == (1.0, 5.0, 0.9, 0.9, 0.1, 0.001)
        assert (c["max_iter"], c["min_iter"], c["min_pairs"], c["fail_only_first"]) == (50, 19, 200, 1)
        assert c["m1"] == (2000 if r["tried"][k][1] == 3 else 100)
    again = refine_sequence.run(common + ["--mode", "consecutive", "--icp", "pt2plane", "--seed-base", "77", "--nn", "brute", "--out", str(tmp / "q" / "00.txt")])
    assert np.array_equal(again["poses"], r["poses"])
    other = refine_sequence.run(common + ["--mode", "consecutive", "--icp", "pt2plane", "--seed-base", "78", "--nn", "brute", "--out", str(tmp / "s" / "00.txt")])
    assert not np.array_equal(other["poses"], r["poses"])   # (another draw of frame 3's planar points)
