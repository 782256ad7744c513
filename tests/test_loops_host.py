"""The host twins of the loop-closure kernels (caelo_host_scan_context, caelo_host_loop_search; csrc/loopclose_host.hip)
against the NumPy restatement tests/loops_ref.py, the entry points' refusals, and the stand-alone program the host sanitizers run.
CPU only; tests/test_loops_gpu.py holds the device to these twins byte for byte.

Measured on this suite's inputs (profiles/loops_errors.txt): the largest |d - restatement| of a dense distance is 6.8e-7 against
the bar of 7.2e-5."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import loops_cases as lc
import loops_ref as lr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the descriptor ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.descriptor_batches()))
def test_descriptor_equals_the_restatement_bit_for_bit(name):
    pts, n_pts = lc.descriptor_batches()[name]
    sc, u, valid = lc.host_scan_context(pts, n_pts)
    for f in range(len(pts)):
        want = lr.scan_context(pts[f, :n_pts[f]])
        assert sc[f].tobytes() == want.tobytes(), (name, f)
        u64, v64 = lr.prepare(want)
        assert np.array_equal(lc.valid_bits(valid[f:f + 1])[0], v64) and np.abs(u[f] - u64).max() <= 2.0 ** -23, (name, f)
        assert n_pts[f] > 0 or (not sc[f].any() and not u[f].any() and valid[f] == 0)


@pytest.mark.parametrize("cols", [3, 4])
def test_crafted_cloud_pins_every_edge(cols):
    """What each crafted point was built to decide (tests/loops_cases.py CRAFTED), written out by hand: the axes open sectors 0, 15, 30,
    45, r = 4 k opens ring k, the float32 below 80 is ring 19 and 80 is out, the maximum of a bin, values below zero, skipped points."""
    pts, n_pts = lc.descriptor_batches()["crafted c=%d" % cols]
    sc, _, valid = lc.host_scan_context(pts, n_pts)
    want = lc.crafted_expected()
    assert sc[0].tobytes() == want.tobytes()
    assert sc[0, 1, 15] == np.float32(2.25) and sc[0, 1, 14] == 0 and sc[0, 1, 30] == np.float32(2.375) and sc[0, 1, 29] == 0
    assert sc[0, 1, 45] == np.float32(2.5) and sc[0, 1, 44] == 0 and sc[0, 19, 15] == np.float32(2.75) and sc[0, 2, 59] == np.float32(2.875)
    assert sc[0, 7, 7] == np.float32(-1.5) and sc[0, 7, 22] == 0 and sc[0, 10, 37] == np.float32(3.5) and sc[0, 0, 0] == np.float32(4.5)
    assert sc[0].max() < 9                                              # no skipped point (z = 9) came through
    assert not (int(valid[0]) >> 22) & 1 and (int(valid[0]) >> 7) & 1   # a column of zeros is not valid, a negative one is


def test_prepare_zero_one_entry_and_negative_columns():
    img = np.zeros((lr.RINGS, lr.SECTORS), np.float32)
    img[4, 9] = 1.75                                                    # one entry: the unit value is 1 exactly
    img[6, 10] = -0.5                                                   # ... or -1
    img[0:3, 11] = (3.0, -4.0, 12.0)                                    # norm 13
    sc, u, valid = lc.host_scan_context(*lc.pack([lc.cloud_of_image(img)]))
    assert sc[0].tobytes() == img.tobytes()
    cols = u[0].reshape(lr.SECTORS, lr.RINGS)
    assert cols[9, 4] == 1.0 and cols[10, 6] == -1.0 and np.count_nonzero(cols[9]) == 1 and np.count_nonzero(cols[10]) == 1
    assert np.array_equal(cols[11, 0:3], np.array([3, -4, 12], np.float32) / np.float32(13))
    assert int(valid[0]) == (1 << 9) | (1 << 10) | (1 << 11) and not cols[[c for c in range(60) if c not in (9, 10, 11)]].any()


# ---- the search -------------------------------------------------------------------------------------------------------------------------
def compare_with_restatement(label, u64, v64, kw, cand, dist, shift, dd, ds):
    """-> the largest |d - restatement| of the dense image"""
    bar = lr.DIST_BAR
    ref = lr.search(u64, v64, **kw)
    fin = np.isfinite(ref["d"])
    assert np.array_equal(np.isfinite(dd), fin) and np.isposinf(dd[~fin]).all() and (ds[~fin] == -1).all(), label
    worst = float(np.abs(dd[fin] - ref["d"][fin]).max()) if fin.any() else 0.0
    assert worst <= bar, (label, worst)
    two = np.sort(ref["all"], axis=2)[:, :, :2]
    with np.errstate(invalid="ignore"):                                 # inf - inf where no shift counts
        clear = fin & ~(two[:, :, 1] - two[:, :, 0] <= 2 * bar)
    assert np.array_equal(ds[clear], ref["shift"][clear]) and (ds[fin] >= 0).all(), label
    # the k best: the t-th smallest of a row moves by no more than its entries do; the candidate is decided where its neighbours in
    # the restatement's order are further than twice the bar away
    got_fin = np.isfinite(dist)
    assert np.array_equal(got_fin, np.isfinite(ref["dist"])) and (cand[~got_fin] == -1).all() and (shift[~got_fin] == -1).all(), label
    assert np.abs(dist[got_fin] - ref["dist"][got_fin]).max(initial=0.0) <= bar, label
    n = len(u64)
    for q in range(n):
        row = np.sort(np.where(np.isfinite(ref["d"][q]), ref["d"][q], np.inf))
        for t in range(kw["k"]):
            if not got_fin[q, t]:
                continue
            lo = row[t] - row[t - 1] if t else np.inf
            hi = row[t + 1] - row[t] if t + 1 < n else np.inf
            if lo > 2 * bar and hi > 2 * bar:
                assert cand[q, t] == ref["cand"][q, t], (label, q, t)
            assert dist[q, t] == dd[q, cand[q, t]] and shift[q, t] == ds[q, cand[q, t]], (label, q, t)
    return worst


@pytest.mark.parametrize("name", sorted(lc.search_cases()))
def test_search_against_the_restatement(name):
    u, valid, u64, v64, kw = lc.search_cases()[name]
    out = lc.host_loop_search(u, valid, dense=True, **kw)
    worst = compare_with_restatement(name, u64, v64, kw, *out)
    print("loops_errors %-24s host twin against the restatement: N = %d, largest |d - d64| = %.3e (bar %.3e)" % (name, len(u), worst, lr.DIST_BAR))
    plain = lc.host_loop_search(u, valid, **kw)                          # the dense images change nothing
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, out[:3]))


def test_planted_pairs_are_found_with_their_shift():
    _, u, valid, _, _ = lc.search_images()
    cand, dist, shift = lc.host_loop_search(u, valid, min_gap=3, k=1)
    for i, j, s in lc.PLANTED:
        assert (cand[i, 0], shift[i, 0]) == (j, s) and dist[i, 0] < 1e-3, (i, j, s)
    others = np.setdiff1d(np.arange(3, 70), [p[0] for p in lc.PLANTED])
    assert dist[others, 0].min() > 0.3                                   # unrelated images are nowhere near


def test_edges_of_the_candidate_range():
    cases = lc.search_cases()
    cand, dist, shift = lc.host_loop_search(*cases["one frame"][:2], **cases["one frame"][4])
    assert cand.tolist() == [[-1]] and np.isposinf(dist).all() and shift.tolist() == [[-1]]
    cand, dist, shift = lc.host_loop_search(*cases["N = min_gap"][:2], **cases["N = min_gap"][4])
    assert (cand == -1).all() and np.isposinf(dist).all() and (shift == -1).all()
    cand, dist, shift = lc.host_loop_search(*cases["N = min_gap + 1"][:2], **cases["N = min_gap + 1"][4])
    assert cand[:5].max() == -1 and cand[5].tolist() == [0, -1] and np.isfinite(dist[5, 0]) and np.isposinf(dist[5, 1]) and shift[5, 1] == -1
    cand, dist, shift = lc.host_loop_search(*cases["fewer than k"][:2], **cases["fewer than k"][4])
    for q in range(6):
        assert sorted(cand[q, :q].tolist()) == list(range(q)) and (cand[q, q:] == -1).all() and (np.diff(dist[q, :q]) >= 0).all()
    # the empty frame: no distance to or from it
    u, valid, _, _, kw = cases["an empty frame"]
    cand, dist, shift, dd, ds = lc.host_loop_search(u, valid, dense=True, **kw)
    assert valid[3] == 0 and (cand[3] == -1).all() and np.isposinf(dd[:, 3]).all() and (ds[:, 3] == -1).all() and not (cand == 3).any()
    assert np.isfinite(dd[8, [0, 1, 2, 4, 5, 6, 7]]).all()


@pytest.mark.parametrize("queries", [(20, 37), (0, 16), (69, 70), (33, 33)])
def test_a_query_range_equals_its_slice_of_the_full_result(queries):
    _, u, valid, _, _ = lc.search_images()
    full = lc.host_loop_search(u, valid, min_gap=3, k=4, dense=True)
    part = lc.host_loop_search(u, valid, min_gap=3, k=4, dense=True, queries=queries)
    for a, b in zip(full, part):
        assert a[queries[0]:queries[1]].tobytes() == b.tobytes()


def test_ties_go_to_the_lower_candidate_and_the_lower_shift():
    u, valid, _, _ = lc.identical_frames()
    cand, dist, shift = lc.host_loop_search(u, valid, min_gap=1, k=4)
    assert cand[4].tolist() == [0, 1, 2, 3] and (shift[4] == 0).all() and len(set(dist[4].tolist())) == 1
    assert cand[2].tolist() == [0, 1, -1, -1]
    u, valid, _, _ = lc.period_30()
    cand, dist, shift, dd, ds = lc.host_loop_search(u, valid, min_gap=1, k=1, dense=True)
    assert cand[1, 0] == 0 and shift[1, 0] == 10 and ds[1, 0] == 10 and dist[1, 0] < 1e-6


def test_min_cols_and_max_dist_at_their_values():
    u, valid, u64, v64 = lc._small(2, 30)
    cand, dist, shift = lc.host_loop_search(u, valid, min_gap=1, k=1)
    _, cnt = lr.shift_distances(u64, v64)
    s0, n0 = int(shift[1, 0]), int(cnt[1, 0, shift[1, 0]])
    assert 1 < n0 < 60
    for min_cols in (n0 - 1, n0):
        got = lc.host_loop_search(u, valid, min_gap=1, k=1, min_cols=min_cols)
        assert got[2][1, 0] == s0 and got[1][1, 0] == dist[1, 0]
    got = lc.host_loop_search(u, valid, min_gap=1, k=1, min_cols=n0 + 1)
    assert got[2][1, 0] != s0 and (got[2][1, 0] == -1 or cnt[1, 0, got[2][1, 0]] > n0)
    d0 = dist[1, 0]
    assert lc.host_loop_search(u, valid, min_gap=1, k=1, max_dist=float(d0))[0][1, 0] == -1               # strictly below
    assert lc.host_loop_search(u, valid, min_gap=1, k=1, max_dist=float(np.nextafter(d0, np.float32(2))))[0][1, 0] == 0


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_device():
    from caelo import _ffi
    lib = _ffi.load()
    header = open(os.path.join(REPO, "include", "caelo.h")).read()
    names = ("caelo_sc_ws_bytes", "caelo_scan_context", "caelo_host_scan_context", "caelo_loop_search_ws_bytes", "caelo_loop_search",
             "caelo_host_loop_search")
    for name in names:
        assert hasattr(lib, name) and name + "(" in header
    assert lib.caelo_abi_version() == _ffi.ABI_VERSION == 6
    assert lib.caelo_sc_ws_bytes(3) >= 3 * 4800 and lib.caelo_sc_ws_bytes(3) % 16 == 0
    assert lib.caelo_loop_search_ws_bytes(100, 0, 100, 50, 8) >= 7 * 1 * 16 * 8 * 8 and lib.caelo_loop_search_ws_bytes(100, 0, 100, 0, 8) == 0
    buf = np.zeros(4096, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    odd = C.c_void_p(buf.ctypes.data + 8)
    assert buf.ctypes.data % 16 == 0
    inf = float("inf")

    def sc_host(text, pts=p, ld=10, cols=3, n_pts=p, f=1, sc=p, u=p, valid=p):
        assert lib.caelo_host_scan_context(pts, ld, cols, n_pts, f, sc, u, valid) == -1
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()

    def sc_device(text, ctx=p, pts=p, ld=10, cols=3, n_pts=p, f=1, sc=p, u=p, valid=p, ws=p):
        # (no context exists here: every pointer is a host buffer that is never read)
        assert lib.caelo_scan_context(ctx, pts, ld, cols, n_pts, f, sc, u, valid, ws, None) == -1
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()

    def ls_host(text, u=p, valid=p, n=10, q0=0, q1=10, min_gap=2, k=1, max_dist=inf, min_cols=1, cand=p, dist=p, shift=p, dd=None, ds=None):
        assert lib.caelo_host_loop_search(u, valid, n, q0, q1, min_gap, k, max_dist, min_cols, cand, dist, shift, dd, ds) == -1
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()

    def ls_device(text, ctx=p, u=p, valid=p, n=10, q0=0, q1=10, min_gap=2, k=1, max_dist=inf, min_cols=1, cand=p, dist=p, shift=p, dd=None,
                  ds=None, ws=p):
        assert lib.caelo_loop_search(ctx, u, valid, n, q0, q1, min_gap, k, max_dist, min_cols, cand, dist, shift, dd, ds, ws, None) == -1
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()
    for refuse in (sc_host, sc_device):
        for name in ("pts", "n_pts", "sc", "u", "valid"):
            refuse("null argument", **{name: None})
        for cols in (0, 2, 5):
            refuse("3 or 4 columns", cols=cols)
        refuse("bad shape", ld=0)
        refuse("bad shape", f=-1)
    sc_device("null argument", ctx=None)
    sc_device("null argument", ws=None)
    sc_device("16-byte aligned", ws=odd)
    sc_device("16-byte aligned", u=odd)
    for refuse in (ls_host, ls_device):
        for name in ("u", "valid", "cand", "dist", "shift"):
            refuse("null argument", **{name: None})
        for k in (0, 9):
            refuse("k outside 1..8", k=k)
        refuse("min_gap < 1", min_gap=0)
        for min_cols in (0, 61):
            refuse("min_cols outside 1..60", min_cols=min_cols)
        refuse("bad frame or query range", n=0)
        refuse("bad frame or query range", q1=11)
        refuse("bad frame or query range", q0=5, q1=4)
        refuse("bad frame or query range", q0=-1)
        refuse("max_dist is a NaN", max_dist=float("nan"))
        refuse("dense outputs come as a pair", dd=p)
        refuse("dense outputs come as a pair", ds=p)
        refuse("above 4096 frames", n=4097, q1=1, dd=p, ds=p)
    ls_device("null argument", ctx=None)
    ls_device("null argument", ws=None)
    ls_device("16-byte aligned", ws=odd)
    ls_device("16-byte aligned", u=odd)
    assert not buf.any()


def test_host_twins_link_and_run_alone(tmp_path):
    """csrc/loopclose_host.hip is plain C++ and needs nothing of the library: compiled with tools/micro/loopclose_main.cpp into a
    stand-alone program under -fsanitize=address,undefined and run once on the capacity and the empty cases (nothing is loaded into
    Python)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "loopclose_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(REPO, "tools", "micro", "loopclose_main.cpp"),
                           os.path.join(REPO, "cae-lo_amd", "csrc", "loopclose_host.hip"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"loopclose ok" in r.stdout, r.stdout.decode()


# ---- evaluate.py loops ------------------------------------------------------------------------------------------------------------------
def test_evaluate_loops_on_a_hand_made_file(tmp_path, capsys):
    """The 16-frame revisit layout (tests/loops_seq.py; no scans are made): the 8 true loops with a known error on each motion, one
    false loop and one true loop left unverified -> recall, both precisions and the errors, through the command line."""
    import loops_seq as ls
    sys_path = os.path.join(REPO, "cae-lo_amd")
    import sys
    if sys_path not in sys.path:
        sys.path.insert(0, sys_path)
    import evaluate as ev_cli
    from caelo import evaluate as ev
    from caelo import loops as lp
    gt, calib = ls.write_ground_truth(tmp_path)
    rows = np.zeros((10, lp.LOOP_COLUMNS))
    for k in range(8):
        R, T = ls.true_motion(8 + k, k)
        a = np.radians(0.1 * k)                                          # an error of 0.1 k degrees about z and of 0.05 k m along x
        dR = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        rows[k, 0:7] = (8 + k, k, 0.25, 3, 0 if k == 7 else 1, 200, 0.4)
        rows[k, 7:16], rows[k, 16:19] = (R @ dR).reshape(9), T + (0.05 * k, 0, 0)
    rows[8, 0:7] = (15, 2, 0.4, 0, 1, 30, 1.0)                          # a false loop, verified: frame 2 is 30 m from frame 15
    rows[8, 7:16] = np.eye(3).reshape(9)
    rows[9, 0:7] = (14, 7, 0.44, 0, 0, 0, 0.0)                          # ... and one that is not
    rows[9, 7:16] = np.eye(3).reshape(9)
    path = lp.write_loops(str(tmp_path / "loops.txt"), rows)
    back = lp.read_loops(path)
    assert back.shape == (10, 19) and np.array_equal(back, np.loadtxt(path)) and np.abs(back - rows).max() < 1e-9
    res = ev.loops(np.loadtxt(gt), ev.read_tr(calib), back, revisit_radius=4.0, min_gap=4)
    assert res["n_revisit_queries"] == 8 and res["recall"] == 1.0 and res["precision"] == 0.8 and res["precision_verified"] == 7 / 8
    assert res["n_verified"] == 8 and np.allclose(res["RRE"][:7], 0.1 * np.arange(7), atol=1e-5) and np.allclose(res["RTE"][:7], 0.05 * np.arange(7), atol=1e-5)   # (Tr is read as float32)
    assert res["success"].tolist() == [True] * 7 + [False] and res["RTE"][7] > 25
    # a revisit radius below the 1.1 m offset: no revisit at all; a gap beyond the sequence as well
    assert ev.loops(np.loadtxt(gt), ev.read_tr(calib), back, revisit_radius=1.0, min_gap=4)["n_revisit_queries"] == 0
    assert ev.loops(np.loadtxt(gt), ev.read_tr(calib), back, revisit_radius=4.0, min_gap=9)["n_revisit_queries"] == 0
    assert ev_cli.main(["loops", "--gt", gt, "--calib", calib, "--loops", path, "--min-gap", "4"]) == 0
    out = capsys.readouterr().out
    assert "recall 1  precision 0.8  precision of verified 0.875" in out and "success 7 of 8" in out
    for bad, text in ((["--min-gap", "0"], "--min-gap must be >= 1"), (["--revisit-radius", "0"], "--revisit-radius must be a positive")):
        with pytest.raises(SystemExit) as e:
            ev_cli.main(["loops", "--gt", gt, "--calib", calib, "--loops", path] + bad)
        assert e.value.code == 2 and text in capsys.readouterr().err
    rows[3, 0] = 16
    lp.write_loops(path, rows)
    with pytest.raises(SystemExit):
        ev_cli.main(["loops", "--gt", gt, "--calib", calib, "--loops", path])
    assert "outside the 16 ground truth poses" in capsys.readouterr().err
    # an empty loops file is a valid answer
    lp.write_loops(path, np.zeros((0, 19)))
    res = ev.loops(np.loadtxt(gt), ev.read_tr(calib), lp.read_loops(path), min_gap=4)
    assert res["n_loops"] == 0 and res["recall"] == 0.0 and np.isnan(res["precision"])


def test_detect_loops_argument_errors(capsys):
    import sys
    if os.path.join(REPO, "cae-lo_amd") not in sys.path:
        sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
    import detect_loops
    for argv, text in ((["--out", "x"], "exactly one of --scans DIR and --synthetic N"),
                       (["--out", "x", "--synthetic", "4", "--scans", "d"], "exactly one of"),
                       (["--out", "x", "--synthetic", "4", "--top-k", "9"], "--top-k must lie in 1..8"),
                       (["--out", "x", "--synthetic", "4", "--min-gap", "0"], "--min-gap must be >= 1"),
                       (["--out", "x", "--synthetic", "4", "--min-cols", "61"], "--min-cols must lie in 1..60"),
                       (["--out", "x", "--synthetic", "4", "--max-dist", "0"], "--max-dist must be a positive number"),
                       (["--out", "x", "--synthetic", "4", "--calib-angle", "nan"], "--calib-angle must be a finite"),
                       (["--out", "x", "--synthetic", "4", "--no-verify", "--no-derotate"], "--no-verify stops after the search"),
                       (["--out", "x", "--synthetic", "4", "--features-from", "/nonexistent/dir"], "is not a directory"),
                       (["--out", "x", "--synthetic", "4", "--seed-base", "-1"], "must lie in [0, 2^32)"),
                       (["--out", "x", "--scans", "/nonexistent/dir"], "no .bin files in")):
        with pytest.raises(SystemExit) as e:
            detect_loops.run(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
