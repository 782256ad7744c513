"""Engine.register_pairs / caelo_register_pairs (csrc/regpairs.hip): a table of frame pairs registered from resident rows gives the
pipeline's results on consecutive pairs and the staged calls' results (caelo_match + caelo_ransac + the host half) on any pair, bit
for bit; run_sequence.py --frame-steps writes what a plain run over every s-th scan writes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

N_FRAMES = 12
SEED0 = 4200
ANY_PAIRS = [(0, 5), (5, 10), (3, 3), (7, 2), (0, 1), (0, 10), (11, 0)]
REL_TOL = 1e-4   # poses against the reference's goldens: within 1e-4 relative, as tests/test_gpu_parity.py asks of every pose
FIELDS = ("R", "T", "R_ransac", "T_ransac", "threshold", "success", "iterations", "n_inliers", "n_pairs")


@pytest.fixture(scope="module")
def seq(engine, scans):
    """12 synthetic frames through the pipeline once, certified and not, with pair (i - 1, i) drawing RandomState(SEED0 + i); the
    rows of the certified run are the resident rows of every test here.  Shared and never written."""
    from caelo.engine import ransac_draws
    dev = engine.device
    pcs = [torch.from_numpy(scans(f)).to(dev) for f in range(N_FRAMES)]
    draws = [ransac_draws(SEED0 + i) for i in range(N_FRAMES)]
    rands = [torch.from_numpy(d).to(dev) for d in draws]
    pipe = engine.pipeline(8)
    exact = pipe.run(pcs, rands, certify=True, rands_host=draws)
    plain = pipe.run(pcs, rands, certify=False)
    torch.cuda.synchronize()
    assert torch.equal(exact.rows, plain.rows) and torch.equal(exact.n_key, plain.n_key)
    return dict(rows=exact.rows[:N_FRAMES].contiguous(), n_key=exact.n_key[:N_FRAMES].contiguous(), draws=draws, rands=rands, exact=exact, plain=plain)


def _same_records(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), "%s: field %s differs" % (what, f)


@pytest.fixture(scope="module")
def staged(engine, seq):
    """The yardstick of any pair: Engine.match + Engine.ransac (+ the host half) on the two frames, computed once per (pair, seed)."""
    from caelo.engine import FrameFeatures
    cache = {}

    def get(a, b, j, certify):
        key = (a, b, j, certify)
        if key not in cache:
            fa = FrameFeatures(seq["rows"][a], None, seq["n_key"][a:a + 1], None, None)
            fb = FrameFeatures(seq["rows"][b], None, seq["n_key"][b:b + 1], None, None)
            if certify:
                r, m, x = engine.match_pose_exact(fa, fb, seq["rands"][j], seq["draws"][j])
                cache[key] = (r, np.asarray(m), x.cpu().numpy())
            else:
                r, m, x = engine.match_pose(fa, fb, seq["rands"][j])
                from caelo import _ffi
                cache[key] = (np.frombuffer(r.cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE)[0], m.cpu().numpy(), x.cpu().numpy())
        return cache[key]
    return get


@pytest.mark.parametrize("certify", [True, False])
def test_consecutive_table_equals_the_pipeline(engine, seq, certify):
    table = [(i - 1, i) for i in range(1, N_FRAMES)]
    out = engine.register_pairs(seq["rows"], seq["n_key"], table, np.stack(seq["draws"][1:]), certify=certify)
    ref = seq["exact"] if certify else seq["plain"]
    from caelo import _ffi
    if certify:
        res, masks = ref.exact[0][1:N_FRAMES], ref.exact[1][1:N_FRAMES]
    else:
        res = np.frombuffer(ref.result[1:N_FRAMES].cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE)
        masks = ref.inlier_mask[1:N_FRAMES].cpu().numpy()
    assert np.array_equal(out.pair_idx.cpu().numpy(), ref.pair_idx[1:N_FRAMES].cpu().numpy())
    assert np.array_equal(out.masks, masks)
    _same_records(out.results, res, "consecutive table vs pipeline")
    assert (out.status == 0).all() and engine.lane_faults() == 0


@pytest.mark.parametrize("certify", [True, False])
@pytest.mark.parametrize("n_pairs", [1, 8, 9, 17])   # one under, at, one over and two slices over a launch of 8 pairs
def test_any_pair_equals_the_staged_calls(engine, seq, staged, n_pairs, certify):
    """(3, 3): every point matches the first point with its descriptor (itself unless patches repeat) -- success, and R = I, T = 0 to what float32 Kabsch leaves of them: 16 eps32 = 1e-6 in R (the
    certificate's own constant), times coordinates of up to ~100 m in T: 1e-4.  Asserted at 1e-5 / 1e-3, and bit for bit against the staged path."""
    table = [ANY_PAIRS[i % len(ANY_PAIRS)] for i in range(n_pairs)]
    js = [i % N_FRAMES for i in range(n_pairs)]   # pair i draws the stream of frame js[i]
    out = engine.register_pairs(seq["rows"], seq["n_key"], table, np.stack([seq["draws"][j] for j in js]), certify=certify)
    idx = out.pair_idx.cpu().numpy()
    for i, ((a, b), j) in enumerate(zip(table, js)):
        r, m, x = staged(a, b, j, certify)
        assert np.array_equal(idx[i], x), "pair %d (%d, %d): pair_idx" % (i, a, b)
        assert np.array_equal(out.masks[i], m), "pair %d (%d, %d): inlier mask" % (i, a, b)
        _same_records(out.results[i], r, "pair %d (%d, %d)" % (i, a, b))
        if a == b:
            k = int(seq["n_key"][a].item())
            # every point matches itself -- or, where patches repeat, the FIRST point with the same descriptor (Match.py:258)
            f = seq["rows"][a, :k, 0:60].cpu().numpy()
            assert (idx[i][:k] <= np.arange(k)).all() and np.array_equal(f[idx[i][:k]], f) and out.results[i]["success"] == 1
            assert np.abs(out.results[i]["R"].reshape(3, 3) - np.eye(3)).max() <= 1e-5 and np.abs(out.results[i]["T"]).max() <= 1e-3


def _golden_rows():
    rows = np.zeros((2, 1024, 64), dtype=np.float32)
    for f in (0, 1):
        g = np.load(os.path.join(GOLDEN, "frame_%d.npz" % f))
        rows[f, :, 0:60], rows[f, :, 60:63], rows[f, :, 63] = g["features"], g["keypts_demo"], 1.0
    return rows


def test_golden_pair_in_the_first_and_in_a_second_slice(engine):
    """tests/golden/pair_0_1.npz (the reference's SolveRelativePose, np.random.seed(0)) at table positions 0 and 9.  The call orders
    its slices by (frame 0, frame 1): the seven (0, 0) fillers sort first, so entry 0 runs in slot 7 of the first launch and entry 9 in
    slot 0 of the second."""
    from caelo.engine import ransac_draws
    g = np.load(os.path.join(GOLDEN, "pair_0_1.npz"))
    rows = torch.from_numpy(_golden_rows()).to(engine.device)
    nk = torch.full((2,), 1024, dtype=torch.int32, device=engine.device)
    table = [(0, 1)] + [(0, 0)] * 7 + [(1, 1)] + [(0, 1)]
    out = engine.register_pairs(rows, nk, table, np.stack([ransac_draws(0)] * len(table)), certify=True)
    idx = out.pair_idx.cpu().numpy()
    for q in (0, 9):
        r = out.results[q]
        assert np.array_equal(idx[q], g["pair_idx"].astype(np.int64))
        assert bool(r["success"]) == bool(g["s0_ok"]) and float(r["threshold"]) == np.float32(g["s0_thr"])
        assert np.array_equal(np.flatnonzero(out.masks[q]), g["s0_idx1"]) and np.array_equal(idx[q][g["s0_idx1"]], g["s0_idx0"])
        assert np.abs(r["R"].reshape(3, 3) - g["s0_R"]).max() <= REL_TOL
        assert np.abs(r["T"].reshape(3, 1) - g["s0_T"]).max() <= REL_TOL * max(1.0, np.abs(g["s0_T"]).max())


@pytest.mark.parametrize("certify", [True, False])
def test_frames_with_fewer_key_points(engine, seq, certify):
    """Frames with n_key 51 and 700 whose rows past n_key hold NaN, paired with each other and with full frames: the staged calls'
    results -- a lane that read past n_key would meet a NaN."""
    from caelo.engine import FrameFeatures
    from caelo import _ffi
    rows = seq["rows"][:4].clone()
    nk = seq["n_key"][:4].clone()
    rows[1, 51:] = float("nan"); nk[1] = 51
    rows[2, 700:] = float("nan"); nk[2] = 700
    table = [(1, 2), (2, 1), (0, 1), (1, 0), (2, 3), (3, 2), (1, 1)]
    draws = [seq["draws"][i] for i in range(len(table))]
    out = engine.register_pairs(rows, nk, table, np.stack(draws), certify=certify)
    idx = out.pair_idx.cpu().numpy()
    for i, (a, b) in enumerate(table):
        fa = FrameFeatures(rows[a], None, nk[a:a + 1], None, None)
        fb = FrameFeatures(rows[b], None, nk[b:b + 1], None, None)
        if certify:
            r, m, x = engine.match_pose_exact(fa, fb, seq["rands"][i], draws[i])
        else:
            r, m, x = engine.match_pose(fa, fb, seq["rands"][i])
            r, m = np.frombuffer(r.cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE)[0], m.cpu().numpy()
        kb = int(nk[b].item())
        assert np.array_equal(idx[i][:kb], x.cpu().numpy()[:kb]) and int(idx[i][:kb].max()) < int(nk[a].item())
        assert np.array_equal(out.masks[i][:kb], np.asarray(m)[:kb]) and not out.masks[i][kb:].any()
        _same_records(out.results[i], r, "pair %d (%d, %d)" % (i, a, b))
        assert np.isfinite(out.results[i]["R"]).all() and np.isfinite(out.results[i]["T"]).all()


def test_refusals_come_before_any_launch(engine, seq):
    """Argument checks only: nothing is launched for a refused table, and the next valid call gives the usual result."""
    from caelo import _ffi
    rows, nk = seq["rows"], seq["n_key"]
    d = np.stack(seq["draws"][:2])
    for bad in ([(0, 1), (0, N_FRAMES)], [(0, 1), (-1, 2)]):
        with pytest.raises(_ffi.CaeloError, match="outside"):
            engine.register_pairs(rows, nk, bad, d, certify=False)
    for count in (0, 1025):
        nk2 = nk.clone()
        nk2[4] = count
        with pytest.raises(_ffi.CaeloError, match="n_key"):
            engine.register_pairs(rows, nk2, [(0, 1), (4, 5)], d, certify=False)
        engine.register_pairs(rows, nk2, [(0, 1), (2, 3)], d, certify=False)      # frame 4 is not in the table: legal
    out = engine.register_pairs(rows, nk, [(0, 1)], d[1:2], certify=False)
    want = np.frombuffer(seq["plain"].result[1:2].cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE)
    _same_records(out.results, want, "after the refusals")


def test_solve_relative_poses_is_the_batched_api(engine, seq):
    """api.SolveRelativePoses against api.SolveRelativePose on the same two frames and draws: every element of the tuple."""
    from caelo import api
    pairs, seeds = [(0, 1), (0, 5), (7, 2)], [SEED0 + 1, SEED0 + 2, SEED0 + 3]
    res = api.SolveRelativePoses(seq["rows"], pairs, seeds)
    rows, nk = seq["rows"].cpu().numpy(), seq["n_key"].cpu().numpy()
    for (a, b), seed, (R, T, ok, i0, i1, thr) in zip(pairs, seeds, res):
        wR, wT, wok, wi0, wi1, wthr = api.SolveRelativePose(rows[a, :nk[a], 60:63], rows[a, :nk[a], 0:60], None, rows[b, :nk[b], 60:63],
                                                           rows[b, :nk[b], 0:60], None, rng=np.random.RandomState(seed))
        assert np.array_equal(R, wR) and np.array_equal(T, wT) and ok == wok and thr == wthr
        assert np.array_equal(i0, wi0) and np.array_equal(i1, wi1)


# ---- run_sequence.py --frame-steps ------------------------------------------------------------------------------------------------
RS = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")
EVP = os.path.join(REPO, "cae-lo_amd", "evaluate.py")
N_SEQ, STEP = 24, 5


def _run(args):
    subprocess.run([sys.executable, RS] + [str(a) for a in args], check=True, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory, scans):
    """A run without the option, and a plain run over scans 0, 5, 10, 15, 20 written to a --scans directory (same --seed-base)."""
    d = tmp_path_factory.mktemp("steps")
    _run(["--synthetic", N_SEQ, "--trajectory", "line", "--matchability", d / "plain" / "m.mat", "--out", d / "plain" / "00.txt"])
    sub = d / "sub" / "velodyne"
    os.makedirs(str(sub))
    for k, f in enumerate(range(0, N_SEQ, STEP)):
        scans(f).astype(np.float32).tofile(str(sub / ("%06d.bin" % k)))
    _run(["--scans", sub, "--matchability", d / "sub" / "m.mat", "--out", d / "sub" / "00.txt"])
    return d


@pytest.mark.parametrize("chunk", [960, 8])   # 8: step-5 pairs cross chunk boundaries
def test_run_sequence_frame_steps(plain_runs, tmp_path, chunk):
    from scipy import io
    d = plain_runs
    _run(["--synthetic", N_SEQ, "--trajectory", "line", "--frame-steps", "1,%d" % STEP, "--chunk", chunk, "--matchability", tmp_path / "m.mat", "--out", tmp_path / "00.txt"])
    rd = lambda p: open(str(p), "rb").read()
    assert rd(tmp_path / "00.txt") == rd(d / "plain" / "00.txt")
    # (a MAT-file opens with 128 bytes of header whose text carries the time of writing: everything behind it, byte for byte)
    assert rd(tmp_path / "m.mat")[128:] == rd(d / "plain" / "m.mat")[128:] and len(rd(tmp_path / "m.mat")) > 128
    step_lines = rd(tmp_path / ("%d_00.txt" % STEP)).splitlines()
    sub_lines = rd(d / "sub" / "00.txt").splitlines()
    assert len(step_lines) == N_SEQ and len(sub_lines) == 5
    assert [step_lines[i] for i in range(0, N_SEQ, STEP)] == sub_lines
    assert all(step_lines[i] == step_lines[i - i % STEP] for i in range(N_SEQ))      # in between: the preceding multiple's row
    ms, mp = io.loadmat(str(tmp_path / ("%d_m.mat" % STEP))), io.loadmat(str(d / "sub" / "m.mat"))
    for key in ("AllProportions", "AllTrialCounts"):
        assert ms[key].shape == (1, 4) and np.array_equal(ms[key], mp[key])
    # evaluate.py registration --frame-step 5 on the step file = --frame-step 1 on the sub-sampled files
    import math
    from caelo import synth
    gt = np.zeros((N_SEQ, 12))
    for i in range(N_SEQ):
        (x, y, z), yaw = synth.sensor_pose(i)   # ("line": the trajectory of the shared scans)
        c, s = math.cos(yaw), math.sin(yaw)
        gt[i] = np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, z]]).reshape(12)
    np.savetxt(str(tmp_path / "gt.txt"), gt)
    np.savetxt(str(tmp_path / "gt_sub.txt"), gt[::STEP])
    cm = np.zeros((5, 12)); cm[4] = np.eye(3, 4).reshape(12)
    np.savetxt(str(tmp_path / "calib_.txt"), cm)
    rows = []
    for gtp, est, m, step in ((tmp_path / "gt.txt", tmp_path / ("%d_00.txt" % STEP), tmp_path / ("%d_m.mat" % STEP), STEP),
                              (tmp_path / "gt_sub.txt", d / "sub" / "00.txt", d / "sub" / "m.mat", 1)):
        out = tmp_path / ("row_%d.mat" % step)
        subprocess.run([sys.executable, EVP, "registration", "--gt", str(gtp), "--est", str(est), "--calib", str(tmp_path / "calib_.txt"),
                        "--matchability", str(m), "--frame-step", str(step), "--out", str(out)], check=True, capture_output=True, timeout=300)
        rows.append(io.loadmat(str(out))["EvaluationResults"])
    assert rows[0].shape == (1, 7) and np.array_equal(rows[0], rows[1], equal_nan=True)



def test_run_sequence_frame_steps_on_two_ranks(plain_runs, tmp_path):
    """--gpus 2 (on one GPU: two ranks sharing it, gloo standing in for RCCL): the step-5 pair (10, 15) straddles the rank boundary at frame 12
    and is registered by rank 0 on rank 1's first frames; the files equal the one-rank run's, i.e. the sub-sampled plain run's."""
    from scipy import io
    d = plain_runs
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "CAELO_DIST_BACKEND")}
    if torch.cuda.device_count() < 2:
        env["CAELO_DIST_BACKEND"] = "gloo"
    subprocess.run([sys.executable, RS, "--synthetic", str(N_SEQ), "--trajectory", "line", "--frame-steps", "1,%d" % STEP, "--gpus", "2",
                    "--matchability", str(tmp_path / "m.mat"), "--out", str(tmp_path / "00.txt")], check=True, capture_output=True, timeout=600, env=env)
    rd = lambda p: open(str(p), "rb").read()
    assert rd(tmp_path / "00.txt") == rd(d / "plain" / "00.txt")
    step_lines = rd(tmp_path / ("%d_00.txt" % STEP)).splitlines()
    assert len(step_lines) == N_SEQ and [step_lines[i] for i in range(0, N_SEQ, STEP)] == rd(d / "sub" / "00.txt").splitlines()
    ms, mp = io.loadmat(str(tmp_path / ("%d_m.mat" % STEP))), io.loadmat(str(d / "sub" / "m.mat"))
    for key in ("AllProportions", "AllTrialCounts"):
        assert np.array_equal(ms[key], mp[key])
