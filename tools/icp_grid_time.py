#!/usr/bin/env python
"""Time Engine.icp under nn="brute" and nn="grid" (DESIGN.md 9l): a whole call, host clock around the launch and the synchronising
read of the result record, warm, median of nine with the range in brackets, the two searches alternating in one process.  Every
pair of runs is also compared byte for byte (result record and moved cloud).

    python tools/icp_grid_time.py [--frames 40] [--seq-repeats 3] [--out profiles/icp_grid_times.txt]

Clouds: the 1 300-point test clouds (tests/icp_clouds.py `points`, MyICP.ICP's defaults); the extended key point sets of synthetic
frames 0 and 1 and of frames 0 and 10 (circuit trajectory), frame 1 brought over by the ground-truth motion as RefinementCore does
with the odometry's; the whole scans of frames 0 and 1, about the 173 056 points an extended set can reach.  Then
refine_sequence.py --dejump --mode keyframes --second-pass over a run_sequence.py --synthetic FRAMES --save-artifacts, whole runs in
this process (key points made again every run), median of --seq-repeats."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

ICP_KW = dict(threshold0=0.5, decay0=0.9, small_shift=0.05, ep=0.001, max_iter=50, min_iter=19, min_pairs=100, fail_only_first=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--seq-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import icp_clouds
    import refine_sequence
    from caelo import synth
    from caelo.engine import default_engine
    eng = default_engine()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def one(pc0, pc1, nn):
        d1 = pc1.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = eng.icp_result(eng.icp(pc0, d1, nn=nn, **ICP_KW))
        dt = time.perf_counter() - t
        return dt, r, bytes(r) + d1.cpu().numpy().tobytes()

    def compare(label, a0, a1):
        pc0, pc1 = torch.from_numpy(a0).to(eng.device), torch.from_numpy(a1).to(eng.device)
        for nn in ("brute", "grid", "brute", "grid"):   # warm: code objects, workspaces
            one(pc0, pc1, nn)
        times = {"brute": [], "grid": []}
        for _ in range(9):
            out = {}
            for nn in ("brute", "grid"):
                dt, r, out[nn] = one(pc0, pc1, nn)
                times[nn].append(dt)
            assert out["brute"] == out["grid"], label
        fmt = lambda v: "%9.3f ms [%9.3f .. %9.3f]" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))   # noqa: E731
        say("%-28s n0 %6d n1 %6d iterations %2d pairs %6d  brute %s  grid %s  brute/grid %.2f" % (
            label, a0.shape[0], a1.shape[0], r.iterations, r.n_inliers_pts, fmt(times["brute"]), fmt(times["grid"]),
            statistics.median(times["brute"]) / statistics.median(times["grid"])))

    say("# Engine.icp, whole call, median of 9 [min .. max], %s" % torch.cuda.get_device_name(0))
    compare("test clouds (points)", *icp_clouds.clouds("points"))
    kp = refine_sequence.KeyPts(eng, 11, synthetic=dict(scene_kind="boxes", trajectory="circuit"))
    ext0 = kp(0)[0]
    for f in (1, 10):
        R, T = synth.relative_pose_gt(0, f, trajectory="circuit")
        moved = np.array((R @ kp(f)[0].T.astype(np.float64) + np.asarray(T, np.float64).reshape(3, 1)).T, dtype=np.float32)
        compare("extended sets, frames 0 / %d" % f, ext0, np.ascontiguousarray(moved))
    # the size an extended set can reach (1 024 key points x 169 pixels = 173 056): whole scans of about that many points
    scan0, scan1 = (np.ascontiguousarray(synth.make_scan(f, trajectory="circuit")[:, 0:3], dtype=np.float32) for f in (0, 1))
    R, T = synth.relative_pose_gt(0, 1, trajectory="circuit")
    compare("whole scans, frames 0 / 1", scan0, np.ascontiguousarray(np.array((R @ scan1.T.astype(np.float64) + np.asarray(T, np.float64).reshape(3, 1)).T, dtype=np.float32)))

    tmp = tempfile.mkdtemp(prefix="icp_grid_time_")
    poses = os.path.join(tmp, "poses_", "00.txt")
    subprocess.run([sys.executable, os.path.join(REPO, "cae-lo_amd", "run_sequence.py"), "--synthetic", str(args.frames), "--save-artifacts", "--out", poses],
                   check=True, capture_output=True)
    seq_times = {"brute": [], "grid": []}
    outs = {}
    for rep in range(args.seq_repeats + 1):   # (the first round warms)
        for nn in ("brute", "grid"):
            t = time.perf_counter()
            r = refine_sequence.run(["--poses", poses, "--inliers-dir", os.path.join(tmp, "poses_", "synthetic", "InliersIdx"), "--synthetic", "--dejump",
                                     "--mode", "keyframes", "--second-pass", "--nn", nn, "--out", os.path.join(tmp, nn, "00.txt"),
                                     "--debug-info", os.path.join(tmp, nn, "DebugInfo.mat")])
            if rep:
                seq_times[nn].append(time.perf_counter() - t)
            outs[nn] = (open(os.path.join(tmp, nn, "00.txt"), "rb").read(), r["tried"], r["second"])
        assert outs["brute"] == outs["grid"]
    say("# refine_sequence.py --dejump --mode keyframes --second-pass, %d synthetic frames, whole run, median of %d [min .. max]" % (args.frames, args.seq_repeats))
    say("registrations %d + %d (second pass), spans %s" % (len(outs["grid"][1]), len(outs["grid"][2]), [b - a for a, b, _ in outs["grid"][1]]))
    for nn in ("brute", "grid"):
        v = seq_times[nn]
        say("%-6s %8.3f s [%8.3f .. %8.3f]" % (nn, statistics.median(v), min(v), max(v)))
    say("brute/grid %.2f" % (statistics.median(seq_times["brute"]) / statistics.median(seq_times["grid"])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
