#!/usr/bin/env python
"""Time caelo_planar_points and compare the two registrations of refine_sequence.py.

    python tools/planar_time.py [--frames 40] [--seq-repeats 3] [--out profiles/planar_times.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/planar_time.py --calls-only     # the two kernels' own times

Engine.planar_points, the whole call (host clock around the call and a stream synchronisation; the two output arrays are allocated
and zeroed inside it), warm, median of nine with the range in brackets, on frame 0 of the synthetic boxes scene (mm-quantised) and on
the capacity image of tests/planar_images.py (every interior pixel a planar point).

Then refine_sequence.py --dejump --mode keyframes --second-pass over a run_sequence.py --synthetic FRAMES --save-artifacts --matchability
run, under --icp pt2pt and under --icp pt2plane --planar-pts ring: whole runs in this process (key points made again every run), median
of --seq-repeats, and RRE / RTE of the poses they write against caelo.synth's ground truth through caelo.evaluate.registration (what
evaluate.py registration prints)."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--seq-repeats", type=int, default=3)
    ap.add_argument("--calls-only", action="store_true", help="stop after the timed calls (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import planar_images as pi
    import refine_sequence
    from caelo import evaluate, stageio, synth
    from caelo.engine import default_engine
    eng = default_engine()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(label, ring, cnt, resp):
        for _ in range(3):   # warm: code objects, the workspace
            eng.planar_points(ring, cnt, resp)
        times = []
        for _ in range(9):
            torch.cuda.synchronize()
            t = time.perf_counter()
            planar, pixels, n = eng.planar_points(ring, cnt, resp)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        say("%-34s planar points %6d  %8.1f us [%8.1f .. %8.1f]" % (label, int(n.item()), 1e6 * statistics.median(times), 1e6 * min(times), 1e6 * max(times)))

    say("# Engine.planar_points, whole call, median of 9 [min .. max], %s" % torch.cuda.get_device_name(0))
    pc = torch.from_numpy(synth.make_scan(0, quantum=1e-3)).to(eng.device)
    ring, cnt, _ = eng.project(pc)
    timed("boxes frame 0 (mm-quantised)", ring, cnt, eng.respond(ring))
    im = pi.capacity()
    timed("capacity image", *(torch.from_numpy(a).to(eng.device) for a in (im.ring, im.counter, im.resp)))
    if args.calls_only:
        return 0

    tmp = tempfile.mkdtemp(prefix="planar_time_")
    poses = os.path.join(tmp, "poses_", "00.txt")
    match = os.path.join(tmp, "matchability.mat")
    subprocess.run([sys.executable, os.path.join(REPO, "cae-lo_amd", "run_sequence.py"), "--synthetic", str(args.frames), "--save-artifacts", "--matchability", match,
                    "--out", poses], check=True, capture_output=True)
    rel = [np.r_[np.asarray(R, np.float64).ravel(), np.asarray(T, np.float64).ravel()] for R, T in (synth.relative_pose_gt(f, f + 1) for f in range(args.frames - 1))]
    gt = os.path.join(tmp, "gt.txt")
    stageio.write_poses(gt, stageio.chain_poses(np.array(rel)))
    calib = os.path.join(tmp, "calib_.txt")
    rows = np.zeros((5, 12))
    rows[4] = np.eye(3, 4).ravel()
    np.savetxt(calib, rows)
    modes = {"pt2pt": ["--icp", "pt2pt"], "pt2plane": ["--icp", "pt2plane", "--planar-pts", "ring"]}
    seq_times, outs = {m: [] for m in modes}, {}
    for rep in range(args.seq_repeats + 1):   # (the first round warms)
        for m, extra in modes.items():
            t = time.perf_counter()
            r = refine_sequence.run(["--poses", poses, "--inliers-dir", os.path.join(tmp, "poses_", "synthetic", "InliersIdx"), "--synthetic", "--dejump",
                                     "--mode", "keyframes", "--second-pass", "--out", os.path.join(tmp, m, "00.txt")] + extra)
            if rep:
                seq_times[m].append(time.perf_counter() - t)
            outs[m] = r
    say("# refine_sequence.py --dejump --mode keyframes --second-pass, %d synthetic frames, whole run, median of %d [min .. max];" % (args.frames, args.seq_repeats))
    say("# RRE (deg) / RTE (m) against synth.relative_pose_gt through caelo.evaluate.registration (mean, std)")
    row, _ = evaluate.registration([gt], [poses], [calib], [match])
    say("%-34s %28s RRE %.5f (%.5f)  RTE %.5f (%.5f)" % ("odometry (run_sequence.py)", "", row[0], row[1], row[2], row[3]))
    for m in modes:
        row, _ = evaluate.registration([gt], [os.path.join(tmp, m, "00.txt")], [calib], [match])
        v, r = seq_times[m], outs[m]
        say("%-34s %7.3f s [%7.3f .. %7.3f]  RRE %.5f (%.5f)  RTE %.5f (%.5f)  registrations %d + %d, failed %d"
            % ("--icp " + " ".join(modes[m][1:]), statistics.median(v), min(v), max(v), row[0], row[1], row[2], row[3], len(r["tried"]), len(r["second"]),
               len(r["failed"])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
