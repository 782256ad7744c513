#!/usr/bin/env python
"""evaluate.py -- the reference's evaluation scripts on this engine's outputs (caelo.evaluate).

    python evaluate.py registration --gt poses/00.txt --est poses_/00.txt --calib calib/00/calib_.txt --matchability m00.mat \\
                                    [--gt ... --est ... --calib ... --matchability ...] [--frame-step s] [--out EvaluationResults.mat]
    python evaluate.py keypoints --keypts-dir 00/Features --source ae --gt poses/00.txt --calib calib/00/calib_.txt \\
                                 [--frame-step s] [--inner] --out AccuracyOfKeyPts_1_0_00.mat
    python evaluate.py reconstruction --autoencoder-h5 AutoencoderModel4VoxelPatch.h5 (--scans <seq>/velodyne | --synthetic N) \\
                                      [--threshold 0.1] [--every k] --out recon.mat
    python evaluate.py loops --gt poses/00.txt --calib calib/00/calib_.txt --loops loops.txt [--revisit-radius 4] [--min-gap 50]

registration (EvaluationOnRegistration.py / EvalOnReg_KeyPts.py): one --gt / --est / --calib / --matchability per sequence, the
sequences concatenated; prints RRE, stdRRE, RTE, stdRTE, success rate (RRE < 1 deg and RTE < 0.5 m), inlier ratio (both
fractions) and average RANSAC trials; --out writes them as the 1 x 7 float32 EvaluationResults.
keypoints (EvaluationOnKeypts.py): key point repeatability of one sequence; the nearest-neighbour search runs on the GPU
(caelo_kp_nn_pairs); prints the counts and writes the reference's {'counts': ...} file.  --inner is the reference's mode 1.
reconstruction (AE4VoxelPatch.py:213,228,242-284): how well an autoencoder file rebuilds the patches of scans -- per frame and scale
the mean binary_crossentropy and the IoU of the voxels with value > threshold (Voxel.VoxelModel2PC's test), and the mean loss over all
patches (Keras's validation-loss figure); the decoder runs on the GPU (caelo_decode).
loops: detect_loops.py's loops file against ground truth -- a frame j <= i - min_gap within the revisit radius of frame i (LiDAR
positions, all pairs on the host) is a revisit; prints the recall over the frames that have one, the precision of the detected and of
the verified loops, and the verified loops' RRE / RTE against the ground-truth motion (success: RRE < 1 deg and RTE < 0.5 m).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from caelo import evaluate as ev  # noqa: E402


def reconstruction_main(ap, a):
    import glob
    if not 0.0 < a.threshold < 1.0:
        ap.error("--threshold must lie in (0, 1)")
    if a.every < 1 or (a.synthetic is not None and a.synthetic < 1):
        ap.error("--every and --synthetic must be >= 1")
    import caelo
    from caelo import synth
    from caelo.engine import Engine
    caelo.configure_runtime()
    eng = Engine()
    eng.load_autoencoder(a.autoencoder_h5, encoder_h5=a.encoder_h5)
    if a.scans:
        files = sorted(glob.glob(os.path.join(a.scans, "*.bin")))[::a.every]
        if not files:
            ap.error("no .bin files in %s" % a.scans)
        scans = (np.fromfile(f, dtype=np.float32).reshape(-1, 4) for f in files)
    else:
        scans = (synth.make_scan(f, quantum=1e-3) for f in range(0, a.synthetic, a.every))
    res = ev.reconstruction(eng, scans, a.threshold)
    ev.save_reconstruction(a.out, res)
    print("reconstruction: %d frames, %d patches, mean loss %.6g, mean IoU per scale %s at threshold %g -> %s" % (
        len(res["n_key"]), res["patch_loss"].size, res["mean_loss"], np.round(np.nanmean(res["iou"], axis=0), 4).tolist(), a.threshold, a.out))
    return 0


def loops_main(ap, a):
    from caelo import loops as lp
    if not a.revisit_radius > 0:
        ap.error("--revisit-radius must be a positive number of metres")
    if a.min_gap < 1:
        ap.error("--min-gap must be >= 1")
    try:
        res = ev.loops(np.loadtxt(a.gt), ev.read_tr(a.calib), lp.read_loops(a.loops), a.revisit_radius, a.min_gap)
    except ValueError as e:
        ap.error(str(e))
    print("loops: %d detected, %d verified; %d frames have a revisit within %g m (min gap %d): recall %.6g  precision %.6g  "
          "precision of verified %.6g" % (res["n_loops"], res["n_verified"], res["n_revisit_queries"], a.revisit_radius, a.min_gap,
                                          res["recall"], res["precision"], res["precision_verified"]))
    if res["n_verified"]:
        print("verified loops: RRE mean %.6g max %.6g deg  RTE mean %.6g max %.6g m (sums of absolute components)  success %d of %d" % (
            res["RRE"].mean(), res["RRE"].max(), res["RTE"].mean(), res["RTE"].max(), int(res["success"].sum()), res["n_verified"]))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("registration", help="per-pair rotation / translation errors -> the 7-column row")
    r.add_argument("--gt", action="append", required=True, help="ground truth poses [n, 12] (once per sequence)")
    r.add_argument("--est", action="append", required=True, help="estimated poses [n, 12], e.g. run_sequence.py's output")
    r.add_argument("--calib", action="append", required=True, help="calib_.txt (row 4 = Tr) or KITTI calib.txt")
    r.add_argument("--matchability", action="append", required=True, help="AllProportions / AllTrialCounts .mat (run_sequence.py --matchability)")
    r.add_argument("--frame-step", type=int, default=1, help="slice both pose files [0:n:step] (EvalOnReg_KeyPts.py:96-99)")
    r.add_argument("--out", help="write EvaluationResults [1, 7] f32 here")
    k = sub.add_parser("keypoints", help="key point repeatability (histogram of nearest-neighbour distances)")
    k.add_argument("--keypts-dir", required=True, help="<frame:06d>.bin.mat (ae: KeyPts/ or Features/) or <frame:06d>.bin files")
    k.add_argument("--source", required=True, choices=ev.SOURCES)
    k.add_argument("--gt", required=True, help="ground truth poses [n, 12], one per key point file")
    k.add_argument("--calib", required=True, help="calib_.txt (row 4 = Tr) or KITTI calib.txt")
    k.add_argument("--frame-step", type=int, default=1)
    k.add_argument("--inner", action="store_true", help="mode 1 (ComputeDispersionOfKeypoints): each frame against itself")
    k.add_argument("--out", required=True, help="the counts file (the reference names it AccuracyOfKeyPts_<step>_<source>_<seq>.mat)")
    c = sub.add_parser("reconstruction", help="an autoencoder's reconstruction loss and IoU on the patches of scans")
    c.add_argument("--autoencoder-h5", required=True, help="the autoencoder file (encoder and decoder)")
    c.add_argument("--encoder-h5", help="the encoder's weights, when --autoencoder-h5 was cut down to the decoder's")
    src = c.add_mutually_exclusive_group(required=True)
    src.add_argument("--scans", help="directory of KITTI velodyne .bin files")
    src.add_argument("--synthetic", type=int, help="number of synthetic 64x2000 scans (caelo.synth)")
    c.add_argument("--threshold", type=float, default=0.1, help="a rebuilt voxel is set when its value exceeds this (0 < t < 1)")
    c.add_argument("--every", type=int, default=1, help="evaluate every k-th scan")
    c.add_argument("--out", required=True, help="the result file (.mat): n_key, loss, iou, patch_loss, mean_loss, threshold")
    lo = sub.add_parser("loops", help="detected loop closures against ground truth: recall, precision, RRE / RTE of the verified ones")
    lo.add_argument("--gt", required=True, help="ground truth poses [n, 12]")
    lo.add_argument("--calib", required=True, help="calib_.txt (row 4 = Tr) or KITTI calib.txt")
    lo.add_argument("--loops", required=True, help="detect_loops.py's output: i j dist shift verified n_inliers threshold R(9) T(3)")
    lo.add_argument("--revisit-radius", type=float, default=4.0, help="frames closer than this (m) are the same place")
    lo.add_argument("--min-gap", type=int, default=50, help="a revisit lies at least this many frames back")
    a = ap.parse_args(argv)
    if a.cmd == "reconstruction":
        return reconstruction_main(ap, a)
    if a.cmd == "loops":
        return loops_main(ap, a)
    if a.frame_step < 1:
        ap.error("--frame-step must be >= 1")

    if a.cmd == "registration":
        row, ok = ev.registration(a.gt, a.est, a.calib, a.matchability, a.frame_step)
        print("RRE %.6g  stdRRE %.6g  RTE %.6g  stdRTE %.6g  success %.6g (%d of %d)  inlier ratio %.6g  trials %.6g" % (
            row[0], row[1], row[2], row[3], row[4], int(np.sum(ok)), ok.shape[0], row[5], row[6]))
        if a.out:
            ev.save_registration(a.out, row)
        return 0

    t0 = time.time()
    poses = np.loadtxt(a.gt)
    Tr = ev.read_tr(a.calib)
    pts = ev.GetAllKeyPts(a.keypts_dir, a.source, poses, Tr, a.frame_step)
    t1 = time.time()
    _, counts = ev.device_distances(pts, a.inner)
    t2 = time.time()
    counts = [np.int64(c) for c in counts]
    ev.save_repeatability(a.out, counts)
    print("counts %s over %d frames (%s) -> %s" % ([int(c) for c in counts], len(pts), "mode 1" if a.inner else "mode 0", a.out))
    print("seconds: reading + world transform %.3f, device pass (incl. engine start) %.3f" % (t1 - t0, t2 - t1), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
