#!/usr/bin/env python
"""correct_scans.py -- the counterpart of the reference's BatchCorrectPC (BatchPreprocess.py:70-88, option 3) on libcaelo: every KITTI
velodyne .bin file of a directory corrected by CorrectPC (Transformations.py:28-39: each point rotated by the calibration angle about
p x z) and written under the same name to another directory, [N,4] float32, the intensity column kept bit for bit.

    python correct_scans.py --scans <seq>/velodyne --out <corrected seq>/velodyne --calib-angle 0.22

One engine for all files, one kernel launch per file (caelo_correct_pc); nothing loops over points.  ``run_sequence.py --calib-angle``
applies the same correction on the fly and needs no corrected copy; this tool is for the reference's other consumers of such files.
"""
import argparse
import glob
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description="CorrectPC over a directory of KITTI .bin scans (BatchCorrectPC)")
    ap.add_argument("--scans", required=True, help="directory of KITTI velodyne .bin files ([N,4] float32)")
    ap.add_argument("--out", required=True, help="directory the corrected files are written to (created; must differ from --scans)")
    ap.add_argument("--calib-angle", type=float, required=True, metavar="DEG", help="the calibration angle in degrees (raw KITTI scans: 0.22)")
    args = ap.parse_args(argv)
    if not math.isfinite(args.calib_angle):
        ap.error("--calib-angle must be a finite number of degrees")
    files = sorted(glob.glob(os.path.join(args.scans, "*.bin")))
    if not files:
        ap.error("no .bin files in %s" % args.scans)
    if os.path.realpath(args.out) == os.path.realpath(args.scans):
        ap.error("--out must not be the directory of the scans")
    os.makedirs(args.out, exist_ok=True)

    import torch
    import caelo
    caelo.configure_runtime()
    from caelo import stageio
    from caelo.engine import Engine
    eng = Engine(respond_h5=None, encoder_h5=None)
    pending = None   # (path, corrected scan on the device): written while the next file is read and corrected
    for f in files:
        pc = torch.from_numpy(stageio.read_scan(f)).to(eng.device, non_blocking=True)
        out = eng.correct_pc(pc, args.calib_angle) if pc.shape[0] else pc
        if pending is not None:
            pending[1].cpu().numpy().tofile(pending[0])
        pending = (os.path.join(args.out, os.path.basename(f)), out)
    pending[1].cpu().numpy().tofile(pending[0])
    print("%d scans corrected by %g degrees -> %s" % (len(files), args.calib_angle, args.out))


if __name__ == "__main__":
    main()
