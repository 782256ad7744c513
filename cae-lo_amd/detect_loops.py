#!/usr/bin/env python
"""detect_loops.py -- loop closures of a sequence: Scan Context place recognition with a yaw estimate on the GPU, then verification
through the extract and pair stages on the yaw-aligned scan (caelo.loops).

    python detect_loops.py --scans <seq>/velodyne --out loops.txt [--calib-angle 0.22] [--min-gap 50] [--max-dist D] [--top-k 1]
    python detect_loops.py --synthetic 16 --out loops.txt
                           [--features-from DIR] [--no-verify] [--no-derotate]

Every scan gets its Scan Context descriptor (caelo_scan_context); every frame i is searched against all frames j <= i - min-gap over all
60 column shifts (caelo_loop_search); each of its --top-k best candidates below --max-dist is verified: scan i is turned by shift * 6
degrees about z, extracted again and registered against frame j by the pipeline's pair stage (certified).  --no-derotate registers the
scan as it is (the failure the turn cures: the patch descriptor is not rotation invariant); --no-verify stops after the search.
--features-from: frame j's key points and descriptors from <DIR>/<frame:06d>.bin.mat (run_sequence.py --save-artifacts) instead of
extracting it again.

--out: one np.loadtxt-readable row per accepted candidate,
    i j dist shift verified n_inliers threshold R(9) T(3)        with p_j ~ R p_i + T
(without verification: verified = n_inliers = threshold = 0, R = Rz(shift * 6 deg), T = 0).  What a pose-graph optimiser would read.
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


class _Files:
    """the scans of a directory, read when asked for"""

    def __init__(self, files):
        self.files = files

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from caelo import stageio
        return stageio.read_scan(self.files[i])


class _Synthetic:
    def __init__(self, n, scene):
        self.n, self.scene, self.cache = n, scene, {}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from caelo import synth
        if i not in self.cache:
            self.cache[i] = synth.make_scan(i, quantum=1e-3, scene_kind=self.scene, trajectory="circuit")
        return self.cache[i]


def run(argv=None, scans=None):
    """``scans``: a sequence of clouds instead of --scans / --synthetic (tests)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", help="directory of KITTI velodyne .bin files")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic 64x2000 scans of the circuit trajectory (caelo.synth)")
    ap.add_argument("--scene", default="boxes", choices=("boxes", "clutter"), help="synthetic scene (caelo.synth)")
    ap.add_argument("--calib-angle", type=float, default=None, metavar="DEG",
                    help="correct every scan by the reference's CorrectPC first (raw KITTI scans: 0.22)")
    ap.add_argument("--features-from", metavar="DIR", help="directory of <frame:06d>.bin.mat files (KeyPts / Features): frame j's rows come from there")
    ap.add_argument("--min-gap", type=int, default=50, help="a candidate lies at least this many frames back")
    ap.add_argument("--max-dist", type=float, default=None, metavar="D",
                    help="accept only candidates with a Scan Context distance below D.  No default is shipped: nobody has measured real KITTI "
                         "with this descriptor yet.  On the synthetic 16-frame revisit sequence (boxes scene) true revisits lie at 0.21 - 0.33 "
                         "and the nearest impostor at 0.58; on the clutter scene 0.14 - 0.22 against 0.33")
    ap.add_argument("--top-k", type=int, default=1, help="candidates per frame (1..8)")
    ap.add_argument("--min-cols", type=int, default=1, help="a shift counts only if this many columns are non-empty in both images (1..60)")
    ap.add_argument("--no-verify", action="store_true", help="stop after the search")
    ap.add_argument("--no-derotate", action="store_true", help="register scan i as it is, without the turn to frame j's heading")
    ap.add_argument("--no-certify", action="store_true", help="the kernels' own RANSAC results without the host half (run_sequence.py --no-certify)")
    ap.add_argument("--seed-base", type=int, default=1000, help="loop number n draws RandomState(seed-base + n)")
    ap.add_argument("--out", required=True, help="the loops file")
    args = ap.parse_args(argv)
    if scans is None and bool(args.scans) == bool(args.synthetic):
        ap.error("give exactly one of --scans DIR and --synthetic N")
    if args.synthetic < 0:
        ap.error("--synthetic must be >= 1")
    if args.min_gap < 1:
        ap.error("--min-gap must be >= 1")
    if not 1 <= args.top_k <= 8:
        ap.error("--top-k must lie in 1..8")
    if not 1 <= args.min_cols <= 60:
        ap.error("--min-cols must lie in 1..60")
    if args.max_dist is not None and not args.max_dist > 0:
        ap.error("--max-dist must be a positive number")
    if args.calib_angle is not None and not np.isfinite(args.calib_angle):
        ap.error("--calib-angle must be a finite number of degrees")
    if args.no_verify and (args.no_derotate or args.features_from or args.no_certify):
        ap.error("--no-verify stops after the search: --no-derotate, --features-from and --no-certify do not go with it")
    if args.features_from and not os.path.isdir(args.features_from):
        ap.error("--features-from %s is not a directory" % args.features_from)
    if scans is None:
        if args.scans:
            files = sorted(glob.glob(os.path.join(args.scans, "*.bin")))
            if not files:
                ap.error("no .bin files in %s" % args.scans)
            scans = _Files(files)
        else:
            scans = _Synthetic(args.synthetic, args.scene)
    if not 0 <= args.seed_base <= (1 << 32) - len(scans) * args.top_k:
        ap.error("--seed-base %d: the seeds seed_base + n of up to %d loops must lie in [0, 2^32)" % (args.seed_base, len(scans) * args.top_k))
    import caelo
    from caelo import loops
    from caelo.engine import default_engine
    caelo.configure_runtime()
    eng = default_engine()
    try:
        rows = loops.detect(eng, scans, min_gap=args.min_gap, max_dist=args.max_dist, top_k=args.top_k, min_cols=args.min_cols,
                            do_verify=not args.no_verify, derotate=not args.no_derotate, features_from=args.features_from,
                            seed_base=args.seed_base, certify=not args.no_certify, calib_angle=args.calib_angle)
    except (ValueError, FileNotFoundError) as e:
        ap.error(str(e))
    loops.write_loops(args.out, rows)
    print("%d frames: %d candidates, %d verified -> %s" % (len(scans), len(rows), int((rows[:, 4] > 0).sum()), args.out))
    return rows


if __name__ == "__main__":
    run()
    sys.exit(0)
