#!/usr/bin/env python
"""detect_keypoints.py -- key points of a hand-crafted detector for every scan of a directory, the rows 'iss', 'harris' and 'sift' of
the reference's key point comparison (PclKeyPts.py:63 lists cae-lo, 3dfeat-net, usip, iss, harris, sift; EvalOnReg_KeyPts.py:23).  The
reference gets them from PCLKeypoint.keypointIss / keypointHarris / keypointSift, a PCL binding it does not ship; here the detectors
run on the GPU (caelo_iss_keypoints; caelo_harris_keypoints; caelo_sift_octave).

    python detect_keypoints.py --method iss --scans <seq>/velodyne --out iss_keypts/00
    python detect_keypoints.py --method harris --scans <seq>/velodyne --out harris_keypts/00
    python detect_sift_keypoints.py --scans <seq>/velodyne --out sift_keypts/00
    python run_sequence.py --scans <seq>/velodyne --python-loader --keypts-source 3dfeatnet --keypts-dir iss_keypts/00 --out poses_/00.txt
    python evaluate.py keypoints --keypts-dir iss_keypts/00 --source 3dfeatnet --gt poses/00.txt --calib calib_.txt --out acc.mat

Per scan, as PclKeyPts.py:77-103 does it: the points are thinned to one per --leaf cell (the first in scan order), at most --max-points
of them are kept (RandomState(--seed + frame).choice without replacement, like :81), the detector runs with the reference's parameters
(:42-46 for iss, :50-51 for harris, :55-58 for sift, whose key points are centroids of its own voxel pyramid, not scan points), and the result is brought to exactly --keypoints points (ensure_keypoint_number, :20-28; the same RandomState goes on) unless
--no-ensure.  --batch frames share one launch of every kernel.  Written as <frame:06d>.bin in LiDAR axes, float32, unrotated:
--layout 3dfeatnet (default) [K,35] with zero descriptors, which run_sequence.py --keypts-source 3dfeatnet and evaluate.py keypoints
--source 3dfeatnet read as they are; --layout xyz plain [K,3].

This script's own command line is what it was before SIFT3D was built: --method takes iss and harris, and sift stays an invalid
choice here.  The sift row is detect_sift_keypoints.py beside it: the same main() with sift among the methods (and as the default)
and sift's four options, everything else shared.
"""
import argparse
import glob
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def frame_number(path, ordinal):
    """The frame a scan file stands for: its name when that is a number (KITTI's 000123.bin), else its place in the sorted directory."""
    stem = os.path.splitext(os.path.basename(path))[0]
    return int(stem) if stem.isdigit() else ordinal


def prepare(eng, scan, frame, leaf, max_points, seed, calib_angle=None):
    """One scan [N,4] f32 (NumPy) -> (the cloud the detector sees [n,3] f32 on the device, the frame's RandomState after the subsample)."""
    import numpy as np
    import torch
    from caelo import iss
    pc = torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float32)).to(eng.device)
    if calib_angle is not None and pc.shape[0]:
        pc = eng.correct_pc(pc, calib_angle)
    pc = iss.voxel_downsample(pc[:, 0:3], leaf)
    rng = np.random.RandomState(seed + frame)
    keep = iss.subsample(pc.shape[0], max_points, rng)
    if keep.shape[0] != pc.shape[0]:
        pc = pc[torch.from_numpy(keep).to(eng.device)]
    return pc.contiguous(), rng


def main(argv=None, with_sift=False):
    """with_sift: detect_sift_keypoints.py's command line -- sift is a method, the default one, and its four options exist."""
    ap = argparse.ArgumentParser(description="hand-crafted key points over a directory of KITTI .bin scans (PclKeyPts.py)")
    if with_sift:
        ap.add_argument("--method", default="sift", choices=["iss", "harris", "sift"], help="the detector (default sift)")
    else:
        ap.add_argument("--method", required=True, choices=["iss", "harris"], help="the detector (sift of the reference's list: detect_sift_keypoints.py)")
    ap.add_argument("--scans", required=True, help="directory of KITTI velodyne .bin files ([N,4] float32)")
    ap.add_argument("--out", required=True, help="directory the key point files are written to (created)")
    ap.add_argument("--leaf", type=float, default=0.2, help="cell size in metres of the thinning before the detector (default 0.2)")
    ap.add_argument("--max-points", type=int, default=16384, help="points the detector sees at most (default 16384, the reference's input_pc_num)")
    ap.add_argument("--keypoints", type=int, default=1024, help="key points per frame after ensure_keypoint_number (default 1024)")
    ap.add_argument("--no-ensure", action="store_true", help="write what the detector found, however many")
    ap.add_argument("--seed", type=int, default=0, help="frame f draws from RandomState(seed + f)")
    ap.add_argument("--calib-angle", type=float, default=None, metavar="DEG", help="correct raw KITTI scans first (CorrectPC; 0.22)")
    ap.add_argument("--layout", choices=["3dfeatnet", "xyz"], default="3dfeatnet")
    ap.add_argument("--batch", type=int, default=8, help="frames per launch (default 8)")
    ap.add_argument("--salient-radius", type=float, default=None, help="iss (default 2.0)")
    ap.add_argument("--non-max-radius", type=float, default=None, help="iss (default 2.0)")
    ap.add_argument("--gamma-21", type=float, default=None, help="iss (default 0.975)")
    ap.add_argument("--gamma-32", type=float, default=None, help="iss (default 0.975)")
    ap.add_argument("--min-neighbors", type=int, default=None, help="iss (default 5)")
    ap.add_argument("--radius", type=float, default=None, help="harris: the radius of normals, response and suppression (default 1.0)")
    ap.add_argument("--threshold", type=float, default=None, help="harris: the least response of a key point (default 0.001)")
    if with_sift:
        ap.add_argument("--min-scale", type=float, default=None, help="sift: the scale of the first octave in metres (default 0.5)")
        ap.add_argument("--n-octaves", type=int, default=None, help="sift: octaves, each at twice the scale of the one before (default 4)")
        ap.add_argument("--n-scales-per-octave", type=int, default=None, help="sift (default 8)")
        ap.add_argument("--min-contrast", type=float, default=None, help="sift: the least |difference of Gaussians| of a key point (default 0.1)")
    args = ap.parse_args(argv)

    from caelo import harris, iss, keysources, sift
    # per method: the module whose DEFAULTS name its options and whose check_params checks them, and its printed name
    methods = {"iss": (iss, "ISS"), "harris": (harris, "Harris3D")}
    if with_sift:
        methods["sift"] = (sift, "SIFT3D")
    for method, (mod, _) in methods.items():
        given = [n for n in mod.DEFAULTS if getattr(args, n) is not None]
        if method != args.method and given:
            ap.error("%s belong%s to --method %s, not to --method %s"
                     % (", ".join("--" + n.replace("_", "-") for n in given), "s" if len(given) == 1 else "", method, args.method))
    mod, shown = methods[args.method]
    try:
        prm = mod.check_params(**{n: getattr(args, n) for n in mod.DEFAULTS if getattr(args, n) is not None})
    except ValueError as e:
        ap.error(str(e))
    if not (math.isfinite(args.leaf) and args.leaf > 0):
        ap.error("--leaf must be finite and positive")
    if not 1 <= args.max_points <= iss.MAX_POINTS:
        ap.error("--max-points must lie in [1, %d]" % iss.MAX_POINTS)
    if args.keypoints < 1 or args.batch < 1 or args.seed < 0:
        ap.error("--keypoints and --batch must be at least 1, --seed at least 0")
    if args.calib_angle is not None and not math.isfinite(args.calib_angle):
        ap.error("--calib-angle must be a finite number of degrees")
    files = sorted(glob.glob(os.path.join(args.scans, "*.bin")))
    if not files:
        ap.error("no .bin files in %s" % args.scans)
    if os.path.realpath(args.out) == os.path.realpath(args.scans):
        ap.error("--out must not be the directory of the scans")
    os.makedirs(args.out, exist_ok=True)

    import numpy as np
    import torch
    import caelo
    caelo.configure_runtime()
    from caelo import stageio
    from caelo.engine import Engine
    eng = Engine(respond_h5=None, encoder_h5=None)
    found = []
    for b0 in range(0, len(files), args.batch):
        group = [(frame_number(f, b0 + k), f) for k, f in enumerate(files[b0:b0 + args.batch])]
        clouds = [prepare(eng, stageio.read_scan(f), fr, args.leaf, args.max_points, args.seed, args.calib_angle) for fr, f in group]
        ld = max(1, max(pc.shape[0] for pc, _ in clouds))
        pts = torch.zeros((len(group), ld, 3), dtype=torch.float32, device=eng.device)
        for k, (pc, _) in enumerate(clouds):
            pts[k, :pc.shape[0]] = pc
        r = getattr(eng, args.method + "_keypoints")(pts, n_pts=[pc.shape[0] for pc, _ in clouds], **prm)
        n_key = r.n_key.cpu().numpy()
        found_rows = (r.xyz if args.method == "sift" else r.key_idx).cpu().numpy()   # sift: the key points themselves; else row indices
        for k, ((fr, _), (pc, rng)) in enumerate(zip(group, clouds)):
            cloud = pc.cpu().numpy()
            kp = found_rows[k, :n_key[k]] if args.method == "sift" else cloud[found_rows[k, :n_key[k]]]
            found.append(int(n_key[k]))
            if not args.no_ensure:
                kp = iss.ensure_keypoint_number(kp, cloud, args.keypoints, rng)
            path = keysources.keypts_path(args.out, fr)
            if args.layout == "3dfeatnet":
                keysources.write_3dfeatnet(path, kp)
            else:
                np.ascontiguousarray(kp, dtype=np.float32).tofile(path)
    print("%d scans: %s found %d .. %d key points per frame (mean %.1f)%s -> %s (%s layout)"
          % (len(files), shown, min(found), max(found), sum(found) / len(found),
             "" if args.no_ensure else ", brought to %d each" % args.keypoints, args.out, args.layout))


if __name__ == "__main__":
    main()
