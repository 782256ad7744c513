#!/usr/bin/env python
"""refine_sequence.py -- the counterpart of the reference's RefinePoses.py on libcaelo: a pose file
of run_sequence.py (poses_/NN.txt) and the InliersIdx files of its --save-artifacts -> de-jumped, refined and second-pass poses.

    python run_sequence.py --scans <seq>/velodyne --calib calib_.txt --out poses_/00.txt --save-artifacts
    python refine_sequence.py --poses poses_/00.txt --calib calib_.txt --inliers-dir <seq>/InliersIdx --scans <seq>/velodyne \\
        --dejump --second-pass --out poses___/00.txt --debug-info <seq>/RefinenmentData/DebugInfo.mat
    python refine_sequence.py --poses poses_/00.txt --inliers-dir poses_/synthetic/InliersIdx --synthetic --out poses___/00.txt

Steps (RefinePoses.py:565-592): FixJumpPoses (--dejump), RefineOdometry (--mode keyframes: key frames by inlier transfer, iOption 1;
consecutive: iOption 0), CloseLoopPipeline (--second-pass).  The host logic is caelo.refine; every registration is one device ICP
loop (caelo_icp / caelo_icp_grid).  The extended key points of a frame come from --keypts-dir files (LoadExtendedKeyPts, :49-55) or
are made on the device on first use from the frame's scan (project, response layer, key points, ExtendKeyPtsInShpericalRing) and
kept in a bounded cache.

--icp pt2pt (default): the reference's own alternative at RefinePoses.py:295, ``ICP(KeyPts0, KeyPts1_)`` with MyICP.ICP's defaults.
--icp pt2plane: the call at :291-294.  GetKeyPtsByAE returns an empty PlanarPts (SphericalRing.py:219,285), on which that call fails
in scikit-learn (MyICP.py:94), so it is accepted only with planar points for every frame: from --keypts-dir files whose PlanarPts are
non-empty, or, with --scans / --synthetic, from --planar-pts ring.
--planar-pts ring: a frame's planar points are made on the device beside its extended key points, from the same ring, counter and
response, by the producer the reference wrote down in GetKeyPtsByAE's commented loop (SphericalRing.py:236-282; caelo_planar_points,
DESIGN.md 9m).  --save-keypts writes them as PlanarPts.  A frame without a planar point is refused with its number.
One GPU."""
import argparse
import collections
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from caelo import evaluate, refine, stageio, synth  # noqa: E402

CACHE_FRAMES = 48   # extended key point sets kept: at most 1024 x 169 points = 2 MB each on the host and on the device


class KeyPts:
    """frame -> (ExtendedKeyPts [n,3] f32, PlanarPts [m,6] f32) on the host, with the device copy of the extended set kept beside it."""

    def __init__(self, eng, n_frames, keypts_dir=None, files=None, synthetic=None, calib_angle=None, save_dir=None, planar_ring=False):
        self.eng, self.n, self.dir, self.files, self.synthetic, self.angle, self.save_dir = eng, n_frames, keypts_dir, files, synthetic, calib_angle, save_dir
        self.planar_ring = planar_ring   # --planar-pts ring
        self.cache = collections.OrderedDict()   # frame -> (host ext, host planar, device ext)

    def path(self, frame):
        return os.path.join(self.dir, "%06d.bin.mat" % frame)

    def planar_counts(self):
        from scipy import io
        return [io.loadmat(self.path(f))["PlanarPts"].shape[0] if os.path.exists(self.path(f)) else -1 for f in range(self.n)]

    def _make(self, frame):
        import torch
        eng = self.eng
        if self.dir:
            from scipy import io
            m = io.loadmat(self.path(frame))
            ext = np.ascontiguousarray(m["ExtendedKeyPts"], dtype=np.float32).reshape(-1, 3)
            planar = np.ascontiguousarray(m["PlanarPts"], dtype=np.float32)
            planar = planar.reshape(-1, 6) if planar.size else np.zeros((0, 6), np.float32)
            return ext, planar, torch.from_numpy(ext).to(eng.device)
        scan = synth.make_scan(frame, **self.synthetic) if self.synthetic is not None else stageio.read_scan(self.files[frame])
        pc = torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float32)).to(eng.device)
        if self.angle is not None:
            pc = eng.correct_pc(pc, self.angle)
        ring, cnt, st = eng.project(pc)
        resp = eng.respond(ring)
        kpts, kpix, nkey, st = eng.keypoints(ring, cnt, resp, status=st)
        planar = np.zeros((0, 6), np.float32)
        if self.planar_ring:   # (before extend_keypts zeroes the key points' windows in cnt)
            pl, _, n_pl = eng.planar_points(ring, cnt, resp)
            planar = pl[:int(n_pl.item())].cpu().numpy()
            if planar.shape[0] == 0:
                raise SystemExit("frame %d has no planar points" % frame)
        k = int(nkey.item())
        from caelo.engine import raise_status
        raise_status(int(st.item()))
        if k == 0:
            raise SystemExit("frame %d has no key points" % frame)
        ext, n_ext = eng.extend_keypts(ring, cnt, kpix[:k].contiguous())
        dev = ext[:int(n_ext.item())].contiguous()
        host = dev.cpu().numpy()
        if self.save_dir:
            where = os.path.abspath(self.save_dir)   # (save_keypts names <seq>/<folder>/<scan name>.mat from the scan's path)
            raw = os.path.join(os.path.dirname(where), "velodyne", os.path.basename(self.files[frame]) if self.files else "%06d.bin" % frame)
            stageio.save_keypts(raw, kpts[:k].cpu().numpy(), ExtendedKeyPts=host, PlanarPts=planar if self.planar_ring else None,
                                folder=os.path.basename(where))
        return host, planar, dev

    def _entry(self, frame):
        frame = int(frame)
        if frame in self.cache:
            self.cache.move_to_end(frame)
        else:
            self.cache[frame] = self._make(frame)
            while len(self.cache) > CACHE_FRAMES:
                self.cache.popitem(last=False)
        return self.cache[frame]

    def __call__(self, frame):
        return self._entry(frame)[0:2]

    def device(self, frame):
        """The frame's extended key points on the device."""
        return self._entry(frame)[2]


def device_icp(eng, keypts, nn, planar):
    """-> ``(iFrame0, iFrame1) ->`` the registration as RefinementCore calls it, on the device, with frame iFrame0's resident copy as
    frame 0.  planar = False: RefinePoses.py:295 literally, MyICP.ICP's defaults (the planar sets and the keyword arguments of :291-294
    are ignored); True: ICP_Pt2PtAndPt2Plane with those arguments."""
    import torch

    def result(res):
        r = eng.icp_result(res)
        return np.array(r.R_star, np.float64).reshape(3, 3), np.array(r.T_star, np.float64).reshape(3, 1), bool(r.success)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device)

    def for_pair(iFrame0, iFrame1):
        dev0 = keypts.device(iFrame0)

        def pt2pt(KeyPts0, KeyPts1_, PlanarPts0, PlanarPts1_, **ignored):
            return result(eng.icp(dev0, up(KeyPts1_), nn=nn, threshold0=0.5, decay0=0.9, small_shift=0.05, ep=0.001, max_iter=50,
                                  min_iter=20 - 1, min_pairs=100, fail_only_first=0))                       # MyICP.py:28

        def pt2plane(KeyPts0, KeyPts1_, PlanarPts0, PlanarPts1_, maxIterTimes, minIterTimes, inlierThreshold0, decay_rate0, inlierThreshold1,
                     decay_rate1, smallShiftThreshold, ep, rng=None):
            PN1 = np.asarray(PlanarPts1_)
            if PN1.shape[0] > 2000:                                                                         # MyICP.py:135-140
                rs = np.random.mtrand._rand if rng is None else rng
                PN1 = PN1[np.array(rs.random_sample((2000,)) * PN1.shape[0], dtype=np.int32), :]
            return result(eng.icp(dev0, up(KeyPts1_), up(np.asarray(PlanarPts0)[:, 0:6]), up(PN1[:, 0:6]), nn=nn,
                                  threshold0=inlierThreshold0, threshold1=inlierThreshold1, decay0=decay_rate0, decay1=decay_rate1,
                                  small_shift=smallShiftThreshold, ep=ep, max_iter=maxIterTimes, min_iter=minIterTimes, min_pairs=200,
                                  fail_only_first=1))
        return pt2plane if planar else pt2pt
    return for_pair


def run(argv=None):
    """-> dict(fixed, tried, failed, second, debug, poses): the decisions and the final poses of one run (what main prints and writes)."""
    ap = argparse.ArgumentParser(prog="refine_sequence.py", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", required=True, help="the odometry's pose file (poses_/NN.txt: one 12-float row per frame)")
    ap.add_argument("--calib", help="calib_.txt or KITTI calib.txt; identity if omitted (like run_sequence.py)")
    ap.add_argument("--gt", help="ground-truth poses: DebugInfo gets the error columns and the mean errors are printed")
    ap.add_argument("--inliers-dir", help="<seq>/InliersIdx of run_sequence.py --save-artifacts (needed by --mode keyframes)")
    ap.add_argument("--scans", help="directory of KITTI velodyne .bin files: extended key points are made on the device")
    ap.add_argument("--synthetic", action="store_true", help="the scans are caelo.synth's (run_sequence.py --synthetic N; N = rows of --poses)")
    ap.add_argument("--scene", default="boxes", choices=("boxes", "clutter"))
    ap.add_argument("--trajectory", default="circuit", choices=synth.TRAJECTORIES)
    ap.add_argument("--calib-angle", type=float, default=None, metavar="DEG", help="CorrectPC on the device before the projection (raw KITTI scans: 0.22)")
    ap.add_argument("--keypts-dir", help="<seq>/KeyPts: <frame:06d>.bin.mat with ExtendedKeyPts and PlanarPts (BatchPreprocess.py:140-148)")
    ap.add_argument("--save-keypts", metavar="DIR", help="write the key points made from --scans / --synthetic to DIR (a KeyPts folder)")
    ap.add_argument("--planar-pts", choices=("ring",), help="make every frame's planar points with normals on the device from its ring image "
                    "(SphericalRing.py:236-282); with --scans / --synthetic, what --icp pt2plane registers with")
    ap.add_argument("--dejump", action="store_true", help="FixJumpPoses first (RefinePoses.py:233-262)")
    ap.add_argument("--mode", default="keyframes", choices=("keyframes", "consecutive"), help="RefineOdometry's iOption 1 / 0")
    ap.add_argument("--start-frame", type=int, default=0, help="iStartFrame")
    ap.add_argument("--second-pass", action="store_true", help="CloseLoopPipeline on the refinement's key frames (RefinePoses.py:477-518)")
    ap.add_argument("--icp", default="pt2pt", choices=("pt2pt", "pt2plane"))
    ap.add_argument("--nn", default="grid", choices=("grid", "brute"), help="nearest neighbours of the device ICP: a cell grid over frame 0 "
                    "(caelo_icp_grid) or the all-pairs walk (caelo_icp); the same pairs and the same bytes either way (DESIGN.md 9l)")
    ap.add_argument("--seed-base", type=int, default=1000, help="--icp pt2plane: the k-th registration subsamples with RandomState(seed_base + k)")
    ap.add_argument("--out", required=True, help="refined poses (poses___/NN.txt)")
    ap.add_argument("--dejumped-out", help="the poses after --dejump (poses__/NN.txt)")
    ap.add_argument("--second-pass-out", help="the poses after --second-pass (default: they go to --out)")
    ap.add_argument("--debug-info", metavar="MAT", help="DebugInfo.mat: {'aDebugInfo': float32 table} as RefinePoses.py:583-584 reads it")
    args = ap.parse_args(argv)
    sources = [bool(args.scans), bool(args.synthetic), bool(args.keypts_dir)]
    if sum(sources) != 1:
        ap.error("give exactly one of --scans, --synthetic and --keypts-dir")
    if args.mode == "keyframes" and not args.inliers_dir:
        ap.error("--mode keyframes follows the inlier pairs from frame to frame: give --inliers-dir")
    if args.calib_angle is not None and (args.keypts_dir or not np.isfinite(args.calib_angle)):
        ap.error("--calib-angle is a finite number of degrees and goes with --scans / --synthetic")
    if args.save_keypts and args.keypts_dir:
        ap.error("--save-keypts writes what --scans / --synthetic make")
    if args.planar_pts and args.keypts_dir:
        ap.error("--planar-pts makes planar points from --scans / --synthetic; --keypts-dir files carry their own")
    poses_ = stageio.read_poses(args.poses)
    n = poses_.shape[0]
    if n < 4:
        ap.error("%s holds %d poses: nothing to refine below 4" % (args.poses, n))
    if not 0 <= args.start_frame:
        ap.error("--start-frame must not be negative")
    Tr = stageio.read_calib_tr(args.calib) if args.calib else np.eye(3, 4, dtype=np.float32)
    gt = stageio.read_poses(args.gt) if args.gt else None
    if gt is not None and gt.shape[0] < n:
        ap.error("%s holds %d poses, %s %d" % (args.gt, gt.shape[0], args.poses, n))
    if args.icp == "pt2plane":   # refused before any launch
        why = ("--icp pt2plane is ICP_Pt2PtAndPt2Plane (RefinePoses.py:291-294), which needs planar points with normals; GetKeyPtsByAE stores an "
               "empty PlanarPts (SphericalRing.py:219,285: its producer is commented out) and scikit-learn refuses to fit it (MyICP.py:94)")
        if not args.keypts_dir and not args.planar_pts:
            ap.error(why + ": give --keypts-dir files that hold PlanarPts, or use --icp pt2pt (RefinePoses.py:295)")
        if args.keypts_dir:
            counts = KeyPts(None, n, keypts_dir=args.keypts_dir).planar_counts()
            bad = [f for f, c in enumerate(counts) if c <= 0]
            if bad:
                ap.error(why + ": no PlanarPts for frame(s) %s of %s" % (bad[:10], args.keypts_dir))
    files = None
    if args.scans:
        files = sorted(glob.glob(os.path.join(args.scans, "*.bin")))
        if len(files) < n:
            ap.error("%d scans in %s for %d poses" % (len(files), args.scans, n))

    import caelo
    caelo.configure_runtime()
    from caelo.engine import default_engine
    eng = default_engine()
    keypts = KeyPts(eng, n, keypts_dir=args.keypts_dir, files=files,
                    synthetic=dict(scene_kind=args.scene, trajectory=args.trajectory) if args.synthetic else None,
                    calib_angle=args.calib_angle, save_dir=args.save_keypts, planar_ring=bool(args.planar_pts))
    planar = args.icp == "pt2plane"
    core = refine.make_core(keypts, Tr, device_icp(eng, keypts, args.nn, planar), seed_base=args.seed_base if planar else None, per_pair=True)
    pairs = None
    if args.inliers_dir:
        seq_dir, folder = os.path.dirname(os.path.abspath(args.inliers_dir)), os.path.basename(os.path.abspath(args.inliers_dir))
        pairs = lambda f0, f1: stageio.load_inliers(seq_dir, f0, f1, folder=folder)   # noqa: E731

    def save(path, poses):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        np.savetxt(path, poses)   # RefinePoses.py:568,579,590

    name = os.path.splitext(os.path.basename(args.poses))[0]
    log = lambda s: print("%s : %d : %s" % (name, n, s))   # noqa: E731
    poses__, fixed, second = poses_, [], []
    if args.dejump:
        poses__, fixed = refine.FixJumpPoses(poses_, log=log)
        print(fixed)
        if args.dejumped_out:
            save(args.dejumped_out, poses__)
    poses___, info, failed, tried = refine.RefineOdometry(poses__, 1 if args.mode == "keyframes" else 0, core, pairs=pairs, gt=gt,
                                                         iStartFrame=args.start_frame, log=log)
    print(failed)
    final = poses___
    if args.second_pass:
        final, second = refine.CloseLoopPipeline(poses___, info, core, log=log)
        if args.second_pass_out:
            save(args.second_pass_out, final)
    save(args.out, poses___ if args.second_pass and args.second_pass_out else final)
    if args.debug_info:
        from scipy import io
        os.makedirs(os.path.dirname(os.path.abspath(args.debug_info)), exist_ok=True)
        io.savemat(args.debug_info, {"aDebugInfo": info})   # RefinePoses.py:685
    if gt is not None:   # RefinePoses.py:668-692
        for label, p in (("odometry", poses_), ("refined", final)):
            _, _, e, t = evaluate.GetErrorRTs(gt[:n], p, Tr)
            print("%-8s mean sum|error Euler| = %.6f deg, mean |error T| = %.6f m" % (label, np.mean(np.sum(np.abs(e), axis=1)), np.mean(np.linalg.norm(t, axis=1))))
    return dict(fixed=fixed, tried=tried, failed=failed, second=second, debug=info, poses=final)


def main(argv=None):
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
