"""One Harris3D call and one ISS call on 8 frames x 16 384 points (the workload of tools/iss_time.py: synthetic scans thinned by
caelo.iss.voxel_downsample at 0.2 m, then subsampled) in ONE process on one engine: --runs timings (default 3) of each detector, each
the mean over --iters back-to-back calls between two HIP events after a warm-up, the pair evaluations per second they stand for (three
all-pairs passes of n^2 pairs per frame for Harris3D, two for ISS), and the key point counts.  profiles/harris_times.txt is this
output, followed by the kernel table of one `rocprofv3 --kernel-trace --stats -- python tools/harris_time.py --iters 3 --runs 1` for
the per-kernel split, with k_iss_scatter / k_iss_nms measured in the same session beside the three new passes.

    python tools/harris_time.py [--runs 3] [--iters 10] [--frames 8] [--points 16384]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
import caelo  # noqa: E402
caelo.configure_runtime()
from caelo import iss, synth  # noqa: E402
from caelo.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--points", type=int, default=16384)
args = ap.parse_args()
eng = Engine(respond_h5=None, encoder_h5=None, device=0)
clouds = []
for f in range(args.frames):
    pc = iss.voxel_downsample(torch.from_numpy(synth.make_scan(f, quantum=1e-3)[:, 0:3].copy()).to(eng.device), 0.2)
    keep = iss.subsample(pc.shape[0], args.points, np.random.RandomState(f))
    clouds.append(pc[torch.from_numpy(keep).to(eng.device)])
counts = [int(c.shape[0]) for c in clouds]
ld = max(counts)
pts = torch.zeros((args.frames, ld, 3), dtype=torch.float32, device=eng.device)
for f, c in enumerate(clouds):
    pts[f, :counts[f]] = c
pairs = float(sum(n * n for n in counts))
print("%d frames, points per frame %s, %.4g pairs per pass; %d runs x %d calls" % (args.frames, counts, pairs, args.runs, args.iters))


def timed(call):
    for _ in range(2):
        r = call()
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            r = call()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) / args.iters)
    return r, runs


r, runs = timed(lambda: eng.harris_keypoints(pts, n_pts=counts, normals=True))
print("harris: ms per call (with the finite check's read-back): %s" % "  ".join("%.3f" % t for t in runs))
print("harris: pair evaluations per second over the three passes, best run: %.3g" % (3 * pairs / (min(runs) * 1e-3)))
nn = r.n_neigh.cpu().numpy()
resp = r.response.cpu().numpy()
valid = [int((resp[f, :counts[f]] != -1.0).sum()) for f in range(args.frames)]
above = [int((resp[f, :counts[f]] >= 0.001).sum()) for f in range(args.frames)]
print("harris: key points per frame %s; neighbours within the radius: mean %.1f, max %d; points with a normal %s, at or above the threshold %s"
      % (r.n_key.cpu().tolist(), float(np.mean([nn[f, :counts[f]].mean() for f in range(args.frames)])), int(nn.max()), valid, above))
r, runs = timed(lambda: eng.iss_keypoints(pts, n_pts=counts, eig=True))
print("iss:    ms per call (with the finite check's read-back): %s" % "  ".join("%.3f" % t for t in runs))
print("iss:    pair evaluations per second over both passes, best run: %.3g" % (2 * pairs / (min(runs) * 1e-3)))
print("iss:    key points per frame %s" % (r.n_key.cpu().tolist(),))
