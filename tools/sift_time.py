"""One SIFT3D octave call, one SIFT3D pyramid call and one Harris3D call on 8 frames x 16 384 points (the workload of
tools/iss_time.py: synthetic scans thinned by caelo.iss.voxel_downsample at 0.2 m, then subsampled) in ONE process on one engine:
--runs timings (default 3) of each, each the mean over --iters back-to-back calls between two HIP events after a warm-up, the pair
evaluations per second of the octave call (two all-pairs passes of n^2 pairs per frame: the scale space and the neighbour
selection), the points per octave of the pyramid and the key point counts.  The octave call runs on the thinned points themselves at
the scales of octave 0 (sigma 0.46 .. 1.09 m), so that its passes walk the same pairs as the Harris3D and ISS passes of
profiles/harris_times.txt; the pyramid call is what detect_sift_keypoints.py does per batch.  profiles/sift_times.txt is this
output, followed by the kernel table of one `rocprofv3 --kernel-trace --stats -- python tools/sift_time.py --iters 3 --runs 1`.

    python tools/sift_time.py [--runs 3] [--iters 5] [--frames 8] [--points 16384]
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
from caelo import iss, sift, synth  # noqa: E402
from caelo.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=5)
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


sigma = sift.octave_scales(sift.DEFAULTS["min_scale"], sift.DEFAULTS["n_scales_per_octave"])
r, runs = timed(lambda: eng.sift_octave(pts, n_pts=counts, sigma=sigma, min_contrast=sift.DEFAULTS["min_contrast"]))
print("sift octave:  ms per call (with the finite check's read-back): %s" % "  ".join("%.3f" % t for t in runs))
print("sift octave:  pair evaluations per second over both all-pairs passes, best run: %.3g" % (2 * pairs / (min(runs) * 1e-3)))
P = pts[0, :counts[0]].double()
d2 = ((P[:512, None, :] - P[None, :, :]) ** 2).sum(dim=2)
inside = [float((d2 <= 9.0 * s * s).sum(dim=1).double().mean()) for s in (sigma[0], sigma[-1])]
print("sift octave:  points inside 3 sigma of the smallest / largest scale (frame 0, its first 512 points): %.0f / %.0f; points with a key per "
      "frame %s" % (inside[0], inside[1], r.n_key.cpu().tolist()))
(r, octs), runs = timed(lambda: eng.sift_keypoints(pts, n_pts=counts, details=True))
print("sift pyramid: ms per call (host loop over the octaves, sorts, read-backs): %s" % "  ".join("%.3f" % t for t in runs))
print("sift pyramid: points per octave (frame 0) %s; key points per frame %s"
      % ([int(o["clouds"][0].shape[0]) for o in octs], r.n_key.cpu().tolist()))
r, runs = timed(lambda: eng.harris_keypoints(pts, n_pts=counts, normals=True))
print("harris:       ms per call (with the finite check's read-back): %s" % "  ".join("%.3f" % t for t in runs))
print("harris:       pair evaluations per second over the three passes, best run: %.3g" % (3 * pairs / (min(runs) * 1e-3)))
