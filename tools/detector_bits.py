"""The bits of both hand-crafted key point detectors, one sha256 per line over the raw bytes of each output: run it once on two builds
of the library (CAELO_LIB selects one, caelo/_ffi.py) and compare the outputs line for line.  What a refactor of csrc/iss.hip,
csrc/harris.hip or what they share (csrc/iss_common.h) must leave identical; profiles/detector_refactor_bits.txt is one such output.

    ISS (key_idx, n_key, saliency, eig, n_neigh) and Harris3D (key_idx, n_key, response, n_neigh, normals) on
        every scene of iss_ref.SCENES and harris_ref.SCENES with its parameters, as one cloud
        the two batches of the GPU tests: 1500, 0 and 257 points under ld = 1536 with NaN padding; 600, 1025 and 257 under ld = 1025
        2 frames x 4 096 points of synth.make_scan thinned as tools/iss_time.py thins them

    python tools/detector_bits.py > bits.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import caelo  # noqa: E402
caelo.configure_runtime()
import harris_ref  # noqa: E402
import iss_ref  # noqa: E402
from caelo import iss, synth  # noqa: E402
from caelo.engine import Engine  # noqa: E402

eng = Engine(respond_h5=None, encoder_h5=None, device=0)


def lines(what, pts, n_pts=None, iss_kw={}, harris_kw={}):
    pts = torch.as_tensor(pts).to(eng.device)
    for name, r in (("iss", eng.iss_keypoints(pts, n_pts=n_pts, eig=True, **iss_kw)),
                    ("harris", eng.harris_keypoints(pts, n_pts=n_pts, normals=True, **harris_kw))):
        for field in r._fields:
            print("%s  %s %s %s" % (hashlib.sha256(getattr(r, field).cpu().numpy().tobytes()).hexdigest(), what, name, field))
    sys.stdout.flush()


def batch(frames, ld, fill):
    pts = np.full((len(frames), ld, 3), fill, np.float32)
    for f, p in enumerate(frames):
        pts[f, :p.shape[0]] = p
    return pts, [p.shape[0] for p in frames]


for (seed, n, ikw), (hseed, hn, hkw) in zip(iss_ref.SCENES, harris_ref.SCENES):
    assert (seed, n) == (hseed, hn)
    lines("scene %d n=%d %s %s" % (seed, n, sorted(ikw.items()), sorted(hkw.items())), iss_ref.scene(seed, n), iss_kw=ikw, harris_kw=hkw)
scenes = [iss_ref.scene(s, n) for s, n, _ in iss_ref.SCENES]
lines("batch 1500 0 257 ld=1536 NaN padding", *batch([scenes[0], np.zeros((0, 3), np.float32), scenes[3]], 1536, np.nan))
lines("batch 600 1025 257 ld=1025 padding 8.0", *batch([scenes[4], scenes[2], scenes[3]], 1025, 8.0))
clouds = []
for f in range(2):
    pc = iss.voxel_downsample(torch.from_numpy(synth.make_scan(f, quantum=1e-3)[:, 0:3].copy()).to(eng.device), 0.2)
    clouds.append(pc[torch.from_numpy(iss.subsample(pc.shape[0], 4096, np.random.RandomState(f))).to(eng.device)].cpu().numpy())
lines("2 thinned scans of 4096 points", *batch(clouds, 4096, 0.0))
