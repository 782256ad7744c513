"""One 24 576-patch encode (8 frames x 3 072 patches, group 3) per activation set, in ONE process on one engine: the same weights (the
shipped encoder's) as tanh / tanh, relu / linear, relu / tanh and tanh / linear, so that only the activation code differs between the
lines.  Per model: --runs timings (default 3), each the mean over --iters back-to-back encodes between two HIP events after a
warm-up, plus the per-kernel split of one profiled call (stage 1, conv3, Dense(200), head).  The relu kernels drop the 6.9 M
transcendental evaluations of a frame; they are expected to be no slower than their tanh siblings beyond the spread of repeated tanh
runs.  profiles/encoder_activations_times.txt is this output.

    python tools/encoder_act_time.py [--runs 3] [--iters 20]
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
from caelo import synth  # noqa: E402
from caelo.engine import ENCODER_H5, Engine, read_keras_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
eng = Engine(device=0)
ws = read_keras_weights(ENCODER_H5)[1]
# the patches of eight synthetic frames, as the pipeline's encoder stage sees them (every patch: no de-duplication)
bits = []
for f in range(8):
    pc = torch.from_numpy(synth.make_scan(f, quantum=1e-3)).to(eng.device)
    ff = eng.extract(pc)
    vm, _ = eng.voxelize_fast(pc, eng.voxmap(slot=5))
    bits.append(eng.patches(vm, ff.key_pts.contiguous())[0])
bits = torch.cat(bits).contiguous()
n = bits.numel() // 64
assert n == 24576
print("%d patches, %d runs x %d encodes per model; times in us per encode" % (n, args.runs, args.iters))
for acts in (("tanh", "tanh"), ("relu", "linear"), ("relu", "tanh"), ("tanh", "linear"), ("tanh", "tanh")):
    eng.set_encoder_weights(ws, activations=acts)
    for _ in range(3):
        eng.encode(bits, group=3)
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            eng.encode(bits, group=3)
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / args.iters)
    ms = eng.encode_profile(bits, group=3)[1]
    print("hidden %-4s code %-6s  %s   kernels (one profiled call): stage1 %.1f  conv3 %.1f  dense1 %.1f  head %.1f"
          % (acts[0], acts[1], "  ".join("%.1f" % r for r in runs), *(float(m) * 1e3 for m in ms[:4])))
    sys.stdout.flush()
print("lane_faults %d" % eng.lane_faults())
