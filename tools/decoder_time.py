"""One 24 576-patch decode (8 frames x 3 072 patches, group 3 on the descriptor rows) in ONE process on one engine, with the
reference's trained autoencoder (the two fixture halves under tests/golden/): --runs timings (default 3), each the mean over --iters
back-to-back calls between two HIP events after a warm-up, of
    decode  loss + bits + counts          (what evaluate.py reconstruction runs)
    decode  the same with prob written    (16 KB per patch more: autoencoder.predict)
    encode  the same patches              (the yardstick: the encoder's kernels are not touched by the decoder)
and the decode / encode ratio.  profiles/decoder_times.txt is this output, followed by one `rocprofv3 --kernel-trace --stats` run of
`--iters 3 --runs 1` for the per-kernel split.

    python tools/decoder_time.py [--runs 3] [--iters 20]
"""
import argparse
import os
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import caelo  # noqa: E402
caelo.configure_runtime()
import netref64_act as na  # noqa: E402
import netref64_dec as nd  # noqa: E402
from caelo import synth  # noqa: E402
from caelo.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
eng = Engine(device=0)
with tempfile.TemporaryDirectory() as tmp:
    print("model", eng.load_autoencoder(nd.fixture_h5(tmp), encoder_h5=na.fixture_h5(tmp)))
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
rows = torch.zeros((n // 3, 64), dtype=torch.float32, device=eng.device)
rows[:, :60] = eng.encode(bits, group=3)
target = bits.view(n, 64)
print("%d patches, %d runs x %d calls; times in us per call" % (n, args.runs, args.iters))
calls = (("decode loss+bits+counts", lambda: eng.decode(rows, group=3, target=target)),
         ("decode + prob", lambda: eng.decode(rows, group=3, target=target, prob=True)),
         ("encode", lambda: eng.encode(bits, group=3)))
best = {}
for name, call in calls:
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            call()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / args.iters)
    best[name] = min(runs)
    print("%-26s %s" % (name, "  ".join("%.1f" % r for r in runs)))
    sys.stdout.flush()
d = eng.decode(rows, group=3, target=target)
print("decode / encode (best runs): %.2f; with prob %.2f" % (best["decode loss+bits+counts"] / best["encode"], best["decode + prob"] / best["encode"]))
print("mean loss %.6f, lane_faults %d" % (float(d.loss.double().mean().item()), eng.lane_faults()))
