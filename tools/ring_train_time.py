"""One reference-sized training step of the ring autoencoder -- 32 images of 64 x 1792 (AE4SphericalRingPC.py:118, 2 GPUs x 16 files) --
in ONE process on one engine, warm: --runs timings (default 3), each the mean over --iters back-to-back calls between two HIP events, of
    grad + adam       caelo_ring_autoencoder_grad + caelo_adam_step (csrc/train_ring.hip) at --chunk, the projected rings read in place
    torch autograd    torch-ROCm's own backward of tests/netref64_ring.py's float32 network + Keras's Adam formula (tensor operations) on
                      the same batch, same GPU, same session: the only yardstick available (Keras / TensorFlow cannot run here)
with images / s and the share of the f32 matrix peak on the algorithmic count (213.8 M MAC per image forward: 99.1 + 29.4 + 33.0 +
16.5 + 33.0 + 2.8; both gradients of every layer but conv2d_1, which has no data gradient: 3 x 213.8 - 99.1 = 542.3 M MAC per image;
157.3 TFLOP/s).  profiles/ring_train_times.txt is this output, followed by one `rocprofv3 --kernel-trace --stats` run of
`--iters 6 --runs 1 --no-torch` for the per-kernel split.

    python tools/ring_train_time.py [--runs 3] [--iters 20] [--chunk 4] [--images 32] [--no-torch]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import caelo  # noqa: E402
caelo.configure_runtime()
import netref64_ring as nr  # noqa: E402
from caelo import synth, train_ring  # noqa: E402
from caelo.engine import Engine  # noqa: E402

MAC_PER_IMAGE = 542.3e6
PEAK_FLOPS = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--chunk", type=int, default=4)
ap.add_argument("--images", type=int, default=32)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
eng = Engine(device=0)
ws = nr.model("shipped")
distinct = train_ring.ring_batch(eng, [synth.make_scan(f, quantum=1e-3) for f in range(4)])      # four scans, repeated: the arithmetic is the same
rings = distinct.repeat((args.images + 3) // 4, 1, 1, 1)[:args.images].contiguous()
n = rings.shape[0]
tr = train_ring.RingTrainer(eng, ws, chunk=args.chunk)
print("%d images of 64 x 1792, chunk %d, %d runs x %d calls; times in us per call" % (n, args.chunk, args.runs, args.iters))


def torch_step():
    params = [p.detach().to(eng.device).requires_grad_(True) for p in nr.to_params(ws, torch.float32)]
    ms = [torch.zeros_like(p) for p in params]
    vs = [torch.zeros_like(p) for p in params]
    x = rings[:, :64, :1792, :3].permute(0, 3, 1, 2).contiguous()
    F = torch.nn.functional
    state = dict(t=0)

    def step():
        k = params
        for p in k:
            p.grad = None
        p1 = F.max_pool2d(torch.relu(nr._conv(torch.relu(nr._conv(x, k[0], k[1])), k[2], k[3])), 2)
        p2 = F.max_pool2d(torch.relu(nr._conv(p1, k[4], k[5])), 2)
        y5 = torch.relu(nr._conv(nr._up(torch.relu(nr._conv(p2, k[6], k[7]))), k[8], k[9]))
        loss = F.mse_loss(nr._conv(nr._up(y5), k[10], k[11]), x)
        loss.backward()
        state["t"] += 1
        lr_t = float(train_ring.adam_lr_t(state["t"]))
        with torch.no_grad():
            for p, m, v in zip(k, ms, vs):
                m.mul_(nr.BETA_1).add_(p.grad, alpha=1.0 - nr.BETA_1)
                v.mul_(nr.BETA_2).addcmul_(p.grad, p.grad, value=1.0 - nr.BETA_2)
                p.sub_(lr_t * m / (v.sqrt() + nr.EPSILON))
        return loss
    return step


calls = [("grad + adam", lambda: tr.step(rings, sync=False))]
if not args.no_torch:
    calls.append(("torch autograd + Adam", torch_step()))
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
    print("%-24s %s   best: %.0f images/s, %.2f %% of the f32 matrix peak" % (
        name, "  ".join("%.1f" % r for r in runs), n / (best[name] * 1e-6), 100 * 2 * MAC_PER_IMAGE * n / (best[name] * 1e-6) / PEAK_FLOPS))
    sys.stdout.flush()
if len(best) == 2:
    print("hand-written / torch (best runs): %.3f" % (best["grad + adam"] / best["torch autograd + Adam"]))
print("loss after the timed steps %.6f, lane_faults %d" % (tr.loss(rings), eng.lane_faults()))
