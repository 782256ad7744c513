"""One reference-sized training step -- 1 536 patches (2 scans x 256 key points x 3 scales) -- in ONE process on one engine, warm:
--runs timings (default 3), each the mean over --iters back-to-back calls between two HIP events, of
    grad + adadelta   caelo_autoencoder_grad + caelo_adadelta_step (csrc/train.hip) at --chunk
    torch autograd    torch-ROCm's own backward of tests/netref64_train.py's float32 network + torch.optim.Adadelta on the same
                      batch, same GPU, same session: the only yardstick available (Keras / TensorFlow cannot run here)
with patches / s and the share of the f32 matrix peak on the algorithmic count (22.8 M MAC per patch for forward plus both
gradients, conv3d_1 without a data gradient; 157.3 TFLOP/s).  profiles/train_times.txt is this output, followed by one
`rocprofv3 --kernel-trace --stats --output-format csv` run of `--iters 3 --runs 1 --no-torch` for the per-kernel split.

    python tools/train_time.py [--runs 3] [--iters 20] [--chunk 256] [--no-torch]
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import caelo  # noqa: E402
caelo.configure_runtime()
import netref64 as nr  # noqa: E402
import netref64_dec as nd  # noqa: E402
import netref64_train as nt  # noqa: E402
from caelo import synth, train  # noqa: E402
from caelo.engine import Engine  # noqa: E402

MAC_PER_PATCH = 22.8e6
PEAK_FLOPS = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--chunk", type=int, default=256)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
eng = Engine(device=0)
with tempfile.TemporaryDirectory() as tmp:
    ews, eact, dws, dact = nd.model("fixture", tmp)
rng = np.random.RandomState(0)
bits = torch.cat([train.training_patches(eng, synth.make_scan(f, quantum=1e-3), 256, rng) for f in range(2)]).contiguous()
n = bits.numel() // 64
assert n == 1536
tr = train.Trainer(eng, ews, eact, dws, dact, chunk=args.chunk)
print("%d patches, chunk %d, model %s / %s, %d runs x %d calls; times in us per call" % (n, args.chunk, eact, dact, args.runs, args.iters))


def torch_step():
    params = [p.detach().to(eng.device).requires_grad_(True) for p in nt.to_params(ews, dws, torch.float32)]
    opt = torch.optim.Adadelta(params, lr=1.0, rho=0.95, eps=1e-7)
    y = torch.from_numpy(nr.unpack(bits.cpu().numpy().view(np.uint64)).astype(np.float32)).to(eng.device).permute(0, 4, 1, 2, 3).contiguous()
    h, c, hd = nt._ACT[eact[0]], nt._ACT[eact[1]], nt._ACT[dact[0]]
    F = torch.nn.functional

    def step():
        k = params
        opt.zero_grad(set_to_none=True)
        p1 = F.max_pool3d(h(nt._conv(y, k[0], k[1])), 2)
        p2 = F.max_pool3d(h(nt._conv(p1, k[2], k[3])), 2)
        f3 = h(nt._conv(p2, k[4], k[5])).permute(0, 2, 3, 4, 1).reshape(n, 2048)
        code = c(h(f3 @ k[6] + k[7]) @ k[8] + k[9])
        g4 = hd(hd(code @ k[10] + k[11]) @ k[12] + k[13])
        y4 = hd(nt._conv(g4.reshape(n, 4, 4, 4, 32).permute(0, 4, 1, 2, 3), k[14], k[15]))
        y5 = hd(nt._conv(nt._up(y4), k[16], k[17]))
        z = nt._conv(nt._up(y5), k[18], k[19])
        loss = F.binary_cross_entropy_with_logits(torch.clamp(z, -nt.LOGIT_CLIP, nt.LOGIT_CLIP), y)
        loss.backward()
        opt.step()
        return loss
    return step


calls = [("grad + adadelta", lambda: tr.step(bits, sync=False))]
if not args.no_torch:
    calls.append(("torch autograd + Adadelta", torch_step()))
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
    print("%-28s %s   best: %.0f patches/s, %.2f %% of the f32 matrix peak" % (
        name, "  ".join("%.1f" % r for r in runs), n / (best[name] * 1e-6), 100 * 2 * MAC_PER_PATCH * n / (best[name] * 1e-6) / PEAK_FLOPS))
    sys.stdout.flush()
if len(best) == 2:
    print("hand-written / torch (best runs): %.2f" % (best["grad + adadelta"] / best["torch autograd + Adadelta"]))
print("loss after the timed steps %.6f, lane_faults %d" % (tr.loss(bits), eng.lane_faults()))
