"""The bits of both device trainers on the tests' seeded inputs, one sha256 per line over the raw bytes of each result: run it once on
two builds of the library (CAELO_LIB selects one, caelo/_ffi.py) and compare the outputs line for line.  What a refactor of
csrc/train.hip, csrc/train_ring.hip or what they share must leave identical; profiles/train_refactor_bits.txt is one such output.
tanhf and expf belong to the ROCm version, so hashes are comparable within one installation only.

    voxel trainer, each model of netref64_dec.MODELS: loss and the 20 gradients at n = 1 and n = 17 (chunk 8) and n = 134 (chunk 64);
        the parameters and both Adadelta accumulators after three steps at n = 17
    ring trainer, each model of netref64_ring.MODELS: loss, the 12 gradients and predict at every (h, w, n, chunk) of
        tests/test_train_ring_gpu.py's SHAPES; the parameters, m and v after three steps at (8, 16, 5, 2); and one batch of two
        full-size projected rings read in place

    python tools/train_bits.py > bits.txt
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import caelo  # noqa: E402
caelo.configure_runtime()
import netref64_dec as nd  # noqa: E402
import netref64_ring as nr  # noqa: E402
from caelo import synth, train, train_ring  # noqa: E402
from caelo.engine import Engine  # noqa: E402

RING_SHAPES = [(4, 4, 1, 1), (4, 8, 3, 2), (8, 16, 5, 2), (12, 20, 4, 3), (16, 36, 4, 4), (16, 36, 5, 2)]   # test_train_ring_gpu.SHAPES


def line(what, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print("%s  %s" % (h.hexdigest(), what))
    sys.stdout.flush()


eng = Engine(device=0)
with tempfile.TemporaryDirectory() as tmp:
    for name in [m[0] for m in nd.MODELS]:
        ews, eact, dws, dact = nd.model(name, tmp)
        bits = nd.patches(name)
        for n, chunk in ((1, 8), (17, 8), (134, 64)):
            loss, grads = train.Trainer(eng, ews, eact, dws, dact, chunk=chunk).grad(bits[:n])
            line("voxel %s n=%d chunk=%d loss+grads" % (name, n, chunk), np.float32(loss), *grads)
        tr = train.Trainer(eng, ews, eact, dws, dact, chunk=8)
        losses = [tr.step(bits[:17]) for _ in range(3)]
        line("voxel %s n=17 chunk=8 three steps: losses, params, acc_g, acc_d" % name, np.float32(losses), tr.params.cpu().numpy(),
             tr.acc_g.cpu().numpy(), tr.acc_d.cpu().numpy())

rings = train_ring.ring_batch(eng, [synth.make_scan(f, quantum=1e-3) for f in (0, 1)])
for name in nr.MODELS:
    ws = nr.model(name)
    for h, w, n, chunk in RING_SHAPES:
        x = nr.images(n, h, w, seed=h)
        tr = train_ring.RingTrainer(eng, ws, chunk=chunk)
        loss, grads = tr.grad(x)
        line("ring %s %dx%d n=%d chunk=%d loss+grads+predict" % (name, h, w, n, chunk), np.float32(loss), *grads, tr.predict(x).cpu().numpy())
    tr = train_ring.RingTrainer(eng, ws, chunk=2)
    x = nr.images(5, 8, 16, seed=8)
    losses = [tr.step(x) for _ in range(3)]
    line("ring %s 8x16 n=5 chunk=2 three steps: losses, params, m, v" % name, np.float32(losses), tr.params.cpu().numpy(), tr.m.cpu().numpy(),
         tr.v.cpu().numpy())
    tr = train_ring.RingTrainer(eng, ws, chunk=2)
    loss, grads = tr.grad(rings)
    line("ring %s 64x1792 n=2 chunk=2 read in place loss+grads+predict" % name, np.float32(loss), *grads, tr.predict(rings).cpu().numpy())
