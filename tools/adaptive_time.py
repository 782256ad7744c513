#!/usr/bin/env python
"""adaptive_time.py -- Engine.register_pairs_adaptive beside Engine.register_pairs on 1 000 pairs over 12 resident frames (the
setting of DESIGN.md 9c's table): host time of the whole Python call, median of nine warm calls and their range.

    python tools/adaptive_time.py [--pairs 1000] [--frames 12] [--calls 9]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

import caelo  # noqa: E402
caelo.configure_runtime()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from caelo import adaptive, synth  # noqa: E402
from caelo.engine import Engine, ransac_draws  # noqa: E402


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--calls", type=int, default=9)
    args = ap.parse_args()
    eng = Engine(device=0)
    pcs = [torch.from_numpy(synth.make_scan(f)).to(eng.device) for f in range(args.frames)]
    rands = [torch.from_numpy(ransac_draws(f)).to(eng.device) for f in range(args.frames)]
    batch = eng.pipeline(8).run(pcs, rands, certify=False)
    rows, n_key = batch.rows[:args.frames].contiguous(), batch.n_key[:args.frames].contiguous()
    rs = np.random.RandomState(0)
    tables = {"random pairs": rs.randint(0, args.frames, (args.pairs, 2)),
              "steps 1 / 5 / 10 per anchor": np.array([(a, min(args.frames - 1, a + s)) for a in rs.randint(0, args.frames - 1, args.pairs // 3 + 1)
                                                       for s in (1, 5, 10)][:args.pairs])}
    draws_m = np.stack([ransac_draws(1000 + q) for q in range(args.pairs)])
    draws_a = torch.from_numpy(adaptive.draw_table(0)).to(eng.device)
    print("n_key %s" % n_key.cpu().numpy().tolist())
    for name, table in tables.items():
        m = timed(lambda: eng.register_pairs(rows, n_key, table, draws_m, certify=False), args.calls)
        a = timed(lambda: eng.register_pairs_adaptive(rows, n_key, table, draws_a, 1.0), args.calls)
        out = eng.register_pairs_adaptive(rows, n_key, table, draws_a, 1.0)
        tr = out.results["trials"]
        print("%-30s register_pairs %.1f ms (%.1f-%.1f) | register_pairs_adaptive %.1f ms (%.1f-%.1f); trials: median %d, max %d, %d of %d at the limit"
              % (name, m[0], m[1], m[2], a[0], a[1], a[2], int(np.median(tr)), int(tr.max()), int((out.results["status"] == 1).sum()), len(tr)))


if __name__ == "__main__":
    main()
