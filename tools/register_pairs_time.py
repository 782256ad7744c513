#!/usr/bin/env python
"""register_pairs_time.py -- Engine.register_pairs on 1 000 pairs over 12 resident frames (DESIGN.md 9c's protocol): host time of the
whole Python call, warm, median and range of nine calls; the table as random pairs and as steps 1 / 5 / 10 per anchor, with the
kernels' own fits (certify=False) and certified.  One process times one library; for an A/B build the other one beside the product
(`make -C cae-lo_amd/csrc BUILD=build_parent OUT=/tmp/libcaelo_parent.so` on the parent's tree), select it with CAELO_LIB and run
the two alternately.  The last line is the four cells as JSON.

    python tools/register_pairs_time.py [--pairs 1000] [--frames 12] [--calls 9]
    CAELO_LIB=/tmp/libcaelo_parent.so python tools/register_pairs_time.py
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

import caelo  # noqa: E402
caelo.configure_runtime()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from caelo import _ffi, synth  # noqa: E402
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
    draws = np.stack([ransac_draws(1000 + q) for q in range(args.pairs)])
    print("%s; n_key %s" % (_ffi.LIB_PATH, n_key.cpu().numpy().tolist()))
    cells = {}
    for name, table in tables.items():
        for certify in (False, True):
            m = timed(lambda: eng.register_pairs(rows, n_key, table, draws, certify=certify), args.calls)
            cells["%s, %s" % (name, "certified" if certify else "certify=False")] = m
            print("%-30s %-14s %.1f ms (%.1f-%.1f)" % (name, "certified" if certify else "certify=False", m[0], m[1], m[2]))
    print(json.dumps({"lib": _ffi.LIB_PATH, "median_min_max_ms": cells}))


if __name__ == "__main__":
    main()
