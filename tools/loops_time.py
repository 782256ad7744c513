#!/usr/bin/env python
"""Time the loop-closure kernels.

    python tools/loops_time.py [--out profiles/loops_times.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/loops_time.py --calls-only     # the kernels' own times

Engine.scan_context for 8 synthetic frames of about 127 k points, and Engine.loop_search at N = 512 and N = 4 541 frames (a KITTI-00
sized run) with min_gap 50, k = 1: the whole call (host clock around the call and a stream synchronisation; the output arrays are
allocated inside it), warm, median of nine with the range in brackets.  The search's operations are counted from its shape -- every query
tile multiplies 16 queries x its candidates x 64 shifts x 1 200 -- and set against the 155 TF the f32 matrix pipe measures; the
pairs the definition needs (j <= i - min_gap, 60 shifts) are listed beside it.  The NumPy restatement (tests/loops_ref.py, float64 on
the host) is timed once at N = 512."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

PEAK_F32_MATRIX = 155e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls-only", action="store_true", help="the timed calls alone, without the NumPy restatement (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import caelo
    caelo.configure_runtime()
    import loops_ref as lr
    from caelo import synth
    from caelo.engine import default_engine
    eng = default_engine()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        for _ in range(3):   # warm: code objects, the workspace
            call()
        times = []
        for _ in range(9):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        return statistics.median(times), min(times), max(times)

    say("# whole calls, median of 9 [min .. max], %s" % torch.cuda.get_device_name(0))
    scans = [synth.make_scan(f, quantum=1e-3, trajectory="circuit") for f in range(8)]
    ld = max(len(s) for s in scans)
    pts = torch.zeros((8, ld, 4), dtype=torch.float32, device=eng.device)
    for f, s in enumerate(scans):
        pts[f, :len(s)] = torch.from_numpy(s).to(eng.device)
    n_pts = torch.tensor([len(s) for s in scans], dtype=torch.int32, device=eng.device)
    med, lo, hi = timed(lambda: eng.scan_context(pts, n_pts))
    say("%-44s %9.1f us [%9.1f .. %9.1f]   %d points" % ("Engine.scan_context, 8 frames", 1e6 * med, 1e6 * lo, 1e6 * hi, int(n_pts.sum())))

    rs = np.random.RandomState(3)
    for n in (512, 4541):
        imgs = rs.uniform(0.2, 3.0, (n, lr.RINGS, lr.SECTORS)).astype(np.float32)
        imgs[rs.uniform(size=imgs.shape) < 0.3] = 0
        imgs[:, :, ::7] *= (rs.uniform(size=(n, 1, 9)) < 0.7)          # some empty columns
        ref = [lr.prepare(i) for i in imgs]
        u64, v64 = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
        u = torch.from_numpy(u64.astype(np.float32)).to(eng.device)
        bits = (v64.astype(np.uint64) << np.arange(60, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)
        valid = torch.from_numpy(bits.view(np.int64)).to(eng.device)
        min_gap = 50
        med, lo, hi = timed(lambda: eng.loop_search(u, valid, min_gap=min_gap, k=1))
        tiles = (n + 15) // 16
        jmax = [min(16 * t + 15, n - 1) - min_gap for t in range(tiles)]          # a tile's last candidate
        live = sum(j // 64 + 1 for j in jmax if j >= 0)
        flop_done = sum(j + 1 for j in jmax if j >= 0) * 16 * 64 * 1200 * 2.0     # 16 queries x 64 shifts x 1 200 per candidate of a tile
        pairs = sum(max(0, i - min_gap + 1) for i in range(n))
        flop_needed = pairs * 60 * 1200 * 2.0
        say("%-44s %9.1f us [%9.1f .. %9.1f]   %d causal pairs, %d live workgroups; multiplied %.3f TFLOP = %.1f TF/s whole call, %.1f %% of the "
            "155 TF f32 matrix figure (the definition needs %.3f TFLOP)" % ("Engine.loop_search, N = %d, min_gap 50, k = 1" % n, 1e6 * med, 1e6 * lo, 1e6 * hi,
                                                                        pairs, live, flop_done / 1e12, flop_done / med / 1e12,
                                                                        100.0 * flop_done / med / PEAK_F32_MATRIX, flop_needed / 1e12))
        if n == 512 and not args.calls_only:
            t = time.perf_counter()
            want = lr.search(u64, v64, min_gap=min_gap, k=1)
            t = time.perf_counter() - t
            cand = eng.loop_search(u, valid, min_gap=min_gap, k=1, dense=True)
            dd = cand[3].cpu().numpy()
            fin = np.isfinite(want["d"])
            say("%-44s %9.1f ms (float64, host, once)   largest |d - d64| over %d pairs %.3e" % ("tests/loops_ref.search, N = 512", 1e3 * t, int(fin.sum()),
                                                                                               float(np.abs(dd[fin] - want["d"][fin]).max())))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
