#!/usr/bin/env python3
"""kp_eligible_share.py [--scene boxes|clutter] [--frames 0,7,16] [FILE.bin ...] -- how much of the front's response and score work
a scan's key point rule can use (CPU only: the oracle's projection and tests/kp_eligible_ref.py's restatement of the map).

Per scan and per ``dist_channels`` mode: the share of the centres of rows 8..55 that pass the range gate (SphericalRing.py:197-198),
the share of the 32-pixel response blocks of rows 6..57 that k_respond_mfma still computes, the share of the 4 x 64 score tiles
k_kp_score still stages, and the last row with an eligible pixel.  Without files the scans are bench.py's own pool (scan_at(i),
mm-quantised, the circuit trajectory); a .bin file is a KITTI velodyne scan ([n, 4] float32)."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "cae-lo_amd"):
    sys.path.insert(0, os.path.join(REPO, p))


def shares(ring, cnt, dist_c):
    import kp_eligible_ref as ker
    elig = ker.eligible(ring, cnt, dist_c)
    bits = ker.map_bits(elig)
    rows = np.nonzero(elig.any(axis=1))[0]
    return (elig[ker.ROW0:ker.ROW1].mean(), ker.needed_blocks(bits)[ker.RESP_ROW0:ker.RESP_ROW1].mean(), ker.live_tiles(bits).mean(),
            int(ker.needed_blocks(bits)[ker.RESP_ROW0:ker.RESP_ROW1].any(axis=1).sum()), int(rows[-1]) if len(rows) else -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help="KITTI velodyne .bin scans (default: the benchmark's synthetic pool)")
    ap.add_argument("--scene", choices=("boxes", "clutter"), default="boxes")
    ap.add_argument("--frames", default="0,7,16", help="pool indices of the synthetic scans")
    a = ap.parse_args()
    import oracle as orc
    from caelo import synth
    orc.build()
    if a.files:
        scans = [(os.path.basename(f), np.fromfile(f, dtype=np.float32).reshape(-1, 4)) for f in a.files]
    else:
        scans = [("%s %d" % (a.scene, i), synth.make_scan(i % synth.CIRCUIT_PERIOD, seed=i, trajectory="circuit", quantum=1e-3, scene_kind=a.scene))
                 for i in (int(t) for t in a.frames.split(","))]
    print("%-24s %6s %17s %22s %12s %13s" % ("scan", "dist_c", "eligible centres", "response blocks (rows)", "score tiles", "last elig. row"))
    for name, pc in scans:
        ring, cnt = orc.ProjectPC2SphericalRing(pc)
        for dist_c in (5, 3):
            e, b, t, nrows, last = shares(ring, cnt, dist_c)
            print("%-24s %6d %17.3f %15.3f (%2d/52) %12.3f %13d" % (name, dist_c, e, b, nrows, t, last))


if __name__ == "__main__":
    main()
