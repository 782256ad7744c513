#!/usr/bin/env python
"""Kernel times of the NN match at descriptor widths 60, 64, 128 and 256, 8 pairs of 1024 x 1024 per launch set.

    rocprofv3 --kernel-trace --stats -d /tmp/mw -o mw -- python tools/match_wide_time.py run [launches]
    python tools/match_wide_time.py report /tmp/mw/mw_results.db > profiles/wide_match_kernel_times.txt

`run`: uniform [-1, 1] descriptors of 9 frames, the 8 consecutive pairs through Engine.register_pairs(desc=) -- one match launch
set per call: k_match_prep + k_match_screen at 60, k_match_mfma at 64, k_match_prep_wide + k_match_screen_wide<nb> at 128 and 256 --
the widths taken in turn, `launches` (default 24) rounds after 3 of warm-up; then one more call per width with the statistics
words cleared, printed as "counters ...".  `report`: median and range per kernel from the trace (rocpd sqlite); a k_match_prep_wide
launch belongs to the width of the screen kernel that follows it."""
import os
import sqlite3
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (60, 64, 128, 256)


def run(launches):
    sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
    import numpy as np
    import torch
    import caelo
    caelo.configure_runtime()
    from caelo.engine import Engine, ransac_draws
    eng = Engine()
    rs = np.random.RandomState(1)
    rows = np.zeros((9, 1024, 64), np.float32)
    rows[:, :, 60:63] = rs.uniform(-40, 40, (9, 1024, 3))
    rows[:, :, 63] = 1.0
    rows = torch.from_numpy(rows).to(eng.device)
    nk = torch.full((9,), 1024, dtype=torch.int32, device=eng.device)
    desc = {d: torch.from_numpy(rs.uniform(-1, 1, (9, 1024, d)).astype(np.float32)).to(eng.device) for d in WIDTHS}
    table = [(i, i + 1) for i in range(8)]
    draws = np.stack([ransac_draws(i) for i in range(8)])
    for r in range(3 + launches):
        for d in WIDTHS:
            eng.register_pairs(rows, nk, table, draws, certify=False, desc=desc[d])
    for d in WIDTHS:
        ws = eng._ws("register_pairs_d%d" % d, int(eng.lib.caelo_register_pairs_ws_bytes_dim(8, d)))
        stride = (int(eng.lib.caelo_match_ws_bytes_dim(1024, d)) + 255) // 256 * 256
        for z in range(8):
            ws[z * stride:z * stride + 256].zero_()
        eng.register_pairs(rows, nk, table, draws, certify=False, desc=desc[d])
        torch.cuda.synchronize()
        st = np.array([ws[z * stride:z * stride + 8].view(torch.int32).cpu().numpy() for z in range(8)]).sum(axis=0)
        print("counters dim %3d: %d columns re-scanned exactly, %d decided among 2..8 rows, of %d" % (d, st[0], st[1], 8 * 1024))


def report(db_path):
    import statistics
    db = sqlite3.connect(db_path)
    rows = list(db.execute("select name, start, end from kernels where name like '%k_match_%' order by start"))
    groups = {}
    for i, (name, t0, t1) in enumerate(rows):
        short = name.split("(")[0]
        if "k_match_prep_wide" in short:
            nxt = rows[i + 1][0].split("(")[0] if i + 1 < len(rows) else "?"
            short = "k_match_prep_wide before " + nxt
        groups.setdefault(short, []).append((t1 - t0) / 1e3)
    print("%-72s %6s %10s %10s %10s" % ("kernel (8 pairs of 1024 x 1024 per launch)", "calls", "median_us", "min_us", "max_us"))
    for k in sorted(groups):
        v = groups[k][3:]      # (the warm-up rounds)
        print("%-72s %6d %10.2f %10.2f %10.2f" % (k[:72], len(v), statistics.median(v), min(v), max(v)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 24)
    else:
        report(sys.argv[2])
