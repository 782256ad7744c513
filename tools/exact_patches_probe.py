#!/usr/bin/env python
"""exact_patches_probe.py [--rates] [--check] [--clutter 600] -- the fused path's exact-patches mode (caelo_extract mode bit 4) measured and checked.

--rates   frames/s of the pipeline (batch 8, certified RANSAC) on the boxes workload (mm-quantised, no tie-split patch: what a tie-free
          frame pays for the two-pass build, the census and the gated launches) for the default mode, exact_voxels and exact_patches,
          alternated in one process; then on `--clutter` clutter frames: exact_patches against the host-orchestrated redo
          (Pipeline.run + Engine.resolve_ties_many + Engine.match_pose_exact_many on the pairs touching a redone frame).
--check   every clutter frame through the exact mode: no flags & 2 left, the ties-left status bit (64) never set; for every frame with a redone
          patch: the rows equal the staged redo's (extract + resolve_ties) bit for bit, the staged redo's bits equal the oracle's
          (oracle.patches_bits on the reference's ordered lists, the logic of tools/tie_redo_check.py), the redone set is the oracle's
          tie-split set and the redone descriptors are within 1e-4 of the oracle encoder's on those bits."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "cae-lo_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _sync():
    import torch
    torch.cuda.synchronize()


def rates(eng, clutter, n_boxes=256, rounds=3):
    import torch
    from caelo import synth
    from caelo.engine import ransac_draws
    dev = eng.device
    pool = [torch.from_numpy(synth.make_scan(f, quantum=1e-3)).to(dev) for f in range(16)]
    pcs = [pool[i % 16] for i in range(n_boxes)]
    draws = [ransac_draws(1000 + i) for i in range(n_boxes)]
    rnd = [torch.from_numpy(d).to(dev) for d in draws]
    pipe = eng.pipeline(8, 3)
    modes = {"default": {}, "exact_voxels": {"exact_voxels": True}, "exact_patches": {"exact_patches": True}}
    for kw in modes.values():   # warm-up (allocations, code objects)
        pipe.run(pcs[:64], rnd[:64], certify=True, rands_host=draws[:64], **kw)
    _sync()
    res = {m: [] for m in modes}
    for _ in range(rounds):
        for m, kw in modes.items():
            _sync()
            t0 = time.perf_counter()
            pipe.run(pcs, rnd, certify=True, rands_host=draws, **kw)
            _sync()
            res[m].append(n_boxes / (time.perf_counter() - t0))
    print("boxes, %d frames per run, batch 8, certified; frames/s per round (alternated):" % n_boxes)
    for m in modes:
        print("  %-14s %s   median %.0f" % (m, " ".join("%.0f" % r for r in res[m]), np.median(res[m])))
    # clutter: exact mode against the host redo, chunks of 120 resident frames
    k = len(clutter)
    dcl = [torch.from_numpy(pc).to(dev) for pc in clutter]
    cdraws = [ransac_draws(2000 + i) for i in range(k)]
    crnd = [torch.from_numpy(d).to(dev) for d in cdraws]
    C = 120

    def host_chunk(lo, hi):
        a = pipe.run(dcl[lo:hi], crnd[lo:hi], certify=True, rands_host=cdraws[lo:hi])
        tied, _ = eng.redo_ties(a, hi - lo, lambda j: dcl[lo + j], lambda j: (crnd[lo + j], cdraws[lo + j]))   # (as run_sequence.py runs it)
        return len(tied)

    def exact_chunk(lo, hi):
        pipe.run(dcl[lo:hi], crnd[lo:hi], certify=True, rands_host=cdraws[lo:hi], exact_patches=True)
        return 0

    host_chunk(0, min(C, k)); exact_chunk(0, min(C, k)); _sync()   # warm-up
    out = {}
    for name, fn in (("host_redo", host_chunk), ("exact_patches", exact_chunk), ("host_redo", host_chunk), ("exact_patches", exact_chunk)):
        _sync()
        t0 = time.perf_counter()
        tied = sum(fn(lo, min(k, lo + C)) for lo in range(0, k, C))
        _sync()
        out.setdefault(name, []).append(k / (time.perf_counter() - t0))
        if name == "host_redo":
            print("  (host redo: %d tied frames)" % tied)
    print("clutter, %d frames in chunks of %d, batch 8, certified; frames/s:" % (k, C))
    for m, v in out.items():
        print("  %-14s %s" % (m, " ".join("%.0f" % r for r in v)))


def check(eng, clutter, first):
    import torch
    import oracle as orc
    wdir = os.path.join(REPO, "weights")
    models = orc.load_models(os.path.join(wdir, "SphericalRingPCRespondLayer.h5"), os.path.join(wdir, "EncoderModel4VoxelPatch.h5"))
    dev = eng.device
    n_redone_frames = n_redone = n_left = n_ties_left = n_row_bad = n_bits_bad = n_set_bad = n_desc_bad = 0
    t0 = time.time()
    for i, pc in enumerate(clutter):
        d = torch.from_numpy(pc).to(dev)
        ex = eng.extract(d, exact_patches=True)
        k = int(ex.n_key.item())
        fl = ex.flags[:k].cpu().numpy()
        st = int(ex.status[0].item())
        n_left += int(((fl & 2) != 0).sum())
        n_ties_left += int(bool(st & 64))
        if not (fl & 4).any():
            continue
        n_redone_frames += 1
        n_redone += int(((fl & 4) != 0).sum())
        ref = eng.extract(d)
        eng.resolve_ties(ref, d)
        _sync()
        if not (torch.equal(ex.rows, ref.rows) and torch.equal(ex.flags, ref.flags)):
            n_row_bad += 1
            print("frame %d: rows / flags differ from the staged redo" % (first + i), flush=True)
        # the staged redo's bits against the oracle (tools/tie_redo_check.py)
        mask = sum(1 << s for s in range(3) if (fl[:, s] & 4).any())
        vm, _ = eng.voxelize(d, eng.voxmap(max(eng.max_points, pc.shape[0]), slot=2))
        eng.voxmap_order(vm, mask)
        kp = ex.key_pts[:k].contiguous()
        bits, _ = eng.patches(vm, kp)
        gb = bits.cpu().numpy().view(np.uint64)
        v = orc.Voxelization(pc[:, 0:3])
        kph = kp.cpu().numpy()
        feats = ex.rows[:k, 0:60].cpu().numpy()
        for s in range(3):
            ob, of = orc.patches_bits(kph, v[6 + s], s)
            bad = np.flatnonzero((gb[:, s] != ob).any(axis=1))
            n_bits_bad += len(bad)
            for j in bad:
                print("frame %d key point %d scale %d: staged redo bits differ from the oracle's" % (first + i, j, s), flush=True)
            if not np.array_equal((fl[:, s] & 4) != 0, (of & 4) != 0):
                n_set_bad += 1
                print("frame %d scale %d: redone set differs from the oracle's tie-split set" % (first + i, s), flush=True)
            sel = np.flatnonzero(fl[:, s] & 4)
            if len(sel):
                want = models[1].predict_bits(ob[sel])
                got = feats[sel, 20 * s:20 * s + 20]
                rel = np.abs(got - want) / np.maximum(np.abs(want), 0.1)
                if (rel > 1e-4).any():
                    n_desc_bad += 1
                    print("frame %d scale %d: a redone descriptor is %.3g off the oracle's" % (first + i, s, rel.max()), flush=True)
        if n_redone_frames % 50 == 0:
            print("  %d frames, %d with redone patches, %d redone   %.0f s" % (i + 1, n_redone_frames, n_redone, time.time() - t0), flush=True)
    print("clutter frames %d..%d: %d frames with a redone patch, %d patches redone (flags & 4); flags & 2 left: %d; ties-left status bit: %d frames; "
          "rows / flags unequal to the staged redo: %d frames; staged redo bits unequal to the oracle's: %d patches; redone set unequal to the "
          "oracle's tie-split set: %d (frame, scale); redone descriptors beyond 1e-4 of the oracle's: %d (frame, scale)"
          % (first, first + len(clutter) - 1, n_redone_frames, n_redone, n_left, n_ties_left, n_row_bad, n_bits_bad, n_set_bad, n_desc_bad))
    return n_left + n_ties_left + n_row_bad + n_bits_bad + n_set_bad + n_desc_bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--clutter", type=int, default=600)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    import parity_soak as ps
    from caelo.engine import Engine
    t0 = time.time()
    clutter = ps.make_scans("clutter", a.clutter, workers=a.workers, first=a.first)
    print("%d clutter scans in %.0f s" % (len(clutter), time.time() - t0), flush=True)
    eng = Engine()
    bad = 0
    if a.rates:
        rates(eng, clutter)
    if a.check:
        bad = check(eng, clutter, a.first)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
