#!/usr/bin/env python
"""run_sequence.py -- the counterpart of the reference's PoseEstimation.py loop on libcaelo (SURVEY.md 8c harness row,
8f-1): consecutive scans -> per-pair relative pose (R, T, nInliers, thr) -> chained KITTI poses [F,12] -> poses file.

    python run_sequence.py --synthetic 20 --out poses_/00.txt
    python run_sequence.py --scans <seq>/velodyne --calib <calib>/00/calib_.txt --out poses_/00.txt --save-artifacts
    python run_sequence.py --scans <raw KITTI seq>/velodyne --calib-angle 0.22 --out poses_/00.txt   # CorrectPC on the fly
    python run_sequence.py --scans <seq>/velodyne --frame-steps 1,5,10 --out poses_/00.txt   # + poses_/5_00.txt, poses_/10_00.txt, one extraction pass
    python run_sequence.py --desc-dir <usip desc>/00 --desc-dim 128 --keypts-source usip --keypts-dir <usip keypts>/00 --out poses_/00.txt
    python run_sequence.py --desc-dir <usip desc>/00 ... --registrar comparison --matchability m/00.mat   # the published comparison's registrar
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 run_sequence.py --synthetic 800 ...

Frames are sharded contiguously over the ranks (one process per GPU); every rank runs its frames through the
native pipeline, ONE all-gather moves the boundary frame rows, pose rows are gathered to rank 0, which chains
them on the host (PoseEstimation.py:253-267) and writes `np.savetxt` rows like PoseEstimation.py:277.

RANSAC draws: the reference uses NumPy's unseeded global generator (Match.py:182); here pair (i, i+1) consumes
RandomState(seed_base + i).random_sample(...), so results do not depend on sharding or chunking.
"""
import argparse
import glob
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from caelo import _ffi, framesteps, stageio, synth  # noqa: E402
import caelo  # noqa: E402
caelo.configure_runtime()  # this script owns its process: before HIP starts (the queue count is left to the caller)
from caelo import dist as cdist  # noqa: E402
from caelo.engine import ENCODER_H5, RESPOND_H5, Engine, FrameBatch, FrameFeatures, note_ties_left, raise_status, ransac_draws  # noqa: E402


def _host_times(host_times):
    ht = host_times if host_times is not None else {}   # seconds per host activity (what a "frames/s incl. loading" figure is made of)
    for k_ in ("load", "pin", "draws", "starved", "pipeline", "ties", "parse", "setup"):
        ht.setdefault(k_, 0.0)
    return ht


def _parse_poses(raw, k):
    """Pose results without per-frame Python: the raw bytes viewed as the record type of caelo_pose_result -> rel_rt [k,12],
    success, threshold, n_inliers."""
    r = np.frombuffer(raw[:k].tobytes(), dtype=_ffi.POSE_DTYPE, count=k)
    out = np.concatenate([r["R"].reshape(k, 9), r["T"].reshape(k, 3)], axis=1).astype(np.float32)
    return out, r["success"] != 0, r["threshold"].astype(np.float32), r["n_inliers"].astype(np.int32)


def _parse_records(raw, k):
    """The RANSAC records --matchability keeps: iterations (cntIters of the last level) and n_pairs, [k] i32 each."""
    r = np.frombuffer(raw[:k].tobytes(), dtype=_ffi.POSE_DTYPE, count=k)
    return r["iterations"].astype(np.int32), r["n_pairs"].astype(np.int32)


def _run_chunks(eng, lo, hi, chunk, submit, ht, t_setup, keep, host_redo, tie_log, certify, records=None):
    """The chunk loop of run_local and run_local_files: frames [lo, hi) in chunks of ``chunk``.  ``submit(ci, c0, c1, prev)`` issues
    chunk ci = frames [c0, c1) (frame c0 matched against ``prev``) -> (FrameBatch, exact_on_host, scan(j), draws(j)): with
    ``exact_on_host`` the certified poses are read from ``batch.exact`` (Pipeline.run_loaded(publish=False)), else from the device;
    ``scan`` and ``draws`` fetch a tied frame's scan and a pair's draws again for the host redo (Engine.redo_ties).
    The poses and status words of chunk c come back through pinned buffers on a side stream and are parsed after chunk c + 1 has
    been issued.  Returns what run_local returns; ``records`` (a list) receives (iterations, n_pairs) per chunk."""
    import gc
    gc.collect()
    gc.freeze()       # what exists now is never scanned again: a full collection of this process (40-90 ms) no longer lands between two batches
    side = torch.cuda.Stream(device=eng.device)
    ht["setup"] = time.time() - t_setup
    rel, ok, thr, nin = [], [], [], []
    prev, first = None, None
    pending = None   # (k, has_prev, host poses, pinned status, event)
    back = []

    def collect(p):
        k, has_prev, res_h, st_h, ev = p
        ev.synchronize()
        t_ = time.time()
        st = st_h.numpy()[:k, 0]
        if st.any():
            for v in st[st != 0]:
                raise_status(int(v))
            note_ties_left(eng, st)
        r, o, t, n = _parse_poses(res_h, k)
        s = 0 if has_prev else 1                                   # slot 0 of the first chunk has no predecessor here
        rel.append(r[s:]); ok.append(o[s:]); thr.append(t[s:]); nin.append(n[s:])
        if records is not None:
            its, nps = _parse_records(res_h, k)
            records.append((its[s:], nps[s:]))
        ht["parse"] += time.time() - t_

    t_loop = time.time()
    for ci, c0 in enumerate(range(lo, hi, chunk)):
        c1 = min(hi, c0 + chunk)
        k = c1 - c0
        batch, exact_on_host, scan, draws = submit(ci, c0, c1, prev)
        t_ = time.time()
        if host_redo:
            # Frames whose 496-nearest cut (Voxel.py:195-196) splits a class of equidistant voxels: the fused path's canonical rule is
            # replaced by scikit-learn's kd-tree order, then the pairs such a frame is part of are matched again.  One synchronisation
            # per chunk; rare (none on KITTI-shaped scans).
            tied, n_t = eng.redo_ties(batch, k, scan, draws, prev=prev, certify=certify)
            if tie_log is not None:
                tie_log.extend((c0 + j, n_) for j, n_ in zip(tied, n_t))
        ht["ties"] += time.time() - t_
        # read this chunk's small outputs back without stalling the stream that issues the next chunk
        done = torch.cuda.Event()
        done.record()
        if not back:   # pinned read-back buffers, allocated once (three: one being parsed, one in flight, one being issued)
            for _i in range(3):
                back.append((torch.empty((min(chunk, hi - lo),) + tuple(batch.result.shape[1:]), dtype=batch.result.dtype, pin_memory=True),
                             torch.empty((min(chunk, hi - lo),) + tuple(batch.status.shape[1:]), dtype=batch.status.dtype, pin_memory=True)))
        res_h, st_h = back[ci % 3]
        with torch.cuda.stream(side):
            side.wait_event(done)
            if not exact_on_host:
                res_h[:k].copy_(batch.result[:k], non_blocking=True)
            st_h[:k].copy_(batch.status[:k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        if pending is not None:
            collect(pending)
        pending = (k, prev is not None, batch.exact[0][:k].copy() if exact_on_host else res_h.numpy(), st_h, ev)
        if first is None:
            first = FrameFeatures.from_rows(batch.rows[0].clone())      # (a loader may reuse the chunk's buffers)
        prev = FrameFeatures.from_rows(batch.rows[k - 1].clone())
        if keep is not None:
            keep(c0, batch.view(0, k))
        del batch, scan, draws      # (back to the caching allocator before the next chunk asks for the same sizes)
    ht["loop"] = time.time() - t_loop
    if pending is not None:
        collect(pending)
    cat = (lambda xs, d: np.concatenate(xs) if xs else np.zeros((0,) + d))
    return cat(rel, (12,)), cat(ok, ()), cat(thr, ()), cat(nin, ()), first, prev


def _corrected(eng, scan, calib_angle):
    """A tied frame's scan for the host redo (Engine.redo_ties): corrected like the pipeline corrected it."""
    return scan if calib_angle is None else eng.correct_pc(scan, calib_angle)


def run_local(eng, load, lo, hi, seed_base, chunk, dist_channels, batch_frames, keep=None, strict_ties=True, tie_log=None, host_times=None,
              loader_threads=4, certify=True, native_ties=False, given=None, records=None, calib_angle=None):
    """Frames [lo, hi) of this rank.  Returns per-pair rows for pairs (i-1, i), i in (lo, hi) -- the pair (lo-1, lo)
    is the caller's (it needs the previous rank's last frame) -- plus the first and last frame's features.

    Three things overlap, as in the reference's producer / consumer split (PoseEstimation.py:214-245, where a generator process
    prepares frame i + 1 while the main loop matches frame i):
      * a loader thread reads (or synthesises) the scans and RANSAC draws of chunk c + 1 into pinned host memory;
      * inside a chunk, a copy stream uploads batch b + 4 while the pipeline works on batch b (Pipeline.run_uploading, paced by this thread);
      * the poses and status words of chunk c come back through pinned buffers on a side stream and are parsed after chunk
        c + 1 has been issued.
    ``native_ties``: the pipeline redoes tie-split patches itself (Pipeline.run_uploading(exact_patches=True)): no host redo, no re-match.
    ``given(i)`` -> ('keypts', [K,3] f32) | ('rows', [K,64] f32): frame i's key points or rows of another source (PoseEstimation.py:26-66,
    caelo.keysources); the chunk then goes through Pipeline.run on resident scans (keypts= / rows_given=), with the tie-split patches
    redone inside the pipeline unless ``strict_ties`` is off.
    ``records``: a list that receives each chunk's (iterations, n_pairs) [k] i32, the pairs in the order of the returned rows.
    ``calib_angle``: degrees; every scan is corrected on the device inside its batch (Pipeline.run(calib_angle=...)); given key points
    and rows are not.
    """
    import queue
    import threading
    t_setup = time.time()
    if given is not None:
        native_ties = native_ties or strict_ties
    chunks = [(c0, min(hi, c0 + chunk)) for c0 in range(lo, hi, chunk)]
    q = queue.Queue(maxsize=2)

    pinned = {}   # a scan served twice (--pool) is pinned once

    def pin(a):
        t = pinned.get(id(a))
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).pin_memory()
            if getattr(load, "repeats", False):
                pinned[id(a)] = t
        return t

    ht = _host_times(host_times)

    # The loader works with a few threads (file reads, NumPy's Mersenne Twister and the ray caster all release the GIL for most of
    # their time) and fills pinned buffers that are allocated once: a pinned allocation per chunk cost more than the copy it serves.
    from concurrent.futures import ThreadPoolExecutor
    n_thr = max(1, loader_threads)
    workers = ThreadPoolExecutor(max_workers=n_thr)
    draw_ring = [torch.empty((min(chunk, hi - lo), 6000), dtype=torch.float64, pin_memory=True) for _ in range(4)]   # queue of 2 + one in use + one being filled

    # Scans that come from files are read STRAIGHT into pinned slots that are allocated once and reused every fourth chunk (the queue
    # holds two chunks, one is in use, one is being filled): page-locking a fresh 2 MB buffer per scan cost 1.4 ms, three times the
    # read itself, and a copy on top.  (A source without `into` -- the synthetic pool -- is pinned per distinct scan as before.)
    ring_slots = {}
    cap = int(eng.max_points)

    ring_lock = threading.Lock()

    def pinned_slot(ci, j):
        # one pinned block per BATCH of a ring position, frame j at a fixed pitch inside it: the scans of a batch are contiguous and go
        # up behind ONE copy command (Pipeline.run_uploading detects the pitch; eight commands per batch cost the pipeline 20 %).
        # Allocated by whichever loader thread gets there first (page-locking 20 MB takes milliseconds: not under a common lock).
        key = (ci % 4, j // batch_frames)
        with ring_lock:
            lk = ring_slots.setdefault(("lock",) + key, threading.Lock())
        with lk:
            blk = ring_slots.get(key)
            if blk is None:
                blk = ring_slots[key] = torch.empty((batch_frames, cap, 4), dtype=torch.float32, pin_memory=True)
        return blk[j % batch_frames]

    def loader():
        try:
            for ci, (c0, c1) in enumerate(chunks):
                t_ = time.time()
                draws = draw_ring[ci % len(draw_ring)][:c1 - c0]
                dn = draws.numpy()

                def fill(j):
                    dn[j] = ransac_draws(seed_base + c0 + j - 1)
                drawn = [workers.submit(fill, j) for j in range(c1 - c0)]   # (beside the reads: both release the GIL for most of their time)
                if hasattr(load, "into"):
                    scans = list(workers.map(lambda j: load.into(c0 + j, pinned_slot(ci, j), pin), range(c1 - c0)))
                    t1_ = t2_ = time.time()
                else:
                    raw = list(workers.map(load, range(c0, c1)))
                    t1_ = time.time()
                    scans = [pin(a) for a in raw]
                    t2_ = time.time()
                for f_ in drawn:
                    f_.result()
                ht["load"] += t1_ - t_; ht["pin"] += t2_ - t1_; ht["draws"] += time.time() - t2_   # (draws: what was left of them after the scans)
                q.put((c0, c1, scans, draws))
        except BaseException as e:   # surfaced in the consumer
            q.put(e)

    threading.Thread(target=loader, daemon=True).start()
    # (the loader is already at work on the first chunks while the pipeline's buffers are allocated)
    pipe = eng.pipeline(batch_frames)

    def submit(ci, c0, c1, prev):
        t_ = time.time()
        item = q.get()
        ht["starved"] += time.time() - t_
        if isinstance(item, BaseException):
            raise item
        _, _, scans, draws = item
        t_ = time.time()
        k = c1 - c0
        draws_d = draws.to(eng.device, non_blocking=True)
        # certify: the exact RANSAC (the pipeline's certifier thread runs the host half on every pair while later batches are on the
        # GPU; the call returns when this chunk's inlier sets and poses -- the reference's bits -- are in batch.result / inlier_mask)
        dn = draws.numpy()
        rands = [draws_d[i] for i in range(k)]
        rands_host = [dn[i] for i in range(k)] if certify else None
        if given is not None:   # other key point sources: resident scans, the sources' inputs written into the batch by Pipeline.run
            gv = [given(c0 + j) for j in range(k)]
            kp = [a if kind == "keypts" else None for kind, a in gv]
            rw = [a if kind == "rows" else None for kind, a in gv]
            batch = pipe.run([None if rw[j] is not None else scans[j].to(eng.device, non_blocking=True) for j in range(k)], rands, prev=prev,
                             dist_channels=dist_channels, certify=certify, rands_host=rands_host, exact_patches=native_ties, keypts=kp, rows_given=rw,
                             calib_angle=calib_angle)
        else:
            batch = pipe.run_uploading(scans, rands, prev=prev, dist_channels=dist_channels, certify=certify, rands_host=rands_host,
                                       exact_patches=native_ties, calib_angle=calib_angle)
        ht["pipeline"] += time.time() - t_
        return batch, False, lambda j: _corrected(eng, scans[j].to(eng.device), calib_angle), lambda j: (draws_d[j], dn[j])

    return _run_chunks(eng, lo, hi, chunk, submit, ht, t_setup, keep, strict_ties and not native_ties, tie_log, certify, records)


def run_local_files(eng, files, lo, hi, seed_base, chunk, dist_channels, batch_frames, keep=None, strict_ties=True, tie_log=None, host_times=None,
                    loader_threads=16, certify=True, device_results=False, native_ties=False, records=None, calib_angle=None):
    """run_local for scans that are FILES (round 6): the native loader (caelo_seqloader: pread into a pinned ring + the RANSAC draws,
    csrc/seqload.hip) works ahead on its own threads, a chunk of batches goes through Pipeline.run_loaded (one copy command per batch
    for scans and draws, jobs built column-wise).  Same returns as run_local; same bits (the draws are NumPy's stream, the pipeline
    is the same).  ``calib_angle``: as in run_local (the correction runs on the device slot, after the batch's copy has landed)."""
    from caelo.engine import SeqLoader
    t_setup = time.time()
    ht = _host_times(host_times)
    B = batch_frames
    # a ring slot holds the LARGEST scan of this rank's files, not the engine's capacity: a batch goes up as one copy of the whole slot, and
    # what the copy engine moves beside the pipeline is what the upload mode costs (20.5 MB per batch at 160 000 points, 16.2 MB at 126 k)
    biggest = max(os.path.getsize(f_) for f_ in files[lo:hi]) // 16
    assert biggest <= eng.max_points, "a scan holds %d points, the engine was created for %d" % (biggest, eng.max_points)
    cap = min(int(eng.max_points), (int(biggest) + 1023) // 1024 * 1024)
    # (page-locking the ring takes tens of milliseconds: on a thread of its own, beside the allocation of the pipeline's buffers)
    import threading
    box = {}

    def make_loader():
        try:
            box["loader"] = SeqLoader(eng, files[lo:hi], first_frame=lo, batch=B, seed_base=seed_base, threads=loader_threads, ring=7, cap=cap)
        except BaseException as e:
            box["error"] = e
    th = threading.Thread(target=make_loader)
    th.start()
    pipe = eng.pipeline(B)
    th.join()
    if "error" in box:
        raise box["error"]
    loader = box["loader"]
    per_chunk = max(1, chunk // B)
    outs = [FrameBatch(eng, per_chunk * B) for _ in range(2)]
    # certified runs: the exact results are written by the host half into host arrays (batch.exact) -- they are read THERE, not
    # published to the device and copied back (publish=False: 51 ms of 0.40 s for 4 541 frames)
    # (device_results -- the artefact writer reads masks and pair indices from the device tensors -- publishes them as before)
    publish = device_results or not certify

    def submit(ci, c0, c1, prev):
        t_ = time.time()
        batch, _ = pipe.run_loaded(loader, (c0 - lo) // B, (c1 - c0 + B - 1) // B, prev=prev, out=outs[ci % 2], dist_channels=dist_channels,
                                   certify=certify, publish=publish, exact_patches=native_ties, calib_angle=calib_angle)
        ht["pipeline"] += time.time() - t_
        t = pipe.last_upload_times   # (ms; this report is in seconds)
        ht["starved"] += t["starved_ms"] / 1e3
        for k_, v_ in t.items():
            ht["loaded_" + k_[:-3] + "_s"] = ht.get("loaded_" + k_[:-3] + "_s", 0.0) + v_ / 1e3

        def scan(j):   # (a tied frame's scan is read again: rare)
            return _corrected(eng, torch.from_numpy(stageio.read_scan(files[c0 + j])).to(eng.device), calib_angle)

        def draws(j):
            d = ransac_draws(seed_base + c0 + j - 1)
            return torch.from_numpy(d).to(eng.device), d
        return batch, not publish, scan, draws

    out = _run_chunks(eng, lo, hi, per_chunk * B, submit, ht, t_setup, keep, strict_ties and not native_ties, tie_log, certify, records)
    ls = loader.stats()
    ht["load"], ht["draws"] = ls["read_s"], ls["draws_s"]      # (summed over the loader's threads)
    loader.close()
    return out


def run_desc(eng, src, n, seed_base, chunk, steps, certify, registrar=None, calib_angle=None):
    """--desc-dir: the pair stage alone on descriptors of another method (caelo.keysources.DescSource; no scan is read, nothing is
    extracted).  Frames [0, n) chunk by chunk: a chunk's key points and descriptors become rows [k,1024,64] (xyz 60:63 | valid 63,
    columns 0:60 zero and unread) and desc [k,1024,D]; ONE Engine.register_pairs(..., desc=) call registers the consecutive pairs
    (i - 1, i) whose frame i the chunk holds and the pairs of every other step whose frame 1 it holds (framesteps.chunk_pairs), the
    last max(steps) frames being carried from chunk to chunk.  Pair k of a step draws RandomState(seed_base + k), as in every other
    run.  ``registrar`` = (draws, threshold): the comparison protocol's registrar instead (Engine.register_pairs_adaptive; every pair
    consumes the same draws); ``calib_angle`` then corrects the key points of sources other than the auto-encoder's on the device
    (GenerateTrajactory.m:186-190).  -> {step: framesteps.pack_results(...)}."""
    order = [1] + [s for s in steps if s != 1]
    stepper = framesteps.StepRegistrar(eng, order, seed_base, certify, 0, registrar=registrar, step_one=True)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        rows = np.zeros((c1 - c0, 1024, 64), np.float32)
        desc = np.zeros((c1 - c0, 1024, src.dim), np.float32)
        nk = np.zeros(c1 - c0, np.int32)
        for j in range(c1 - c0):
            pts, d = src.frame(c0 + j)
            k = pts.shape[0]
            if k < 1:
                raise ValueError("frame %d has no key points" % (c0 + j))
            rows[j, :k, 60:63], rows[j, :k, 63], desc[j, :k], nk[j] = pts, 1.0, d, k
        rows, desc, nk = (torch.from_numpy(a).to(eng.device) for a in (rows, desc, nk))
        if calib_angle is not None and src.keypts_source != "ae":   # (a padding row's origin would turn into NaN: it stays zero)
            moved = eng.correct_pc(rows[:, :, 60:63].reshape(-1, 3).contiguous(), calib_angle).view(-1, 1024, 3)
            rows[:, :, 60:63] = torch.where(rows[:, :, 63:64] > 0, moved, torch.zeros_like(moved))
        stepper.push(c0, rows, nk, desc)
    return {s: stepper.step_results(s) for s in order}


def _write_step(args, s, n, Tr, rel, ok, nin, npairs, its, what="", say=True):
    """A step's files and its summary line: the poses chained through Tr (one row per input frame for s != 1, framesteps.expand_rows)
    at framesteps.step_path(--out, s), --matchability (it needs npairs and its) under the same prefix."""
    assert len(rel) == len(framesteps.step_pairs(n, s)), "step %d: %d pairs registered, %d scheduled" % (s, len(rel), len(framesteps.step_pairs(n, s)))
    poses = stageio.chain_poses(rel, Tr)
    stageio.write_poses(framesteps.step_path(args.out, s), poses if s == 1 else framesteps.expand_rows(poses, n, s))
    if args.matchability:
        from caelo import evaluate as ev
        ev.save_matchability(framesteps.step_path(args.matchability, s), nin, npairs, its)
    if say:
        print("step %d: %d pairs (%d solved)%s -> %s" % (s, len(rel), int(np.sum(ok)), what, framesteps.step_path(args.out, s)))


def _registrar(args):
    """--registrar: None for Match.py's RANSAC4RT, (draws [10001,3], threshold) for the comparison protocol's ransacfitRt.m."""
    if args.registrar != "comparison":
        return None
    from caelo import adaptive
    return adaptive.draw_table(args.draw_seed), float(args.inlier_threshold)


def main_desc(args, ap, steps):
    """The --desc-dir run (one GPU): the files every other run writes, under the same names."""
    from caelo import keysources
    if args.gpus > 1:
        ap.error("--desc-dir runs on one GPU (--gpus %d): a pair table of a whole sequence takes seconds; sharding it is not implemented" % args.gpus)
    if args.scans or args.synthetic or args.save_artifacts or (args.calib_angle is not None and args.registrar != "comparison"):
        ap.error("--desc-dir reads no scans: --scans, --synthetic, --save-artifacts and --calib-angle do not go with it "
                 "(--registrar comparison takes --calib-angle: it corrects the key points of --keypts-source 3dfeatnet|usip)")
    if args.calib_angle is not None and not np.isfinite(args.calib_angle):
        ap.error("--calib-angle must be a finite number of degrees")
    src = keysources.DescSource(args.desc_dir, args.desc_dim, args.keypts_source, args.keypts_dir, args.features_from)
    n = src.n_frames()
    if n < 2:
        raise ValueError("--desc-dir %s: need at least frames 0 and 1 (%s, %s)" % (args.desc_dir, keysources.desc_path(args.desc_dir, 0), keysources.desc_path(args.desc_dir, 1)))
    if not (0 <= args.seed_base and args.seed_base + n - 2 < 2 ** 32):
        ap.error("--seed-base %d: the seeds seed_base + i - 1 of pairs i = 1 .. %d must lie in [0, 2^32)" % (args.seed_base, n - 1))
    if framesteps.carry_frames(steps) > n:
        ap.error("--frame-steps %s: the largest step exceeds the %d frames" % (args.frame_steps, n))
    eng = Engine(device=0)
    Tr = stageio.read_calib_tr(args.calib) if args.calib else None
    t0 = time.time()
    res = run_desc(eng, src, n, args.seed_base, args.chunk, steps, not args.no_certify, _registrar(args), args.calib_angle)
    dt = time.time() - t0
    for s_, r in res.items():
        _write_step(args, s_, n, Tr, *r, what=" on %d-d descriptors" % src.dim)
    print("%d frames in %.2f s (reading key points and descriptors included)" % (n, dt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic 64x2000 scans (caelo.synth)")
    ap.add_argument("--quantum", type=float, default=0.0, help="round the synthetic coordinates to multiples of this (m), e.g. 0.001")
    ap.add_argument("--scans", help="directory of KITTI velodyne .bin files")
    ap.add_argument("--calib", help="calib_.txt (PoseEstimation.py:199-203) or KITTI calib.txt; identity if omitted")
    ap.add_argument("--out", default="poses_/00.txt")
    ap.add_argument("--seed-base", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=960, help="frames resident on the GPU at a time (the rows of a chunk: 0.26 MB per frame)")
    ap.add_argument("--dist-channels", type=int, default=5, choices=(3, 5), help="5 = demo mode, 3 = batch mode (SURVEY 8a-3')")
    ap.add_argument("--batch", type=int, default=8, help="frames per launch (caelo_pipeline)")
    ap.add_argument("--scene", default="boxes", choices=("boxes", "clutter"), help="synthetic scene (caelo.synth)")
    ap.add_argument("--trajectory", default="circuit", choices=synth.TRAJECTORIES,
                    help="synthetic sensor path (caelo.synth.sensor_pose): 'circuit' = a periodic world with structure at every frame index; "
                         "'line' = the law of the goldens, which leaves the scene after ~150 frames")
    ap.add_argument("--pool", type=int, default=0, help="synthesise only this many distinct scans and walk them back and forth (0 1 .. P-1 "
                                                        "P-2 .. 0 1 ..: every pair stays a pair of neighbours); ray casting a scan costs ~0.5 s of CPU")
    ap.add_argument("--loader-threads", type=int, default=min(16, os.cpu_count() or 1), help="threads that read / synthesise scans and draw RANSAC's random numbers")
    ap.add_argument("--python-loader", action="store_true", help="--scans through round 5's Python loader threads instead of the native loader (caelo_seqloader)")
    ap.add_argument("--save-artifacts", action="store_true", help="write Features/*.mat and InliersIdx/*.mat next to the scans")
    ap.add_argument("--matchability", help="write the per-pair RANSAC inlier proportions (n_inliers / n_pairs) and trial counts (cntIters) "
                                           "here, in frame order: AllProportions / AllTrialCounts [1, n] (evaluate.py registration)")
    ap.add_argument("--no-strict-ties", action="store_true", help="keep the fused path's canonical rule where the 496-nearest cut splits a "
                                                                  "tie class (default: such frames are redone in scikit-learn's kd-tree order)")
    ap.add_argument("--native-ties", action="store_true", help="the pipeline redoes tie-split patches itself in scikit-learn's order "
                                                               "(CAELO_EXTRACT_EXACT_PATCHES): no host redo and re-match; same results")
    ap.add_argument("--no-certify", action="store_true", help="the kernels' own RANSAC results (float64 fits) without the host half that makes "
                                                              "inlier sets and poses the reference's bits (csrc/certify.hip)")
    ap.add_argument("--keypts-source", default="ae", choices=("ae", "3dfeatnet", "usip"),
                    help="key points of the pair loop (PoseEstimation.py iKeyPtSource 0 / 1 / 2): the auto-encoder detector, or the files "
                         "<keypts-dir>/<frame:06d>.bin of 3DFeatNet ([-1, 35] f32) or USIP ([-1, 3] f32, rotated by R90; float32 after "
                         "the rotation); at most 1024 per frame (larger sets: the staged API)")
    ap.add_argument("--keypts-dir", help="directory of the --keypts-source files")
    ap.add_argument("--features-from", help="directory of <frame:06d>.bin.mat files (KeyPts / Features / Weights, isLoadFeaturesFromFile, "
                                            "PoseEstimation.py:49-66): only the pair stage runs on them")
    ap.add_argument("--desc-dir", help="register on descriptors of another method: <desc-dir>/<frame:06d>.bin, [-1, --desc-dim] f32 (the published "
                                       "comparison's layout, GenerateTrajactory.m:193-197), up to 256 wide.  Key points: --keypts-source 3dfeatnet|usip "
                                       "with --keypts-dir, or the KeyPts of --features-from files (their Features are ignored).  No scans are read; "
                                       "only the pair stage runs (Engine.register_pairs(desc=)), with the seeds, --frame-steps, --matchability, "
                                       "--no-certify and --out naming of every other run.  One GPU")
    ap.add_argument("--desc-dim", type=int, default=None, help="width of the --desc-dir descriptors (e.g. 128 for USIP, 32 for 3DFeatNet)")
    ap.add_argument("--calib-angle", type=float, default=None, metavar="DEG",
                    help="correct every scan by the reference's CorrectPC (Transformations.py:28-39: each point rotated by DEG degrees about "
                         "p x z, the HDL-64E's vertical-angle calibration; raw KITTI scans: 0.22) on the device, inside the batch launch, before "
                         "anything else reads it -- no corrected copy of the data set on disk.  Default: no correction.  Only scans are "
                         "corrected, as in the reference: key points given by --keypts-source / --features-from are used as they are")
    ap.add_argument("--frame-steps", default="1", metavar="S[,S...]",
                    help="also register the sequence at these frame steps, from the rows of the ONE extraction pass: step s pairs scan k*s with "
                         "scan (k+1)*s (the reference's GenerateTrajactory.m:124-126), pair k drawing RandomState(seed_base + k) -- what a plain "
                         "run over every s-th scan computes.  Step 1 is the pipeline's run and is always written to --out; every other step s "
                         "is registered with Engine.register_pairs on the chunk's resident rows (the last max(S) frames' rows are carried "
                         "from chunk to chunk) and written to --out with '<s>_' in front of its file name: one row per input frame, the "
                         "multiples of s holding the pose chained through Tr, the frames in between repeating the preceding multiple's row.  "
                         "(The reference's MATLAB writer cannot be run here: the in-between rows are this project's choice; evaluate.py "
                         "--frame-step s reads the multiples only.)  --matchability M gets the same prefix per step.  With --gpus > 1 a rank "
                         "registers the step pairs whose frame 0 it owns: its halo is the next rank's first max(S) frames' rows (one more "
                         "all-gather), and every rank needs at least max(S) frames")
    ap.add_argument("--registrar", default="match", choices=("match", "comparison"),
                    help="how a pair is registered.  match (default): Match.py's RANSAC4RT -- for each key point of frame 1 the nearest descriptor "
                         "of frame 0, 4-point samples, 500 trials per threshold level.  comparison: the protocol behind the reference's published "
                         "table (Scripts/GenerateTrajactory.m -> External/ransacfitRt.m): for each key point of frame 0 the nearest descriptor of "
                         "frame 1, 3-point samples, a quaternion fit, ONE inlier threshold, an adaptive trial count (p = 0.99, at least 100, "
                         "the identity after 10 000) and a refit on the inliers; a pair that fails repeats the motion of the pair before it; "
                         "--matchability then holds n_inliers / n_pairs and the trial counts of that protocol.  Every pair consumes the same "
                         "draws (--draw-seed).  On the pipeline path the pairs of every step, step 1 included, are registered from the "
                         "resident rows (Engine.register_pairs_adaptive).  One GPU; not with --save-artifacts")
    ap.add_argument("--inlier-threshold", type=float, default=1.0, metavar="M", help="--registrar comparison: the inlier distance in metres (the script's 1.0)")
    ap.add_argument("--draw-seed", type=int, default=0, help="--registrar comparison: RandomState(seed) gives the 10 001 x 3 uniform doubles of the trials")
    ap.add_argument("--encoder-h5", metavar="PATH", help="the patch encoder's Keras .h5 instead of the shipped EncoderModel4VoxelPatch.h5: a bare "
                    "encoder or a full autoencoder (its encoder half is taken), tanh or relu hidden layers, tanh or linear code -- "
                    "e.g. what the reference's AE4VoxelPatch.py trains.  Every rank loads it")
    ap.add_argument("--respond-h5", metavar="PATH", help="the response layer's Keras .h5 instead of the shipped SphericalRingPCRespondLayer.h5")
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")),
                    help="ranks = GPUs; without a launcher the script starts them itself (caelo.dist.ensure_ranks)")
    args = ap.parse_args()
    # the model files are parsed (layer stack, activations, shapes) before any device work; the engines load them below
    for opt, path, kind in (("--encoder-h5", args.encoder_h5, "encoder"), ("--respond-h5", args.respond_h5, "respond")):
        if path:
            from caelo import keras_config
            try:
                got = keras_config.read_model(path)[0]
            except (OSError, KeyError, ValueError) as e:
                ap.error("%s %s: %s" % (opt, path, e))
            if got != kind:
                ap.error("%s %s holds the %s network" % (opt, path, "response" if got == "respond" else "encoder"))
    if args.registrar == "comparison":
        if args.gpus > 1 or args.save_artifacts:
            ap.error("--registrar comparison runs on one GPU and writes no Features / InliersIdx artefacts (--gpus %d%s)"
                     % (args.gpus, ", --save-artifacts" if args.save_artifacts else ""))
        if not (args.inlier_threshold > 0.0 and np.isfinite(args.inlier_threshold)):
            ap.error("--inlier-threshold must be a positive number of metres")
        if not 0 <= args.draw_seed < 2 ** 32:
            ap.error("--draw-seed %d: RandomState takes seeds in [0, 2^32)" % args.draw_seed)
    if args.desc_dir or args.desc_dim is not None:
        if not args.desc_dir:
            ap.error("--desc-dim goes with --desc-dir")
        if args.encoder_h5 or args.respond_h5:
            ap.error("--desc-dir reads descriptors from files: no network runs, --encoder-h5 / --respond-h5 do not go with it")
        try:
            return main_desc(args, ap, framesteps.parse_steps(args.frame_steps))
        except ValueError as e:
            ap.error(str(e))
    # pair (i - 1, i) draws RandomState(seed_base + i - 1), which takes seeds in [0, 2^32): both loaders refuse a base that leaves it
    # for any frame with a pair (frame 0 has none) -- before any device work, the same way whichever loader would run
    n_frames = len(glob.glob(os.path.join(args.scans, "*.bin"))) if args.scans else args.synthetic
    if n_frames >= 2 and not (0 <= args.seed_base and args.seed_base + n_frames - 2 < 2 ** 32):
        ap.error("--seed-base %d: the seeds seed_base + i - 1 of pairs i = 1 .. %d must lie in [0, 2^32)" % (args.seed_base, n_frames - 1))

    try:
        steps = framesteps.parse_steps(args.frame_steps)
    except ValueError as e:
        ap.error("--frame-steps: %s" % e)
    if n_frames and framesteps.carry_frames(steps) and n_frames // max(1, args.gpus) < framesteps.carry_frames(steps):
        ap.error("--frame-steps %s on %d GPUs: every rank needs at least max(steps) = %d of the %d frames (its first frames are the halo "
                 "of the rank before it)" % (args.frame_steps, args.gpus, framesteps.carry_frames(steps), n_frames))
    if args.calib_angle is not None and not np.isfinite(args.calib_angle):
        ap.error("--calib-angle must be a finite number of degrees")
    given = None
    if args.keypts_source != "ae" or args.features_from:
        if args.keypts_source != "ae" and args.features_from:
            ap.error("--keypts-source and --features-from exclude each other")
        if args.keypts_source != "ae" and not args.keypts_dir:
            ap.error("--keypts-source %s needs --keypts-dir" % args.keypts_source)
        if args.scans and not args.python_loader:
            ap.error("--keypts-source / --features-from run on the Python loader path (add --python-loader): the native scan loader "
                     "(caelo_seqloader) does not read key point or feature files")
        from caelo import keysources

        def given(i):
            if args.features_from:
                kp, feats, _ = keysources.load_features_dir(args.features_from, i)
                return "rows", keysources.rows_from_features(kp, feats)
            return "keypts", keysources.load_keypts(args.keypts_source, args.keypts_dir, i)
    world, rank, local_rank = cdist.ensure_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:])
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    backend = os.environ.get("CAELO_DIST_BACKEND", "nccl")   # gloo: several ranks on one GPU (functional tests)
    local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    eng = Engine(respond_h5=args.respond_h5 or RESPOND_H5, encoder_h5=args.encoder_h5 or ENCODER_H5, device=local_rank)
    if world > 1:
        dist.init_process_group(backend=backend, **({"device_id": torch.device("cuda", local_rank)} if backend == "nccl" else {}))
    if args.scans:
        files = sorted(glob.glob(os.path.join(args.scans, "*.bin")))
        n = len(files)

        def load(i):
            return stageio.read_scan(files[i])

        def load_into(i, slot, pin):   # the file's bytes into a pinned slot [capacity, 4]; a scan larger than the slot is pinned on its own
            nbytes = os.path.getsize(files[i])
            if nbytes % 16 or nbytes // 16 > slot.shape[0]:
                return pin(stageio.read_scan(files[i]))
            raw = slot.numpy().reshape(-1).view(np.uint8)
            with open(files[i], "rb") as f:
                got = f.readinto(memoryview(raw)[:nbytes])
            assert got == nbytes, "short read: %s" % files[i]
            return slot[:nbytes // 16]
        load.into = load_into
    else:
        import threading
        cache, locks, guard = {}, {}, threading.Lock()

        def load(i):   # (called from the loader's threads: a pooled scan is synthesised once, by whoever asks first)
            if args.pool <= 1:
                return synth.make_scan(i, quantum=args.quantum or None, scene_kind=args.scene, trajectory=args.trajectory)
            i %= 2 * (args.pool - 1)
            i = i if i < args.pool else 2 * (args.pool - 1) - i
            with guard:
                lk = locks.setdefault(i, threading.Lock())
            with lk:
                if i not in cache:
                    cache[i] = synth.make_scan(i, quantum=args.quantum or None, scene_kind=args.scene, trajectory=args.trajectory)
            return cache[i]
        load.repeats = args.pool > 1

        n = args.synthetic
        files = [os.path.join(os.path.dirname(os.path.abspath(args.out)), "synthetic", "velodyne", "%06d.bin" % i) for i in range(n)]
    assert n >= 2, "need at least two scans (--synthetic N or --scans DIR)"
    Tr = stageio.read_calib_tr(args.calib) if args.calib else None

    lo, hi = cdist.shard_frames(n, rank, world)
    t0 = time.time()

    registrar = _registrar(args)   # (comparison: step 1 is registered from the resident rows too, the pipeline's own pair results are not used)
    stepper = (framesteps.StepRegistrar(eng, steps, args.seed_base, not args.no_certify, lo, registrar=registrar)
               if any(s_ != 1 for s_ in steps) or registrar is not None else None)

    def keep(c0, batch):
        if stepper is not None:   # (after the host redo of tied frames: the rows are final)
            stepper.keep(c0, batch)
        if not args.save_artifacts:
            return
        rows = batch.rows.cpu().numpy(); nk = batch.n_key.cpu().numpy()
        idx = batch.pair_idx.cpu().numpy(); mask = batch.inlier_mask.cpu().numpy().astype(bool)
        for j in range(len(nk)):
            k = int(nk[j])
            stageio.save_features(files[c0 + j], rows[j, :k, 60:63], rows[j, :k, 0:60])
            if c0 + j > lo:
                m = mask[j, :k]
                stageio.save_inliers(os.path.dirname(os.path.dirname(files[c0 + j])), c0 + j - 1, c0 + j, idx[j, :k][m], np.arange(k)[m])

    tie_log = []
    host_times = {}
    records = [] if args.matchability else None
    if args.scans and not args.python_loader:
        rel, ok, thr, nin, first, last = run_local_files(eng, files, lo, hi, args.seed_base, args.chunk, args.dist_channels,
                                                         args.batch, keep, strict_ties=not args.no_strict_ties, tie_log=tie_log, host_times=host_times,
                                                         loader_threads=args.loader_threads, certify=not args.no_certify, device_results=args.save_artifacts,
                                                         native_ties=args.native_ties, records=records, calib_angle=args.calib_angle)
    else:
        rel, ok, thr, nin, first, last = run_local(eng, load, lo, hi, args.seed_base, args.chunk, args.dist_channels,
                                                   args.batch, keep, strict_ties=not args.no_strict_ties, tie_log=tie_log, host_times=host_times,
                                                   loader_threads=args.loader_threads, certify=not args.no_certify, native_ties=args.native_ties,
                                                   given=given, records=records, calib_angle=args.calib_angle)
    if tie_log:
        print("rank %d: %d frame(s) redone in scikit-learn's tie order (%d patches): %s" % (
            rank, len(tie_log), sum(n for _, n in tie_log), [f for f, _ in tie_log][:20]), file=sys.stderr)
    if world > 1:   # the pair that straddles the rank boundary: ONE all-gather of the boundary rows
        gathered = cdist.all_gather_boundary(last.rows)
        if rank > 0:   # (exact unless --no-certify, like every other pair)
            both = torch.stack([gathered[rank - 1], first.rows])
            n_key = both[:, :, 63].sum(dim=1).round().to(torch.int32)   # (as FrameFeatures.from_rows counts them)
            raw = eng.register_pairs(both, n_key, [(0, 1)], [args.seed_base + lo - 1], certify=not args.no_certify).results
            r1, o1, t1, n1 = _parse_poses(raw, 1)
            rel = np.concatenate([r1, rel]); ok = np.r_[o1, ok]; thr = np.r_[t1, thr]; nin = np.r_[n1, nin]
            if records is not None:
                records.insert(0, _parse_records(raw, 1))
        cols = [rel, ok, thr, nin]
        if records is not None:   # (two more columns: small integers, exact in float32)
            cols += [np.concatenate([a for a, _ in records]) if records else np.zeros(0), np.concatenate([b for _, b in records]) if records else np.zeros(0)]
        extra = torch.from_numpy(np.c_[tuple(cols)].astype(np.float32)).to(eng.device)
        allrows = cdist.gather_poses(extra, n).cpu().numpy()
        rel, ok, thr, nin = allrows[:, :12], allrows[:, 12] > 0, allrows[:, 13], allrows[:, 14].astype(np.int32)
        if records is not None:
            records = [(allrows[:, 15].astype(np.int32), allrows[:, 16].astype(np.int32))]
    if stepper is not None and world > 1:   # the step pairs that straddle a rank boundary: frame 0's owner registers them on the next rank's head
        heads = cdist.all_gather_boundary(stepper.head_rows())
        if rank < world - 1:
            stepper.boundary(heads[rank + 1], hi, n)
        exports = [None] * world
        dist.all_gather_object(exports, stepper.export())
        if rank == 0:
            stepper.merge(exports)
    torch.cuda.synchronize()
    dt = time.time() - t0
    if rank == 0:
        if registrar is not None:
            rel, ok, nin, np_c, it_c = stepper.step_results(1)
            thr = np.full(len(rel), args.inlier_threshold, np.float32)
            records = [(it_c, np_c)] if records is not None else None
        np_1, it_1 = (np.concatenate([b for _, b in records]), np.concatenate([a for a, _ in records])) if records is not None else (None, None)
        _write_step(args, 1, n, Tr, rel, ok, nin, np_1, it_1, say=False)   # (step 1's lines, one per pair, follow the other steps')
        for s_ in ([s_ for s_ in stepper.steps if s_ != 1] if stepper is not None else []):
            _write_step(args, s_, n, Tr, *stepper.step_results(s_))
        for i in range(len(rel) if len(rel) <= 200 else 0):
            print("%06d-%06d ok=%d thr=%.1f inliers=%4d T=[% .3f % .3f % .3f]" % (i, i + 1, ok[i], thr[i], nin[i], rel[i, 9], rel[i, 10], rel[i, 11]))
        print("%d frames, %d pairs on %d GPU(s) in %.2f s (%.1f frames/s incl. scan loading / synthesis, upload and read-back; %d of %d poses solved) -> %s" % (
            n, len(rel), world, dt, n / dt, int(np.sum(ok)), len(rel), args.out))
        h = host_times
        print("rank 0 host seconds -- loader thread: reading / synthesising scans %.2f, pinning %.2f, RANSAC draws %.2f; issuing thread: "
              "pipeline creation + heap freeze %.2f, waiting for the loader (%d threads) %.2f, pipeline calls (uploads paced, %d frames) %.2f, tie check + read-back issue %.2f, "
              "parsing results %.2f (the chunk loop as a whole %.2f)" % (h["load"], h["pin"], h["draws"], h["setup"], args.loader_threads, h["starved"], hi - lo, h["pipeline"], h["ties"], h["parse"], h.get("loop", 0.0)))
        if any(k_.startswith("loaded_") for k_ in h):
            print("        inside the pipeline calls (Pipeline.run_loaded): " + ", ".join("%s %.3f" % (k_[7:], v_) for k_, v_ in sorted(h.items()) if k_.startswith("loaded_")))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
