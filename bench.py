#!/usr/bin/env python
"""bench.py -- end-to-end CAE-LO hot path on MI355X: frames/s for
project -> response CNN -> keypoints -> voxelize -> patch gather -> 3D-CAE descriptors -> NN match -> RANSAC pose.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...)

A step = one batch of --batch (8) KITTI-shaped scans (64 beams x 2000 azimuths, ~126k points each, already resident in HBM)
taken through the whole path on every rank.  Frames shard across ranks (weak scaling: K frames per rank; --scaling strong
splits the steps instead); the timed region per rank is
    K x (extract, then match + RANSAC against the predecessor frame)  with the RCCL all-gather of per-frame rows [1024,64] f32
    (--gather all, default: every frame, batch by batch on a side stream as soon as a batch is encoded; --gather boundary:
    each rank's last frame, one collective at the end)
    ->  (ranks > 0) the pair that straddles the rank boundary (a rank's first frame against the previous rank's last
    one, taken from the gathered rows; rank 0's first frame against the last warm-up frame).
The frames go through the native executor (caelo_pipeline): --batch consecutive frames share ONE launch of every front kernel,
one encoder launch set and one match / RANSAC launch; the three stages of successive batches overlap on three HIP streams
(front(b+1) || encoder(b) || pairs(b-1)).

Rank 0 prints one JSON line: `value` (frames/s over the timed steps), `ms_per_step` and what the run checked on the way (poses
solved, status words, the exact-RANSAC counters, the collective).  A plain run does only that: set up, warm up, time the steps,
--dump-outputs, the line.  --full adds, after the timed steps and never part of `value`:
    roofline      the dominant kernel (k_enc_stage1x, conv1+conv2 of the 3D-CAE encoder), executed MFMA
                  FLOPs / HIP-event time measured live through caelo_encode_profile; roofline_match likewise for the NN match
    secondary     short legs of other configurations and scenes through the same pipeline (N == 1 only)
    cpu_baseline  the CPU oracle (oracle/, the reference restated in C/NumPy) on the host cores,
                  bounded sample, rank 0 at N == 1 only.
"""
import argparse
import gc
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from caelo import synth  # noqa: E402
import caelo  # noqa: E402
caelo.configure_runtime()  # before the first device call (the hardware-queue count is left to the caller: three pipeline streams by default)
from caelo import _ffi  # noqa: E402
from caelo import dist as cdist  # noqa: E402
from caelo.engine import Engine, FrameBatch, FrameFeatures, ransac_draws  # noqa: E402

POOL = 17  # distinct consecutive synthetic frames per rank, walked back and forth (0 1 .. 16 15 .. 1 0 1 ..) so that every
           # timed pair is a pair of NEIGHBOURING scans, like a real sequence (cycling 16 -> 0 would make a 14 m jump whose
           # match fails and escalates RANSAC to 1.6 m).  2 x 8 + 1 frames: the walk's period is four batches of 8 and its
           # turning points fall on batch boundaries, so NO BATCH HOLDS A SCAN TWICE -- equal patches are looked for across
           # the frames of a batch, and a repeated scan would be encoded for free (a pool of 6 did that: 20.4 k frames/s
           # instead of 18.x k; a real sequence never repeats a scan)
TRAJECTORY = "circuit"  # caelo.synth.sensor_pose: 0.9 m per frame through a world that repeats every 54 m -- structure (>= 22 % non-ground
                        # returns) at EVERY frame index, closed after 600 frames.  Rounds 1-5 used the "line" law of the goldens, on which the
                        # sensor has left the scene by frame ~150: every scan past ~200 was the same bare ground plane (missing 1)


def scan_at(index, **kw):
    """synthetic scan number `index` of the endless sequence: pose = the circuit's at index mod 600 (closed: 599 -> 0 is a pair of neighbours
    like any other), range noise / intensities seeded by the index itself (no two scans are equal)"""
    return synth.make_scan(index % synth.CIRCUIT_PERIOD, seed=index, trajectory=TRAJECTORY, **kw)



CERTIFY = True  # exact RANSAC (device certificates + the host half inside the pipeline) in every leg; --no-certify turns it off
QUANTUM = 1e-3  # coordinates in whole millimetres, like the metrically quantised values of real scans: every frame then
                # holds points exactly on voxel faces (tests/golden/frame_q0.npz: 14 of 126 k), which the voxelization
                # resolves like the reference's float64 index arithmetic (Voxel.py:118-152)

# algorithmic FLOPs per patch (SURVEY.md 8d / BASELINE.md section 4): 2 x MACs
FLOP_CONV1 = 2 * 4096 * 27 * 8
FLOP_CONV2 = 2 * 512 * 216 * 16
FLOP_CONV3 = 2 * 64 * 432 * 32
FLOP_DENSE1 = 2 * 2048 * 200
FLOP_DENSE2 = 2 * 200 * 20
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense f32-input matrix peak (v_mfma_f32_16x16x4_f32)
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 matrix peak (v_mfma_f32_16x16x32_bf16)
# conv3 / Dense(200) evaluate every f32 product as SIX bf16 x bf16 partial products on the bf16 pipe:
# the ceiling for their f32-equivalent (algorithmic) rate is the bf16 peak / 6
X3_F32_EQUIV_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 6.0
FLOP_PER_MFMA_F32 = 2 * 16 * 16 * 4


def cpu_baseline(n_frames=16, max_seconds=30.0):
    """CPU oracle end to end (all host cores via OpenMP) on a bounded sample of the same workload."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle as orc
    resp_m, enc_m = orc.load_models(os.path.join(REPO, "weights", "SphericalRingPCRespondLayer.h5"),
                                    os.path.join(REPO, "weights", "EncoderModel4VoxelPatch.h5"))
    cores = orc.num_threads()
    clouds = [scan_at(f, quantum=QUANTUM) for f in range(n_frames + 1)]

    def extract(pc):
        ring, cnt = orc.ProjectPC2SphericalRing(pc)
        resp = resp_m.predict(ring[None, 0:64, 0:1792, 0:3])[0]
        kp, _, _ = orc.GetKeyPtsByAE(ring, cnt, resp)
        v = orc.Voxelization(pc[:, 0:3])
        feats = np.concatenate([enc_m.predict_bits(orc.patches_bits(kp, v[6 + s], s)[0]) for s in range(3)], axis=1)
        return kp, feats

    # three samples of the same frames, each bounded by max_seconds / 3: the host is shared (128 threads of OpenMP beside whatever else
    # runs on the box) and one sample wandered between 1.5 and 2.0 frames/s from run to run -- `value` is the
    # median, `range` the spread
    rates, frames_done, secs = [], 0, 0.0
    for _ in range(3):
        prev = extract(clouds[0])
        t0 = time.time()
        done = 0
        for f in range(1, n_frames + 1):
            cur = extract(clouds[f])
            orc.SolveRelativePose(prev[0], prev[1], None, cur[0], cur[1], None, rng=np.random.RandomState(f))
            prev = cur
            done += 1
            if time.time() - t0 > max_seconds / 3.0:
                break
        dt = time.time() - t0
        rates.append(done / dt)
        frames_done += done
        secs += dt
    return {"value": round(float(np.median(rates)), 4), "range": [round(min(rates), 4), round(max(rates), 4)], "unit": "frames/s", "cores": int(cores), "kind": "port",
            "sample": "3 samples of up to %d synthetic frames each (64x2000 scan, 1024 keypoints, 3072 patches each; %d frames, %.1f s in all), full path incl. "
                      "match+RANSAC, oracle C/NumPy restatement with OpenMP on %d threads; value = median of the three rates, range = min / max" % (n_frames, frames_done, secs, cores)}


def bench_dense128(args, eng, world, rank, backend, dev):
    """BASELINE configs[4]: synthetic 128-beam x 4000-azimuth scan (~507 k points), 32^3 voxel patches (the 3D-conv MFMA
    stress; DESIGN.md 4.5 states the definition).  A step = one scan: key points by the 16^3 path, 3 x 1024 patches of
    32^3 voxels, the encoder stack on them.  One stream; every rank runs its own frames (weak scaling)."""
    K, W = args.steps, args.warmup
    pool = [torch.from_numpy(scan_at(rank * 7 + i, n_beams=128, n_az=4000, quantum=QUANTUM)).to(dev) for i in range(2)]
    wd1, bd1 = eng.seeded_dense1_32()
    eng.set_encoder32_dense(wd1, bd1)
    big = max(p.shape[0] for p in pool)
    for p in pool:
        eng.extract32(p)
    torch.cuda.synchronize()
    for i in range(W):
        eng.extract32(pool[i % 2])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(K):
        ff = eng.extract32(pool[i % 2])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    if args.dump_outputs and rank == 0 and K > 0:   # the last timed step: one frame
        dump_outputs(args.dump_outputs, frame_outputs(ff.rows[None], ff.key_pixels[None], ff.n_key, ff.status[None])[0])
    roofline = cpu = None
    if rank == 0 and args.full:
        vmap = eng.voxmap(max(eng.max_points, big))
        eng.voxelize(pool[0], vmap)
        bits = eng.patches32(vmap, ff.key_pts.contiguous(), ff.n_key)
        for _ in range(2):
            eng.encode32_profile(bits, group=3)
        ms = np.array([eng.encode32_profile(bits, group=3)[1] for _ in range(8)]).mean(axis=0)
        npat = bits.numel() // 512
        # dense FLOPs per 32^3 patch (2 x MACs): conv1 32^3 x 27 x 8, conv2 16^3 x 216 x 16, conv3 8^3 x 432 x 32, dense 16384 x 200 (+ 200 x 20)
        flops = npat * np.array([2 * 32768 * 27 * 8, 2 * 4096 * 216 * 16, 2 * 512 * 432 * 32, 2 * 16384 * 200 + 2 * 200 * 20], dtype=np.float64)
        names = ["k5_conv1pool_x3", "k5_conv2_x3", "k5_conv3_x3", "k_enc_dense1<16384> + k_enc_head"]
        # conv1's input is binary (exact in bf16): 3 bf16 MFMAs per product block; conv2 / conv3 6; Dense(200) (f16 x 2) 3
        peaks = [BF16_MFMA_PEAK_TFLOPS / 3.0, X3_F32_EQUIV_PEAK_TFLOPS, X3_F32_EQUIV_PEAK_TFLOPS, BF16_MFMA_PEAK_TFLOPS / 3.0]
        tf = flops / (ms * 1e-3) / 1e12
        dom = int(np.argmax(ms))
        table = {n: {"ms": round(float(m), 4), "f32_equiv_tflops": round(float(t), 2), "pipe_peak": round(pk, 1), "pipe_frac": round(float(t / pk), 4)}
                 for n, m, t, pk in zip(names, ms, tf, peaks)}
        # matrix-pipe busy share by the hardware counters (separate rocprofv3 --pmc passes of the same 8-frame launch, committed):
        # SQ_VALU_MFMA_BUSY_CYCLES summed over 1024 SIMDs against SQ_BUSY_CYCLES summed over 32 shader engines
        pmc_busy = None
        try:
            cur, vals = None, {}
            for line in open(os.path.join(REPO, "profiles", "r02_pmc_mfma_busy.txt")):
                t = line.split()
                if len(t) >= 1 and not line.startswith(" "):
                    cur = line.strip().replace("void ", "").split("<")[0]
                elif cur and len(t) >= 4 and t[0] in ("SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES"):
                    vals.setdefault(cur, {})[t[0]] = float(t[-1])
            pmc_busy = {k: round(v["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0 / (v["SQ_BUSY_CYCLES"] / 32.0), 3) for k, v in vals.items()
                        if len(v) == 2 and v["SQ_VALU_MFMA_BUSY_CYCLES"] > 0 and k in ("k_enc_stage1", "k_enc_conv3", "k_enc_dense1p", "k_enc_dense1")}
            pmc_busy["source"] = "profiles/r02_pmc_mfma_busy.txt (SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs over SQ_BUSY_CYCLES / 32 SEs, 8-frame launch)"
        except Exception:
            pmc_busy = None
        roofline = {"bound": "mfma", "kernel": names[dom], "achieved": round(float(tf[dom]), 2), "peak": round(peaks[dom], 1),
                    "unit": "TFLOP/s", "frac": round(float(tf[dom] / peaks[dom]), 4), "traffic": None,
                    "launch_ms": round(float(ms[dom]), 4),
                    "achieved_is": "dense (= executed: these kernels skip nothing) f32-equivalent FLOPs of the layer / launch time, "
                                   "against the bf16 matrix peak / 6 (six bf16 MFMAs per f32 product block, DESIGN.md 4.6)",
                    "mfma_busy_pmc": pmc_busy,
                    "encoder_kernels": table, "encoder_total_ms": round(float(ms.sum()), 4),
                    "encoder_total_f32_equiv_tflops": round(float(flops.sum() / (ms.sum() * 1e-3) / 1e12), 2)}
        if world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baseline_dense128()
    if rank == 0:
        print(json.dumps({
            "metric": "frames/sec keypoint + 32^3-patch descriptor extraction, 128-beam dense scan (configs[4])",
            "value": round(world * K / dt, 2), "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": round(dt / K * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[4]: synthetic 128-beam x 4000-azimuth scan, 2x voxel-patch resolution (32^3), 1 mm "
                                   "coordinates; not a reference code path (PatchSize = 16 there): definition in DESIGN.md 4.5",
                       "arithmetic": "f32 in / out / accumulate; every conv / dense product as exact bf16 partial products on the bf16 "
                                     "matrix pipe (f32-grade, DESIGN.md 4.6)",
                       "points_per_frame": int(pool[0].shape[0]), "keypoints": int(ff.n_key.item()), "patches_per_frame": 3 * int(ff.key_pts.shape[0]),
                       "patch_voxels": 32768, "frames_per_gpu": K, "parallelism": "frames sharded x%d, no collective" % world},
            "roofline": roofline, "cpu_baseline": cpu}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def cpu_baseline_dense128(n_patches=96):
    """CPU oracle of the 32^3 encoder on a bounded sample, scaled to a frame (3072 patches); the front stages (ring image,
    response, key points, voxelization) are timed on one whole frame."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle as orc
    resp_m, enc_m = orc.load_models(os.path.join(REPO, "weights", "SphericalRingPCRespondLayer.h5"),
                                    os.path.join(REPO, "weights", "EncoderModel4VoxelPatch.h5"))
    from caelo.engine import Engine as _E
    wd1, bd1 = _E.seeded_dense1_32()
    enc32 = orc.PatchEncoder32(enc_m.w, wd1, bd1)
    pc = scan_at(0, n_beams=128, n_az=4000, quantum=QUANTUM)
    t0 = time.time()
    ring, cnt = orc.ProjectPC2SphericalRing(pc)
    resp = resp_m.predict(ring[None, 0:64, 0:1792, 0:3])[0]
    kp, _, _ = orc.GetKeyPtsByAE(ring, cnt, resp)
    v = orc.Voxelization(pc[:, 0:3])
    t_front = time.time() - t0
    t0 = time.time()
    per = n_patches // 3
    for s_ in range(3):
        enc32.predict_bits(orc.patches32_bits(kp[:per], v[6 + s_], s_))
    t_enc = (time.time() - t0) * (3 * len(kp)) / (3 * per)
    return {"value": round(1.0 / (t_front + t_enc), 4), "unit": "frames/s", "cores": int(orc.num_threads()), "kind": "port",
            "sample": "front stages of one 128-beam frame (%.1f s) + the 32^3 oracle encoder on %d of its %d patches scaled to the "
                      "frame (%.1f s), oracle C/NumPy restatement with OpenMP on %d threads" % (t_front, 3 * per, 3 * len(kp), t_enc, orc.num_threads())}


def _pmc_busy():
    """matrix-pipe busy share by the hardware counters (separate rocprofv3 --pmc passes of the same 8-frame launch, committed):
    SQ_VALU_MFMA_BUSY_CYCLES summed over 1024 SIMDs against SQ_BUSY_CYCLES summed over 32 shader engines"""
    for name in ("r04_pmc_mfma_busy.txt", "r03_pmc_mfma_busy.txt", "r02_pmc_mfma_busy.txt"):
        try:
            cur, vals = None, {}
            for line in open(os.path.join(REPO, "profiles", name)):
                t = line.split()
                if len(t) >= 1 and not line.startswith(" "):
                    cur = line.strip().replace("void ", "").split("<")[0].split("(")[0]
                elif cur and len(t) >= 4 and t[0] in ("SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES"):
                    vals.setdefault(cur, {})[t[0]] = float(t[-1])
            out = {k: round(v["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0 / (v["SQ_BUSY_CYCLES"] / 32.0), 3) for k, v in vals.items()
                   if len(v) == 2 and v["SQ_VALU_MFMA_BUSY_CYCLES"] > 0 and k.startswith("k_enc")}
            if out:
                out["source"] = "profiles/%s (SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs over SQ_BUSY_CYCLES / 32 SEs, 8-frame launch)" % name
                return out
        except Exception:
            pass
    return None


DUMP_LIMIT = 64 << 20   # bytes: --dump-outputs writes at most this much


def dump_outputs(path, arrays):
    """--dump-outputs: one .npy per array, float32 kept as is, every other type widened to float64 (exact for the integers here)"""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32 if np.asarray(v).dtype == np.float32 else np.float64) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    assert total <= DUMP_LIMIT, "--dump-outputs: %d bytes > %d" % (total, DUMP_LIMIT)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v)
    print("bench.py: %d arrays (%.2f MB) written to %s" % (len(arrays), total / 1e6, path), file=sys.stderr)


def frame_outputs(rows, key_pixels, n_key, status):
    """a caller's view of extracted frames [F, ...]: slots past a frame's key-point count are not part of the result (zeroed)"""
    n_key = n_key.cpu().numpy().astype(np.int64)
    valid = np.arange(rows.shape[1])[None, :] < n_key[:, None]
    rows = rows.cpu().numpy()
    return {"descriptors": np.where(valid[..., None], rows[:, :, 0:60], 0), "key_pts": np.where(valid[..., None], rows[:, :, 60:63], 0),
            "key_pixels": np.where(valid[..., None], key_pixels.cpu().numpy(), 0), "n_key": n_key, "status": status.cpu().numpy()}, valid


def pose_outputs(res, masks, pair_idx, valid):
    """the pairs' results: poses (PoseResult fields), inlier masks and NN match indices of each frame's key points"""
    out = {"pose_" + f: res[f] for f in res.dtype.names}
    out["inlier_mask"] = np.where(valid, masks, 0)
    out["pair_idx"] = np.where(valid, pair_idx.cpu().numpy(), 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120, help="timed steps; a step = one batch of --batch frames (one launch set of "
                                                           "the pipeline) through the whole path")
    ap.add_argument("--warmup", type=int, default=6, help="untimed warm-up steps (batches)")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure what the headline figure does not need: the "
                                                        "roofline objects, the secondary legs and the CPU baseline (each can be left out "
                                                        "with its --no-* option)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-pmc", action="store_true", help="--full without the rocprofv3 --pmc passes that measure `roofline.traffic` and the matrix-pipe busy "
                                                          "share in this run (three sub-processes, ~1 min); the committed figures are used and marked stale_possible")
    ap.add_argument("--no-certify", action="store_true", help="the kernels' own RANSAC results (float64 fits) without the host half that "
                                                              "makes inlier sets and poses the reference's bits (never the headline)")
    ap.add_argument("--no-secondary", action="store_true", help="--full without the short untimed-for-`value` legs after the timed region "
                                                                "(configs[1], configs[4], no de-duplication, the clutter scene, upload included)")
    ap.add_argument("--batch", type=int, default=8, help="frames per launch = frames per step (1..8): the front kernels, the encoder "
                                                         "launch set and the match / RANSAC launches each cover a whole batch")
    ap.add_argument("--buffers", type=int, default=3, help="batches of patches in flight between the front and the encoder")
    ap.add_argument("--config", choices=("odometry", "extract", "dense128"), default="odometry",
                    help="odometry = BASELINE configs[2] (the headline metric); extract = configs[1] (keypoints + descriptors "
                         "only); dense128 = configs[4] (128-beam x 4000-azimuth scan, 32^3 patches: 3D-conv MFMA stress)")
    ap.add_argument("--extract-only", action="store_true", help="same as --config extract")
    ap.add_argument("--scene", choices=("boxes", "clutter"), default="boxes", help="synthetic scene of the timed region")
    ap.add_argument("--include-h2d", action="store_true", help="the timed region also uploads every scan from pinned host memory "
                                                               "on a copy stream, double buffered (PCIe-inclusive rate; never the headline `value`)")
    ap.add_argument("--gather-overlap", type=int, default=1,
                    help="--gather all: 1 (default) = the rows of every batch are gathered on a side stream as soon as the batch is "
                         "encoded, under the extraction of the next batches (host-paced: caelo_pipeline_sync_encoded); 0 = one collective after "
                         "the last frame")
    ap.add_argument("--gather-timed", type=int, default=0,
                    help="1 = every per-batch collective is issued synchronously on a side stream between two events (config.collective."
                         "all_gather_ms); 0 = asynchronously on RCCL's stream, nothing waits for it until the end (the default: a wait "
                         "pending in a queue costs the pipeline throughput)")
    ap.add_argument("--gather", choices=("boundary", "all"), default="all",
                    help="rows moved by the single all-gather: every frame's [1024,64] rows (the north-star's per-frame descriptor "
                         "gather, default) or each rank's last frame only (all that consecutive-pair matching needs)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --steps batches per rank; strong: --steps batches in total, split over the ranks (one workload, 1/2/4/8 a curve)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned for its LAST step (rank 0's frames) as DIR/<name>.npy, "
                         "float32 / float64: descriptors, key points, poses, inlier sets (the inputs are the same seeded scans in every run)")
    args = ap.parse_args()
    global CERTIFY
    CERTIFY = not args.no_certify
    if args.config == "extract":
        args.extract_only = True
    elif args.extract_only:
        args.config = "extract"

    # `python bench.py --gpus N` without a launcher starts its N ranks itself (torch.distributed.run, one per GPU) and exits
    # with their status; a WORLD_SIZE that differs from --gpus, or fewer than N visible GPUs without the gloo functional-test
    # backend, is an error (exit 2, no JSON line) -- never a one-rank line (caelo.dist.ensure_ranks)
    world, rank, local_rank = cdist.ensure_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:])
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # CAELO_DIST_BACKEND=gloo: functional test of the multi-rank path with several ranks on one GPU (RCCL wants one
    # device per rank); the driver's runs use the default, nccl == RCCL over xGMI
    backend = os.environ.get("CAELO_DIST_BACKEND", "nccl")
    local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    eng = Engine(device=local_rank)
    certify_note = None
    if CERTIFY:
        try:
            eng.host_blas()   # the host half needs the BLAS / LAPACK entry points of this process's NumPy, verified bit for bit
        except Exception as e:   # an exotic NumPy build: the line is still produced, from the kernels' own RANSAC, and says so
            CERTIFY = False
            certify_note = "exact RANSAC off: %s" % str(e)[:300]
            print("bench.py: " + certify_note, file=sys.stderr)
    if args.config == "dense128":
        if world > 1:
            dist.init_process_group(backend=backend, **({"device_id": dev} if backend == "nccl" else {}))
        return bench_dense128(args, eng, world, rank, backend, dev)
    # the pipeline's streams come first; RCCL creates its own afterwards.  If the runtime refuses a stream (hardware queues
    # exhausted next to RCCL's), the pipeline falls back to fewer streams by itself (caelo_pipeline_create) and reports it.
    pipe = eng.pipeline(args.batch, args.buffers)
    if world > 1:
        dist.init_process_group(backend=backend, **({"device_id": dev} if backend == "nccl" else {}))
    B = pipe.batch
    global POOL
    POOL = 2 * B + 1   # (see the comment at the top: the walk's turning points fall on batch boundaries)
    steps_rank = args.steps if args.scaling == "weak" else max(1, args.steps // world)
    K, W = steps_rank * B, args.warmup * B          # frames per rank in the timed region / in the warm-up

    def make_pool(scene_kind, base):
        return [torch.from_numpy(scan_at(base + i, quantum=QUANTUM, scene_kind=scene_kind)).to(dev) for i in range(POOL)]

    # synthetic scans of this rank's stretch of the trajectory, uploaded before the clock starts
    base = rank * K
    pool = make_pool(args.scene, base)
    rand_host = [ransac_draws(1000 + rank * 7919 + i) for i in range(POOL)]
    rand = [torch.from_numpy(r).to(dev) for r in rand_host]
    n_points = int(np.mean([p.shape[0] for p in pool]))

    def walk(i, plen=None):          # 0 1 2 3 4 5 4 3 2 1 0 1 ...
        plen = plen or POOL
        i %= 2 * (plen - 1)
        return i if i < plen else 2 * (plen - 1) - i

    class Runner:
        """frames through the native pipeline: extract, then match + RANSAC against frame i-1, `batch` frames per launch"""

        def __init__(self, pool_, **kw):
            self.pool, self.kw, self.pos = pool_, kw, 0   # pos: position of the last frame handed out (`prev` is frame walk(0) = 0)
            self.prev = eng.extract(pool_[0])

        def peek(self, n):
            return [walk(self.pos + 1 + i, len(self.pool)) for i in range(n)]

        def order(self, n):
            o = self.peek(n)
            self.pos += n
            return o

        def run(self, n, out=None, pairs=True, scans=None, on_encoded=None):
            o = self.order(n)
            assert n % B or all(len(set(o[i:i + B])) == B for i in range(0, n, B)), "a batch holds a scan twice"
            # certify: the exact RANSAC -- the pipeline's certifier threads run the host half (the reference's own BLAS / LAPACK calls
            # on the hypotheses that decide) on every pair while later batches are on the GPU; run() returns when all are written
            batch = pipe.run(scans if scans is not None else [self.pool[j] for j in o], [rand[j % POOL] for j in o],
                             prev=self.prev if pairs else None, pairs=pairs, out=out, on_encoded=on_encoded,
                             certify=pairs and CERTIFY, rands_host=[rand_host[j % POOL] for j in o] if pairs and CERTIFY else None,
                             publish=False, **self.kw)   # (the exact poses / inlier sets are delivered in host arrays, like the reference's: batch.exact)
            self.last_order = o
            self.prev = batch.frame(n - 1)
            return batch

    Runner.walk = staticmethod(walk)
    main_run = Runner(pool)

    overlap = world > 1 and args.gather == "all" and args.gather_overlap and not args.extract_only and not args.include_h2d

    def run_ranks(n, out, gather_stats):
        """n frames through the pipeline and across the ranks.  Overlapped gather: every batch's rows leave on a side stream as soon
        as the batch is encoded, under the extraction of the next batches; then the pair that straddles the rank boundary."""
        if not overlap:
            batch = main_run.run(n, out, pairs=not args.extract_only)
            finish_ranks(batch, n, gather_stats)
            return batch
        out = out or FrameBatch(eng, n)
        g = cdist.ChunkedFrameGather(out.rows, n, B, timed=args.gather_timed)

        batch = main_run.run(n, out, on_encoded=g.chunk)   # (host-paced: the rows of [lo, hi) are written when the collective is enqueued)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()                     # the pipeline's own work ends here on this stream ...
        frame_of = g.finish()           # ... and what is left of the gathers after it is the exposed part
        e1.record()
        if rank > 0:
            boundary_pair(batch, FrameFeatures.from_rows(frame_of(rank - 1, n - 1)))
        gather_stats.append((e0, e1, g.nbytes(), g))
        return batch

    def boundary_pair(batch, prev_ff):
        """this rank's first frame against the previous rank's last one (from the gathered rows), exact like every other pair"""
        if CERTIFY:
            r, m, idx = eng.match_pose_exact(prev_ff, batch.frame(0), rand[0], rand_host[0])
            batch.result[0].copy_(torch.from_numpy(np.frombuffer(r.tobytes(), np.uint8).copy()))
            batch.inlier_mask[0].copy_(torch.from_numpy(m))
            if batch.exact is not None:
                batch.exact[0][0], batch.exact[1][0], batch.exact[3][0] = r, m, 0
        else:
            batch.result[0].copy_(eng.match_pose(prev_ff, batch.frame(0), rand[0])[0])

    def finish_ranks(batch, n, gather_stats):
        """ONE collective over xGMI (every frame's rows, or the boundary frames), then the pair that straddles the rank boundary"""
        if world == 1 or args.extract_only:
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if args.gather == "all":
            allrows = cdist.all_gather_frames(batch.rows, n * world)
            prev_rows = allrows[rank * n - 1] if rank > 0 else None
            nbytes = allrows.numel() * 4
        else:
            last = cdist.all_gather_boundary(batch.rows[n - 1])
            prev_rows = last[rank - 1] if rank > 0 else None
            nbytes = last.numel() * 4
        e1.record()
        if rank > 0:   # this rank's first frame pairs with the previous rank's last one (from the gathered rows)
            boundary_pair(batch, FrameFeatures.from_rows(prev_rows))
        gather_stats.append((e0, e1, nbytes, None))

    gc.collect()
    gc.freeze()          # (before the warm-up: a pause here would let the GPU's clocks drop right in front of a 9 ms timed region)
    timed_out = FrameBatch(eng, K)   # the timed frames' output rows / poses: allocated like any other resident buffer, before the warm-up (an
                                     # allocation between warm-up and clock start is milliseconds of an idle GPU in front of a 9 ms region)
    # one-time initialisation, not a warm-up step: the stage streams and every hand-off buffer are touched once (a
    # HIP stream allocates its hardware queue on first use, ~ms), so that a run with a small --warmup does not time that
    gstats = []
    run_ranks(pipe.buffers * B, None, gstats)
    torch.cuda.synchronize()
    if W > 0:
        run_ranks(W, None, gstats)
    torch.cuda.synchronize()
    host_scans = None
    if args.include_h2d:
        host_scans = [p.cpu() for p in pool]
        staged = Staging(host_scans, B, walk, dev)           # the loader's ring of pinned batch slots (not timed)
        # the upload path's device buffers and copy stream exist before the clock starts (they are created on first use)
        run_with_uploads(eng, pipe, main_run, staged, 2 * B, FrameBatch(eng, 2 * B), rand, pairs=not args.extract_only)
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    pipe.stats()
    # Python's cycle collector stays out of the timed region (like timeit): a full collection of this process's objects takes 40-90 ms --
    # five to ten batches -- and used to land in one run of the upload mode out of three (its loop creates a few hundred objects)
    gc.disable()
    gstats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.include_h2d:
        batch = run_with_uploads(eng, pipe, main_run, staged, K, timed_out, rand, pairs=not args.extract_only)
        t_ru = time.perf_counter() - t0
        finish_ranks(batch, K, gstats)
        t_fr = time.perf_counter() - t0
    else:
        batch = run_ranks(K, timed_out, gstats)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()          # (everything allocated so far is frozen: the collections of the legs below only look at what they create)
    per_rank_fps = [round(K / dt, 1)]
    if world > 1:
        mine = torch.tensor([dt], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        per_rank_fps = [round(K / float(t.item()), 1) for t in every]     # each rank's own rate (its barrier-to-barrier time)
        dt = max(float(t.item()) for t in every)                          # the job's time = the slowest rank's
    if args.include_h2d and os.environ.get("CAELO_BENCH_VERBOSE"):
        # is the staging block itself slow to read for the GPU (where its pages sit), or only the run?
        flat = staged.block.reshape(-1)
        d_ = torch.empty((1 << 22,), dtype=torch.float32, device=dev)
        sc_ = torch.cuda.Stream(dev)
        for off in (0, flat.numel() // 2, flat.numel() - (1 << 22)):
            with torch.cuda.stream(sc_):
                d_.copy_(flat[off:off + (1 << 22)], non_blocking=True); sc_.synchronize()
                t_ = time.perf_counter()
                for _ in range(4):
                    d_.copy_(flat[off:off + (1 << 22)], non_blocking=True)
                sc_.synchronize()
            print("staging block, 16 MB at element %d: %.1f GB/s" % (off, 4 * (1 << 24) / (time.perf_counter() - t_) / 1e9), file=sys.stderr)
        print("timed region: %.2f ms (run_with_uploads returned at %.2f, finish_ranks at %.2f) for %d frames  %s" % (1e3 * dt, 1e3 * t_ru, 1e3 * t_fr, K, {k_: (round(v_, 1) if isinstance(v_, float) else v_) for k_, v_ in pipe.last_upload_times.items()}), pipe.cert_stats(), file=sys.stderr)
    if args.dump_outputs and rank == 0 and K >= B:
        last = batch.view(K - B, B)          # the last timed step: one batch of B frames
        arrays, valid = frame_outputs(last.rows, last.key_pixels, last.n_key, last.status)
        if not args.extract_only:
            if last.exact is not None:       # the certified results are delivered in host arrays
                res, masks = last.exact[0], last.exact[1]
            else:
                res, masks = last.result.cpu().numpy().view(_ffi.POSE_DTYPE).reshape(B), last.inlier_mask.cpu().numpy()
            arrays.update(pose_outputs(res, masks, last.pair_idx, valid))
        dump_outputs(args.dump_outputs, arrays)
    host = pipe.stats()
    cert = pipe.cert_stats() if (CERTIFY and not args.extract_only) else None
    # sanity: every pose solved (not timed)
    if args.extract_only:
        ok = 0
    elif batch.exact is not None:
        ok = int((batch.exact[0]["success"][:K] != 0).sum())
        assert (batch.exact[3][:K] == 0).all(), "a pair of the timed region was not certified"
    else:
        ok = sum(int(eng.pose_result(batch.result[i]).success) for i in range(K))
    # every timed frame's status word (OR of the CAELO_ST_* bits; 0 = no frame needed anything but the fast path)
    st = batch.status[:K, 0].cpu().numpy()
    status, frames_flagged = int(np.bitwise_or.reduce(st)), int((st != 0).sum())
    lane_faults = eng.lane_faults()   # pose kernels' lane-agreement self-check: 0 on healthy hardware
    collective = None
    if gstats:
        e0, e1, nbytes, g = gstats[-1]
        collective = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "gather": args.gather,
                      "bytes_received_per_rank": int(nbytes)}
        if g is None:   # one collective after the last frame: its own time, all of it exposed
            collective.update({"overlapped": False, "all_gather_ms": round(e0.elapsed_time(e1), 4)})
        else:           # per-batch collectives under the extraction: their summed durations, and what was left after the last frame
            cms = g.collective_ms()   # None: issued asynchronously (no stream of ours waits for a collective until the end); --gather-timed 1 times them
            collective.update({"overlapped": True, "collectives": len(g.bounds), "all_gather_ms": None if cms is None else round(cms, 4),
                               "all_gather_exposed_ms": round(e0.elapsed_time(e1), 4)})
            # not timed: the pieces against ONE collective over the same rows
            whole, frame_of = cdist.all_gather_frames(batch.rows[:K], K * world), g.finish()
            collective["chunks_equal_one_gather"] = all(bool(torch.equal(whole[r * K + i], frame_of(r, i)))
                                                        for r in range(world) for i in (0, B - 1, K // 2, K - 1))
        try:
            collective["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            collective["rccl_version"] = None

    if world > 1:
        if collective is None:   # extraction only: no data-path collective, the ranks are still one job
            collective = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "gather": None, "bytes_received_per_rank": 0}
        # the line below says n_gpus = world: it must be what actually ran, on the backend that was asked for
        assert collective["world_size"] == args.gpus == world, "ranks that ran != --gpus"
        assert collective["backend"] == backend and (backend == "nccl" or os.environ.get("CAELO_DIST_BACKEND") == backend), \
            "multi-rank line on a backend nobody asked for"
        collective["ranks_on_distinct_gpus"] = bool(torch.cuda.device_count() >= world)

    out = None
    roofline = roofline_match = secondary = cpu = dedup_share = dedup_share_frame = streams_note = None
    if rank == 0 and host["streams"] != 4:
        streams_note = ("%d pipeline streams instead of 4: GPU_MAX_HW_QUEUES was %r when HIP initialised (needs >= 8 before the first "
                        "device call; the package leaves it to the caller) or the runtime refused a stream" % (host["streams"], os.environ.get("GPU_MAX_HW_QUEUES")))
        print("bench.py: " + streams_note, file=sys.stderr)
    if rank == 0 and args.full:
        # ---- roofline of the encoder kernels, HIP events on the launch stream.  Two launch shapes: the one the timed region
        # issues -- `batch` frames per launch (every patch: the profiling entry point takes no de-duplication tables) -- is the
        # headline; one frame per launch (round 1's figure) is reported beside it.
        names = ["k_enc_stage1x", "k_enc_conv3", "k_enc_dense1", "k_enc_head"]
        # stage 1 and conv3: every f32 product as two f16 terms per operand on the f16 matrix pipe (stage 1 sums all four partial
        # products in three MFMAs per tap row, conv3 and Dense(200) three of the four in three MFMAs per K = 32 slab)
        peaks = [BF16_MFMA_PEAK_TFLOPS, BF16_MFMA_PEAK_TFLOPS / 3.0, BF16_MFMA_PEAK_TFLOPS / 3.0, None]

        def encoder_table(bits):
            n_patches = bits.numel() // 64
            for _ in range(3):
                eng.encode_profile(bits, group=3)
            prof = np.array([eng.encode_profile(bits, group=3)[1] for _ in range(20)])
            ms_avg = prof[:, 0:4].mean(axis=0)
            mfma_exec = float(prof[:, 4].mean()) * 1e6                 # MFMA instructions stage 1 executed (counted by the kernel)
            flop_per_mfma = float(prof[0, 5])
            flops = n_patches * np.array([FLOP_CONV1 + FLOP_CONV2, FLOP_CONV3, FLOP_DENSE1, FLOP_DENSE2])
            alg_tf = flops / (ms_avg * 1e-3) / 1e12
            # what each kernel's matrix pipe actually did, against the peak of THAT pipe (always <= 1):
            #   stage 1: the FLOPs of the v_mfma_f32_16x16x32_f16 instructions it executed (it skips all-background rows exactly)
            #   conv3 / Dense(200): f32-equivalent rate against the pipe's peak / MFMAs per f32 product block
            exec_tf = [mfma_exec * flop_per_mfma / (ms_avg[0] * 1e-3) / 1e12, alg_tf[1], alg_tf[2], None]
            table = {}
            for i, nme in enumerate(names):
                table[nme] = {"ms": round(float(ms_avg[i]), 4), "algorithmic_tflops": round(float(alg_tf[i]), 2)}
                if peaks[i]:
                    table[nme].update({"pipe_tflops": round(float(exec_tf[i]), 2), "pipe_peak": round(peaks[i], 1),
                                       "pipe_frac": round(float(exec_tf[i] / peaks[i]), 4)})
            # dense conv2 as three f16 MFMAs per (m-tile, tap row): 32 m-tiles x 9 rows x 3 (+ conv1: 16 per 16 queued cells)
            return table, ms_avg, alg_tf, mfma_exec / (n_patches * 32 * 9 * 3), n_patches

        def frame_patches(p):
            return eng.patches(eng.voxelize(p)[0], eng.extract(p).key_pts.contiguous())[0]

        frame_bits = [frame_patches(pool[i]) for i in range(min(POOL, B))]
        one_table, one_ms, _, _, _ = encoder_table(frame_bits[0])
        batch_bits = torch.cat([frame_bits[i % len(frame_bits)].reshape(-1, 64) for i in range(B)], dim=0).contiguous()
        table, ms_avg, alg_tf, exec_share, n_patches = encoder_table(batch_bits)
        dom = int(np.argmax(ms_avg))
        # share of the patches of a batch (B different consecutive scans) that are copies of another patch of the batch; and of
        # a frame alone (what round 2 exploited)
        distinct = [len(torch.unique(b.reshape(-1, 64), dim=0)) for b in frame_bits]
        dedup_share_frame = round(1.0 - float(np.mean(distinct)) / 3072.0, 4)
        dedup_share = round(1.0 - len(torch.unique(batch_bits.reshape(-1, 64), dim=0)) / float(batch_bits.numel() // 64), 4)
        # HBM traffic and matrix-pipe busy share by the hardware counters: measured NOW by three rocprofv3 --pmc passes of the same
        # launch shapes in sub-processes (tools/pmc_live.py); only when rocprofv3 is missing or a pass fails, the committed file of an
        # earlier round -- marked stale_possible
        pmc_live = None
        if not args.no_pmc and world == 1:
            try:
                sys.path.insert(0, os.path.join(REPO, "tools"))
                import pmc_live as _pmc
                torch.cuda.synchronize()
                pmc_live = _pmc.collect()
            except Exception as e:   # never let a measurement aid take the line down
                print("bench.py: pmc_live failed: %s" % e, file=sys.stderr)
        traffic, traffic_note, stale = None, None, True
        if pmc_live and names[dom] in pmc_live["kernels"] and "fetch_kb" in pmc_live["kernels"][names[dom]]:
            k = pmc_live["kernels"][names[dom]]
            traffic = int((k["fetch_kb_corrected"] + k.get("write_kb", 0.0)) * 1024)
            traffic_note, stale = pmc_live["source"], False
        else:
            for pmc_file in ("r05_pmc_live.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json"):
                try:
                    pmc = json.load(open(os.path.join(REPO, "profiles", pmc_file)))
                    k = pmc["kernels"][names[dom]] if names[dom] in pmc["kernels"] else pmc["kernels"][names[dom].rstrip("x")]
                    traffic = int((k.get("fetch_kb_corrected", 2.0 * k.get("FETCH_SIZE_KB", 0.0)) + k.get("write_kb", k.get("WRITE_SIZE_KB", 0.0))) * 1024)
                    traffic_note = "profiles/%s (committed; not measured in this run)" % pmc_file
                    break
                except Exception:
                    pass
        busy = ({k: v["mfma_busy"] for k, v in pmc_live["kernels"].items() if "mfma_busy" in v} if pmc_live else None) or _pmc_busy()
        if pmc_live and busy is not None:
            busy["source"] = pmc_live["source"]
        # the NN match in the pipeline's launch shape (B pairs behind one k_match_prep + one k_match_screen launch), HIP events
        chain = [eng.extract(pool[i]) for i in range(min(POOL, B + 1))]
        m_ms, m_prep, _ = eng.match_profile(chain, repeats=30)
        m_pairs = len(chain) - 1
        m_flop = m_pairs * 2.0 * 1024 * 1024 * 60           # 2 K0 K1 60 per pair (0.1258 GFLOP)
        m_screen_ms = m_ms - m_prep
        mk = (pmc_live or {}).get("kernels", {}).get("k_match_screen", {})
        roofline_match = {
            "bound": "mfma", "kernel": "k_match_screen", "unit": "TFLOP/s",
            "achieved": round(m_flop / (m_screen_ms * 1e-3) / 1e12, 2), "peak": F32_MFMA_PEAK_TFLOPS,
            "frac": round(m_flop / (m_screen_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4),
            "achieved_is": "SURVEY 8d's algorithmic FLOPs of the all-pairs distance matrix (2 x 1024 x 1024 x 60 per pair) / the screen kernel's launch "
                           "time, against the f32 matrix peak (the reference computes it in float64: cdist); the kernel evaluates every product "
                           "from 2-way f16 splits -- 3 v_mfma_f32_16x16x32_f16 per 16 x 16 x 64 block, in each of two sweeps -- and certifies the argmin in float64",
            "launch": "%d pairs per launch (the pipeline's shape)" % m_pairs, "launch_ms": round(m_screen_ms, 4), "prep_ms": round(m_prep, 4),
            "frac_of_f16_pipe_executed": round(m_pairs * 2.0 * (1024 * 1024 * 64 * 2.0 * 3) / (m_screen_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
            "traffic": int((mk["fetch_kb_corrected"] + mk.get("write_kb", 0.0)) * 1024) if "fetch_kb" in mk else None,
            "traffic_unit": "bytes/launch", "algorithmic_bytes": m_pairs * (2 * 1024 * 60 * 4 + 1024 * 8),
            "mfma_busy_pmc": mk.get("mfma_busy"), "stale_possible": False if pmc_live else None}
        roofline = {"bound": "mfma", "kernel": names[dom], "achieved": table[names[dom]]["pipe_tflops"],
                    "peak": table[names[dom]]["pipe_peak"], "unit": "TFLOP/s", "frac": table[names[dom]]["pipe_frac"],
                    "traffic": traffic, "traffic_unit": "bytes/launch", "traffic_source": traffic_note, "stale_possible": stale,
                    "algorithmic_bytes": int(n_patches * 512 + n_patches * 4096),
                    "algorithmic_bytes_note": "bit-packed patches in (512 B each) + P2 out (4 KB each): what this kernel must move as the encoder is split today",
                    # SURVEY 8d's definition next to the executed-instruction one: algorithmic FLOPs (dense Keras conv1 + conv2) per launch / launch time
                    "algorithmic_frac_f32": round(float(alg_tf[dom]) / F32_MFMA_PEAK_TFLOPS, 3),
                    "algorithmic_frac_pipe": round(float(alg_tf[dom]) / BF16_MFMA_PEAK_TFLOPS, 4),
                    "algorithmic_frac_note": "algorithmic_frac_f32 = algorithmic_tflops / 157.3 (f32 matrix peak, the path's arithmetic type); above 1 because "
                                             "the kernel does NOT do the dense f32 work: all-background tap rows are skipped exactly (an added zero) and every "
                                             "product runs as 2-way f16 splits on the f16 pipe; algorithmic_frac_pipe = the same FLOPs against that pipe's 2500; "
                                             "`frac` = executed MFMA FLOPs / 2500",
                    "launch": "%d frames = %d patches per launch, as the timed region issues it (every patch: without de-duplication)" % (B, n_patches),
                    "launch_ms": round(float(ms_avg[dom]), 4),
                    "achieved_is": "FLOPs of the MFMA instructions the kernel EXECUTED (counted by the kernel: v_mfma_f32_16x16x32_f16, "
                                   "16 384 FLOP each) / launch time, against the dense peak of the f16 / bf16 matrix pipe; always <= 1.  "
                                   "Round 3 moved stage 1 from the f32 pipe (0.39 of 157 TFLOP/s, 341 us) to 2-way f16 splits (224 us), round 4 to "
                                   "three workgroups per CU and plane-wise fragment fetches (195 us).  Round 6 found 30 us of every one of those figures in "
                                   "the MEASUREMENT: the profiled instantiation of the kernel ended each wavefront with an atomic on one counter word "
                                   "(3 072 same-address atomics, ~12 ns each); counted per workgroup on eight lines the same kernel takes 155-170 us "
                                   "(profiles/r06_s1x_ablation.txt), as the production instantiation always did.  The pipe is not what bounds the "
                                   "kernel (LDS round trips and instruction issue do)",
                    "pipe_rate_in_a_bare_loop": {"tflops": 2420.0, "source": "profiles/r04_mfma_rates.txt (tools/micro/mfma_rates.hip): v_mfma_f32_16x16x32_f16 and "
                                                 "v_mfma_f32_32x32x16_f16 both sustain 2.41-2.44 PFLOP/s on this chip; `peak` stays the guide's dense figure"},
                    "algorithmic_tflops": round(float(alg_tf[dom]), 2),
                    "algorithmic_note": "dense Keras FLOPs of the layers the kernel replaces / launch time; stage 1 executes %.1f %% of "
                                        "the dense conv2 MFMAs on this scene (all-background rows add exact zeros and are skipped)" % (100.0 * exec_share),
                    "executed_mfma_share": round(exec_share, 4), "scene": args.scene,
                    "mfma_busy_pmc": busy,
                    "encoder_kernels": table,
                    "encoder_total_ms_all_patches": round(float(ms_avg.sum()), 4),
                    "single_frame_launch": {"patches": 3072, "frac": one_table[names[dom]].get("pipe_frac"),
                                            "launch_ms": round(float(one_ms[dom]), 4), "encoder_kernels": one_table,
                                            "encoder_total_ms_all_patches": round(float(one_ms.sum()), 4)}}
        # ---- secondary legs: other configs / scenes / shortcuts through the SAME pipeline object, after the timed region, never
        # part of `value` (one driver-written record carries them all)
        if world == 1 and not args.no_secondary:
            gc.disable()      # (the legs' timed stretches are 15-250 ms long: a cycle collection inside one is a visible share of it)
            try:
                secondary = secondary_legs(args, eng, pipe, dev, pool, rand, rand_host, Runner, frame_patches, encoder_table, host_scans, names)
            finally:
                gc.enable()
        if world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baseline()
    if rank == 0:
        out = {
            "metric": "KITTI frames/sec end-to-end (keypts+desc+match+RANSAC)" if not args.extract_only else
                      "KITTI frames/sec keypoint+descriptor extraction only (configs[1])",
            "value": round(world * K / dt, 2), "unit": "frames/s", "n_gpus": world, "steps": steps_rank, "warmup": args.warmup,
            "ms_per_step": round(dt / steps_rank * 1e3, 4), "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[2]: KITTI-seq-00-shaped full odometry (extract + NN match + RANSAC pose) on "
                                   "synthetic 64-beam x 2000-azimuth scans, coordinates quantised to 1 mm (points on voxel "
                                   "faces in every frame, as in real scans); scene: %s" % args.scene,
                       "step": "one batch of %d consecutive frames = one launch set of the pipeline (front kernels, encoder, match + RANSAC)" % B,
                       "frames_per_step": B, "frames_timed_per_gpu": K, "timed_region_ms": round(dt * 1e3, 3),
                       "arithmetic": "f32 in / out / accumulate; conv1, conv2, conv3 and Dense(200) evaluate every f32 product from 2-way f16 "
                                     "operand splits (|x - hi - lo| <= max(2^-22 |x|, 2^-25): the low half of a small value is an f16 subnormal) on the f16 matrix "
                                     "pipe -- f32-grade (descriptors 1.5e-6 from the f32 oracle, which is itself 1.3e-6 from an f64 "
                                     "evaluation; per-layer budget in tests); NN match: f16 screen + float64 certification = the float64 argmin",
                       "dedup": "bit-identical patches of a batch of frames are encoded once (exact; DESIGN.md 4.7, 4.13; no batch "
                                "holds a scan twice); the roofline object times the encoder kernels on all 3072 patches of every frame",
                       "dedup_share": dedup_share, "dedup_share_within_frames": dedup_share_frame,
                       "value_no_dedup": (secondary or {}).get("no_dedup", {}).get("frames_per_s"),
                       "value_no_dedup_note": None if dedup_share is None else
                                              "the same workload with every patch encoded (secondary.no_dedup): the rate to expect from a scene without "
                                              "equal patches; `value` exploits that %.0f %% of this scene's patches are copies of another patch of their batch" % (100.0 * dedup_share),
                       "uploads_in_timed_region": bool(args.include_h2d),
                       "trajectory": TRAJECTORY + " (caelo.synth.sensor_pose: structure at every frame index; closed after %d frames)" % synth.CIRCUIT_PERIOD,
                       "scan_indices_per_rank": [[r * K, r * K + POOL - 1] for r in range(world)],
                       "scan_indices_note": "rank r's pool = the %d consecutive scans [r K, r K + %d] of the endless synthetic sequence (K = frames per "
                                            "rank), walked back and forth; every one of them has >= 22 %% non-ground returns "
                                            "(tests/test_synth_world.py)" % (POOL, POOL - 1),
                       "points_per_frame": n_points, "keypoints": 1024, "patches_per_frame": 3072,
                       "frames_per_gpu": K, "hip_streams_per_gpu": host["streams"], "hip_streams_note": streams_note,
                       "frames_per_launch": B, "host_issue_us_per_frame": round(host["issue_us_per_frame"], 1),
                       "parallelism": "frames sharded x%d, one RCCL all-gather of %s [1024,64] f32 frame rows" % (
                           world, "the boundary" if args.gather == "boundary" else "all"),
                       "collective": collective, "per_rank_frames_per_s": per_rank_fps,
                       "poses_solved": "%d/%d" % (ok, K), "status_bits": status, "frames_flagged": frames_flagged,
                       "lane_faults": lane_faults,
                       "exact_ransac_note": certify_note,
                       "exact_ransac": None if cert is None else {
                           "what": "every pair of the timed region: the kernels score the 500 hypotheses and bound what the reference's float32 / BLAS "
                                   "arithmetic can give each (certificate); the pipeline's certifier threads replay Match.py:181-214 over the bounds and "
                                   "re-evaluate the deciding hypotheses through NumPy's own cblas_sgemm / cblas_sgemv / dgesdd while later batches run: "
                                   "inlier sets, R_star / T_star and refits are the reference's bits; inside the timed region",
                           "pairs": cert["pairs"], "host_hypotheses_per_pair": round(cert["evals_per_pair"], 2),
                           "certifier_thread_us_per_pair": round(cert["host_us_per_pair"], 1), "bound_violations": eng.bound_violations(),
                           "blas": (eng.host_blas() or {}).get("library")}},
            "roofline": roofline, "roofline_match": roofline_match, "cpu_baseline": cpu, "secondary": secondary,
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _make_scan_job(job):
    """(worker process of the resident_4541 leg) one synthetic scan"""
    from caelo import synth as _synth
    frame, quantum, scene = job
    return _synth.make_scan(frame % _synth.CIRCUIT_PERIOD, seed=frame, quantum=quantum, scene_kind=scene, trajectory=TRAJECTORY)


class Staging:
    """Where a loader leaves the scans (run_sequence.py's does): a RING of pinned batch slots at a fixed pitch, so that the scans of a
    batch go up behind one copy command (Pipeline.run_uploading; eight commands per batch cost the pipeline 20 %,
    tools/upload_contention_probe.py).  The runner's walk over the pool is periodic, so one period of it IS the ring: slot s holds
    scan walk(s + 1), a batch that starts at walk position p reads slots p .. p + B - 1 (mod the period), and nothing has to be
    refilled while the clock runs.  Like any ring the device has read its pages before (one untimed pass here): the FIRST device read
    of freshly pinned pages is slow when they are 4 KB pages -- a 60-batch run over a block read once took 30 or 120 ms, process by
    process, depending on whether the kernel had huge pages for it."""

    def __init__(self, host_pool, batch, walk_fn, device):
        P = len(host_pool)
        period = 2 * (P - 1)
        self.L = period * batch // math.gcd(period, batch)
        cap = max(int(p.shape[0]) for p in host_pool)
        self.block = torch.empty((self.L, cap, 4), dtype=torch.float32, pin_memory=True)
        self.rows = []
        for s_ in range(self.L):
            src = host_pool[walk_fn(s_ + 1, P)]
            self.block[s_, :src.shape[0]] = src
            self.rows.append(int(src.shape[0]))
        scratch = torch.empty((batch, cap, 4), dtype=torch.float32, device=device)
        for s0 in range(0, self.L, batch):
            scratch.copy_(self.block[s0:s0 + batch], non_blocking=True)
        torch.cuda.synchronize()

    def views(self, pos, n):
        return [self.block[(pos + i) % self.L][:self.rows[(pos + i) % self.L]] for i in range(n)]


def run_with_uploads(eng, pipe, runner, staging, n, out, rand, pairs=True):
    """The timed region with every scan coming from pinned host memory (Pipeline.run_uploading: a copy stream uploads batch
    b + 4 while the pipeline works on batch b, like the producer process of PoseEstimation.py:214-245)."""
    scans = staging.views(runner.pos, n)
    order = runner.order(n)
    pipe.run_uploading(scans, [rand[j] for j in order], prev=runner.prev if pairs else None, pairs=pairs, out=out,
                       certify=pairs and CERTIFY)
    runner.prev = out.frame(n - 1)
    return out


def secondary_legs(args, eng, pipe, dev, pool, rand, rand_host, Runner, frame_patches, encoder_table, host_scans, names):
    """Short legs after the timed region (each 32 batches, synchronised on both sides); frames/s each, plus what the scene does to
    the shortcuts (distinct patches, executed MFMA share) and the stage-1 time on it."""
    B, n = pipe.batch, 32 * pipe.batch

    def leg(runner, **kw):
        runner.run(2 * B, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.run(n, **kw)
        torch.cuda.synchronize()
        return round(n / (time.perf_counter() - t0), 1)

    sec = {"frames_per_leg": n, "note": "after the timed region, same pipeline object, %d frames each, not part of `value`" % n}
    sec["extract"] = {"frames_per_s": leg(Runner(pool), pairs=False), "workload": "configs[1]: keypoints + descriptors only"}
    sec["no_dedup"] = {"frames_per_s": leg(Runner(pool, dedup=False)), "workload": "configs[2] with every patch encoded (CAELO_EXTRACT_NO_DEDUP)"}
    if host_scans is None:
        host_scans = [p.cpu() for p in pool]
    r = Runner(pool)
    staged = Staging(host_scans, B, Runner.walk, dev)
    ob = FrameBatch(eng, n)
    run_with_uploads(eng, pipe, r, staged, 4 * B, FrameBatch(eng, 4 * B), rand)
    torch.cuda.synchronize()
    # three identical runs, all listed, the median quoted: ONE copy call of one of the first runs stalls for ~7 ms inside the runtime
    # (nothing of ours waits there; warm-ups of 4-32 batches do not prevent it, later runs never see it again) -- 40 % of a 16 ms leg,
    # nothing of a sequence
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_with_uploads(eng, pipe, r, staged, n, ob, rand)
        torch.cuda.synchronize()
        runs.append(round(n / (time.perf_counter() - t0), 1))
        if os.environ.get("CAELO_BENCH_VERBOSE"):
            print("include_h2d leg: %s" % pipe.last_upload_times, file=sys.stderr)
    sec["include_h2d"] = {"frames_per_s": float(np.median(runs)), "best_frames_per_s": max(runs), "runs_frames_per_s": runs,
                          "workload": "configs[2] with every scan uploaded from pinned host memory on a copy stream (one copy command per batch of "
                                      "eight: the scans of a batch sit in one slot of a pinned ring, as run_sequence.py's loader leaves them), four batches "
                                      "ahead; MEDIAN of three identical runs (all listed: one copy call of an early run stalls ~7 ms inside the runtime)"}
    del staged
    other = "clutter" if args.scene == "boxes" else "boxes"
    # (from scan 96 on: a stretch of the circuit where the clutter family's 496-nearest cuts DO split tie classes -- 7 of the frames 98..107,
    # profiles/r06_tie_redo_check_clutter_600.txt -- so that the leg exercises the redo; scans 0..16 hold none)
    pool2 = [torch.from_numpy(scan_at(96 + i, quantum=QUANTUM, scene_kind=other)).to(dev) for i in range(POOL)]
    r2 = Runner(pool2)

    def leg_exact_ties(runner):
        """like leg(), plus what makes the other scene's figure a reference-exact one: frames whose 496-nearest cut splits a class of
        equidistant voxels (flag bit 2: the fused path used its canonical rule) are redone in scikit-learn's kd-tree order
        (Engine.resolve_ties) and the pairs they are part of matched again -- inside the timed stretch"""
        runner.run(2 * B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ob_ = runner.run(n)
        tied, patches = eng.resolve_ties_many([(ob_.frame(j), runner.pool[runner.last_order[j]]) for j in range(n)], batch=ob_)
        patches = sum(patches)
        redo = sorted({t for u in tied for t in (u, u + 1) if 0 < t < n})
        if redo:
            o_ = [runner.last_order[j] % POOL for j in redo]
            if CERTIFY:
                rs_, ms_, xs_ = eng.match_pose_exact_many([(ob_.frame(j - 1), ob_.frame(j)) for j in redo], [rand[o] for o in o_], [rand_host[o] for o in o_])
                sel = torch.tensor(redo, device=dev)
                ob_.result[sel] = torch.from_numpy(rs_.view(np.uint8).reshape(len(redo), -1).copy()).to(dev)
                ob_.inlier_mask[sel] = torch.from_numpy(ms_).to(dev)
                for j, x_ in zip(redo, xs_):
                    ob_.pair_idx[j].copy_(x_)
            else:
                for j, o in zip(redo, o_):
                    r_, m_, x_ = eng.match_pose(ob_.frame(j - 1), ob_.frame(j), rand[o])
                    ob_.result[j].copy_(r_); ob_.inlier_mask[j].copy_(m_); ob_.pair_idx[j].copy_(x_)
        torch.cuda.synchronize()
        if os.environ.get("CAELO_BENCH_VERBOSE"):
            print("leg_exact_ties: total %.1f ms, tie redo %s" % (1e3 * (time.perf_counter() - t0), getattr(eng, "last_tie_times", None)), file=sys.stderr)
        return round(n / (time.perf_counter() - t0), 1), len(tied), patches, len(redo)

    leg_exact_ties(r2)          # (first use of the redo path: the side streams' voxel maps are allocated here, like any warm-up)
    fps2, frames_redone, patches_redone, pairs_redone = leg_exact_ties(r2)
    ob = r2.run(2 * B)
    torch.cuda.synchronize()
    ok2 = (int((ob.exact[0]["success"][:2 * B] != 0).sum()) if ob.exact is not None else
           sum(int(eng.pose_result(ob.result[i]).success) for i in range(2 * B)))
    bits2 = [frame_patches(p) for p in pool2[:min(POOL, B)]]
    t2, ms2, _, share2, _ = encoder_table(torch.cat([bits2[i % len(bits2)].reshape(-1, 64) for i in range(B)], dim=0).contiguous())
    sec["scene_" + other] = {"frames_per_s": fps2, "poses_solved": "%d/%d" % (ok2, 2 * B),
                             "frames_redone": frames_redone, "tie_split_patches_redone": patches_redone, "pairs_rematched": pairs_redone,
                             "frames_redone_note": "frames whose 496-nearest cut splits a tie class, redone in scikit-learn's kd-tree order inside the timed "
                                                   "stretch on 8 side streams (Engine.resolve_ties_many; Voxel.py:195-196), their pairs matched and certified again: a reference-exact figure",
                             "workload": "configs[2] on the other synthetic scene (%s)" % other,
                             "dedup_share": round(1.0 - len(torch.unique(torch.cat([b.reshape(-1, 64) for b in bits2]), dim=0)) / float(3072 * len(bits2)), 4),
                             "dedup_share_within_frames": round(1.0 - float(np.mean([len(torch.unique(b.reshape(-1, 64), dim=0)) for b in bits2])) / 3072.0, 4),
                             "executed_mfma_share": round(share2, 4), "stage1_launch_ms": round(float(ms2[0]), 4),
                             "stage1_pipe_frac": t2[names[0]]["pipe_frac"], "encoder_total_ms_all_patches": round(float(ms2.sum()), 4)}
    # ---- failing_pairs: hostile data.  One scan of the pool is replaced by a scan of ANOTHER world: the two pairs it
    # is part of find no consensus at 0.4 m, escalate to 0.8 and 1.6 m and fail as a value (Match.py:207-214) -- 2 of every 16 pairs of the
    # walk.  Round 5's host half evaluated the ~1000 hypotheses of the higher levels of such a pair like the reference's loop (5 ms of a
    # certifier thread); round 6's kernels leave bounds for those levels too (k_ransac_hyp_up)
    try:
        pool3 = list(pool)
        pool3[POOL // 2] = pool2[0]
        r3 = Runner(pool3)
        r3.run(2 * B)
        torch.cuda.synchronize()
        pipe.cert_stats()
        t0 = time.perf_counter()
        ob3 = r3.run(n)
        torch.cuda.synchronize()
        dt3 = time.perf_counter() - t0
        cs3 = pipe.cert_stats() if CERTIFY else None
        thr3 = ob3.exact[0]["threshold"][:n] if ob3.exact is not None else None
        sec["failing_pairs"] = {"frames_per_s": round(n / dt3, 1),
                                "pairs_failed": None if ob3.exact is None else int((ob3.exact[0]["success"][:n] == 0).sum()),
                                "pairs_beyond_0.4m": None if thr3 is None else int((thr3 > 0.5).sum()),
                                "host_hypotheses_per_pair": None if cs3 is None else round(cs3["evals_per_pair"], 2),
                                "certifier_thread_us_per_pair": None if cs3 is None else round(cs3["host_us_per_pair"], 1),
                                "workload": "configs[2] with one scan of the 17-scan pool replaced by a scan of another world: its two pairs escalate "
                                            "through 0.8 and 1.6 m and fail as a value (Match.py:207-214); exact RANSAC included"}
    except Exception as e:
        sec["failing_pairs"] = {"error": str(e)[:200]}
    # ---- resident_4541: a KITTI-00-sized run (4 541 frames = 568 batches, > 0.2 s of GPU time) over a pool of 161 DISTINCT scans
    # (2 MB each: 320 MB of points, more than the 256 MB Infinity Cache) walked back and forth -- what the 17-scan pool of the timed
    # region cannot show: whether the rate depends on the scans staying on-die
    try:
        import concurrent.futures as cf
        import multiprocessing as mp
        big_n = 20 * B + 1
        t0 = time.perf_counter()
        with cf.ProcessPoolExecutor(min(32, max(1, (os.cpu_count() or 2) // 2)), mp_context=mp.get_context("spawn")) as ex:
            big_np = list(ex.map(_make_scan_job, [(300 + i, QUANTUM, args.scene) for i in range(big_n)], chunksize=4))
        t_synth = time.perf_counter() - t0
        big = [torch.from_numpy(a).to(dev) for a in big_np]
        rb = Runner(big)
        n_big = 4541 // B * B + B          # 4 544: whole batches
        rb.run(4 * B)
        torch.cuda.synchronize()
        out_big = FrameBatch(eng, n_big)
        t0 = time.perf_counter()
        ob_big = rb.run(n_big, out=out_big)
        torch.cuda.synchronize()
        dt_big = time.perf_counter() - t0
        ok_big = int((ob_big.exact[0]["success"][:n_big] != 0).sum()) if ob_big.exact is not None else None
        sec["resident_4541"] = {"frames_per_s": round(n_big / dt_big, 1), "frames": n_big, "seconds": round(dt_big, 4), "distinct_scans": big_n,
                                "scan_bytes_resident": int(sum(a.numel() * 4 for a in big)), "poses_solved": ok_big,
                                "workload": "configs[2] at KITTI-00 length over %d distinct resident scans (%.0f MB of points > the 256 MB Infinity Cache), "
                                            "walked back and forth; exact RANSAC included" % (big_n, sum(a.numel() * 4 for a in big) / 1e6),
                                "scan_synthesis_s_not_timed": round(t_synth, 2)}
        del big, out_big, ob_big
    except Exception as e:
        sec["resident_4541"] = {"error": str(e)[:200]}
    # configs[4]: one frame's time through the 32^3 path (bench.py --config dense128 gives its own full line)
    try:
        pc128 = torch.from_numpy(scan_at(0, n_beams=128, n_az=4000, quantum=QUANTUM)).to(dev)
        wd1, bd1 = eng.seeded_dense1_32()
        eng.set_encoder32_dense(wd1, bd1)
        for _ in range(2):
            eng.extract32(pc128)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            eng.extract32(pc128)
        torch.cuda.synchronize()
        sec["dense128"] = {"frames_per_s": round(8 / (time.perf_counter() - t0), 1),
                           "workload": "configs[4]: 128-beam x 4000-azimuth scan, 32^3 patches (one stream, staged calls)"}
    except Exception as e:     # never let a secondary leg take the headline line down
        sec["dense128"] = {"error": str(e)[:200]}
    return sec


if __name__ == "__main__":
    main()
