"""GPU: the frame pipeline's hand-offs when one stage falls behind.

Every other pipeline test runs under normal timing, where each stage keeps up with the others.  Here one stream at a time -- front,
encoder, pair, voxel maps, the upload copy stream or the caller's stream -- is held back by one bounded busy kernel (~200 ms,
calibrated once) enqueued BEFORE the call, so that all of that stage's work of the call queues behind it while the host issues every
batch.  Whatever a stage reads must still be what the unstalled run read: every output equals the unstalled run bit for bit.

The cases run in ONE child process started with GPU_MAX_HW_QUEUES=8.  HIP deals its streams onto the hardware queues; with the
default four, the pipeline's stages, the copy stream, the certificate stream and the caller's stream share queues, and a stall on one
stream also holds back whatever shares its queue -- the copy that overwrites a slot, say, which hides exactly the races these tests are
for.  With eight queues every stream here has a queue of its own, and the pipeline also creates its voxel stream,
which is then covered too.  The child writes its findings per group to a JSON file; each test below checks one group.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STALL_MS = 200          # the length of one stall: the host issues every batch of a case many times over meanwhile
SEED_BASE = 500         # pair (f - 1, f) draws RandomState(SEED_BASE + f - 1)
CERT_RING = 6           # batches whose certificates the pipeline holds at once (caelo_pipeline::CERT_RING, csrc/pipeline.hip)
STREAMS = ("none", "front", "encoder", "pair", "voxel", "copy", "caller")
GROUPS = ("run", "uploading", "loaded", "loaded_exact_patches", "loaded_twice", "loaded_min_keep", "oracle", "run_sequence")
FIELDS = ("rows", "key_pixels", "pair_idx", "inlier_mask", "result", "status")


# ---------------------------------------------------------------------------------------------------------------------------------
# the child process
# ---------------------------------------------------------------------------------------------------------------------------------
def _child(out_path, scan_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (os.path.join(repo, "cae-lo_amd"), os.path.join(repo, "oracle")):
        sys.path.insert(0, p)
    import caelo
    caelo.configure_runtime()
    import torch
    from caelo import _ffi, synth
    from caelo.engine import Engine, FrameBatch, SeqLoader, ransac_draws

    eng = Engine()
    dev = eng.device
    report = {"groups": {}}

    def save():
        with open(out_path + ".tmp", "w") as f:
            json.dump(report, f, indent=1)
        os.replace(out_path + ".tmp", out_path)

    # ---- one bounded stall: torch.cuda._sleep spins for a number of clock ticks; calibrated once against timing events
    def timed_sleep(cycles):
        s = torch.cuda.Stream(device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            torch.cuda._sleep(int(cycles))
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    timed_sleep(1000)                                   # (loads the kernel)
    probe = 20_000_000
    ms = timed_sleep(probe)
    cycles = int(probe * STALL_MS / max(ms, 1e-3))
    report["stall_ms"] = timed_sleep(cycles)
    save()
    assert 0.5 * STALL_MS <= report["stall_ms"] <= 2.0 * STALL_MS, report["stall_ms"]

    def stall(pipe, which):
        """One stall, enqueued before the call, on the named stream of `pipe`.  -> False when the pipeline has no such stream."""
        if which == "none":
            return True
        if which == "caller":
            torch.cuda._sleep(cycles)                   # (the current stream: what the pipeline's begin and flush hand over on)
            return True
        if which == "copy":
            if pipe._copy is None:
                pipe._copy = torch.cuda.Stream(device=dev)
            handle = pipe._copy.cuda_stream
        else:
            handle = pipe.streams()[which]
            if not handle:
                return False
        with torch.cuda.stream(torch.cuda.ExternalStream(handle, device=dev)):
            torch.cuda._sleep(cycles)
        return True

    # ---- the frames: distinct scans, in memory, on the device and as KITTI .bin files
    n_max = 59
    host = [synth.make_scan(i, quantum=1e-3) for i in range(n_max)]
    paths = []
    for i, pc in enumerate(host):
        paths.append(os.path.join(scan_dir, "%06d.bin" % i))
        pc.astype(np.float32).tofile(paths[-1])
    dscans = [torch.from_numpy(pc).to(dev) for pc in host]
    draws = [ransac_draws(max(SEED_BASE + f - 1, 0)) for f in range(n_max)]
    drand = [torch.from_numpy(d).to(dev) for d in draws]
    pinned = [torch.from_numpy(pc).pin_memory() for pc in host]
    cap = (max(pc.shape[0] for pc in host) + 1023) // 1024 * 1024
    block = torch.zeros((n_max, cap, 4), dtype=torch.float32).pin_memory()
    for i, pc in enumerate(pinned):
        block[i, :pc.shape[0]] = pc
    views = [block[i, :pc.shape[0]] for i, pc in enumerate(pinned)]
    report["streams"] = {k: bool(v) for k, v in eng.pipeline(4, 3).streams().items()}
    save()

    def snap(out, k, certify):
        torch.cuda.synchronize()
        d = {f: getattr(out, f)[:k].cpu().numpy().view(np.uint8).copy() for f in FIELDS}
        if certify:
            for i, a in enumerate(out.exact):
                d["exact%d" % i] = np.ascontiguousarray(a[:k]).view(np.uint8).copy()
        return d

    def join(a, b):
        return {f: np.concatenate([a[f], b[f]]) for f in a}

    def differ(want, got):
        bad = []
        for f in want:
            w, g = want[f], got[f]
            if w.shape != g.shape:
                bad.append("%s: shape %s != %s" % (f, w.shape, g.shape))
                continue
            rows_bad = np.flatnonzero((w.reshape(w.shape[0], -1) != g.reshape(g.shape[0], -1)).any(axis=1))
            if len(rows_bad):
                bad.append("%s: frames %s" % (f, rows_bad.tolist()))
        return bad

    refs = {}

    def reference(B, buffers, n, certify, exact_patches=False):
        key = (B, buffers, n, bool(certify), exact_patches)
        if key not in refs:
            pipe = eng.pipeline(B, buffers)
            kw = dict(certify=True, rands_host=draws[:n]) if certify else {}
            refs[key] = snap(pipe.run(dscans[:n], drand[:n], exact_patches=exact_patches, **kw), n, certify)
        return refs[key]

    def frames(B, ahead):
        """at least ahead + 4 batches, so that every device slot is reused, the last one partial"""
        return (ahead + 3) * B + max(1, B // 2 - 1)

    def group(name, cases):
        """cases: (label, fn) -> fn returns a list of findings (empty: as it should be)"""
        import time
        t0 = time.time()
        found = []
        for label, fn in cases:
            try:
                found += ["%s: %s" % (label, m) for m in fn()]
            except (_ffi.CaeloError, AssertionError, ValueError) as e:   # (a refusal or a wrong run: a finding of the case)
                found.append("%s: %s: %s" % (label, type(e).__name__, e))
                if "error -2:" in str(e):   # (CAELO_ERR_HIP: the device failed -- nothing more runs on it)
                    report["groups"][name] = found
                    save()
                    raise
        report["groups"][name] = found
        report.setdefault("seconds", {})[name] = round(time.time() - t0, 2)
        save()

    def loader(n, B, ring=4, keep=96):
        return SeqLoader(eng, paths[:n], batch=B, seed_base=SEED_BASE, threads=4, ring=ring, keep=keep, cap=cap)

    # ---- Pipeline.run on resident scans: pace -1 / 0 / 1, certify off / on
    def run_case(pace, certify, which):
        def fn():
            B, n = 4, 22
            pipe = eng.pipeline(B, 3)
            want = reference(B, 3, n, certify)
            old = pipe.pace
            pipe.set_pace(pace)
            try:
                if not stall(pipe, which):
                    return []
                kw = dict(certify=True, rands_host=draws[:n]) if certify else {}
                got = snap(pipe.run(dscans[:n], drand[:n], **kw), n, certify)
            finally:
                pipe.set_pace(old)
            return differ(want, got)
        return ("pace %d certify %d stall %s" % (pace, certify, which), fn)
    group("run", [run_case(p, c, w) for p in (-1, 0, 1) for c in (False, True) for w in STREAMS if w != "copy"])

    # ---- Pipeline.run_uploading: one copy per frame / one pitched block per batch
    def upload_case(layout, certify, which):
        def fn():
            B, ahead = 4, 4
            n = frames(B, ahead)
            pipe = eng.pipeline(B, 3)
            want = reference(B, 3, n, certify)
            src = pinned[:n] if layout == "frames" else views[:n]
            if not stall(pipe, which):
                return []
            kw = dict(certify=True, rands_host=draws[:n]) if certify else {}
            got = snap(pipe.run_uploading(src, drand[:n], ahead=ahead, **kw), n, certify)
            return differ(want, got)
        return ("%s certify %d stall %s" % (layout, certify, which), fn)
    group("uploading", [upload_case(lay, c, w) for lay in ("frames", "block") for c in (False, True) for w in STREAMS])

    # ---- Pipeline.run_loaded over a SeqLoader: batch 4 / 8, buffers 2 / 3, ahead 1 / 4
    def loaded_case(B, buffers, ahead, certify, which, exact_patches=False):
        def fn():
            n = frames(B, ahead)
            pipe = eng.pipeline(B, buffers)
            want = reference(B, buffers, n, certify, exact_patches)
            ld = loader(n, B)
            try:
                if not stall(pipe, which):
                    return []
                out, k = pipe.run_loaded(ld, 0, ld.n_batches, certify=certify, ahead=ahead, exact_patches=exact_patches)
                return differ(want, snap(out, k, certify))
            finally:
                ld.close()
        return ("batch %d buffers %d ahead %d certify %d stall %s" % (B, buffers, ahead, certify, which), fn)
    configs = ((4, 3, 4), (8, 2, 1), (4, 2, 1), (8, 3, 4))
    group("loaded", [loaded_case(B, bu, a, c, w) for B, bu, a in configs for c in (False, True) for w in STREAMS])
    group("loaded_exact_patches", [loaded_case(4, 3, 4, True, w, exact_patches=True) for w in ("none", "front", "encoder", "pair", "copy")])

    # ---- two run_loaded calls in a row, the second issued while the first call's pair stage is still held back: the second call
    # reuses the device slots (same ahead) or replaces them (another ahead: another slot count)
    def twice_case(ahead2, certify):
        def fn():
            B, ahead, n = 4, 4, frames(4, 4)
            pipe = eng.pipeline(B, 3)
            want = reference(B, 3, n, certify)
            ld = loader(n, B)
            try:
                stall(pipe, "pair")
                nb1 = 4
                out1, k1 = pipe.run_loaded(ld, 0, nb1, certify=certify, ahead=ahead)
                slots1 = pipe._slots[0]
                out2, k2 = pipe.run_loaded(ld, nb1, ld.n_batches - nb1, prev=out1.frame(k1 - 1), certify=certify, ahead=ahead2)
                found = differ(want, join(snap(out1, k1, certify), snap(out2, k2, certify)))
                if (pipe._slots[0] == slots1) != (ahead2 == ahead):
                    found.append("slot layout %s -> %s" % (slots1, pipe._slots[0]))
                return found
            finally:
                ld.close()
        return ("second call ahead %d certify %d" % (ahead2, certify), fn)
    group("loaded_twice", [twice_case(a2, c) for a2 in (4, 1) for c in (False, True)])

    # ---- the host copy of the draws (the certifier's) at the smallest ring the pipeline accepts, and one below it
    def min_keep_case(which):
        def fn():
            B, ahead, ring = 4, 4, 4
            n = frames(B, ahead)
            pipe = eng.pipeline(B, 3)
            want = reference(B, 3, n, True)
            keep = ring + CERT_RING + 1
            found = []
            ld = loader(n, B, ring=ring, keep=keep - 1)
            try:
                pipe.run_loaded(ld, 0, ld.n_batches, certify=True, ahead=ahead)
                found.append("keep %d (ring %d) was accepted" % (keep - 1, ring))
            except _ffi.CaeloError as e:
                if "keep" not in str(e):
                    found.append("refused for another reason: %s" % e)
            finally:
                ld.close()
            ld = loader(n, B, ring=ring, keep=keep)
            try:
                stall(pipe, which)
                out, k = pipe.run_loaded(ld, 0, ld.n_batches, certify=True, ahead=ahead)
                found += differ(want, snap(out, k, True))
            finally:
                ld.close()
            return found
        return ("stall %s" % which, fn)
    group("loaded_min_keep", [min_keep_case(w) for w in ("pair", "none")])

    # ---- a stalled loader run, certify off, against the plain float64 reference on the pipeline's own matches
    def oracle_case():
        import oracle as orc
        orc.build()
        B, ahead = 4, 4
        n = frames(B, ahead)
        pipe = eng.pipeline(B, 3)
        ld = loader(n, B)
        try:
            stall(pipe, "pair")
            out, k = pipe.run_loaded(ld, 0, ld.n_batches, certify=False, ahead=ahead)
            torch.cuda.synchronize()
        finally:
            ld.close()
        rows, pidx, nk = out.rows.cpu().numpy(), out.pair_idx.cpu().numpy(), out.n_key.cpu().numpy()
        res = out.result.cpu().numpy().view(_ffi.POSE_DTYPE).reshape(-1)
        mask = out.inlier_mask.cpu().numpy()
        found = []
        for f in (1, 3, B + 2, 2 * B + 1, n - 1):   # (batches 0 and 1: their device slots are the ones the run overwrites)
            N = int(nk[f])
            P0 = np.ascontiguousarray(rows[f - 1][pidx[f][:N], 60:63])
            P1 = np.ascontiguousarray(rows[f][:N, 60:63])
            R, T, ok, m, thr = orc.RANSAC4RT(P0, P1, rng=np.random.RandomState(SEED_BASE + f - 1))[:5]
            r = res[f]
            if bool(r["success"]) != bool(ok) or abs(float(r["threshold"]) - float(thr)) > 1e-6:
                found.append("frame %d: success / threshold %s %s vs %s %s" % (f, bool(r["success"]), float(r["threshold"]), bool(ok), thr))
            if not np.array_equal(mask[f, :N].astype(bool), np.asarray(m, bool)):
                found.append("frame %d: inlier set (%d vs %d)" % (f, int(mask[f, :N].sum()), int(np.asarray(m).sum())))
            if ok and (np.abs(r["R_ransac"].reshape(3, 3).astype(np.float64) - R).max() > 1e-4 or
                       np.abs(r["T_ransac"].reshape(3, 1).astype(np.float64) - T).max() > 1e-3):
                found.append("frame %d: R_star / T_star" % f)
        return found
    group("oracle", [("stall pair certify 0", oracle_case)])

    # ---- run_sequence's file loader (run_loaded, in chunks) under a stalled pair stage == its Python loader, unstalled
    def sequence_case(certify):
        def fn():
            import run_sequence as rs
            B, n = 4, 29

            def load(i):
                return host[i]
            want = rs.run_local(eng, load, 0, n, SEED_BASE, 32, 5, B, certify=certify)
            stall(eng.pipeline(B), "pair")   # (one chunk of 8 batches: the run reuses the device slots of its first two)
            got = rs.run_local_files(eng, paths, 0, n, SEED_BASE, 32, 5, B, certify=certify, loader_threads=4)
            return ["%s differs" % name for name, a, b in zip(("rel", "ok", "thr", "nin"), want[:4], got[:4])
                    if not np.array_equal(np.asarray(a), np.asarray(b))]
        return ("certify %d" % certify, fn)
    group("run_sequence", [sequence_case(c) for c in (False, True)])

    report["lane_faults"] = eng.lane_faults()
    report["done"] = True
    save()


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stall_report(tmp_path_factory):
    d = tmp_path_factory.mktemp("stalls")
    out = str(d / "report.json")
    scan_dir = d / "velodyne"
    scan_dir.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(scan_dir)], env=env, capture_output=True, text=True,
                          timeout=1200)
    report = json.load(open(out)) if os.path.exists(out) else {"groups": {}}
    report["returncode"] = proc.returncode
    report["stderr"] = proc.stderr[-3000:]
    return report


def test_stall_harness_reaches_every_stream(stall_report):
    """The child ran to the end, its stall lasted about STALL_MS, and the pipeline had every stream, the voxel stream included."""
    assert stall_report["returncode"] == 0 and stall_report.get("done"), stall_report["stderr"]
    assert 0.5 * STALL_MS <= stall_report["stall_ms"] <= 2.0 * STALL_MS
    assert all(stall_report["streams"].values()), stall_report["streams"]
    assert stall_report["lane_faults"] == 0


@pytest.mark.parametrize("name", GROUPS)
def test_stalled_stage_changes_no_result(stall_report, name):
    assert name in stall_report["groups"], "the child did not reach group %s: %s" % (name, stall_report["stderr"])
    assert stall_report["groups"][name] == []


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
