"""The front chain without a voxel stream: the voxel build runs in further workgroups of the key point chain's launches
(csrc/ring.hip: the k_front_* kernels; the build's bodies are csrc/voxel_front.inc).  It re-schedules, so every comparison here is on bits.

What the fused launches are compared with:
  (a) the staged single calls in this process (caelo_project, caelo_respond, caelo_keypoints, caelo_voxelize_fast, caelo_patches):
      they run the stand-alone kernels -- ring image, key points and pixels, n_key, status, patch bits and flags, the voxel sets of
      all three scales and the build's counters (caelo_voxmap_counts);
  (b) one child process under CAELO_PIPE_VOX_STREAM=1, the forked path (stand-alone kernels on two streams): rows, key pixels,
      n_key, flags and status of every frame of the pipeline runs below;
and the pipeline's frames (sets of 1, 2 and 8 frames per launch) with the single-frame extract of the same scan, which ties (b) to (a).

The frames are the smallest at which a shared launch can go wrong: 4, 255, 256, 257 and 1000 points (one workgroup of a role, the
edges of one), a thinned scan of ~21 k points, all of them mixed in one set so that every role has another number of live
workgroups in every frame; frames without, with 1, with 128 and with more than 128 points within an ulp of a voxel face (the LDS
list of vox_suspects_first and its table probe), several such points in one voxel behind a point that is not; a frame with no
pixel the key point rule's range gate passes and one where every occupied pixel passes; a NaN point; points on the faces of the
1.28 m blocks and outside the voxel volume.  The face points are found with a NumPy restatement of the index arithmetic
(float64 operations, the same on both sides) and the build's own counter of such points must agree with it.

The child is started the way tests/test_env_knobs_gpu.py starts its children: alone, under its own time limit; if it ends by signal,
abort or timeout the session ends there.  In a process that has a voxel stream of its own (8 or more hardware queues) the pipeline
tests skip: both sides would be the forked path.  The pipeline hands out no voxel map or patch buffer of a frame, so for sets of
more than one frame maps, counters, patch bits and tables are held through what is computed from them (rows, flags, status) and
through the single-frame extract of the same scan, which test (a) compares directly."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORKED = {"CAELO_PIPE_VOX_STREAM": "1"}
VIS = (99.84, 99.84, 14.72)
FIELDS = ("rows", "key_pixels", "n_key", "flags", "status")


# ---------------------------------------------------------------------------------------------------------------------------------
# the voxel index arithmetic restated (csrc/voxel_front.inc: voxel_indices; Voxel.py:118-152), to find points that are not consistent
# ---------------------------------------------------------------------------------------------------------------------------------
def _trunc_div(p, d):
    """int(p / d) in float64, truncated toward zero (vox_trunc_div returns exactly this: its multiply is only a shortcut)"""
    return np.trunc(p / d).astype(np.int64)


def voxel0(pts):
    """-> (scale-0 voxel index [n,3], inconsistent [n]): per point inside the volume and on the grid, whether its own scale-1 / 2
    indices differ from its scale-0 index >> 3 / >> 5"""
    pts = np.asarray(pts, np.float32)
    ok = np.isfinite(pts[:, :3]).all(1) & (np.abs(pts[:, 0]) <= np.float32(VIS[0])) & (np.abs(pts[:, 1]) <= np.float32(VIS[1])) \
        & (np.abs(pts[:, 2]) <= np.float32(VIS[2]))
    bad = np.zeros(len(pts), bool)
    g = np.zeros((len(pts), 3), np.int64)
    for a in range(3):
        p = np.where(ok, pts[:, a], 0).astype(np.float64) + VIS[a]
        b = _trunc_div(p, 1.28)
        rem = p - b * 1.28
        v = _trunc_div(rem, 0.02)
        ok &= (v >= 0) & (v < 64)
        g[:, a] = v + b * 64
        bad |= (_trunc_div(p, 0.02 * 8) != (g[:, a] >> 3)) | (_trunc_div(p, 0.02 * 32) != (g[:, a] >> 5))
    return g, ok & bad


def inconsistent(pts):
    return voxel0(pts)[1]


def face_points(n, seed):
    """n points within an ulp of a 0.16 m voxel face in x, each in a voxel of its own, that the restatement finds inconsistent"""
    k = np.arange(600 * 200)
    x = (np.float64(0.16) * (300 + k % 600) - VIS[0]).astype(np.float32)    # multiples of 0.16 m above the volume's corner
    cand = np.stack([x, (-40.0 + 0.37 * (k // 600)).astype(np.float32), np.full(len(k), -1.5 + 0.11 * seed, np.float32),
                     np.random.RandomState(seed).random_sample(len(k)).astype(np.float32)], 1)
    cand = cand[inconsistent(cand)]
    assert len(cand) >= n, "no face points found"
    return np.ascontiguousarray(cand[np.random.RandomState(seed).permutation(len(cand))[:n]])


def make_frames(scans):
    base = scans(0)                                     # float32 as synthesised: no point on a face
    quant = scans(1, quantum=1e-3)                      # mm-quantised: a few points on faces, as real scans have them
    thin = np.ascontiguousarray(base[::6])
    few = np.ascontiguousarray(base[::60])
    assert not inconsistent(thin).any() and 1 <= inconsistent(quant[::6]).sum() <= 128

    def pick(n):
        return np.ascontiguousarray(base[np.linspace(0, len(base) - 1, n).astype(np.int64)])

    def with_faces(n, seed):
        f = np.concatenate([few, face_points(n, seed)])
        return np.ascontiguousarray(f[np.random.RandomState(seed).permutation(len(f))])

    frames = {"n4": pick(4), "n255": pick(255), "n256": pick(256), "n257": pick(257), "n1000": pick(1000), "thin": thin,
              "quantised": np.ascontiguousarray(quant[::6]), "face1": with_faces(1, 1), "face128": with_faces(128, 2), "face300": with_faces(300, 3)}
    # several inconsistent points in one voxel, behind a consistent point of the same voxel (its first point decides)
    fp = face_points(2, 4)
    inside = fp.copy()
    for j in range(2):                                  # same 2 cm voxel, off the face (whichever side of it the voxel lies)
        for dx in (0.005, -0.005):
            inside[j, 0] = fp[j, 0] + np.float32(dx)
            if np.array_equal(voxel0(inside[j:j + 1])[0], voxel0(fp[j:j + 1])[0]):
                break
    assert not inconsistent(inside).any() and np.array_equal(voxel0(inside)[0], voxel0(fp)[0])
    frames["face_shared"] = np.ascontiguousarray(np.concatenate([few[:500], inside[:1], fp[:1], fp[:1], fp[:1], few[500:], fp[1:], fp[1:], inside[1:]]))
    near = thin.copy()
    near[:, :3] *= np.float32(0.05)                     # every range below 10 m: no pixel passes the gate
    frames["near"] = near
    r = np.sqrt((thin[:, :3].astype(np.float64) ** 2).sum(1))
    far = thin[(r >= 12.0) & (np.abs(thin[:, 2]) < 14.0)].copy()   # every occupied pixel passes it
    frames["far"] = np.ascontiguousarray(far)
    nan = thin.copy()
    nan[1234, 0] = np.nan
    frames["nan"] = nan
    edge = few.copy()                                   # block faces, the volume's own faces, points beyond them
    edge[10:16, 0] = np.float32([1.28 * 3 - 99.84, 99.84, -99.84, 150.0, -150.0, 1.28 * 77 - 99.84])
    edge[20:23, 2] = np.float32([14.72, -14.72, 20.0])
    frames["edge"] = edge
    return frames


SETS = (("n4",), ("thin", "n255"),
        ("n4", "thin", "n255", "face300", "n256", "quantised", "n257", "n1000"),
        ("face1", "near", "face128", "far", "nan", "edge", "face_shared", "thin"),
        ("quantised", "face300", "n1000", "near", "n4", "far", "thin", "face128"))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_sets(eng, pipe, frames, sets=SETS, workspaces=False):
    """each set through ``pipe`` (one after the other: every slot of it gets another tenant) -> per set, per field, host arrays;
    what lies behind a frame's n_key rows is not written by anyone (but the valid column, which is) and is zeroed here.
    ``workspaces``: also every frame's ring image (as uint32) and eligibility map, read before the next set runs (a set is one batch)"""
    import torch
    out = []
    for names in sets:
        res = pipe.run([torch.from_numpy(frames[n]).to(eng.device) for n in names], pairs=False)
        torch.cuda.synchronize()
        r = {f: getattr(res, f)[:len(names)].cpu().numpy().copy() for f in FIELDS}
        for j, k in enumerate(r["n_key"]):
            r["rows"][j, k:, :63] = 0
            r["key_pixels"][j, k:] = 0
            r["flags"][j, k:] = 0
        if workspaces:
            assert len(names) <= pipe.batch
            both = [pipe.extract_ring_and_map(j) for j in range(len(names))]
            r["ring"], r["elig"] = [b[0].view(np.uint32).ravel() for b in both], [b[1] for b in both]
        out.append(r)
    return out


def _digests(results):
    return {"set %d %s" % (i, f): _sha(r[f]) for i, r in enumerate(results) for f in FIELDS}


def _child(frame_file):
    for p in (os.path.join(REPO, "cae-lo_amd"), os.path.join(REPO, "oracle")):
        sys.path.insert(0, p)
    import caelo
    caelo.configure_runtime()
    from caelo.engine import Engine
    eng = Engine()
    z = np.load(frame_file)
    pipe = eng.pipeline(8, 3)
    d = _digests(run_sets(eng, pipe, {k: z[k] for k in z.files}))
    d["voxel stream"] = str(pipe.streams()["voxel"] is not None)
    d["lane faults"] = str(eng.lane_faults())
    print("DIGESTS " + json.dumps(d))


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(scans):
    return make_frames(scans)


@pytest.fixture(scope="module")
def fused_sets(engine, frames):
    """The sets through the engine's pipeline in this process (default environment: no voxel stream, the fused launches)."""
    pipe = engine.pipeline(8, 3)
    if pipe.streams()["voxel"] is not None:
        pytest.skip("this process builds its voxel maps on a voxel stream (8 or more hardware queues): the pipeline would run the forked "
                    "path here as well, and every comparison with it would be forked against forked")
    return run_sets(engine, pipe, frames, workspaces=True)


@pytest.fixture(scope="module")
def single(engine, frames):
    """name -> the single-frame fused extract (a set of one on the caller's stream) and what it left behind"""
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            pc = torch.from_numpy(frames[name]).to(engine.device)
            vmap = engine.voxmap(slot="fused")
            f = engine.extract(pc, vmap=vmap)
            ws = engine._ws("extract", int(engine.lib.caelo_extract_ws_bytes()))
            off = int(engine.lib.caelo_extract_ws_ring_offset())
            torch.cuda.synchronize()
            cache[name] = dict(
                rows=f.rows.cpu().numpy(), key_pixels=f.key_pixels.cpu().numpy(), n_key=int(f.n_key.item()), flags=f.flags.cpu().numpy(),
                status=f.status.cpu().numpy(), ring=ws[off:off + 69 * 1800 * 5 * 4].cpu().numpy().view(np.uint32).copy(),
                elig=engine.extract_kp_eligible(), bits=engine.extract_patch_bits().cpu().numpy(), tables=engine.extract_frame_tables(),
                vox=[engine.voxmap_voxels(vmap, s) for s in range(3)], counts=engine.voxmap_counts(vmap))
        return cache[name]
    return get


NAMES = ("n4", "n255", "n256", "n257", "n1000", "thin", "quantised", "face1", "face128", "face300", "face_shared", "near", "far", "nan", "edge")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fused_extract_equals_the_staged_calls(engine, frames, single, name):
    import torch
    from caelo.engine import ST_COL_OOB, ST_FEW_KEYPTS, ST_FEW_VOXELS, ST_MAP_FULL, ST_NONFINITE, ST_VOXEL_OOB
    eng, pc_host = engine, frames[name]
    got = single(name)
    pc = torch.from_numpy(pc_host).to(eng.device)
    ring, counter, st_p = eng.project(pc)
    resp = eng.respond(ring)
    kpts, kpix, nkey, st_k = eng.keypoints(ring, counter, resp)
    vmap, st_v = eng.voxelize_fast(pc, vmap=eng.voxmap(slot="staged"))
    k = int(nkey.item())
    n_face = int(inconsistent(pc_host).sum())
    counts = eng.voxmap_counts(vmap)
    print("%s: %d points, K %d, status %d, counts %s, %d points on faces" % (name, len(pc_host), k, int(got["status"][0]), counts[:7], n_face))
    # the frame is what its name says
    assert counts[6] == n_face and n_face == {"face1": 1, "face128": 128, "face300": 300, "face_shared": 5}.get(name, n_face)
    if name in ("thin", "near", "far", "n4", "n1000"):
        assert n_face == 0
    if name == "near":
        assert not got["elig"].any() and k == 0
    if name == "far":
        occupied = (counter[:64, :1792] > 0).cpu().numpy()
        want = np.zeros(64, np.uint64)
        for y, b in zip(*np.nonzero(occupied.reshape(64, 56, 32).any(2))):
            want[y] |= np.uint64(1) << np.uint64(b)
        assert occupied.any() and np.array_equal(got["elig"], want)
    if name == "nan":
        assert int(got["status"][0]) & ST_NONFINITE
    # the voxel maps: sets of all three scales and the counters
    for s in range(3):
        assert np.array_equal(got["vox"][s], eng.voxmap_voxels(vmap, s)), (name, "scale", s)
    for i in (0, 1, 2, 4, 5, 6):
        assert got["counts"][i] == counts[i], (name, "counts", i, got["counts"][:7], counts[:7])
    assert [len(v) for v in got["vox"]] == [int(c) for c in counts[:3]]
    # ring image, key points
    assert np.array_equal(got["ring"], ring.cpu().numpy().view(np.uint32).ravel()), name
    assert got["n_key"] == k
    assert np.array_equal(got["key_pixels"][:k], kpix[:k].cpu().numpy()), name
    assert np.array_equal(got["rows"][:k, 60:63].view(np.uint32), kpts[:k].cpu().numpy().view(np.uint32)), name
    assert np.array_equal(got["rows"][:, 63], (np.arange(1024) < k).astype(np.float32)), name
    # patches of those key points from the staged map
    st_g = eng.zeros((1,), torch.int32)
    bits, flags = eng.patches(vmap, kpts.contiguous(), n_key=nkey, status=st_g)
    staged_status = int(st_p.item()) | int(st_k.item()) | int(st_v.item()) | int(st_g.item())
    mask = ST_COL_OOB | ST_FEW_KEYPTS | ST_FEW_VOXELS | ST_MAP_FULL | ST_NONFINITE | ST_VOXEL_OOB
    assert int(got["status"][0]) & mask == staged_status & mask, (name, int(got["status"][0]), staged_status)
    if not staged_status & ST_FEW_VOXELS:
        assert np.array_equal(got["bits"][:k], bits[:k].cpu().numpy()), name
        assert np.array_equal(got["flags"][:k], flags[:k].cpu().numpy()), name
        # the de-duplication tables behind the bits: as many entries as the staged patches have distinct rows
        tb, count, lst, slot_of = got["tables"]
        assert np.array_equal(tb[:3 * k], bits[:k].cpu().numpy().view(np.uint64).reshape(3 * k, 64)), name
        assert k == 0 or len(np.unique(tb[:3 * k], axis=0)) <= count <= 3 * k, (name, count)   # (a hash collision may cost a sharing)
    assert eng.lane_faults() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SETS)))
def test_sets_of_frames_equal_single_frames(engine, fused_sets, single, i):
    """Sets of 1, 2 and 8 frames per launch, ragged: frame j of a set is the single-frame extract of the same scan, its ring image
    and eligibility map included (read from the pipeline's workspaces right after the set ran)."""
    res = fused_sets[i]
    for j, name in enumerate(SETS[i]):
        one = single(name)
        k = one["n_key"]
        assert int(res["n_key"][j]) == k, (i, name)
        assert np.array_equal(res["status"][j], one["status"]), (i, name, res["status"][j], one["status"])
        assert np.array_equal(res["key_pixels"][j][:k], one["key_pixels"][:k]), (i, name)
        assert np.array_equal(res["rows"][j][:k].view(np.uint32), one["rows"][:k].view(np.uint32)), (i, name)
        assert np.array_equal(res["rows"][j][:, 63], one["rows"][:, 63]), (i, name)
        assert np.array_equal(res["flags"][j][:k], one["flags"][:k]), (i, name)
        assert np.array_equal(res["ring"][j], one["ring"]), (i, name)
        assert np.array_equal(res["elig"][j], one["elig"]), (i, name)


@pytest.mark.gpu
def test_reused_slots_equal_a_fresh_pipeline(engine, frames, fused_sets):
    """The fixture ran five sets through one pipeline: every map and workspace of it had other tenants before (k_vox_clear_lists
    wipes what the fused build listed).  A pipeline that has seen nothing gives the last three sets the same bits."""
    from caelo.engine import Pipeline
    fresh = Pipeline(engine, 8, 3)
    for want, got in zip(fused_sets[2:], [run_sets(engine, fresh, frames, (s,))[0] for s in SETS[2:]]):
        for f in FIELDS:
            assert np.array_equal(want[f].view(np.uint8), got[f].view(np.uint8)), f
    del fresh


@pytest.mark.gpu
def test_fused_sets_equal_the_forked_path(engine, frames, fused_sets, tmp_path):
    path = str(tmp_path / "frames.npz")
    np.savez(path, **frames)
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **FORKED), capture_output=True, text=True,
                              timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("the forked-path child ran into its time limit: nothing more is started on this GPU", returncode=1)
    if proc.returncode < 0 or proc.returncode in (134, 139, 124, 137):
        pytest.exit("the forked-path child ended with %d: nothing more is started on this GPU\n%s" % (proc.returncode, proc.stderr[-3000:]),
                    returncode=1)
    assert proc.returncode == 0, "child: exit %d\n%s" % (proc.returncode, proc.stderr[-3000:])
    lines = [l for l in proc.stdout.splitlines() if l.startswith("DIGESTS ")]
    assert len(lines) == 1
    got = json.loads(lines[0][8:])
    assert got.pop("voxel stream") == "True", "the child did not build its maps on a voxel stream"
    assert got.pop("lane faults") == "0"
    want = _digests(fused_sets)
    differing = sorted(k for k in want if got.get(k) != want[k])
    assert not differing and set(got) == set(want), "differ from the forked path: %s" % differing


if __name__ == "__main__":
    _child(sys.argv[1])
