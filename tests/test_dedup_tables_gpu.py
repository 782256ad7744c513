"""GPU: the tables of the patch de-duplication (csrc/dedup.hip) and its collision path.

Equal patches of a frame are encoded once.  They are grouped by a 40-bit hash and every patch is then compared word by word with its
group's representative (k_dd_verify); with 40 bits two different patches of a frame never share a hash, so under the default
environment that comparison only ever answers "same".  Here
  * the tables the library leaves behind the frame's patch bits (count, list, slot_of: caelo_dedup_tables, read through
    caelo_extract_ws_frame_offset) are compared with a NumPy restatement on the bits themselves -- a library that stopped sharing, or
    shared what is not equal, fails;
  * child processes run with CAELO_DEDUP_HASH_BITS = 1, 3, 12, where most groups hold different patches: extract and the pipeline
    must still equal the runs without de-duplication bit for bit, the tables must still be consistent, and for 1 and 3 bits they must
    hold more entries than there are distinct patches, which shows that the collision path ran.
Children run one at a time under their own time limit; after one that ended by signal, abort or timeout no further child is started."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3072                                   # patches of a frame: key point * 3 + scale
ORDER = np.array([(o & 1023) * 3 + (2 - (o >> 10)) for o in range(N)], dtype=np.int32)   # k_dd_scan: scale 2 first, key points ascending
FRAMES = ("boxes0", "boxes1", "boxes2", "ragged", "clutter23")
HASH_BITS = (1, 3, 12)
SEED_BASE = 300
# the pipeline run: >= 19 frames, the same scan twice inside a batch (of 8 and of 3), clutter frames 20 .. 27
PIPE_FRAMES = [("boxes", 0), ("boxes", 1), ("boxes", 1), ("boxes", 2), ("boxes", 3)] + [("clutter", f) for f in range(20, 28)] + \
              [("boxes", 4), ("boxes", 4), ("boxes", 5), ("boxes", 0), ("boxes", 6), ("boxes", 7), ("boxes", 2)]


def frame_scan(make, name):
    """make(frame, quantum=, scene_kind=) -> scan [n, 4] f32 (the session's cache in the parent, the parent's file in a child)."""
    if name == "ragged":
        return np.ascontiguousarray(make(0, quantum=1e-3, scene_kind="boxes")[::7])
    if name == "clutter23":
        return make(23, quantum=1e-3, scene_kind="clutter")
    return make(int(name[5:]), quantum=1e-3, scene_kind="boxes")


def restate(bits):
    """-> (representative of every patch = the smallest patch index holding equal 512 bytes, number of distinct patches)"""
    _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inv).ravel()].astype(np.int64), len(first)


def expected_tables(rep):
    """count, list, slot_of of caelo_dedup_tables for the representatives `rep`"""
    own = rep == np.arange(N)
    lst = ORDER[own[ORDER]]
    slot_of = -(rep + 1)
    slot_of[lst] = np.arange(len(lst))
    return len(lst), lst, slot_of


def table_findings(bits, count, lst, slot_of, exact):
    """Invariants of the tables against the bits; `exact`: every equal patch is shared (no collision lost any sharing)."""
    found = []
    rep_min, distinct = restate(bits)
    p = np.arange(N)
    rep = np.where(slot_of >= 0, p, -slot_of.astype(np.int64) - 1)
    if not ((rep >= 0) & (rep < N)).all():
        return ["a representative outside the frame"], distinct
    own = rep == p
    if count != int(own.sum()):
        found.append("count %d, %d patches represent themselves" % (count, int(own.sum())))
    want = ORDER[own[ORDER]]
    if not np.array_equal(lst[:len(want)], want):
        found.append("list is not the self-representing patches in the scan's order")
    elif not np.array_equal(slot_of[want], np.arange(len(want))):
        found.append("slot_of of a representative is not its position in list")
    if not own[rep].all():
        found.append("a representative does not represent itself")
    if not (bits[rep] == bits).all():
        found.append("a copy's 512 bytes differ from its representative's")
    if not (rep[~own] < p[~own]).all():
        found.append("a representative's index is not smaller than its copy's")
    if count < distinct:
        found.append("count %d < %d distinct patches" % (count, distinct))
    if exact and not np.array_equal(rep, rep_min):
        found.append("%d patches are not represented by the smallest equal patch" % int((rep != rep_min).sum()))
    return found, distinct


def rows_digest(rows, k):
    """sha256 of what extract writes: every descriptor, and the whole rows of the key points (the rest of columns 60:64 is not written)"""
    h = hashlib.sha256(np.ascontiguousarray(rows[:, 0:60]).tobytes())
    h.update(np.ascontiguousarray(rows[:k]).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------------
# the child process: one value of CAELO_DEDUP_HASH_BITS (set by the parent in its environment)
# ---------------------------------------------------------------------------------------------------------------------------------
def _child(out_path, scan_file):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(repo, "cae-lo_amd"), os.path.join(repo, "oracle")):
        sys.path.insert(0, p)
    import caelo
    caelo.configure_runtime()
    import torch
    from caelo.engine import Engine, ransac_draws
    eng = Engine()
    dev = eng.device
    report = {"frames": {}, "pipeline": {}}
    stored = np.load(scan_file)          # the parent's scans (synthesising them takes longer than everything below)

    def make(frame, quantum=None, scene_kind="boxes"):
        return stored["%s%d" % (scene_kind, frame)]

    def differ(a, b, k):
        bad = []
        ra, rb = a.rows.cpu().numpy().view(np.uint32), b.rows.cpu().numpy().view(np.uint32)
        if not (np.array_equal(ra[:, 0:60], rb[:, 0:60]) and np.array_equal(ra[:k], rb[:k])):
            bad.append("rows")
        if not torch.equal(a.key_pixels[:k], b.key_pixels[:k]):
            bad.append("key pixels")
        if not torch.equal(a.flags[:k], b.flags[:k]):
            bad.append("flags")
        if int(a.status[0].item()) != 0 or int(b.status[0].item()) != 0:
            bad.append("status %d / %d" % (int(a.status[0].item()), int(b.status[0].item())))
        return bad

    for name in FRAMES:
        pc = torch.from_numpy(frame_scan(make, name)).to(dev)
        rec = report["frames"][name] = {"findings": []}
        modes = [dict()] + ([dict(exact_patches=True)] if name == "clutter23" else [])
        for kw in modes:
            tag = "exact_patches " if kw else ""
            a = eng.extract(pc, **kw)
            bits, count, lst, slot_of = eng.extract_frame_tables()
            b = eng.extract(pc, dedup=False, **kw)
            k = int(a.n_key.item())
            rec["findings"] += [tag + m for m in differ(a, b, k)]
            t_found, distinct = table_findings(bits, count, lst, slot_of, exact=False)
            rec["findings"] += [tag + m for m in t_found]
            if not kw:
                rec.update(count=count, distinct=distinct, n_key=k, sha256=rows_digest(a.rows.cpu().numpy(), k))
            # the same with the key points given: the detector's own, so that the patches are the frame's
            kp = a.key_pts[:k].contiguous().clone()
            g = eng.extract(pc, key_pts=kp, **kw)
            g_tab = eng.extract_frame_tables()
            h = eng.extract(pc, key_pts=kp, dedup=False, **kw)
            rec["findings"] += [tag + "key_pts=: " + m for m in differ(g, h, k) if m != "key pixels"]
            rec["findings"] += [tag + "key_pts=: " + m for m in table_findings(*g_tab, exact=False)[0]]
            if not np.array_equal(g.rows[:k, 0:60].cpu().numpy().view(np.uint32), a.rows[:k, 0:60].cpu().numpy().view(np.uint32)):
                rec["findings"].append(tag + "key_pts=: descriptors differ from the detector's run")

    scans = [torch.from_numpy(make(f, quantum=1e-3, scene_kind=kind)).to(dev) for kind, f in PIPE_FRAMES]
    n = len(scans)
    draws = [torch.from_numpy(ransac_draws(SEED_BASE + i)).to(dev) for i in range(n)]
    fields = ("rows", "key_pixels", "pair_idx", "inlier_mask", "result", "status")
    for batch in (8, 3):
        pipe = eng.pipeline(batch, 2)
        for exact in (False, True):
            runs = []
            for dd in (True, False):
                out = pipe.run(scans, draws, pairs=True, dedup=dd, exact_patches=exact)
                torch.cuda.synchronize()
                runs.append({f: getattr(out, f)[:n].cpu().numpy().view(np.uint8).reshape(n, -1) for f in fields})
            bad = []
            for f in fields:
                rows_bad = np.flatnonzero((runs[0][f] != runs[1][f]).any(axis=1))
                if len(rows_bad):
                    bad.append("%s: frames %s" % (f, rows_bad.tolist()))
            report["pipeline"]["batch %d exact_patches %d" % (batch, exact)] = bad
    report["n_pipeline_frames"] = n
    report["lane_faults"] = eng.lane_faults()
    report["done"] = True
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------
_first_failure = None    # the first child that ended by signal, abort or timeout: no further child is started


def _run_child(tmp_path, scan_file, nbits):
    global _first_failure
    if _first_failure:
        pytest.skip("no further child after: " + _first_failure)
    out = str(tmp_path / "report.json")
    env = dict(os.environ, CAELO_DEDUP_HASH_BITS=str(nbits))
    label = "child CAELO_DEDUP_HASH_BITS=%d" % nbits
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), out, scan_file], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _first_failure = label + " ran into its time limit"
        pytest.fail(_first_failure)
    if proc.returncode < 0 or proc.returncode in (134, 139, 124, 137):
        _first_failure = "%s ended with %d" % (label, proc.returncode)
    assert proc.returncode == 0, "%s: exit %d\n%s" % (label, proc.returncode, proc.stderr[-3000:])
    return json.load(open(out))


@pytest.fixture(scope="module")
def scan_file(scans, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("dedup") / "scans.npz")
    np.savez(path, **{"%s%d" % (kind, f): scans(f, quantum=1e-3, scene_kind=kind) for kind, f in set(PIPE_FRAMES)})
    return path


@pytest.fixture(scope="module")
def default_frames(engine, scans):
    """Every frame under the default 40-bit hash, in this process: tables, and the digest of the rows the children must reproduce."""
    import torch
    out = {}
    for name in FRAMES:
        pc = torch.from_numpy(frame_scan(scans, name)).to(engine.device)
        a = engine.extract(pc)
        bits, count, lst, slot_of = engine.extract_frame_tables()
        k = int(a.n_key.item())
        b = engine.extract(pc, dedup=False)
        plain = engine.extract_frame_tables()
        assert int(a.status[0].item()) == 0 and int(b.status[0].item()) == 0
        out[name] = dict(bits=bits, count=count, list=lst, slot_of=slot_of, plain=plain, n_key=k,
                         sha256=rows_digest(a.rows.cpu().numpy(), k), sha256_plain=rows_digest(b.rows.cpu().numpy(), k))
    return out


@pytest.mark.parametrize("name", FRAMES)
def test_tables_equal_a_numpy_restatement(default_frames, name):
    """Default hash: a patch's representative is the smallest patch index with equal bits, count is the number of distinct rows, list
    holds exactly the self-representing patches in k_dd_scan's order, slot_of a representative's position or -(representative + 1)."""
    d = default_frames[name]
    rep, distinct = restate(d["bits"])
    count, lst, slot_of = expected_tables(rep)
    print("%s: %d key points, %d distinct patches of %d" % (name, d["n_key"], distinct, N))
    assert count == distinct and d["count"] == distinct
    assert np.array_equal(d["list"][:count], lst)
    assert np.array_equal(d["slot_of"], slot_of)
    assert table_findings(d["bits"], d["count"], d["list"], d["slot_of"], exact=True)[0] == []
    if name.startswith("boxes"):
        assert d["count"] < 2600           # the frame really holds copies
    if name == "ragged":
        assert 50 < d["n_key"] < 1024      # the rows past the key points hold empty patches, which collapse into one
        assert (rep[3 * d["n_key"]:] == rep[3 * d["n_key"]]).all() and not d["bits"][3 * d["n_key"]:].any()
    assert d["sha256"] == d["sha256_plain"]


@pytest.mark.parametrize("name", FRAMES)
def test_tables_without_dedup_list_every_patch(default_frames, name):
    bits, count, lst, slot_of = default_frames[name]["plain"]
    assert np.array_equal(bits, default_frames[name]["bits"])
    assert count == N and np.array_equal(lst, ORDER) and (slot_of >= 0).all()
    assert np.array_equal(slot_of[ORDER], np.arange(N))


@pytest.mark.parametrize("nbits", HASH_BITS)
def test_forced_hash_collisions_change_no_result(default_frames, scan_file, tmp_path, nbits):
    r = _run_child(tmp_path, scan_file, nbits)
    assert r.get("done") and r["lane_faults"] == 0
    for name in FRAMES:
        f = r["frames"][name]
        print("%d bits, %s: %d table entries for %d distinct patches" % (nbits, name, f["count"], f["distinct"]))
        assert f["findings"] == [], (name, f["findings"])
        assert f["count"] >= f["distinct"] and f["distinct"] == default_frames[name]["count"] and f["n_key"] == default_frames[name]["n_key"]
        if nbits in (1, 3) and name.startswith("boxes"):
            assert f["count"] > f["distinct"], "%s: no patch lost its sharing to a collision -- the collision path did not run" % name
        assert f["sha256"] == default_frames[name]["sha256"], name
    assert r["n_pipeline_frames"] >= 19 and len(r["pipeline"]) == 4
    for case, bad in r["pipeline"].items():
        assert bad == [], (case, bad)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
