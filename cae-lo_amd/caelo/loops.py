"""Loop closure detection: place recognition with a yaw estimate, then verification through the extract and pair stages on the
yaw-aligned scan.

    descriptors   Scan Context of every scan (Engine.scan_context: caelo_scan_context)
    candidates    the all-pairs column-shifted search (Engine.loop_search: caelo_loop_search) -> (i, j, distance, shift)
    verify        the descriptor of the pair stage encodes sensor-frame voxel patches and is not rotation invariant: a revisit at
                  another heading does not register as it stands.  Scan i is turned by the search's shift * 6 degrees about z to frame
                  j's heading, extracted again (Engine.extract) and registered against frame j (Engine.register_pairs) -- the step the
                  reference sketched as ReExtractFeatures (RefinePoses.py:76-99) and never finished.
    detect        the three in a row over a sequence

The reported motion of a loop (i, j) maps frame i into frame j: p_j ~ R_loop p_i + T_loop with R_loop = R Rz(shift * 6 deg), T_loop = T,
(R, T) the registration of the turned scan.  What to do with the loops (pose-graph optimisation) is not part of this module.
"""
import math

import numpy as np
import torch

from . import keysources
from .engine import MAX_K, ST_TIES_LEFT

SECTOR_DEG = 6.0
# one row of a loops file: i j dist shift verified n_inliers threshold R(9) T(3)
LOOP_COLUMNS = 19
SC_BATCH = 8


def rz(shift):
    """Rz(shift * 6 degrees), float64 [3, 3]"""
    a = math.radians(SECTOR_DEG * float(shift))
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _device_scan(eng, scan, calib_angle=None):
    """a scan [n, 4] f32 (host array or device tensor) on the device, corrected by the calibration angle when one is given"""
    t = scan if isinstance(scan, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float32))
    t = t.to(device=eng.device, dtype=torch.float32).contiguous()
    return t if calib_angle is None else eng.correct_pc(t, calib_angle)


def descriptors(eng, scans, calib_angle=None):
    """scans: a sequence of [n, 3 or 4] f32 clouds (read one batch at a time) -> (sc [F,20,60] f32, u [F,1200] f32, valid [F] i64) on the
    device, SC_BATCH frames per call."""
    out = []
    for b0 in range(0, len(scans), SC_BATCH):
        clouds = [_device_scan(eng, scans[f], calib_angle) for f in range(b0, min(b0 + SC_BATCH, len(scans)))]
        cols = clouds[0].shape[1]
        pts = torch.zeros((len(clouds), max(1, max(c.shape[0] for c in clouds)), cols), dtype=torch.float32, device=eng.device)
        for k, c in enumerate(clouds):
            pts[k, :c.shape[0]] = c
        n_pts = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=eng.device)
        out.append(eng.scan_context(pts, n_pts))
    if not out:
        raise ValueError("no scans")
    return tuple(torch.cat([o[k] for o in out]) for k in range(3))


def candidates(eng, u, valid, min_gap=50, max_dist=None, top_k=1, min_cols=1, queries=None):
    """-> [m, 4] float64 rows (i, j, dist, shift) of every accepted candidate, by query then rank"""
    cand, dist, shift = (t.cpu().numpy() for t in eng.loop_search(u, valid, min_gap=min_gap, k=top_k, max_dist=max_dist, min_cols=min_cols,
                                                                  queries=queries))
    q0 = 0 if queries is None else int(queries[0])
    q, t = np.nonzero(cand >= 0)
    return np.c_[q + q0, cand[q, t], dist[q, t].astype(np.float64), shift[q, t]].reshape(-1, 4)


def turned(scan, shift):
    """scan [n, 4] f32 on the device turned by shift * 6 degrees about z (x, y in float32; z and intensity are copied)"""
    r = torch.from_numpy(rz(shift)[0:2, 0:2].astype(np.float32)).to(scan.device)
    out = scan.clone()
    out[:, 0:2] = scan[:, 0:2] @ r.T
    return out


def verify(eng, scans, cands, derotate=True, features_from=None, seed_base=1000, certify=True, calib_angle=None):
    """cands [m, 4] (i, j, dist, shift) -> loops [m, 19]: the candidates' columns, then verified (RANSAC4RT's success), n_inliers,
    threshold, R_loop (row-major) and T_loop.  Every distinct frame j and every distinct turned frame (i, shift) is extracted once
    (frame j's rows come from ``features_from`` -- a directory of <frame:06d>.bin.mat files -- when given); all loops are registered in
    one pair table, loop number n with the draws of seed ``seed_base + n``.  A loop one of whose frames has no usable key point set is
    reported unverified.  Synchronises."""
    cands = np.asarray(cands, dtype=np.float64).reshape(-1, 4)
    m = len(cands)
    loops = np.zeros((m, LOOP_COLUMNS))
    loops[:, 0:4] = cands
    if not (0 <= seed_base and seed_base + m <= 1 << 32):
        raise ValueError("seed_base %d: the seeds seed_base + n of loops n = 0 .. %d must lie in [0, 2^32)" % (seed_base, m - 1))
    slots = {}                                                      # ("j", frame) or ("i", frame, shift) -> row block index
    for i, j, _, s in cands:
        slots.setdefault(("j", int(j)), len(slots))
        slots.setdefault(("i", int(i), int(s) if derotate else 0), len(slots))
    rows = torch.zeros((max(len(slots), 1), MAX_K, 64), dtype=torch.float32, device=eng.device)
    n_key = torch.zeros((max(len(slots), 1),), dtype=torch.int32, device=eng.device)
    status = []
    for key, k in slots.items():
        if key[0] == "j" and features_from is not None:
            KeyPts, Features, _ = keysources.load_features_dir(features_from, key[1])
            r = keysources.rows_from_features(KeyPts, Features)
            rows[k, :r.shape[0]] = torch.from_numpy(r).to(eng.device)
            n_key[k] = r.shape[0]
            status.append(None)
            continue
        scan = _device_scan(eng, scans[key[1]], calib_angle)
        if scan.shape[1] != 4:
            raise ValueError("verification extracts features: scans need 4 columns (x, y, z, intensity), got %d" % scan.shape[1])
        if key[0] == "i" and key[2]:
            scan = turned(scan, key[2])
        ff = eng.extract(scan, rows=rows[k])
        n_key[k:k + 1] = ff.n_key
        status.append(ff.status)
    nk = n_key.cpu().numpy()
    bad = {k for k, st in enumerate(status) if st is not None and int(st[0].item()) & ~ST_TIES_LEFT}
    bad |= {k for k in range(len(slots)) if not 1 <= nk[k] <= MAX_K}
    table, seeds, which = [], [], []
    for n, (i, j, _, s) in enumerate(cands):
        a, b = slots[("j", int(j))], slots[("i", int(i), int(s) if derotate else 0)]
        if a in bad or b in bad:
            continue
        table.append((a, b)); seeds.append(seed_base + n); which.append(n)
    if table:
        res = eng.register_pairs(rows, n_key, np.array(table), seeds, certify=certify)   # (checks the n_key of the table's frames only)
        for r, n in zip(res.results, which):
            turn = rz(cands[n, 3]) if derotate else np.eye(3)
            loops[n, 4], loops[n, 5], loops[n, 6] = float(r["success"]), float(r["n_inliers"]), float(r["threshold"])
            loops[n, 7:16] = (np.asarray(r["R"], dtype=np.float64).reshape(3, 3) @ turn).reshape(9)
            loops[n, 16:19] = np.asarray(r["T"], dtype=np.float64)
    return loops


def unverified(cands):
    """cands [m, 4] -> loops [m, 19] without registration: verified = n_inliers = threshold = 0, R = Rz(shift * 6 deg) (the search's
    yaw alone), T = 0"""
    cands = np.asarray(cands, dtype=np.float64).reshape(-1, 4)
    loops = np.zeros((len(cands), LOOP_COLUMNS))
    loops[:, 0:4] = cands
    for n in range(len(cands)):
        loops[n, 7:16] = rz(cands[n, 3]).reshape(9)
    return loops


def detect(eng, scans, min_gap=50, max_dist=None, top_k=1, min_cols=1, do_verify=True, derotate=True, features_from=None, seed_base=1000,
           certify=True, calib_angle=None):
    """Scan Context, the search and the verification over a sequence of scans -> loops [m, 19] (``write_loops`` writes them)."""
    _, u, valid = descriptors(eng, scans, calib_angle)
    cands = candidates(eng, u, valid, min_gap=min_gap, max_dist=max_dist, top_k=top_k, min_cols=min_cols)
    if not do_verify:
        return unverified(cands)
    return verify(eng, scans, cands, derotate=derotate, features_from=features_from, seed_base=seed_base, certify=certify, calib_angle=calib_angle)


def write_loops(path, loops):
    """One np.loadtxt-readable row per loop: i j dist shift verified n_inliers threshold R(9) T(3)."""
    import os
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fmt = ["%d", "%d", "%.9g", "%d", "%d", "%d", "%.9g"] + ["%.17g"] * 12
    np.savetxt(path, np.asarray(loops, dtype=np.float64).reshape(-1, LOOP_COLUMNS), fmt=fmt,
               header="i j dist shift verified n_inliers threshold R(9) T(3): p_j ~ R p_i + T")
    return path


def read_loops(path):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # (an empty file is a valid answer: no loops)
        a = np.loadtxt(path, ndmin=2)
    if a.size and a.shape[1] != LOOP_COLUMNS:
        raise ValueError("%s: %d columns, a loops file has %d (i j dist shift verified n_inliers threshold R(9) T(3))" % (path, a.shape[1], LOOP_COLUMNS))
    return a.reshape(-1, LOOP_COLUMNS)
