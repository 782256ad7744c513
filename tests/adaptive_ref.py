"""A float64 NumPy restatement, written for this project, of the comparison protocol's registrar: External/ransac.m,
ransacfitRt.m, estimateRigidTransform.m (the 4 x 4 matrix B, np.linalg.svd, the last right singular vector), quat2rot.m, and the
chain of Scripts/GenerateTrajactory.m:203-237 WITH the motion prior applied as the script applies it.  The sample rule is the
project's own (include/caelo.h): MATLAB's randsample stream cannot be reproduced.

Beside the result every run reports how close it came to a decision that rounding could turn:
  min_residual_gap   the smallest |d - t| over every residual of every trial walked (and of the final inlier pass)
  min_sv_gap         the smallest (S3 - S4) / S1 of B over every fit: how well the quaternion is determined
  min_N_gap          the smallest distance from an integer of an N = log(1 - p) / log(1 - frac^3) that the clamp max(N, 100) leaves
                     alone and that a trial count can reach (100 < N <= 10 001): only such an N is ever compared with a trial
                     count it could be mistaken about (a larger N ends no walk before the limit does, a smaller one is 100)
The tests assert margins on these for their cases before they compare anything with the library.
"""
import functools

import numpy as np

MAX_TRIALS = 10000
EPS = np.finfo(np.float64).eps


def sample_indices(u, n):
    """Three distinct 0-based indices below n from three uniform doubles (the project's rule)."""
    i0 = min(int(np.floor(u[0] * n)), n - 1)
    j1 = min(int(np.floor(u[1] * (n - 1))), n - 2)
    i1 = j1 + (1 if j1 >= i0 else 0)
    j2 = min(int(np.floor(u[2] * (n - 2))), n - 3)
    i2 = j2 + (1 if j2 >= min(i0, i1) else 0)
    if i2 >= max(i0, i1):
        i2 += 1
    return i0, i1, i2


def quat2rot(q):
    q0, q1, q2, q3 = q
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def cross_matrix(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def estimate_rt(x, y, stats=None):
    """x, y [3, N] -> Rt [3, 4] with x ~ R y + T: the smallest right singular vector of B = sum A_i^T A_i as a quaternion."""
    n = x.shape[1]
    xc, yc = x.sum(axis=1) / n, y.sum(axis=1) / n
    xz, yz = x - xc[:, None], y - yc[:, None]
    r12, r21, r22 = (yz - xz).T, xz - yz, yz + xz
    B = np.zeros((4, 4))
    for i in range(n):
        A = np.zeros((4, 4))
        A[0, 1:] = r12[i]
        A[1:, 0] = r21[:, i]
        A[1:, 1:] = cross_matrix(r22[:, i])
        B = B + A.T @ A
    _, S, Vt = np.linalg.svd(B)
    if stats is not None:
        stats["min_sv_gap"] = min(stats["min_sv_gap"], (S[2] - S[3]) / S[0] if S[0] > 0 else 0.0)
    rot = quat2rot(Vt[3])
    T1, T2, T3 = np.eye(4), np.eye(4), np.eye(4)
    T1[:3, 3], T2[:3, :3], T3[:3, 3] = -yc, rot, xc
    return (T3 @ T2 @ T1)[:3]


def _inliers(Rt, x, y, t, stats):
    d = np.sqrt(np.sum((x - (Rt[:, :3] @ y + Rt[:, 3:4])) ** 2, axis=0))
    if stats is not None and d.size:
        stats["min_residual_gap"] = min(stats["min_residual_gap"], float(np.min(np.abs(d - t))))
    return np.flatnonzero(np.abs(d) < t)


def new_stats():
    return {"min_residual_gap": np.inf, "min_sv_gap": np.inf, "min_N_gap": np.inf}


def ransacfit_rt(x1, x2, t, draws, stats=None):
    """x1, x2 [n, 3] with x1 ~ R x2 + T.  -> dict(Rt [3,4] | None (n < 3), Rt_ransac, inliers (indices), trials, best_trial, status)."""
    x, y = np.asarray(x1, np.float64).T, np.asarray(x2, np.float64).T
    n = x.shape[1]
    eye = np.c_[np.eye(3), np.zeros(3)]
    if n < 3:
        return dict(Rt=None, Rt_ransac=eye, inliers=np.zeros(0, np.int64), trials=0, best_trial=-1, status=2)
    if n == 3:
        Rt = estimate_rt(x, y, stats)
        return dict(Rt=Rt, Rt_ransac=Rt, inliers=np.arange(3), trials=0, best_trial=-1, status=0)
    p = 0.99
    best_m, best_inl, best_score, best_trial = None, None, 0, -1
    N, trials = 1.0, 0
    while N > trials:
        ind = list(sample_indices(draws[trials], n))
        M = estimate_rt(x[:, ind], y[:, ind], stats)
        inl = _inliers(M, x, y, t, stats)
        if len(inl) >= best_score:
            best_score, best_inl, best_m, best_trial = len(inl), inl, M, trials
            p_no = 1.0 - (len(inl) / n) ** 3
            p_no = min(1.0 - EPS, max(EPS, p_no))
            N = np.log(1.0 - p) / np.log(p_no)
            if stats is not None and 100.0 < N <= MAX_TRIALS + 1:
                stats["min_N_gap"] = min(stats["min_N_gap"], abs(N - np.round(N)))
            N = max(N, 100.0)
        trials += 1
        if trials > MAX_TRIALS:
            return dict(Rt=eye, Rt_ransac=eye, inliers=np.zeros(0, np.int64), trials=MAX_TRIALS, best_trial=-1, status=1)
    if len(best_inl) >= 3:
        Rt = estimate_rt(x[:, best_inl], y[:, best_inl], stats)
    else:
        Rt, best_inl = eye, np.zeros(0, np.int64)
    return dict(Rt=Rt, Rt_ransac=best_m, inliers=best_inl, trials=trials, best_trial=best_trial, status=0)


def chain(pairs, t, draws):
    """The script's loop over a list of (x1 [n,3], x2 [n,3]) matched clouds, the prior applied as written: cloud 2 is moved by the
    previous relative motion, registered, and the update composed with it.  -> (relative [p, 12] (R | T), proportions [p], trials [p])."""
    prev_r, prev_t = np.eye(3), np.zeros(3)
    rel, prop, cnt = [], [], []
    for x1, x2 in pairs:
        moved = (prev_r @ np.asarray(x2, np.float64).T + prev_t[:, None]).T
        out = ransacfit_rt(x1, moved, t, draws)
        prop.append(len(out["inliers"]) / len(x1))
        cnt.append(out["trials"])
        if out["Rt"] is not None:
            up_r, up_t = out["Rt"][:, :3], out["Rt"][:, 3]
        else:
            up_r, up_t = np.eye(3), np.zeros(3)
        prev_r, prev_t = up_r @ prev_r, up_r @ prev_t + up_t
        rel.append(np.r_[prev_r.ravel(), prev_t])
    return np.array(rel).reshape(-1, 12), np.array(prop), np.array(cnt)


# ---- the cases the host and the GPU tests share ------------------------------------------------------------------------------------

def random_rigid(rng, angle=0.2, shift=2.0):
    q = np.r_[1.0, rng.uniform(-angle, angle, 3)]
    return quat2rot(q / np.linalg.norm(q)), rng.uniform(-shift, shift, 3)


def make_pair(seed, n, share, noise=0.05, span=40.0, duplicates=0.0):
    """n matched pairs, a share of them x1 = R x2 + T + noise, the others unrelated; ``duplicates``: that share of the x2 rows repeats
    another row (several points of frame a matched to ONE point of frame b)."""
    rng = np.random.RandomState(seed)
    x2 = rng.uniform(-span, span, (n, 3)) * np.array([1.0, 1.0, 0.1])
    if duplicates:
        k = int(round(duplicates * n))
        x2[rng.choice(n, k, replace=False)] = x2[rng.randint(0, n, k)]
    R, T = random_rigid(rng)
    x1 = (R @ x2.T).T + T + noise * rng.standard_normal((n, 3))
    out = rng.permutation(n)[:n - int(round(share * n))]
    x1[out] = rng.uniform(-span, span, (len(out), 3)) * np.array([1.0, 1.0, 0.1])
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2)


def base_draws(seed=0):
    return np.random.RandomState(seed).random_sample((MAX_TRIALS + 1, 3))


THRESHOLD = 1.0


def _case_later_repeat():
    """A later trial repeats the best trial's triple: with `>=` the LATER index is the best trial."""
    x1, x2 = make_pair(31, 200, 0.5, noise=0.2)
    d = base_draws(3)
    first = ransacfit_rt(x1, x2, THRESHOLD, d)
    later = first["trials"] - 1
    assert first["status"] == 0 and first["best_trial"] < later
    d[later] = d[first["best_trial"]]
    return x1, x2, d, dict(best_trial=later, trials=first["trials"])


def _case_past_the_stop():
    """The trial just past the stopping index would score MORE than the best trial walked: it must not win."""
    x1, x2 = make_pair(32, 200, 0.5, noise=0.3)
    d = base_draws(4)
    first = ransacfit_rt(x1, x2, THRESHOLD, d)
    assert first["status"] == 0
    stop, best = first["trials"], len(first["inliers"])
    x, y = x1.T, x2.T
    rng = np.random.RandomState(5)
    for _ in range(4000):
        u = rng.random_sample(3)
        ind = list(sample_indices(u, len(x1)))
        if len(_inliers(estimate_rt(x[:, ind], y[:, ind]), x, y, THRESHOLD, None)) > best:
            d[stop] = u
            return x1, x2, d, dict(best_trial=first["best_trial"], trials=stop, n_inliers=best)
    raise AssertionError("no better triple found: change the seeds of this case")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (x1, x2, draws, expected facts or None).  Built once per process."""
    d0 = base_draws(0)
    out = {}
    for n in (2, 3, 4, 5, 64, 65, 1000, 1024):
        out["n%d" % n] = make_pair(100 + n, n, 1.0 if n <= 5 else 0.6) + (d0, None)
    out["trials_100"] = make_pair(11, 300, 0.5) + (d0, dict(trials=100))
    out["trials_hundreds"] = make_pair(12, 400, 0.25) + (d0, None)
    out["trials_thousands"] = make_pair(13, 500, 0.11) + (d0, None)
    out["limit_n64"] = make_pair(14, 64, 0.0) + (d0, dict(status=1, trials=MAX_TRIALS, n_inliers=0))
    out["later_repeat"] = _case_later_repeat()
    out["past_the_stop"] = _case_past_the_stop()
    # (three points of which two are ONE point of frame b leave the rotation about their axis open: the share is small enough that
    #  no walked trial draws such a triple -- the gap assertion of the tests would say so)
    out["duplicates"] = make_pair(15, 256, 0.6, duplicates=0.05) + (d0, None)
    x = make_pair(16, 128, 1.0)[1]
    out["same_frame"] = (x, x.copy(), d0, dict(trials=100, best_trial=99, n_inliers=128))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (result dict of ransacfit_rt, stats) of a case.  Computed once per process."""
    x1, x2, d, _ = cases()[name]
    stats = new_stats()
    return ransacfit_rt(x1, x2, THRESHOLD, d, stats), stats


def compare(record, mask, name):
    """A library result (a record of _ffi.ADAPTIVE_DTYPE and its mask) against the restatement of case ``name``: the walk's integers and
    the mask must be EQUAL; -> the worst absolute difference over R, T, R_ransac, T_ransac (what the bars are about)."""
    ref, _ = reference(name)
    n = len(cases()[name][0])
    want = np.zeros(n, np.uint8)
    want[ref["inliers"]] = 1
    got = (int(record["trials"]), int(record["best_trial"]), int(record["status"]), int(record["n_inliers"]), int(record["n_pairs"]))
    assert got == (ref["trials"], ref["best_trial"], ref["status"], len(ref["inliers"]), n), (name, got)
    assert np.array_equal(np.asarray(mask, np.uint8), want), name
    Rt = ref["Rt"] if ref["Rt"] is not None else np.c_[np.eye(3), np.zeros(3)]
    return max(np.abs(record["R"].reshape(3, 3) - Rt[:, :3]).max(), np.abs(record["T"] - Rt[:, 3]).max(),
               np.abs(record["R_ransac"].reshape(3, 3) - ref["Rt_ransac"][:, :3]).max(), np.abs(record["T_ransac"] - ref["Rt_ransac"][:, 3]).max())
