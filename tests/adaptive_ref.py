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

Two registries of inputs: cases() (drawn at random) and, further down, the edge cases -- walks planted to stop at the kernel's chunk
and limit edges, residuals known to the bit around the threshold, degenerate and non-finite triples, the sample rule's edge draws.
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


# ---- the edge cases: walks steered to the kernel's chunk, limit and threshold edges -------------------------------------------------
# (a registry of their own: cases() above and the tables measured on it stay as they are)

CHUNK = 128            # the kernel scores this many trials ahead of the walk (csrc/adaptive.hip AD_C)
TOP = 1.0 - 2.0 ** -53
IDENTITY = np.c_[np.eye(3), np.zeros(3)]


def trials_needed(c, n):
    """ransac.m's N for a best trial with c of n inliers, before the clamp max(N, 100)."""
    p_no = min(1.0 - EPS, max(EPS, 1.0 - (c / n) ** 3))
    return np.log(1.0 - 0.99) / np.log(p_no)


@functools.lru_cache(maxsize=None)
def _trials_needed_table(n_hi):
    """N[n, c] for 3 <= c < n <= n_hi (NaN elsewhere)."""
    n, c = np.meshgrid(np.arange(n_hi + 1, dtype=np.float64), np.arange(n_hi + 1, dtype=np.float64), indexing="ij")
    with np.errstate(divide="ignore", invalid="ignore"):
        p_no = np.minimum(1.0 - EPS, np.maximum(EPS, 1.0 - (c / n) ** 3))
        N = np.log(1.0 - 0.99) / np.log(p_no)
    N[(c < 3) | (c >= n)] = np.nan
    return N


def find_nc(k, n_lo=64, n_hi=1024):
    """-> (n, c, N): the pair n_lo <= n <= n_hi, 3 <= c < n whose N lies in (k - 1, k) farthest from both ends (the first such pair in
    the order of n, then c).  None when the enumeration finds no pair."""
    N = _trials_needed_table(1024)[n_lo:n_hi + 1]
    margin = np.where((N > k - 1) & (N < k), np.minimum(N - (k - 1), k - N), -1.0)
    i, c = np.unravel_index(int(np.argmax(margin)), margin.shape)
    if margin[i, c] < 0:
        return None
    n = n_lo + int(i)
    return n, int(c), trials_needed(int(c), n)


def _sv_gaps(x, y, idx):
    """(S3 - S4) / S1 of estimate_rt's B for many triples at once: x, y [3, n], idx [k, 3] -> [k]."""
    xs, ys = x.T[idx], y.T[idx]                                # [k, 3, 3] (triple, point, axis)
    xz, yz = xs - xs.sum(axis=1, keepdims=True) / 3, ys - ys.sum(axis=1, keepdims=True) / 3
    d, s = yz - xz, yz + xz
    A = np.zeros(idx.shape + (4, 4))
    A[..., 0, 1:], A[..., 1:, 0] = d, -d
    A[..., 1, 2], A[..., 1, 3], A[..., 2, 1], A[..., 2, 3], A[..., 3, 1], A[..., 3, 2] = -s[..., 2], s[..., 1], s[..., 2], -s[..., 0], -s[..., 1], s[..., 0]
    S = np.linalg.svd(np.einsum("kiab,kiac->kbc", A, A), compute_uv=False)
    return (S[:, 2] - S[:, 3]) / S[:, 0]


def planted(n, c, good_at, seed):
    """A walk that stops where it is told to: c of the n pairs are exact inliers (x1 = R x2 + T, no noise), the others lie hundreds
    of metres away in z, and the draw table is filled by rejection so that trial t samples an all-inlier triple if and only if
    t is in ``good_at`` (every other trial samples at least one outlier and scores a handful).  Triples whose (S3 - S4) / S1 is below
    1e-4 are rejected as well (near-collinear outlier triples otherwise reach 3e-6).  -> (x1, x2, draws, inlier mask [n] u8)."""
    rng = np.random.RandomState(seed)
    x2 = rng.uniform(-40.0, 40.0, (n, 3)) * np.array([1.0, 1.0, 0.1])
    R, T = random_rigid(rng)
    x1 = (R @ x2.T).T + T
    inl = np.ones(n, bool)
    inl[rng.permutation(n)[:n - c]] = False
    far = np.flatnonzero(~inl)
    x1[far, 2] += rng.uniform(200.0, 800.0, len(far)) * rng.choice([-1.0, 1.0], len(far))
    x, y = x1.T, x2.T
    good = np.zeros(MAX_TRIALS + 1, bool)
    good[list(good_at)] = True
    draws = np.empty((MAX_TRIALS + 1, 3))
    todo = np.arange(MAX_TRIALS + 1)
    while len(todo):   # rejection, a round over every trial still open
        u = rng.random_sample((max(len(todo), 4096), 3))
        idx = np.array([sample_indices(v, n) for v in u])
        all_in, determined = inl[idx].all(axis=1), _sv_gaps(x, y, idx) >= 1e-4
        ok, bad = np.flatnonzero(all_in & determined), np.flatnonzero(~all_in & determined)
        open_good, open_bad = todo[good[todo]], todo[~good[todo]]
        k_good, k_bad = min(len(open_good), len(ok)), min(len(open_bad), len(bad))
        draws[open_good[:k_good]], draws[open_bad[:k_bad]] = u[ok[:k_good]], u[bad[:k_bad]]
        todo = np.r_[open_good[k_good:], open_bad[k_bad:]]
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2), draws, inl.astype(np.uint8)


# name -> (where N has to lie: ("window", k, n_lo, n_hi) = in (k - 1, k) by find_nc | ("nc", n, c) = as given, good_at, seed,
#          expected (trials, best_trial, status, n_inliers or None = c))
PLANTED = {
    "stop_128_n_small": (("window", 128, 65, 127), (0,), 1, (128, 0, 0, None)),             # exactly one chunk; a partial last wavefront
    "stop_128_n_large": (("window", 128, 1000, 1024), (0,), 2, (128, 0, 0, None)),
    "stop_129": (("window", 129, 64, 1024), (0,), 3, (129, 0, 0, None)),                     # one trial of chunk 2
    "stop_256": (("window", 256, 64, 1024), (0,), 4, (256, 0, 0, None)),
    "stop_257": (("window", 257, 64, 1024), (0,), 5, (257, 0, 0, None)),
    "slot_63": (("nc", 200, 100), (63,), 6, (100, 63, 0, None)),                              # N = 100 after the clamp
    "slot_64": (("nc", 200, 100), (64,), 7, (100, 64, 0, None)),
    "slot_127": (("nc", 200, 100), (127,), 8, (128, 127, 0, None)),
    "slot_128": (("nc", 200, 100), (128,), 9, (129, 128, 0, None)),
    "late_good": (("nc", 200, 100), (200,), 10, (201, 200, 0, None)),                         # N <= trials as soon as it is found
    "tie_across_chunks": (("window", 132, 64, 1024), (5, 130), 11, (132, 130, 0, None)),
    "tie_past_the_stop_in_chunk": (("window", 130, 64, 1024), (5, 130), 12, (130, 5, 0, None)),      # trial 130 was computed: it must not win
    "tie_first_slot_past_the_stop": (("window", 128, 64, 1024), (0, 128), 13, (128, 0, 0, None)),
    "tie_first_slot_walked": (("window", 129, 64, 1024), (0, 128), 14, (129, 128, 0, None)),
    "stop_9984": (("window", 9984, 64, 1024), (0,), 15, (9984, 0, 0, None)),                 # the 78 full chunks, the short one not needed
    "stop_9985": (("window", 9985, 64, 1024), (0,), 16, (9985, 0, 0, None)),                 # the first trial of the 17-trial chunk
    "last_trial_wins": (("nc", 200, 100), (9999,), 17, (10000, 9999, 0, None)),
    "one_too_late": (("nc", 200, 100), (10000,), 18, (10000, -1, 1, 0)),
    "found_yet_limit": (("window", 10001, 64, 1024), (0,), 19, (10000, -1, 1, 0)),           # ransac.m:217-226, though trial 0 was perfect
}


def planted_nc(name):
    """-> (n, c, N) of a planted case."""
    where = PLANTED[name][0]
    if where[0] == "window":
        return find_nc(*where[1:])
    return where[1], where[2], trials_needed(where[2], where[1])


@functools.lru_cache(maxsize=None)
def planted_inputs(name):
    """-> planted(...) of a planted case.  Built once per process."""
    n, c, _ = planted_nc(name)
    return planted(n, c, PLANTED[name][1], PLANTED[name][2])


# ---- the threshold, exactly ----------------------------------------------------------------------------------------------------------
def _probe(e):
    """A pair (x, y) whose residual under the identity is EXACTLY e: y is zero wherever e is not, and x = y + e there."""
    e = np.asarray(e, np.float64)
    y = np.where(e == 0.0, np.array([7.25, -3.5, 1.75]), 0.0)
    return y + e, y


def threshold_band(t):
    """Exact pairs (x == y bit for bit) at the first indices, every draw among them: every trial's model is exactly the identity.  Behind
    them probe pairs with residual vectors known to the bit, at, just below and just above t, and pairs far out so that N lies in
    (100, 256), at least 0.1 from an integer.
    -> (x1, x2, draws, want: the mask np.sqrt(e0*e0 + e1*e1 + e2*e2) < t gives in float64, operations in that order)."""
    m = 12
    rng = np.random.RandomState(41)
    exact = rng.uniform(-40.0, 40.0, (m, 3)) * np.array([1.0, 1.0, 0.3])
    lo, hi = np.nextafter(t, 0.0), np.nextafter(t, np.inf)
    es = []
    for axis in range(3):
        for v in (t, lo, hi, -t, -lo, -hi):
            e = np.zeros(3)
            e[axis] = v
            es.append(e)
    if t == 5.0:
        es += [np.array([3.0, 4.0, 0.0]), np.array([3.0, np.nextafter(4.0, 0.0), 0.0]), np.array([0.0, np.nextafter(3.0, 0.0), 4.0]),
               np.array([np.nextafter(3.0, np.inf), 0.0, 4.0]), np.array([4.0, 0.0, np.nextafter(3.0, 0.0)])]
    for k in range(1, 7):
        for sign in (-1.0, 1.0):
            e = np.zeros(3)
            e[k % 3] = t * (1.0 + sign * k * 2.0 ** -53)
            es.append(e)
            e = np.zeros(3)                          # the same number of steps of the format itself
            v = t
            for _ in range(k):
                v = np.nextafter(v, np.inf if sign > 0 else 0.0)
            e[(k + 1) % 3] = v
            es.append(e)
    es = np.array(es)
    want_probe = np.array([bool(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) < t) for e in es])
    count = m + int(want_probe.sum())
    pad = 0
    while True:   # pairs far out until N is in (100, 256) and away from an integer
        N = trials_needed(count, m + len(es) + pad)
        if 100.5 < N < 256 and abs(N - np.round(N)) > 0.1:
            break
        pad += 1
    n = m + len(es) + pad
    x1, x2 = np.zeros((n, 3)), np.zeros((n, 3))
    x1[:m], x2[:m] = exact, exact
    for i, e in enumerate(es):
        x1[m + i], x2[m + i] = _probe(e)
        assert np.array_equal(x1[m + i] - x2[m + i], e)
    far = rng.uniform(-40.0, 40.0, (pad, 3))
    x1[m + len(es):], x2[m + len(es):] = far + np.array([500.0, 0.0, 0.0]), far
    draws = base_draws(7) * np.array([m / n, (m - 1) / (n - 1), (m - 2) / (n - 2)])
    assert all(max(sample_indices(u, n)) < m for u in draws)
    want = np.r_[np.ones(m, bool), want_probe, np.zeros(pad, bool)].astype(np.uint8)
    return x1, x2, draws, want


# ---- degenerate and non-finite triples -----------------------------------------------------------------------------------------------
def repeat_draw(u):
    return np.ascontiguousarray(np.tile(np.asarray(u, np.float64), (MAX_TRIALS + 1, 1)))


def degenerate_inputs():
    """name -> (x1, x2, draws): small hand-made clouds whose every trial samples the pairs 0, 1, 2 (u = 0)."""
    d = repeat_draw((0.0, 0.0, 0.0))
    out = {}
    # all three sampled pairs are ONE pair: the 4 x 4 matrix is exactly zero
    x = np.array([[1.5, -2.25, 0.5]] * 3 + [[30.0, 4.0, 1.0], [-20.0, 9.0, 2.0]])
    y = np.array([[0.25, 4.0, -1.0]] * 3 + [[-7.0, 11.0, 0.5], [13.0, -8.0, 1.5]])
    out["one_pair_thrice"] = (x, y, d)
    # two of the three share one y with different x (several points of frame a matched to ONE point of frame b)
    rs = np.random.RandomState(61)
    y = rs.uniform(-20.0, 20.0, (6, 3))
    R, T = random_rigid(rs)
    y[1] = y[0] + np.array([0.2, -0.1, 0.1])
    x = (R @ y.T).T + T
    y[1] = y[0]          # (the true motion leaves 0.25 m at pair 1 and nothing elsewhere: the least-squares fit to the triple no more)
    out["shared_y"] = (np.ascontiguousarray(x), y, d)
    # an exactly collinear rigid triple: the rotation about the line is open
    y = rs.uniform(-20.0, 20.0, (7, 3))
    p, v = np.array([1.0, -2.0, 0.5]), np.array([0.5, 0.25, -1.0])
    y[:3] = p + np.array([[-2.0], [0.5], [3.0]]) * v          # (exact in float64)
    R = quat2rot(np.array([0.5, 0.5, 0.5, 0.5]))              # an exact rotation: a cyclic permutation of the axes
    x = (R @ y.T).T + np.array([2.0, -1.0, 0.25])
    out["collinear_rigid"] = (np.ascontiguousarray(x), y, d)
    return out


def nonfinite_inputs():
    """name -> (x1, x2, draws, bad index): exact rigid pairs of which ONE holds a NaN or an infinity, draws from base_draws."""
    out = {}
    for name, n, bad, side, axis, value in (("nan_x_first", 8, 0, 0, 1, np.nan), ("inf_y_last", 8, 7, 1, 0, np.inf),
                                            ("minus_inf_x_middle", 6, 3, 0, 2, -np.inf), ("nan_y_second_wavefront", 65, 64, 1, 2, np.nan)):
        rs = np.random.RandomState(70 + n + bad)
        y = rs.uniform(-40.0, 40.0, (n, 3)) * np.array([1.0, 1.0, 0.1])
        R, T = random_rigid(rs)
        x = (R @ y.T).T + T
        (x, y)[side][bad, axis] = value
        out[name] = (np.ascontiguousarray(x), np.ascontiguousarray(y), base_draws(0), bad)
    return out


def nonfinite_expected(name):
    """The walk by hand: a trial that samples the bad pair scores 0, every other trial all the n - 1 finite pairs (they are exact
    inliers): N is 100 after the clamp, the best trial is the last of the first 100 that does not sample the bad pair."""
    x1, _, draws, bad = nonfinite_inputs()[name]
    n = len(x1)
    clean = [t for t in range(100) if bad not in sample_indices(draws[t], n)]
    want = np.ones(n, np.uint8)
    want[bad] = 0
    assert trials_needed(n - 1, n) < 100 and clean
    return dict(trials=100, best_trial=clean[-1], status=0, n_inliers=n - 1), want


def sample_rule_inputs(n):
    """-> (x1, x2, [u]): a noisy cloud whose every triple gives another motion, and the draws every trial repeats: the rule's edges
    (u = 0 and the largest draw there is, u = 1 - 2^-53) and a few in between."""
    x1, x2 = make_pair(900 + n, n, 1.0, noise=0.3)
    rs = np.random.RandomState(50 + n)
    return x1, x2, [np.zeros(3), np.full(3, TOP), np.array([TOP, 0.0, TOP]), np.array([0.0, TOP, 0.0])] + list(rs.random_sample((4, 3)))


@functools.lru_cache(maxsize=None)
def edge_cases():
    """name -> (x1, x2, draws, threshold, expected facts, expected mask or None).  Built once per process."""
    out = {}
    for name, (_, good_at, seed, (trials, best, status, n_in)) in PLANTED.items():
        n, c, _ = planted_nc(name)
        x1, x2, d, inl = planted_inputs(name)
        want = inl if status == 0 else np.zeros(n, np.uint8)
        out[name] = (x1, x2, d, THRESHOLD, dict(trials=trials, best_trial=best, status=status, n_inliers=c if n_in is None else n_in), want)
    return out


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """-> (result dict of ransacfit_rt, stats) of an edge case.  Computed once per process."""
    x1, x2, d, t = edge_cases()[name][:4]
    stats = new_stats()
    return ransacfit_rt(x1, x2, t, d, stats), stats


def compare_edge(record, mask, name):
    """compare() for an edge case."""
    ref, _ = edge_reference(name)
    n = len(edge_cases()[name][0])
    want = np.zeros(n, np.uint8)
    want[ref["inliers"]] = 1
    got = (int(record["trials"]), int(record["best_trial"]), int(record["status"]), int(record["n_inliers"]), int(record["n_pairs"]))
    assert got == (ref["trials"], ref["best_trial"], ref["status"], len(ref["inliers"]), n), (name, got)
    assert np.array_equal(np.asarray(mask, np.uint8), want), name
    return rt_error(record, ref["Rt"], ref["Rt_ransac"])


def rt_error(record, Rt, Rt_ransac):
    """The worst absolute difference of a library record's R, T, R_ransac, T_ransac from two [3, 4] matrices."""
    return max(np.abs(record["R"].reshape(3, 3) - Rt[:, :3]).max(), np.abs(record["T"] - Rt[:, 3]).max(),
               np.abs(record["R_ransac"].reshape(3, 3) - Rt_ransac[:, :3]).max(), np.abs(record["T_ransac"] - Rt_ransac[:, 3]).max())


def same_walk(a, amask, b, bmask, tol=1e-12):
    """Two library results (device and host twin): the integers and the mask EQUAL, R_ransac and T_ransac within tol."""
    for f in ("trials", "best_trial", "status", "n_inliers", "n_pairs"):
        assert int(a[f]) == int(b[f]), (f, int(a[f]), int(b[f]))
    assert np.array_equal(amask, bmask)
    diff = np.abs(np.r_[a["R_ransac"], a["T_ransac"]] - np.r_[b["R_ransac"], b["T_ransac"]])
    assert not np.isnan(diff).any() and diff.max() <= tol, diff.max()
