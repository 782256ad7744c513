"""Frame steps (run_sequence.py --frame-steps): the pairs, seeds and files of a sequence registered at steps s = 1, 2, 5, 10 ...,
and their schedule over the chunks of ONE extraction pass.

The reference evaluates poses_/<step>_... and Matchablity_<step>_... for steps 1, 2, 5 and 10; its trajectory writer pairs scan
k s with scan (k + 1) s (GenerateTrajactory.m:124-126), i.e. it runs the odometry over every s-th scan.  Here the rows of every
scan are resident once a chunk is through the pipeline, so the pairs of every step are registered from them
(Engine.register_pairs) instead of extracting a sub-sampled file list once per step.
"""
import os

import numpy as np


def parse_steps(text):
    """"1,5,10" -> [1, 5, 10] (positive, no repeats, in the order given)."""
    steps = [int(t) for t in str(text).split(",") if t.strip()]
    if not steps or any(s < 1 for s in steps) or len(set(steps)) != len(steps):
        raise ValueError("frame steps: a list of distinct positive integers, e.g. 1,5,10")
    return steps


def step_pairs(n, s):
    """The pairs of step s over n frames: (k s, (k + 1) s) for k = 0 .. floor((n - 1) / s) - 1."""
    return [(k * s, (k + 1) * s) for k in range((n - 1) // s)]


def step_seeds(n, s, seed_base):
    """Pair k of step s draws RandomState(seed_base + k): the seed a plain run over every s-th scan gives its pair k."""
    return [seed_base + k for k in range((n - 1) // s)]


def step_path(path, s):
    """The step's file: ``path`` itself for s = 1, else <s>_ in front of its file name (poses_/5_00.txt)."""
    if s == 1:
        return path
    d, b = os.path.split(path)
    return os.path.join(d, "%d_%s" % (s, b))


def expand_rows(chained, n, s):
    """chained [n_pairs + 1, 12] (the poses of frames 0, s, 2 s, ...) -> one row per input frame [n, 12]: a multiple of s holds its
    pose, the frames in between repeat the preceding multiple's row (this project's choice: evaluate.py --frame-step s reads the
    multiples only)."""
    chained = np.asarray(chained).reshape(-1, 12)
    return chained[np.arange(n) // s]


def carry_frames(steps):
    """Frames of earlier chunks whose rows a chunk still needs: the largest step that does not go through the pipeline."""
    return max([s for s in steps if s != 1], default=0)


def chunk_pairs(c0, c1, s, lo=0):
    """The step-s pairs registered when frames [c0, c1) arrive: those whose frame 1 lies in the chunk (frame 0 is at most s frames
    back: in the chunk or among the carried rows).  -> [(k, frame 0, frame 1)], k the pair's number within its step."""
    first = max((c0 + s - 1) // s, (lo + s - 1) // s + 1)   # smallest k + 1 with (k + 1) s >= c0 and k s >= lo
    return [(j - 1, (j - 1) * s, j * s) for j in range(first, (c1 - 1) // s + 1)]


def schedule(lo, hi, chunk, steps):
    """The whole run: per chunk (c0, c1, first carried frame, [(s, k, frame 0, frame 1), ...]).  Every pair of every step appears
    exactly once, in its step's order, and both its frames are in [first carried frame, c1)."""
    m = carry_frames(steps)
    out = []
    for c0 in range(lo, hi, chunk):
        c1 = min(hi, c0 + chunk)
        out.append((c0, c1, max(lo, c0 - m), [(s, k, a, b) for s in steps for k, a, b in chunk_pairs(c0, c1, s, lo)]))
    return out


def boundary_pairs(lo, hi, n, s):
    """The step-s pairs a rank that owns frames [lo, hi) of n registers after its chunk loop: frame 0 its own, frame 1 the next
    rank's (at most s frames past hi: in that rank's first max(steps) frames, the halo).  -> [(k, frame 0, frame 1)]."""
    return [(k, a, b) for k, (a, b) in enumerate(step_pairs(n, s)) if lo <= a < hi <= b]


class StepRegistrar:
    """run_sequence.py's hook: called with every finished chunk (frames [c0, c0 + k) of a FrameBatch) of a rank that owns frames
    [lo, hi), it registers the pairs of the steps other than 1 whose frame 1 the chunk holds and whose frame 0 the rank owns -- all
    steps in ONE pair table, so that the pairs that share an anchor frame meet in a launch -- and carries the last max(steps) frames'
    rows over to the next chunk.  run_sequence.run_desc ``push``es chunks of rows with another method's descriptor block beside
    them.  Several ranks: every rank also keeps its FIRST max(steps) frames' rows (``head``), the halo of the rank before it, which
    registers the pairs that straddle the boundary (``boundary``: frame 0 its own); ``export`` / ``merge`` bring every step's
    results together in pair order."""

    def __init__(self, eng, steps, seed_base, certify, lo=0, registrar=None, step_one=False):
        """``registrar``: None = Match.py's RANSAC4RT (Engine.register_pairs; step 1 is the pipeline's own unless ``step_one``), or
        (draws, threshold) = the comparison protocol's ransacfitRt.m (Engine.register_pairs_adaptive) -- then step 1 is registered
        here as well, from the same resident rows.  Whenever step 1 is registered here one more frame is carried for it."""
        self.eng, self.seed_base, self.certify, self.lo = eng, int(seed_base), certify, int(lo)
        self.registrar = registrar
        step_one = step_one or registrar is not None
        self.steps = [s for s in steps if s != 1 or step_one]
        self.m = max(1, carry_frames(steps)) if step_one else carry_frames(steps)
        self.rows = self.n_key = self.desc = None     # the carried frames [base, base + len); desc: their descriptor block, if one is pushed
        self.base = lo
        self.head = []                    # rows of the rank's first m frames (chunk by chunk)
        self.head_n = 0
        self.results = {s: [] for s in self.steps}   # per step: (pair numbers k, record array (_ffi.POSE_DTYPE))

    def _register(self, rows, nk, base, todo, desc=None):
        """todo [(s, k, frame 0, frame 1)] on the window rows = frames [base, base + len(rows)) (desc: the same frames' descriptors)."""
        if not todo:
            return
        table = [(a - base, b - base) for _, _, a, b in todo]
        assert all(0 <= i < rows.shape[0] for ab in table for i in ab), "a scheduled pair lies outside the resident window"
        kw = {} if desc is None else {"desc": desc}   # (without descriptors the registrars are called as they always were)
        if self.registrar is not None:
            out = self.eng.register_pairs_adaptive(rows.contiguous(), nk.contiguous(), table, self.registrar[0], self.registrar[1], **kw)
        else:
            out = self.eng.register_pairs(rows.contiguous(), nk.contiguous(), table, [self.seed_base + kk for _, kk, _, _ in todo],
                                          certify=self.certify, **kw)
        for s in self.steps:
            sel = [i for i, t in enumerate(todo) if t[0] == s]
            if sel:
                self.results[s].append((np.array([todo[i][1] for i in sel], dtype=np.int64), out.results[sel]))

    def push(self, c0, rows, n_key, desc=None):
        """Frames [c0, c0 + len(rows)): rows [k,1024,64], n_key [k] and, optionally, the descriptors [k,1024,D] the match runs on
        (every chunk with them or none)."""
        import torch
        k = rows.shape[0]
        if self.head_n < self.m:
            take = min(k, self.m - self.head_n)
            self.head.append(rows[:take].clone())
            self.head_n += take
        if self.rows is not None:
            assert self.base + self.rows.shape[0] == c0, "chunks must arrive in order"
            rows, n_key = torch.cat([self.rows, rows]), torch.cat([self.n_key, n_key])
            desc = None if desc is None else torch.cat([self.desc, desc])
        else:
            self.base = c0
        self._register(rows, n_key, self.base, [(s, kk, a, b) for s in self.steps for kk, a, b in chunk_pairs(c0, c0 + k, s, self.lo)], desc)
        keep_n = min(self.m, rows.shape[0])
        self.base = c0 + k - keep_n
        self.rows, self.n_key = rows[rows.shape[0] - keep_n:].clone(), n_key[n_key.shape[0] - keep_n:].clone()
        self.desc = None if desc is None else desc[desc.shape[0] - keep_n:].clone()

    def keep(self, c0, batch):
        self.push(c0, batch.rows[:batch.k], batch.n_key[:batch.k])

    def head_rows(self):
        """[max(steps), 1024, 64]: the rank's first frames (what the rank before it needs); zero rows past a shorter shard."""
        import torch
        h = torch.cat(self.head)
        if h.shape[0] < self.m:
            h = torch.cat([h, h.new_zeros((self.m - h.shape[0],) + tuple(h.shape[1:]))])
        return h.contiguous()

    def boundary(self, next_head, hi, n):
        """After the chunk loop of a rank that owns [lo, hi) and is not the last: ``next_head`` = the next rank's head_rows() (frames
        hi .. hi + max(steps)); the key point counts of those rows are their valid columns' sums, as for every gathered row."""
        import torch
        assert self.base + self.rows.shape[0] == hi
        nk_next = next_head[:, :, 63].sum(dim=1).round().to(torch.int32)
        self._register(torch.cat([self.rows, next_head]), torch.cat([self.n_key, nk_next]), self.base,
                       [(s, kk, a, b) for s in self.steps for kk, a, b in boundary_pairs(self.lo, hi, n, s)])

    def export(self):
        """This rank's results as plain arrays (what the ranks exchange)."""
        return {s: [(ks, r.tobytes()) for ks, r in v] for s, v in self.results.items()}

    def merge(self, exports):
        """Rank 0: every rank's export() -> this object holds all results."""
        from . import _ffi
        dt = _ffi.POSE_DTYPE if self.registrar is None else _ffi.ADAPTIVE_DTYPE
        self.results = {s: [(ks, np.frombuffer(raw, dtype=dt)) for e in exports for ks, raw in e[s]] for s in self.steps}

    def step_results(self, s):
        """-> (rel [p, 12] f32 (R | T), success [p], n_inliers [p], n_pairs [p], iterations [p]) of step s, in pair order."""
        return pack_results(self.results[s], s)


def pack_results(entries, s):
    """entries [(pair numbers k, record array (_ffi.POSE_DTYPE))] of step s, in any order -> what StepRegistrar.step_results returns.
    Records of the comparison protocol's registrar (_ffi.ADAPTIVE_DTYPE): the relative motions are chained by the script's rule (a
    pair that is not solved repeats the motion of the pair before it, caelo.adaptive.chain_relative) and stay float64; ``iterations``
    are the trial counts."""
    from . import _ffi
    ks = np.concatenate([k_ for k_, _ in entries]) if entries else np.zeros(0, dtype=np.int64)
    r = np.concatenate([r_ for _, r_ in entries]) if entries else np.zeros(0, dtype=_ffi.POSE_DTYPE)
    order = np.argsort(ks, kind="stable")
    assert np.array_equal(ks[order], np.arange(len(ks))), "step %d: pairs %s registered" % (s, ks[order].tolist())
    r = r[order]
    p = len(r)
    if r.dtype == _ffi.ADAPTIVE_DTYPE:
        from . import adaptive
        rel, solved = adaptive.fit_rows(r)
        return adaptive.chain_relative(rel, solved), solved, r["n_inliers"].astype(np.int32), r["n_pairs"].astype(np.int32), r["trials"].astype(np.int32)
    rel = np.concatenate([r["R"].reshape(p, 9), r["T"].reshape(p, 3)], axis=1).astype(np.float32)
    return rel, r["success"] != 0, r["n_inliers"].astype(np.int32), r["n_pairs"].astype(np.int32), r["iterations"].astype(np.int32)
