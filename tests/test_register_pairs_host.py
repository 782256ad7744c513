"""The host side of the frame steps (caelo/framesteps.py) and of caelo_register_pairs' C ABI: no GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

from caelo import _ffi, framesteps as fs


def _reference_pairs(n, s):
    """GenerateTrajactory.m:124-126 restated literally: the trajectory of step s walks the scans 1 : s : n (1-based) and registers
    each with its successor in that list."""
    picked = list(range(1, n + 1, s))                              # MATLAB 1 : s : n
    return [(picked[k] - 1, picked[k + 1] - 1) for k in range(len(picked) - 1)]   # 0-based frame indices


@pytest.mark.parametrize("n", [1, 2, 5, 6, 11])
@pytest.mark.parametrize("s", [1, 2, 5, 10])
def test_pair_schedule_seeds_and_file_names(n, s, tmp_path):
    pairs = fs.step_pairs(n, s)
    assert pairs == _reference_pairs(n, s)
    assert len(pairs) == (max(n - 1, 0)) // s
    # pair k draws seed_base + k: the seed of pair (k, k + 1) in a plain run over the scans 0, s, 2 s, ...
    assert fs.step_seeds(n, s, 1000) == [1000 + k for k in range(len(pairs))]
    out = str(tmp_path / "poses_" / "00.txt")
    want = out if s == 1 else str(tmp_path / "poses_" / ("%d_00.txt" % s))
    assert fs.step_path(out, s) == want and fs.step_path("m.mat", s) == ("m.mat" if s == 1 else "%d_m.mat" % s)
    # the pose file: one row per frame; multiples of s hold their chained pose, the others the preceding multiple's
    from caelo import stageio
    rel = np.tile(np.r_[np.eye(3).ravel(), 1.0, 0.0, 0.0].astype(np.float32), (len(pairs), 1))     # 1 m along x per pair
    rows = fs.expand_rows(stageio.chain_poses(rel, None), n, s)
    assert rows.shape == (n, 12)
    for i in range(n):
        assert rows[i, 3] == float(i // s) and np.array_equal(rows[i], rows[i - i % s])
    if s > n - 1:   # an empty schedule: only the first row, repeated
        assert pairs == [] and all(np.array_equal(r, rows[0]) for r in rows)
        assert np.array_equal(rows[0], np.eye(3, 4, dtype=np.float32).ravel())


def test_parse_steps():
    assert fs.parse_steps("1") == [1] and fs.parse_steps("1,5,10") == [1, 5, 10] and fs.carry_frames([1, 5, 10]) == 10 and fs.carry_frames([1]) == 0
    for bad in ("", "0", "1,1", "2,-5", "a"):
        with pytest.raises(ValueError):
            fs.parse_steps(bad)


@pytest.mark.parametrize("chunk", [8, 16])
def test_chunk_carry_over_registers_every_pair_once_and_in_order(chunk):
    n, steps = 40, [1, 5, 10]
    sched = fs.schedule(0, n, chunk, steps)
    assert [(c0, c1) for c0, c1, _, _ in sched] == [(c0, min(n, c0 + chunk)) for c0 in range(0, n, chunk)]
    for s in steps:
        got = [(k, a, b) for _, _, _, ps in sched for (ss, k, a, b) in ps if ss == s]
        assert [(a, b) for _, a, b in got] == fs.step_pairs(n, s)              # exactly once, in order
        assert [k for k, _, _ in got] == list(range(len(got)))
    for c0, c1, first, ps in sched:                                            # both frames resident: in the chunk or carried over
        assert first == max(0, c0 - 10)
        for _, _, a, b in ps:
            assert first <= a < b < c1 and c0 <= b


def test_abi_symbols_version_and_refusals_without_a_device():
    lib = _ffi.load()
    assert lib.caelo_abi_version() == 6 == _ffi.ABI_VERSION
    assert hasattr(lib, "caelo_register_pairs") and hasattr(lib, "caelo_register_pairs_ws_bytes")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "caelo.h")).read()
    assert "caelo_register_pairs(" in header and "caelo_register_pairs_ws_bytes(" in header
    small, large = lib.caelo_register_pairs_ws_bytes(1), lib.caelo_register_pairs_ws_bytes(100000)
    assert small >= 8 * (lib.caelo_match_ws_bytes(1024) + lib.caelo_ransac_ws_bytes()) and large == small
    assert lib.caelo_register_pairs_ws_bytes(-1) == 0
    buf = np.zeros(64, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)

    def call(ctx=None, rows=p, n_frames=2, n_key=p, pairs=p, n_pairs=1, rand=p, idx=p, res=p, mask=p, cert=None, ws=p):
        return lib.caelo_register_pairs(ctx, rows, n_frames, n_key, pairs, n_pairs, rand, idx, res, mask, cert, ws, None)

    def refused(text, **kw):
        assert call(**kw) < 0
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()

    refused("null pair table", pairs=None)
    refused("n_frames", n_frames=0)
    refused("n_pairs", n_pairs=-1)
    refused("null argument")                 # no context
    refused("null argument", rows=None)



class _StubEngine:
    """Engine.register_pairs' interface on CPU tensors: records every call and answers with the frames it was shown -- R[0], R[1] =
    the global numbers written into the two frames' rows, T[0] = the pair's seed."""

    def __init__(self):
        self.calls = []
        self.desc_frames = []      # per call: None, or the frame markers of (the rows window, the desc window)

    def register_pairs(self, rows, n_key, pairs, seeds, certify=True, desc=None):
        import collections
        assert rows.shape[0] == n_key.shape[0] and len(pairs) == len(seeds)
        self.desc_frames.append(None if desc is None else ([int(v) for v in rows[:, 0, 0]], [int(v) for v in desc[:, 0, 0]]))
        res = np.zeros(len(pairs), dtype=_ffi.POSE_DTYPE)
        for q, ((a, b), seed) in enumerate(zip(pairs, seeds)):
            assert 0 <= a < rows.shape[0] and 0 <= b < rows.shape[0], "table index outside the resident window"
            res["R"][q, 0], res["R"][q, 1], res["T"][q, 0] = float(rows[a, 0, 0]), float(rows[b, 0, 0]), seed
            res["n_pairs"][q] = int(n_key[b])
        self.calls.append((int(rows.shape[0]), list(pairs)))
        return collections.namedtuple("Out", "results")(res)


def _batch(c0, c1):
    import collections
    import torch
    rows = torch.zeros((c1 - c0, 1024, 64))
    rows[:, 0, 0] = torch.arange(c0, c1, dtype=torch.float32)
    rows[:, :100, 63] = 1.0                       # 100 valid rows: the count a gathered head is given
    return collections.namedtuple("B", "k rows n_key")(c1 - c0, rows, torch.full((c1 - c0,), 100, dtype=torch.int32))


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("chunk", [8, 16])
def test_step_registrar_carries_rows_and_splits_ranks(chunk, world):
    """The code that carries rows (StepRegistrar.keep / boundary / merge), on a stub engine: over 40 frames, steps 5 and 10, on 1, 2 and 3
    ranks every pair is registered exactly once, from the right two frames, with its seed, and every table index lies inside the
    window of carried + chunk (+ halo) rows -- which never exceeds max(steps) + chunk frames."""
    from caelo import dist as cdist
    n, steps, seed_base = 40, [1, 5, 10], 700
    regs, bounds = [], [cdist.shard_frames(n, r, world) for r in range(world)]
    for lo, hi in bounds:
        eng = _StubEngine()
        reg = fs.StepRegistrar(eng, steps, seed_base, True, lo)
        for c0 in range(lo, hi, chunk):
            reg.keep(c0, _batch(c0, min(hi, c0 + chunk)))
        assert all(w <= 10 + chunk for w, _ in eng.calls)
        regs.append(reg)
    heads = [r.head_rows() for r in regs]
    for r, (lo, hi) in enumerate(bounds[:-1]):
        assert heads[r + 1].shape[0] == 10 and [int(v) for v in heads[r + 1][:, 0, 0]] == list(range(hi, hi + 10))
        regs[r].boundary(heads[r + 1], hi, n)
    regs[0].merge([r.export() for r in regs])
    for s in (5, 10):
        rel, ok, nin, npairs, its = regs[0].step_results(s)
        want = fs.step_pairs(n, s)
        assert len(rel) == len(want) and (npairs == 100).all()
        assert [(int(r[0]), int(r[1])) for r in rel] == want and [int(r[9]) for r in rel] == fs.step_seeds(n, s, seed_base)


@pytest.mark.parametrize("chunk", [4, 7, 23])
@pytest.mark.parametrize("steps", [[1, 5], [5, 1]])
def test_step_registrar_with_descriptors_registers_step_one_too(steps, chunk):
    """StepRegistrar(step_one=True).push(c0, rows, n_key, desc) -- what run_sequence.run_desc does: over 23 frames every pair of steps
    1 and 5 is registered exactly once and in step order, pair k with seed_base + k, from the right two frames; every table index
    lies inside the window handed over (the stub refuses others), and row i of the descriptor window is the frame of row i of the
    rows window.  A chunk of 4 is smaller than the largest step: the carried window then spans more than one earlier chunk."""
    import torch
    n, seed_base = 23, 300
    eng = _StubEngine()
    reg = fs.StepRegistrar(eng, steps, seed_base, True, 0, step_one=True)
    assert reg.steps == steps and reg.m == 5
    for c0 in range(0, n, chunk):
        b = _batch(c0, min(n, c0 + chunk))
        desc = torch.zeros((b.k, 1024, 32))
        desc[:, 0, 0] = b.rows[:, 0, 0]
        reg.push(c0, b.rows, b.n_key, desc)
    assert eng.calls and all(w <= 5 + chunk for w, _ in eng.calls)
    assert all(d is not None and d[0] == d[1] and d[0] == list(range(d[0][0], d[0][0] + len(d[0]))) for d in eng.desc_frames)
    assert sum(len(pairs) for _, pairs in eng.calls) == sum(len(fs.step_pairs(n, s)) for s in steps)      # exactly once
    for s in steps:
        rel, ok, nin, npairs, its = reg.step_results(s)          # (pack_results asserts the pair numbers 0 .. p - 1, each once)
        want = fs.step_pairs(n, s)
        assert len(rel) == len(want) and (npairs == 100).all()
        assert [(int(r[0]), int(r[1])) for r in rel] == want and [int(r[9]) for r in rel] == fs.step_seeds(n, s, seed_base)
        ks = np.concatenate([k for k, _ in reg.results[s]])
        assert ks.tolist() == list(range(len(want)))              # registered in step order, chunk after chunk
