"""The key point chain of csrc/ring.hip (k_kp_score -> k_kp_hist -> k_kp_gather -> k_kp_emit, the single-workgroup fallback and its
radix select) on inputs designed to land on its branches -- tests/kp_images.py makes them, tests/test_keypoint_select_host.py holds
every recipe against the oracle and the bins it claims.  The expectation is ``kp_images.expected_selection`` (SphericalRing.py:192-218
as a list rule) with the oracle as the second witness; everything is compared bit for bit.

Part A runs the staged entry (caelo_keypoints) on lattice images: candidate counts around 0 / 51 / 1025, ties against the capacity of
the selection list (2048), the cut in either bin of a thread's pair, in the last bin and in the lowest one, the float64 threshold,
every gate of the candidate rule, and +inf in a pixel's own response.  It also reads the frame's state words
(cand_count[0 .. 2] = M, keys listed, branch; they lie behind the 64 x 1792 candidate keys of the workspace), so a frame that gives
the right answer through the wrong branch still fails.
Part B runs the fused path (caelo_extract) and the frame pipeline on clouds: every branch side by side in one launch, in two orders,
and pipeline slots whose previous tenant took another branch."""

import numpy as np
import pytest

import kp_images as kpi

pytestmark = pytest.mark.gpu

CC_BYTE_OFFSET = kpi.NET_H * kpi.NET_W * 8      # caelo_keypoints' workspace: the candidate keys, then cand_count


@pytest.fixture(scope="module")
def api(engine):
    from caelo import api as _api
    return _api


def _staged(engine, ring, cnt, resp):
    """One caelo_keypoints call -> (key points [K,3], key pixels [K,2], K, status, (M, listed, state))."""
    import torch
    t = lambda a: torch.from_numpy(a).to(engine.device)   # noqa: E731
    kpts, kpix, nkey, st = engine.keypoints(t(ring), t(cnt), t(resp))
    ws = engine._ws("keypoints", engine.lib.caelo_keypoints_ws_bytes())
    words = ws[CC_BYTE_OFFSET:CC_BYTE_OFFSET + 12].clone().view(torch.int32).cpu().numpy()
    k = int(nkey.item())
    return kpts[:k].cpu().numpy(), kpix[:k].cpu().numpy(), k, int(st.item()), tuple(int(w) for w in words)


def _check_staged(engine, api, orc, ring, cnt, resp, want, d=None):
    from caelo.engine import ST_FEW_KEYPTS
    want_pts = ring[want[:, 0], want[:, 1], 0:3]
    kpts, kpix, k, st, words = _staged(engine, ring, cnt, resp)
    print("K %d status %d (M, listed, state) %s" % (k, st, words))
    assert k == len(want) and kpix.dtype == np.int64 and np.array_equal(kpix, want) and np.array_equal(kpts, want_pts)
    assert st == (ST_FEW_KEYPTS if k <= 50 else 0)
    if d is not None:
        assert words == (d.M, d.nsel_word, d.state), (words, d)
    o_pts, o_pix, _ = kpi.oracle_keypoints(orc, ring, cnt, resp)
    assert np.array_equal(kpix, o_pix) and np.array_equal(kpts, o_pts)
    if k <= 50:
        with pytest.raises(AssertionError):
            api.GetKeyPtsByAE(ring, cnt, resp)
    else:
        a_pts, a_pix, planar = api.GetKeyPtsByAE(ring, cnt, resp)
        assert np.array_equal(a_pix, want) and np.array_equal(a_pts, want_pts) and planar.size == 0
    assert engine.lane_faults() == 0


# ---- A. the staged entry on lattice images --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [5, 3])
@pytest.mark.parametrize("name", list(kpi.staged_cases()))
def test_staged_selection_on_lattice_images(engine, api, orc, name, channels):
    """Every recipe of kp_images.staged_cases, demo mode (5-channel ring) and batch mode (3-channel ring): key pixels, key points,
    n_key and CAELO_ST_FEW_KEYPTS (set exactly when K <= 50) equal expected_selection and the oracle; the state words say the frame
    took the branch the recipe was designed for (no threshold at all up to M = 1025; listed up to nsel = 2048; the fallback beyond)."""
    case = kpi.staged_cases()[name]
    d = kpi.design(case.scores)
    for key, claimed in case.claim.items():
        assert getattr(d, key) == claimed
    ring, cnt, resp = kpi.lattice_images(case.values, case.centres, channels)
    _check_staged(engine, api, orc, ring, cnt, resp, kpi.expected_selection(case.centres, case.scores), d)


@pytest.mark.parametrize("channels", [5, 3])
def test_staged_candidate_gates(engine, api, orc, channels):
    """kp_images.gate_images: one probe per gate of the candidate rule (4 / 5 occupied neighbours, an unoccupied centre, ring norm just
    below / exactly 10 over the ring's own channels, the row and column borders with the 56..63 quirk, a value in another response
    channel and in all eight).  A probe is a candidate exactly where its statement says so."""
    ring, cnt, resp, probes, base = kpi.gate_images(channels)
    want = kpi.gate_expected(probes, base)
    chosen = {(int(r), int(c)) for r, c in want}
    best = max((p for p in probes if p.candidate), key=lambda p: p.score)      # the single best is dropped (:216,:218)
    for p in probes:
        assert ((p.row, p.col) in chosen) == (p.candidate and p is not best), p
    _check_staged(engine, api, orc, ring, cnt, resp, want)


def test_staged_value_in_another_channel_scores_the_same(engine, api, orc):
    """The same lattice values in response channel 6 instead of 0: the same selection (the norm runs over all eight channels)."""
    case = kpi.staged_cases()["count_3000"]
    ring, cnt, resp = kpi.lattice_images(case.values, case.centres, 5, chan=6)
    assert not resp[..., 0].any() and np.count_nonzero(resp[..., 6]) == 3000
    _check_staged(engine, api, orc, ring, cnt, resp, kpi.expected_selection(case.centres, case.scores), kpi.design(case.scores))


def test_staged_workspace_is_clean_between_branches(engine, api, orc):
    """One workspace, one call after the other: fallback -> M = 1 -> listed and full (2048) -> M = 0 -> fallback -> listed.  A state
    word (candidate count, list length, branch) that survived a call would change the next frame's selection or its words."""
    cases = kpi.staged_cases()
    for name in ("ties_5000", "count_1", "ties_2048", "count_0", "last_bin_fallback", "nsel_2048", "count_1026", "ties_2049", "count_52"):
        case = cases[name]
        ring, cnt, resp = kpi.lattice_images(case.values, case.centres, 5)
        _check_staged(engine, api, orc, ring, cnt, resp, kpi.expected_selection(case.centres, case.scores), kpi.design(case.scores))


# ---- B. the fused path and the pipeline on clouds ----------------------------------------------------------------------------------------
class _Want:
    """What one cloud must give: key pixels and key points (from the oracle's ring image), computed once."""

    def __init__(self, orc, layer, kind, m, device):
        import torch
        pc, centres = kpi.fused_cloud(kind, m)
        ring, cnt = orc.ProjectPC2SphericalRing(pc)
        resp = layer.predict(ring[None, 0:64, 0:1792, 0:3])[0]
        o_pts, o_pix, smap = kpi.oracle_keypoints(orc, ring, cnt, resp)
        if kind == "clamp":   # every score is 1.0: the ascending flat indices [-1025:-1]
            flat = np.sort(centres[:, 0] * kpi.NET_W + centres[:, 1])[-kpi.KEEP:-1]
            self.pix = np.stack([flat // kpi.NET_W, flat % kpi.NET_W], axis=1).reshape(-1, 2)
        else:
            self.pix = kpi.expected_selection(centres, smap[centres[:, 0], centres[:, 1]])
        assert np.array_equal(self.pix, o_pix) and int((smap.astype(np.float64) > 0.2).sum()) == m
        self.pts = ring[self.pix[:, 0], self.pix[:, 1], 0:3]
        self.k = len(self.pix)
        assert self.k == min(max(m, 1) - 1, 1024)
        self.pc = torch.from_numpy(np.array(pc)).to(device)   # (a writable copy: the cached cloud is read-only)
        self.single = None   # the frame's own single extract call (FrameFeatures), once it has been checked


def _check_frame(f, w, tag):
    """key_pixels[:K], n_key, the key point columns, the valid column over all 1024 rows and the FEW_KEYPTS bit against the expectation."""
    from caelo.engine import ST_FEW_KEYPTS
    k = int(f.n_key.item())
    assert k == w.k, (tag, k, w.k)
    assert np.array_equal(f.key_pixels[:k].cpu().numpy(), w.pix), tag
    rows = f.rows.cpu().numpy()
    assert np.array_equal(rows[:k, 60:63], w.pts), tag
    assert np.array_equal(rows[:, 63], (np.arange(1024) < k).astype(np.float32)), tag
    assert bool(int(f.status[0].item()) & ST_FEW_KEYPTS) == (k <= 50), tag


def _check_equals_single(f, w, tag):
    """A pipeline frame against the same cloud's single extract call: the checks of _check_frame, and the rows (descriptors, key
    points) and the whole status word bit for bit."""
    import torch
    _check_frame(f, w, tag)
    s, k = w.single, w.k
    assert torch.equal(f.rows[:k], s.rows[:k]) and torch.equal(f.key_pixels[:k], s.key_pixels[:k]), tag
    assert int(f.status[0].item()) == int(s.status[0].item()), tag


def _singles(eng, wants):
    for key, w in wants.items():
        if w.single is None:
            f = eng.extract(w.pc)
            _check_frame(f, w, key)
            w.single = f
    assert eng.lane_faults() == 0
    return wants


@pytest.fixture(scope="module")
def shipped(engine, orc, models):
    return {m: _Want(orc, models[0], "shipped", m, engine.device) for m in kpi.SHIPPED_M}


@pytest.fixture(scope="module")
def clamp_engine(engine):   # (the session fixture first: it skips without a GPU)
    import torch
    from test_weight_families_gpu import _fresh
    e = _fresh(respond=kpi.clamp_respond_weights())     # a context of its own: the session engine never sees these weights
    yield e
    del e
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def clamped(clamp_engine, orc):
    layer = orc.RespondLayer(*kpi.clamp_respond_weights())
    return {m: _Want(orc, layer, "clamp", m, clamp_engine.device) for m in kpi.CLAMP_M}


@pytest.mark.parametrize("m", kpi.SHIPPED_M)
def test_fused_extract_counts_under_the_shipped_weights(engine, shipped, m):
    """Single caelo_extract calls on clouds whose candidates are exactly M lattice centres: the selection of the fused path (response
    rows 6..57 only, occupancy from the winner image) equals expected_selection on the oracle's scores."""
    w = shipped[m]
    f = engine.extract(w.pc)
    _check_frame(f, w, m)
    f3 = engine.extract(w.pc, dist_channels=3)      # batch mode: the 10 m gate over xyz alone selects the same centres here
    _check_frame(f3, w, (m, 3))
    assert engine.lane_faults() == 0


@pytest.mark.parametrize("m", kpi.CLAMP_M)
def test_fused_extract_exact_ties_under_clamp_weights(clamp_engine, clamped, m):
    """Every candidate scores exactly 1.0: up to M = 1025 the raw list is ranked, up to 2048 the selection list is exactly full, from
    2049 on the fallback's radix select orders the keys by flat index alone."""
    w = clamped[m]
    _check_frame(clamp_engine.extract(w.pc), w, m)
    assert clamp_engine.lane_faults() == 0


def _run_and_compare(eng, pipe, wants, order, tag):
    import torch
    out = pipe.run([wants[m].pc for m in order], pairs=False)
    torch.cuda.synchronize()
    for i, m in enumerate(order):
        _check_equals_single(out.frame(i), wants[m], (tag, i, m))
    assert eng.lane_faults() == 0


@pytest.mark.parametrize("batch,buffers", [(8, 3), (3, 2)])
def test_pipeline_one_launch_every_branch_shipped(engine, shipped, batch, buffers):
    """The nine shipped-weight clouds (M = 0 .. 3000) side by side in the launches of one pipeline run, in the given and in a fixed
    shuffled order: each frame equals its own single extract call."""
    wants = _singles(engine, shipped)
    pipe = engine.pipeline(batch, buffers)
    order = list(kpi.SHIPPED_M)
    _run_and_compare(engine, pipe, wants, order, "given")
    _run_and_compare(engine, pipe, wants, [order[i] for i in np.random.RandomState(5).permutation(len(order))], "shuffled")


def test_pipeline_one_launch_every_branch_clamp(clamp_engine, clamped):
    """The eight clamp-weight clouds as ONE batch of 8: no candidate, one, K <= 50, the raw list (1025), the listed branch (1026 and
    exactly full at 2048) and the fallback (2049, 3000) in one launch of every kernel of the chain, in two orders."""
    wants = _singles(clamp_engine, clamped)
    pipe = clamp_engine.pipeline(8, 2)
    order = list(kpi.CLAMP_M)
    _run_and_compare(clamp_engine, pipe, wants, order, "given")
    _run_and_compare(clamp_engine, pipe, wants, [order[i] for i in np.random.RandomState(5).permutation(len(order))], "shuffled")


@pytest.mark.parametrize("batch,buffers", [(4, 2), (1, 3)])
def test_pipeline_slots_retenanted_by_another_branch(clamp_engine, clamped, batch, buffers):
    """24 frames cycling fallback (3000 ties) -> M = 1 -> listed and full (2048) -> M = 0 through pipeline(4, 2) and pipeline(1, 3), then
    the same pipeline object again with the cycle shifted by one: a frame's workspace is taken over by a frame of another branch.
    With 3 buffers of one frame a workspace sees every kind in turn; a batch of 4 holds exactly one period, so there a third and a
    fourth run use a period of 5 (... -> listed, 1026), under which position j of consecutive batches changes branch every time.
    Every frame equals its single-call result."""
    wants = _singles(clamp_engine, clamped)
    pipe = clamp_engine.pipeline(batch, buffers)
    for cycle in ([3000, 1, 2048, 0], [3000, 1, 2048, 0, 1026]):
        for shift in (0, 1):
            order = [cycle[(i + shift) % len(cycle)] for i in range(24)]
            _run_and_compare(clamp_engine, pipe, wants, order, "period %d shift %d" % (len(cycle), shift))
