"""The designed inputs of tests/kp_images.py, held against the CPU oracle and against the bins they claim to hit -- so that
tests/test_keypoint_select_gpu.py cannot pass on an input that missed its branch.  For every recipe: the oracle's score map is the
designed one (the designed scores at the centres, nothing else above 0.2), the candidate count is the designed M, the oracle's key
pixels are ``expected_selection`` (SphericalRing.py:192-218 as a list rule) and, for the bin cases, kp_bin recomputed in NumPy gives
the claimed cut bin, nsel and branch."""
import numpy as np
import pytest

import kp_images as kpi


def _check_against_oracle(orc, ring, cnt, resp, centres, scores, want):
    kp, kpix, smap = kpi.oracle_keypoints(orc, ring, cnt, resp)
    cand = np.asarray(scores, np.float32).astype(np.float64) > 0.2
    designed = np.zeros((kpi.NET_H, kpi.NET_W), np.float32)
    designed[centres[cand, 0], centres[cand, 1]] = scores[cand]
    assert np.array_equal(smap, designed)                                   # the designed scores at the centres, 0 elsewhere
    assert int((smap.astype(np.float64) > 0.2).sum()) == int(cand.sum())    # M
    assert np.array_equal(kpix, want) and np.array_equal(kp, ring[want[:, 0], want[:, 1], 0:3])
    if len(want) > 50:   # the reference-shaped call returns there (it asserts K > 50 like SphericalRing.py:286)
        o = orc.GetKeyPtsByAE(ring, cnt, resp)
        assert np.array_equal(o[1], want)
    else:
        with pytest.raises(AssertionError):
            orc.GetKeyPtsByAE(ring, cnt, resp)


def test_lattice_is_isolated_and_clear_of_the_column_quirk():
    lat = kpi.lattice()
    assert lat.shape == (9392, 2) and len(np.unique(lat[:, 0] * kpi.NET_W + lat[:, 1])) == 9392
    assert lat[:, 0].min() == 8 and lat[:, 0].max() == 53 and lat[:, 1].min() == 8 and lat[:, 1].max() == 1781
    assert not ((lat[:, 1] >= 53) & (lat[:, 1] <= 66)).any()
    occ = np.zeros((kpi.NET_H, kpi.NET_W), np.int32)
    occ[lat[:, 0], lat[:, 1]] = 1
    win = sum(np.roll(np.roll(occ, dy, 0), dx, 1) for dy in range(-2, 3) for dx in range(-2, 3))
    assert win[lat[:, 0], lat[:, 1]].max() == 1                             # no centre's 5 x 5 window holds another centre
    assert len(kpi.pick(4696, 1, rows_from=kpi.CLAMP_ROWS_FROM)) == 4696
    with pytest.raises(AssertionError):
        kpi.pick(4697, 1, rows_from=kpi.CLAMP_ROWS_FROM)


def test_bins_and_threshold_constants():
    f = np.float32
    assert kpi.kp_bin(f(0.2)) == kpi.BIN_0P2 == 76 and kpi.kp_bin(f(2.5)) == kpi.BIN_2P5 == 544
    assert kpi.kp_bin(f(2.0)) == 512 and kpi.kp_bin(f(2.015625)) == 513 and kpi.kp_bin(np.nextafter(f(2.03125), f(0))) == 513
    assert kpi.kp_bin(kpi.V8160) == 2047 and kpi.kp_bin(kpi.BELOW_8160) == 2046 and kpi.kp_bin(f(8128.0)) == 2046
    assert kpi.kp_bin(f(1.8e19)) == 2047 and kpi.kp_bin(f(3e38)) == 2047 and kpi.kp_bin(f(0.0)) == 0
    assert np.float64(f(0.2)) > 0.2 and not np.float64(np.nextafter(f(0.2), f(0))) > 0.2
    v = np.random.RandomState(3).uniform(0.2, 1e19, 5000).astype(f)
    assert np.array_equal(kpi.scores_of(v), v)                              # sqrt(v * v) == v in float32


def test_expected_selection_rule():
    c = np.array([(8, 8), (8, 11), (11, 8), (11, 11), (14, 8)], np.int64)
    s = np.array([1.0, np.nan, 1.0, 0.2 - 1e-3, 3.0], np.float32)
    assert kpi.expected_selection(c, s).tolist() == [[8, 8], [11, 8]]       # ties by flat index, the single best dropped, NaN no candidate
    assert kpi.expected_selection(c, s, range_ok=[0, 1, 1, 1, 1]).tolist() == [[11, 8]]
    assert kpi.expected_selection(c[:1], s[:1]).shape == (0, 2) and kpi.expected_selection(c[:0], s[:0]).shape == (0, 2)
    d = kpi.design(np.full(2049, 2.5, np.float32))
    assert d == kpi.Design(2049, 1024, 544, 2049, kpi.STATE_FALLBACK, 0)
    assert kpi.design(np.full(1025, 2.5, np.float32)) == kpi.Design(1025, 1024, None, 0, kpi.STATE_NONE, 0)


@pytest.mark.parametrize("name", list(kpi.staged_cases()))
def test_staged_case_is_what_it_claims(orc, name):
    case = kpi.staged_cases()[name]
    d = kpi.design(case.scores)
    for key, want in case.claim.items():
        assert getattr(d, key) == want, (name, key, getattr(d, key), want)
    assert d.K == min(max(d.M, 1) - 1, 1024) and len(case.centres) == len(case.values)
    if d.M > kpi.KEEP:   # the cut bin holds the 1025th largest score, and fewer than 1025 lie above it
        s = np.sort(case.scores[case.scores.astype(np.float64) > 0.2])[::-1]
        assert kpi.kp_bin(s[kpi.KEEP - 1]) == d.cut_bin and (kpi.kp_bin(s) > d.cut_bin).sum() < kpi.KEEP <= d.nsel
    want = kpi.expected_selection(case.centres, case.scores)
    assert len(want) == d.K
    for channels in (5, 3):
        ring, cnt, resp = kpi.lattice_images(case.values, case.centres, channels)
        assert ring.shape == ((69, 1800, 5) if channels == 5 else (64, 1792, 3)) and cnt.shape == ring.shape[:2] and cnt.min() == 1
        assert all(kpi.ring_norm(ring[r, c]) == np.float32(20.0) for r, c in ((0, 0), (33, 900), (ring.shape[0] - 1, ring.shape[1] - 1)))
        _check_against_oracle(orc, ring, cnt, resp, case.centres, case.scores, want)


def test_parity_cases_cover_both_bins_of_a_pair():
    cases = kpi.staged_cases()

    def hist(name):
        return np.bincount(kpi.kp_bin(cases[name].scores), minlength=2048)
    h = hist("cut_odd_513")
    assert h[514:].sum() < 1025 <= h[513:].sum()                             # the 1025th largest lies in the odd bin
    h = hist("cut_even_512")
    assert h[513:].sum() < 1025 <= h[512:].sum() and h[513] > 0             # even bin; the odd partner plus everything above stays below
    h = hist("cut_even_512_partner_holds_1024")
    assert h[513] == 1024 and h[514:].sum() == 0 and h[512] > 0             # even bin while the odd partner alone holds 1024
    h = hist("cut_odd_513_holds_1025")
    assert h[513] == 1025 and h[514:].sum() == 0
    h = hist("last_bin_fallback")
    top = cases["last_bin_fallback"].scores
    top = top[top >= kpi.V8160].view(np.uint32)
    assert h[2047] == 2100 and len(np.unique(top >> 24)) > 8 and len(np.unique((top >> 16) & 255)) > 200   # the radix select has score bytes to separate
    for name, want in (("edge_8160_top1024", kpi.BELOW_8160), ("edge_8160_top1025", kpi.V8160)):
        s = np.sort(cases[name].scores)
        assert s[-1025] == want and kpi.V8160 in s and kpi.BELOW_8160 in s  # scores on both sides of 8160.0, the cut on either
    s = cases["threshold_among_1100"].scores
    assert (s == np.float32(0.2)).sum() == 1 and (s < np.float32(0.2)).sum() == 1
    want = kpi.expected_selection(cases["threshold_cut_in_bin_0x4c"].centres, cases["threshold_cut_in_bin_0x4c"].scores)
    assert np.array_equal(want[0], cases["threshold_cut_in_bin_0x4c"].centres[2])   # row 0 is nextafter(0.2, 1); float32(0.2) is cut


@pytest.mark.parametrize("channels", [5, 3])
def test_gate_probes_against_the_oracle(orc, channels):
    ring, cnt, resp, probes, base = kpi.gate_images(channels)
    names = {p.name for p in probes}
    assert {"occupied_4", "occupied_5", "unoccupied_centre", "norm_just_below_10", "norm_exactly_10", "channel_5_only", "all_8_channels"} <= names
    assert {"row_%d" % r for r in (7, 8, 55, 56)} | {"col_%d" % c for c in (7, 8, 55, 56, 63, 64, 1783, 1784)} <= names
    assert ("norm_with_range_channel" in names) == (channels == 5)
    kp, kpix, smap = kpi.oracle_keypoints(orc, ring, cnt, resp)
    for p in probes:   # the per-pixel statement: a candidate carries its score, anything else 0
        assert smap[p.row, p.col] == (p.score if p.candidate else 0.0), p
        window = cnt[p.row - 2:p.row + 3, p.col - 2:p.col + 3]
        if p.name.startswith("occupied_"):
            assert window.sum() - 1 == int(p.name[-1])
    assert [p.candidate for p in probes if p.name.startswith(("row_", "col_"))] == [False, True, True, False] + [False, True, True, False, False, True, True, False]
    want = kpi.gate_expected(probes, base)
    assert len(want) == 120 + sum(p.candidate for p in probes) - 1 and np.array_equal(kpix, want)
    assert int((smap.astype(np.float64) > 0.2).sum()) == len(want) + 1


@pytest.mark.parametrize("kind,m", kpi.fused_recipes())
def test_cloud_recipe_against_the_oracle(orc, models, kind, m):
    pc, centres = kpi.fused_cloud(kind, m)
    assert pc.shape == (64 * 1792, 4) and pc.dtype == np.float32 and len(centres) == m
    ring, cnt = orc.ProjectPC2SphericalRing(pc)
    assert (cnt[0:64, 0:1792] == 1).all() and cnt.sum() == 64 * 1792       # every net pixel exactly one point, none elsewhere
    is_centre = np.zeros((64, 1792), bool)
    is_centre[centres[:, 0], centres[:, 1]] = True
    rng = ring[0:64, 0:1792, 4]
    assert (np.abs(rng[~is_centre] - 5.0) < 1e-5).all() and (rng[is_centre] >= (12.0 if kind == "shipped" else 40.0) - 1e-4).all()
    layer = models[0] if kind == "shipped" else orc.RespondLayer(*kpi.clamp_respond_weights())
    resp = layer.predict(ring[None, 0:64, 0:1792, 0:3])[0]
    for channels in (5, 3):
        r, c = (ring, cnt) if channels == 5 else (np.ascontiguousarray(ring[0:64, 0:1792, 0:3]), np.ascontiguousarray(cnt[0:64, 0:1792]))
        kp, kpix, smap = kpi.oracle_keypoints(orc, r, c, resp)
        assert np.array_equal(smap.astype(np.float64) > 0.2, is_centre)     # the candidates are exactly the centres: M = m
        scores = smap[centres[:, 0], centres[:, 1]]
        if kind == "clamp":
            assert (resp[..., 0][is_centre] == 1.0).all() and (resp[..., 0][~is_centre] == 0.0).all() and not resp[..., 1:].any()
            assert (scores == 1.0).all()
            flat = np.sort(centres[:, 0] * 1792 + centres[:, 1])[-1025:-1]      # the ascending flat indices [-1025:-1]
            assert np.array_equal(kpix[:, 0] * 1792 + kpix[:, 1], flat)
        elif m:
            assert scores.min() >= 1.2
        assert np.array_equal(kpix, kpi.expected_selection(centres, scores))
        assert len(kpix) == min(max(m, 1) - 1, 1024)
    d = kpi.design(np.ones(m, np.float32)) if kind == "clamp" else None
    if kind == "clamp" and m > 1025:
        assert d.state == (kpi.STATE_LISTED if m <= 2048 else kpi.STATE_FALLBACK) and d.nsel == m
