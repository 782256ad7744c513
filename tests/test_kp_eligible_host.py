"""The skip rule of the fused key point chain against the reference rule, without a GPU.

tests/kp_eligible_ref.py restates the eligibility map (k_ring_fill), the needed response blocks (k_respond_mfma) and the live score
tiles (k_kp_score).  Here every cloud of its ``cases`` goes through the oracle -- projection, response layer, GetKeyPtsByAE's score
map -- in both ``dist_channels`` modes, and every centre the reference could select (a stored score: it passed every gate) must be
eligible, lie in a live tile and have every pixel of its 5 x 5 window in a needed block.  The cases must also hit what they were made
for: the corners, the gate columns, the exact threshold, the pixel that is eligible over five channels only, the +inf point."""
import numpy as np
import pytest

import kp_eligible_ref as ker
import kp_images as kpi


@pytest.fixture(scope="module")
def seen(orc, models):
    """name -> dist_c -> (eligible [64,1792], candidates [n,2], ring) from the oracle, computed once."""
    out = {}
    for name, pc in ker.cases().items():
        if name in ker.ORACLE_FREE:
            continue
        ring, cnt = orc.ProjectPC2SphericalRing(pc)
        with np.errstate(invalid="ignore", over="ignore"):
            resp = models[0].predict(ring[None, 0:64, 0:1792, 0:3])[0]
        out[name] = {}
        for dist_c in (5, 3):
            r, c = (ring, cnt) if dist_c == 5 else (np.ascontiguousarray(ring[:64, :1792, :3]), np.ascontiguousarray(cnt[:64, :1792]))
            _, _, smap = kpi.oracle_keypoints(orc, r, c, resp)
            cand = np.argwhere(smap.astype(np.float64) > 0.2)
            out[name][dist_c] = (ker.eligible(ring, cnt, dist_c), cand, ring)
    return out


@pytest.mark.parametrize("dist_c", [5, 3])
@pytest.mark.parametrize("name", [n for n in ker.cases() if n not in ker.ORACLE_FREE])
def test_every_selectable_centre_reads_only_needed_blocks(seen, name, dist_c):
    elig, cand, _ = seen[name][dist_c]
    bits = ker.map_bits(elig)
    need, live = ker.needed_blocks(bits), ker.live_tiles(bits)
    print("%s dist_c %d: %d eligible pixels, %d map bits, %d needed blocks of rows 6..57, %d live tiles, %d candidates"
          % (name, dist_c, elig.sum(), bits.sum(), need[ker.RESP_ROW0:ker.RESP_ROW1].sum(), live.sum(), len(cand)))
    assert np.array_equal(ker.bits_of_words(ker.map_words(elig)), bits)
    assert elig[cand[:, 0], cand[:, 1]].all()
    assert live[(cand[:, 0] - ker.ROW0) // ker.TILE_ROWS, cand[:, 1] // ker.TILE_COLS].all()
    rows, blocks = ker.window_blocks(cand)
    assert need[rows, blocks].all()
    assert ((rows >= ker.RESP_ROW0) & (rows < ker.RESP_ROW1)).all()
    # the block rule is a superset of "within two columns and two rows of an eligible pixel"
    ys, xs = np.nonzero(elig)
    rows, blocks = ker.window_blocks(np.stack([ys, np.clip(xs, 2, ker.NET_W - 3)], axis=1)[(ys >= 2) & (ys < ker.NET_H - 2)])
    assert need[rows, blocks].all()


def _is_candidate(seen, name, dist_c, pixel):
    return bool((seen[name][dist_c][1] == np.asarray(pixel)).all(axis=1).any())


def test_cases_hit_their_corners(seen):
    """The crafted pixels are the only eligible ones of their clouds, they are candidates, and their windows reach into blocks and
    tile rows that hold no eligible pixel of their own."""
    for dist_c in (5, 3):
        elig, cand, _ = seen["corners"][dist_c]
        assert sorted(map(tuple, np.argwhere(elig))) == sorted(ker.CORNERS) == sorted(map(tuple, cand))
        bits = ker.map_bits(elig)
        for row, col in ker.CORNERS:
            assert col % 32 in (0, 31) and (row - 8) % 4 in (0, 3)
            rows, blocks = ker.window_blocks([(row, col)])
            assert len(set(blocks)) == 2 and not bits[rows, blocks].all()      # a neighbouring block with no bit
            assert len({(r - 8) // 4 for r in rows}) == 2                       # and a neighbouring tile row
        for i, c in enumerate(ker.CORNERS):
            elig, cand, _ = seen["corner_%d" % i][dist_c]
            assert [tuple(p) for p in np.argwhere(elig)] == [c] == [tuple(p) for p in cand]
        elig, cand, _ = seen["gates"][dist_c]
        assert sorted(map(tuple, np.argwhere(elig))) == sorted(ker.GATE_IN + ker.GATE_OUT)
        assert sorted(map(tuple, cand)) == sorted(ker.GATE_IN)
        assert not seen["none"][dist_c][0].any() and len(seen["none"][dist_c][1]) == 0
        assert seen["all"][dist_c][0].all() and len(seen["all"][dist_c][1]) > 1025
        left, right = ker.needed_blocks(ker.map_bits(seen["left"][dist_c][0])), ker.needed_blocks(ker.map_bits(seen["right"][dist_c][0]))
        assert left.any() and right.any() and not (left & right).any()


def test_threshold_case_sits_on_the_threshold(seen):
    for dist_c in (5, 3):
        elig, cand, ring = seen["threshold"][dist_c]
        norm = ker.ring_norm(ring[:64, :1792], dist_c)
        for name, (row, col, ch, v) in ker.THRESHOLD.items():
            if ch == dist_c:
                assert norm[row, col] == v, (name, norm[row, col])
                assert elig[row, col] == (v >= np.float32(10.0))
                assert _is_candidate(seen, "threshold", dist_c, (row, col)) == bool(elig[row, col]), name
        assert elig[ker.ONLY_5] == (dist_c == 5) and _is_candidate(seen, "threshold", dist_c, ker.ONLY_5) == (dist_c == 5)
    # over five channels the xyz-tuned pixels are simply far (norm 14), over three the other two are near (norm 7)
    e5, e3 = seen["threshold"][5][0], seen["threshold"][3][0]
    assert e5[30, 400] and e5[30, 440] and not e3[20, 400] and not e3[20, 440]


def test_inf_case_makes_an_eligible_pixel_of_an_infinite_point(seen):
    """The point (inf, 0, 0) wins INF_PIXEL: its norm is +inf, which passes the gate.  (The response layer's relu turns the NaN sums
    around it into 0, so what the rule makes of that pixel and of the far pixel beside it is plain arithmetic; the GPU tests compare
    with the oracle.)"""
    for dist_c in (5, 3):
        elig, cand, ring = seen["inf"][dist_c]
        assert np.isinf(ring[ker.INF_PIXEL][0]) and np.isinf(ker.ring_norm(ring, dist_c)[ker.INF_PIXEL])
        assert elig[ker.INF_PIXEL] and elig[ker.BESIDE_INF]
        assert set(map(tuple, cand)) >= set(ker.CORNERS)


def test_gate_without_the_square_root():
    """k_ring_fill writes the gate `sqrtf(d2) >= 10.0f` as `d2 >= 0x42C7FFFF` (99.99999237): over the floats around 100 the two agree
    (the correctly rounded square root is monotone, so they agree everywhere else), NaN fails both and +inf passes both -- and the
    constant in the source is that one."""
    import os
    t = np.array([0x42C7FFFF], np.uint32).view(np.float32)[0]
    f = np.arange(0x42C80000 - 65536, 0x42C80000 + 65536, dtype=np.uint32).view(np.float32)
    assert np.array_equal(np.sqrt(f) >= np.float32(10.0), f >= t)
    assert np.sqrt(t) == np.float32(10.0) and np.sqrt(np.nextafter(t, np.float32(0.0))) == ker.JUST_BELOW_10
    with np.errstate(invalid="ignore"):
        for v in (np.float32(np.nan), np.float32(np.inf), np.float32(0.0)):
            assert bool(np.sqrt(v) >= np.float32(10.0)) == bool(v >= t)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cae-lo_amd", "csrc", "ring.hip")).read()
    assert "d2 >= __uint_as_float(0x42C7FFFFu)" in src
