"""k_project_points (csrc/ring.hip) on the points of tests/golden/ring_edges.npz: the device's f64 atan2 and asin against the host's C
library where one ulp decides the pixel (tests/test_ring_edges_host.py holds the fixture against the oracle and shows that it is sharp).

The whole fixture in file order and reversed, the same-pixel group, the column-1800 points, launches of 4 / 255 / 256 / 257 points
with guard words behind every buffer and live points behind the cloud, the fused path's eligibility map on the probes that sit on the
edges of its 32-column blocks, and two frames of unequal length behind one launch.  A failure names the points that moved."""
import os

import numpy as np
import pytest

import kp_eligible_ref as ker
import ring_ref as rr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NPIX = rr.RING_H * rr.RING_W
GUARD = 0x5EEDBEEF
GUARD_WORDS = 64


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "ring_edges.npz")))


def _device(engine, pc):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pc, np.float32)).to(engine.device)


def _moved(fx, ring, o_ring):
    """The points the device put elsewhere than the oracle, one line each (the intensity of a ring pixel is its point's index + 1)."""
    pts, lines = np.concatenate([fx["points"], fx["oob_points"]]), []
    got, want = ring.reshape(NPIX, 5)[:, 3].astype(np.int64) - 1, o_ring.reshape(NPIX, 5)[:, 3].astype(np.int64) - 1
    where_got = {int(i): int(p) for p, i in enumerate(got) if i >= 0}
    for p in np.flatnonzero(got != want):
        for i in (want[p], got[p]):
            if i >= 0:
                e = fx["pixel"][i] if i < len(fx["points"]) else fx["oob_pixel"][i - len(fx["points"])]
                g = divmod(where_got[int(i)], rr.RING_W) if int(i) in where_got else None
                lines.append("point %d (x %r, y %r): expected pixel (%d, %d), %s" % (
                    i, float(pts[i, 0]), float(pts[i, 1]), e[0], e[1], "got (%d, %d)" % g if g else "not the winner of any pixel"))
    return "\n".join(sorted(set(lines)))


def _check(engine, orc, fx, pc, tag):
    """One caelo_project of ``pc`` against the oracle: ring, counter and status word, bit for bit."""
    ring, counter, status = engine.project(_device(engine, pc))
    ring, counter, status = ring.cpu().numpy(), counter.cpu().numpy(), int(status.item())
    o_ring, o_cnt = orc.ProjectPC2SphericalRing(pc)
    same = np.array_equal(ring.view(np.uint32), o_ring.view(np.uint32))
    assert same, "%s: the ring differs from the oracle's\n%s" % (tag, _moved(fx, ring, o_ring))
    assert np.array_equal(counter, o_cnt), "%s: the counter differs at pixels %s" % (tag, np.argwhere(counter != o_cnt)[:8].tolist())
    assert status == 0, (tag, status)
    return ring, counter


def test_whole_fixture_equals_the_oracle(engine, orc, fx):
    ring, counter = _check(engine, orc, fx, fx["points"], "file order")
    occ = np.flatnonzero(counter.ravel())
    assert np.array_equal(occ, fx["ring_pixels"]) and np.array_equal(counter.ravel()[occ], fx["ring_counts"])
    assert np.array_equal(ring.reshape(NPIX, 5)[occ, 3], fx["ring_winners"].astype(np.float32) + 1)
    assert engine.lane_faults() == 0


def test_reversed_order_and_the_same_pixel_group(engine, orc, fx):
    """The winners and the counts follow file order: in either order a group's pixel holds the group's last point and counts three."""
    pts = fx["points"]
    for tag, pc in (("file order", pts), ("reversed", pts[::-1])):
        ring, counter = _check(engine, orc, fx, pc, tag)
        for g in range(3):
            m = np.flatnonzero(fx["group"] == g)
            row, col = fx["pixel"][m[0]]
            last = m[-1] if tag == "file order" else m[0]
            assert counter[row, col] == 3 and ring[row, col, 3] == pts[last, 3], (tag, g)
    # a group alone, padded to n > 3 with points of zero range, in every order of its three points
    for g in range(3):
        m = np.flatnonzero(fx["group"] == g)
        for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            pc = np.concatenate([np.zeros((2, 4), np.float32), pts[m[list(order)]]])
            _check(engine, orc, fx, pc, "group %d order %r" % (g, order))


def test_column_1800_sets_the_status_bit_and_raises(engine, orc, fx):
    from caelo import api
    from caelo.engine import ST_COL_OOB
    pad = fx["points"][fx["kind"] == rr.ROW_PROBE][:3]
    for i, p in enumerate(fx["oob_points"]):
        pc = np.concatenate([pad, p[None]])
        _, _, status = engine.project(_device(engine, pc))
        assert int(status.item()) == ST_COL_OOB, (i, p, int(status.item()))
        with pytest.raises(IndexError):
            orc.ProjectPC2SphericalRing(pc)
    for pc in (np.concatenate([pad, fx["oob_points"][:1]]), np.concatenate([fx["points"], fx["oob_points"]])):
        with pytest.raises(IndexError):
            api.ProjectPC2SphericalRing(pc)
        with pytest.raises(IndexError):
            orc.ProjectPC2SphericalRing(pc)
    _, _, status = engine.project(_device(engine, pad.repeat(2, axis=0)))      # the same pad without such a point: no bit
    assert int(status.item()) == 0


@pytest.mark.parametrize("n", [4, 255, 256, 257])
def test_launch_edges_write_nothing_behind_their_buffers(engine, orc, fx, n):
    """The first n points: one workgroup not full, full, and one point into the second.  Guard words behind the ring, the counter and
    the winner buffer stay, and the points that lie behind the cloud in memory -- live probes -- are not projected."""
    import torch
    from caelo import _ffi
    from caelo.engine import _ptr
    pts = fx["points"]
    assert len(pts) >= n + 64
    pc = _device(engine, pts[:n + 64])
    ring = torch.full((NPIX * 5 + GUARD_WORDS,), GUARD, dtype=torch.int32, device=engine.device)
    counter = torch.full((NPIX + GUARD_WORDS,), GUARD, dtype=torch.int32, device=engine.device)
    winner = torch.full((NPIX + GUARD_WORDS,), GUARD, dtype=torch.int32, device=engine.device)
    status = torch.zeros((1 + GUARD_WORDS,), dtype=torch.int32, device=engine.device)
    status[1:] = GUARD
    _ffi.check(engine.lib.caelo_project(engine.ctx, _ptr(pc), n, _ptr(ring), _ptr(counter), _ptr(winner), _ptr(status), engine.stream))
    torch.cuda.synchronize()
    ring, counter, winner, status = ring.cpu().numpy(), counter.cpu().numpy(), winner.cpu().numpy(), status.cpu().numpy()
    for name, buf, size in (("ring", ring, NPIX * 5), ("counter", counter, NPIX), ("winner", winner, NPIX), ("status", status, 1)):
        assert (buf[size:] == np.int32(GUARD)).all(), "%s: guard words overwritten (n = %d)" % (name, n)
    o_ring, o_cnt = orc.ProjectPC2SphericalRing(pts[:n])
    got = ring[:NPIX * 5].view(np.float32).reshape(rr.RING_H, rr.RING_W, 5)
    assert np.array_equal(got.view(np.uint32), o_ring.view(np.uint32)), "n = %d\n%s" % (n, _moved(fx, got, o_ring))
    assert np.array_equal(counter[:NPIX].reshape(rr.RING_H, rr.RING_W), o_cnt) and status[0] == 0
    want_winner = np.where(o_cnt.ravel() > 0, o_ring.reshape(NPIX, 5)[:, 3].astype(np.int64) - 1, -1)      # (n <= 257: index = intensity - 1)
    assert np.array_equal(winner[:NPIX], want_winner) and winner[:NPIX].max() < n


def _block_edge_frame(fx):
    """The off-axis probes on the edges of the eligibility map's 32-column blocks, at 10 m or more, inside the map's rows."""
    pts, edge = fx["points"], fx["edge"]
    m = np.isin(fx["kind"], (rr.OFF_AXIS, rr.OFF_AXIS_EXTRA)) & (edge % 32 == 0) & (rr.ranges(pts) >= 10) & (fx["pixel"][:, 0] < ker.NET_H)
    assert len(set(edge[m])) >= 16 and m.sum() > 3
    return np.ascontiguousarray(pts[m]), fx["pixel"][m], edge[m]


@pytest.mark.parametrize("dist_c", [5, 3])
def test_fused_path_eligibility_map_on_block_edges(engine, orc, fx, dist_c):
    """counter == nullptr and k_ring_fill's map: a probe on the wrong side of its edge sets the neighbouring block's bit, which no
    other probe of its row does (the tool keeps both blocks of a probe's row free of other such probes)."""
    from caelo.engine import ST_COL_OOB, ST_FEW_KEYPTS, ST_NONFINITE
    pc, pixel, edge = _block_edge_frame(fx)
    o_ring, o_cnt = orc.ProjectPC2SphericalRing(pc)
    want = ker.map_words(ker.eligible(o_ring, o_cnt, dist_c))
    bits = ker.bits_of_words(want)
    inside = pixel[:, 1] < ker.NET_W
    assert bits.sum() == inside.sum() > 16                # every probe inside the net columns has a bit of its own ...
    for (row, col), c in zip(pixel, edge):                # ... and the block on the other side of its edge is empty in its row
        other = c // 32 if col < c else c // 32 - 1
        assert 0 <= other and (other >= ker.NBLK or not bits[row, other]), (row, col, c)
    f = engine.extract(_device(engine, pc), dist_channels=dist_c)
    words = engine.extract_kp_eligible()
    assert int(f.status[0].item()) & (ST_COL_OOB | ST_FEW_KEYPTS | ST_NONFINITE) == ST_FEW_KEYPTS and int(f.n_key.item()) == 0
    wrong = np.argwhere(ker.bits_of_words(words) != bits)
    assert np.array_equal(words, want), "dist_c %d: (row, block) of the map bits that differ: %s" % (dist_c, wrong.tolist())
    assert engine.lane_faults() == 0


def test_two_frames_of_unequal_length_behind_one_launch(engine, orc, fx):
    """The fixture as two frames that lie back to back in memory, through the pipeline's frame set (blockIdx.z, the i >= F.n guard: a
    frame that read past its end would project its neighbour's probes): each frame's ring image and map equal its single extract's and
    the oracle's."""
    import torch
    from caelo.engine import ST_COL_OOB, ST_NONFINITE
    pts = fx["points"]
    cut = 257 + 64 * 3 + 7
    both = _device(engine, pts)
    frames = [both[:cut], both[cut:]]
    assert frames[0].shape[0] != frames[1].shape[0] and min(f.shape[0] for f in frames) > 3
    off = int(engine.lib.caelo_extract_ws_ring_offset())
    singles = []
    for f, lo, hi in ((frames[0], 0, cut), (frames[1], cut, len(pts))):
        ff = engine.extract(f.clone(), dist_channels=5)
        words = engine.extract_kp_eligible()
        ws = engine._ws("extract", int(engine.lib.caelo_extract_ws_bytes()))
        ring = ws[off:off + NPIX * 20].cpu().numpy().view(np.float32).reshape(rr.RING_H, rr.RING_W, 5).copy()
        o_ring, o_cnt = orc.ProjectPC2SphericalRing(pts[lo:hi])
        assert np.array_equal(ring.view(np.uint32), o_ring.view(np.uint32)), "single frame %d..%d\n%s" % (lo, hi, _moved(fx, ring, o_ring))
        assert np.array_equal(words, ker.map_words(ker.eligible(o_ring, o_cnt, 5)))
        singles.append((ring, words, int(ff.status[0].item())))
    pipe = engine.pipeline(2, 2)
    for order in ((0, 1), (1, 0)):
        out = pipe.run([frames[i] for i in order], dist_channels=5, pairs=False)
        torch.cuda.synchronize()
        for slot, i in enumerate(order):
            ring, words = pipe.extract_ring_and_map(slot)
            assert np.array_equal(ring.view(np.uint32), singles[i][0].view(np.uint32)), "frame %d in slot %d\n%s" % (
                i, slot, _moved(fx, ring, singles[i][0]))
            assert np.array_equal(words, singles[i][1]), (i, slot)
            status = int(out.status[slot, 0].item())
            assert status == singles[i][2] and not status & (ST_COL_OOB | ST_NONFINITE), (i, slot, status)
    assert engine.lane_faults() == 0
