"""The fused path's eligibility map and what k_respond_mfma / k_kp_score skip by it (csrc/ring.hip), on the clouds of
tests/kp_eligible_ref.py (tests/test_kp_eligible_host.py holds each of them against the oracle and against the corner it was made for).

Every case, in both ``dist_channels`` modes: the fused ``extract`` equals the staged chain caelo_project -> caelo_respond ->
caelo_keypoints -- which has no map and computes all 64 response rows -- bit for bit in key pixels, key points, n_key, the status bits
of the chain and the candidate count; it equals the oracle's key points; and the map read back from the workspace equals the NumPy
restatement exactly (a set, not a superset).  Then: a frame with no eligible pixel leaves the response image untouched; two frames
with disjoint needed blocks share one workspace in both orders with the response image overwritten by NaN patterns in between; eight
frames of different eligibility go through one pipeline launch and equal their single calls."""
import numpy as np
import pytest

import kp_eligible_ref as ker
import kp_images as kpi

pytestmark = pytest.mark.gpu

RING_BYTES = (kpi.RING_H * kpi.RING_W * 5 * 4 + 255) // 256 * 256
RESP_BYTES = kpi.NET_H * kpi.NET_W * 8 * 4
NAN_PATTERN = 0x7FC00BAD     # a quiet NaN no kernel produces


class _Staged:
    """One cloud through the staged chain (everything computed) and the oracle, per dist_channels mode, computed once."""

    def __init__(self, engine, orc, layer, name):
        import torch
        from caelo.engine import ST_COL_OOB, ST_FEW_KEYPTS, ST_NONFINITE
        self.name = name
        pc = ker.cases()[name]
        self.pc = torch.from_numpy(np.array(pc)).to(engine.device)
        ring, counter, status = engine.project(self.pc)
        self.resp = engine.respond(ring)
        self.mode = {}
        for dist_c in (5, 3):
            r, c = (ring, counter) if dist_c == 5 else (ring[:64, :1792, :3].contiguous(), counter[:64, :1792].contiguous())
            st = status.clone()
            kpts, kpix, nkey, st = engine.keypoints(r, c, self.resp, status=st)
            ws = engine._ws("keypoints", engine.lib.caelo_keypoints_ws_bytes())
            off = kpi.NET_H * kpi.NET_W * 8
            m = int(ws[off:off + 4].clone().view(torch.int32).item())
            k = int(nkey.item())
            self.mode[dist_c] = dict(k=k, pix=kpix[:k].cpu().numpy(), pts=kpts[:k].cpu().numpy(), m=m,
                                     status=int(st.item()) & (ST_COL_OOB | ST_FEW_KEYPTS | ST_NONFINITE))
        self.ring, self.cnt = ring.cpu().numpy(), counter.cpu().numpy()
        if name not in ker.ORACLE_FREE:
            o_ring, o_cnt = orc.ProjectPC2SphericalRing(pc)
            assert np.array_equal(o_ring.view(np.uint32), self.ring.view(np.uint32)) and np.array_equal(o_cnt, self.cnt)
            with np.errstate(invalid="ignore", over="ignore"):
                o_resp = layer.predict(o_ring[None, 0:64, 0:1792, 0:3])[0]
            for dist_c in (5, 3):
                r, c = (o_ring, o_cnt) if dist_c == 5 else (np.ascontiguousarray(o_ring[:64, :1792, :3]), np.ascontiguousarray(o_cnt[:64, :1792]))
                o_pts, o_pix, _ = kpi.oracle_keypoints(orc, r, c, o_resp)
                s = self.mode[dist_c]
                assert np.array_equal(s["pix"], o_pix) and np.array_equal(s["pts"].view(np.uint32), o_pts.view(np.uint32)), (name, dist_c)

    def map_words(self, dist_c):
        return ker.map_words(ker.eligible(self.ring, self.cnt, dist_c))


@pytest.fixture(scope="module")
def staged(engine, orc, models):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Staged(engine, orc, models[0], name)
        return cache[name]
    return get


def _offsets(engine):
    off = int(engine.lib.caelo_extract_ws_kp_eligible_offset())
    return off - 256, off, off + 512 + RING_BYTES      # cand_count | the map | (the ring image) | the response image


def _ws(engine):
    return engine._ws("extract", int(engine.lib.caelo_extract_ws_bytes()))


def _fill_resp(engine, pattern=NAN_PATTERN):
    import torch
    resp_off = _offsets(engine)[2]
    _ws(engine)[resp_off:resp_off + RESP_BYTES].view(torch.int32).fill_(pattern)


def _read_resp(engine):
    import torch
    resp_off = _offsets(engine)[2]
    return _ws(engine)[resp_off:resp_off + RESP_BYTES].clone().view(torch.int32).view(kpi.NET_H, kpi.NET_W, 8).cpu().numpy()


def _check_fused(engine, s, dist_c, tag):
    """One fused extract of ``s`` against its staged chain and the restated map -> the FrameFeatures."""
    import torch
    from caelo.engine import ST_COL_OOB, ST_FEW_KEYPTS, ST_NONFINITE
    f = engine.extract(s.pc, dist_channels=dist_c)
    words = engine.extract_kp_eligible()
    cc_off = _offsets(engine)[0]
    m = int(_ws(engine)[cc_off:cc_off + 4].clone().view(torch.int32).item())
    want, k = s.mode[dist_c], int(f.n_key.item())
    print("%s: K %d, M %d, status %d, %d map bits" % (tag, k, m, int(f.status[0].item()), ker.bits_of_words(words).sum()))
    assert np.array_equal(words, s.map_words(dist_c)), tag
    assert k == want["k"] and m == want["m"], (tag, k, m, want["k"], want["m"])
    assert np.array_equal(f.key_pixels[:k].cpu().numpy(), want["pix"]), tag
    rows = f.rows.cpu().numpy()
    assert np.array_equal(rows[:k, 60:63].view(np.uint32), want["pts"].view(np.uint32)), tag
    assert np.array_equal(rows[:, 63], (np.arange(1024) < k).astype(np.float32)), tag
    assert int(f.status[0].item()) & (ST_COL_OOB | ST_FEW_KEYPTS | ST_NONFINITE) == want["status"], tag
    return f


@pytest.mark.parametrize("dist_c", [5, 3])
@pytest.mark.parametrize("name", ["corners", "corner_0", "corner_1", "corner_2", "corner_3", "gates", "all", "threshold", "inf", "nan",
                                  "upper_half"])
def test_fused_extract_equals_the_staged_chain(engine, staged, name, dist_c):
    """Corners of blocks and tiles, the gate columns and rows, every pixel eligible, the exact threshold in either mode and the pixel
    eligible over five channels only, an infinite and a NaN coordinate, the upper half of the image."""
    from caelo.engine import ST_NONFINITE
    s = staged(name)
    _fill_resp(engine)      # whatever an earlier frame left must not matter
    _check_fused(engine, s, dist_c, "%s/%d" % (name, dist_c))
    assert bool(s.mode[dist_c]["status"] & ST_NONFINITE) == (name == "nan")
    assert engine.lane_faults() == 0


def test_every_pixel_eligible_computes_the_whole_response(engine, staged):
    """With every map bit set the fused path's response rows 6..57 are the staged layer's, bit for bit (this also pins where the
    response image lies in the workspace, which the NaN fills of this file rely on)."""
    s = staged("all")
    _fill_resp(engine)
    _check_fused(engine, s, 5, "all")
    got, want = _read_resp(engine), s.resp.cpu().numpy().view(np.int32)
    assert np.array_equal(got[ker.RESP_ROW0:ker.RESP_ROW1], want[ker.RESP_ROW0:ker.RESP_ROW1])
    assert (got[:ker.RESP_ROW0] == NAN_PATTERN).all() and (got[ker.RESP_ROW1:] == NAN_PATTERN).all()


@pytest.mark.parametrize("dist_c", [5, 3])
def test_no_eligible_pixel_computes_no_response_block(engine, staged, dist_c):
    from caelo.engine import ST_FEW_KEYPTS
    s = staged("none")
    _fill_resp(engine)
    f = _check_fused(engine, s, dist_c, "none/%d" % dist_c)
    assert int(f.n_key.item()) == 0 and s.mode[dist_c]["m"] == 0 and int(f.status[0].item()) & ST_FEW_KEYPTS
    assert (_read_resp(engine) == NAN_PATTERN).all()


def test_only_needed_blocks_are_written(engine, staged):
    """Four isolated eligible pixels: exactly the needed blocks of rows 6..57 hold the staged layer's values afterwards, every other
    block keeps the pattern it was filled with."""
    s = staged("corners")
    _fill_resp(engine)
    _check_fused(engine, s, 5, "corners")
    got, want = _read_resp(engine), s.resp.cpu().numpy().view(np.int32)
    need = ker.needed_blocks(ker.bits_of_words(s.map_words(5)))
    need[:ker.RESP_ROW0] = False
    need[ker.RESP_ROW1:] = False
    px = np.repeat(need, ker.BLK, axis=1)
    assert need.sum() == 54 and np.array_equal(got[px], want[px]) and (got[~px] == NAN_PATTERN).all()


@pytest.mark.parametrize("order", [("left", "right"), ("right", "left")])
def test_workspace_retenanted_by_a_frame_with_other_blocks(engine, staged, order):
    """Two frames whose needed blocks are disjoint, back to back through one workspace; in between the response image is overwritten
    with NaN patterns.  The second frame equals its staged chain and, row for row, its own run on a wiped workspace."""
    import torch
    first, second = staged(order[0]), staged(order[1])
    _ws(engine).zero_()
    fresh = _check_fused(engine, second, 5, "fresh " + order[1])
    fresh_rows, fresh_k = fresh.rows.clone(), int(fresh.n_key.item())
    _check_fused(engine, first, 5, order[0])
    _fill_resp(engine)
    again = _check_fused(engine, second, 5, order[1] + " after " + order[0])
    assert int(again.n_key.item()) == fresh_k and torch.equal(again.rows[:fresh_k], fresh_rows[:fresh_k])
    assert torch.equal(again.key_pixels[:fresh_k], fresh.key_pixels[:fresh_k]) and torch.equal(again.status, fresh.status)
    assert engine.lane_faults() == 0


@pytest.mark.parametrize("dist_c", [5, 3])
def test_pipeline_one_launch_of_eight_eligibilities(engine, staged, dist_c):
    """none / all / the upper half / one pixel / corners / gates / threshold / the left third as ONE batch of eight, in the given
    order and reversed: every frame equals its single extract call (which equals the staged chain) in rows, key pixels and status."""
    import torch
    singles = {}
    for name in ker.PIPELINE_ORDER:
        singles[name] = _check_fused(engine, staged(name), dist_c, "single %s/%d" % (name, dist_c))
    pipe = engine.pipeline(8, 2)
    for order in (list(ker.PIPELINE_ORDER), list(ker.PIPELINE_ORDER)[::-1]):
        out = pipe.run([staged(n).pc for n in order], dist_channels=dist_c, pairs=False)
        torch.cuda.synchronize()
        for i, name in enumerate(order):
            f, s = out.frame(i), singles[name]
            k = int(s.n_key.item())
            assert int(f.n_key.item()) == k, (name, i)
            assert torch.equal(f.rows[:k], s.rows[:k]) and torch.equal(f.key_pixels[:k], s.key_pixels[:k]), (name, i)
            assert torch.equal(f.rows[:, 63], s.rows[:, 63]) and int(f.status[0].item()) == int(s.status[0].item()), (name, i)
    assert engine.lane_faults() == 0
