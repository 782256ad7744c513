"""caelo_planar_points on the device (k_planar_rule, k_planar_compact; csrc/planar.hip): the crafted image in both ring
layouts, the empty and the capacity image and two synthetic frames through Engine.planar_points -- pixels and points byte-equal to the
host twin, normals within the bar, the comparison rule of tests/planar_ref.py against the NumPy restatement (fed the DEVICE's response
image on the frames, so response parity is no part of this test) --, run-to-run determinism, the rows behind n, the independence of
Engine.icp from the normals' sign, and the api functions."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_clouds as ic
import planar_images as pi
import planar_ref as pr

pytestmark = pytest.mark.gpu


def _device(engine, ring, counter, resp):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)   # noqa: E731
    planar, pixels, n = engine.planar_points(up(ring), up(counter), up(resp))
    k = int(n.item())
    return planar.cpu().numpy(), pixels.cpu().numpy(), k


def _check(engine, label, ring, counter, resp, ref=None, max_undecided=None):
    """device against the host twin, and against the restatement where one is given -> (rows, pixels)"""
    planar, pixels, k = _device(engine, ring, counter, resp)
    rows_h, pixels_h, n_h, _ = pi.host_planar(ring, counter, resp)
    assert k == n_h, (label, k, n_h)
    assert np.array_equal(pixels[:k], pixels_h) and planar[:k, 0:3].tobytes() == rows_h[:, 0:3].tobytes(), label
    worst = float(np.abs(planar[:k, 3:6].astype(np.float64) - rows_h[:, 3:6]).max()) if k else 0.0
    print("planar_errors %-28s device against the host twin: %d rows, normal diff %.3e" % (label, k, worst))
    assert worst <= pr.NORMAL_BAR, (label, worst)
    assert not planar[k:].any() and not pixels[k:].any(), label      # Engine.planar_points hands out zeroed arrays
    if ref is not None:
        pr.compare(ref, planar[:k], pixels[:k], max_undecided=max_undecided, label=label + " (device)")
    return planar[:k], pixels[:k]


@pytest.mark.parametrize("ring_c,height,width", [(3, 64, 1792), (5, 69, 1800)])
def test_crafted_image(engine, ring_c, height, width):
    im, expect = pi.crafted(ring_c, height, width)
    ref = pr.planar_points(im.ring, im.counter, im.resp)
    rows, pixels = _check(engine, "crafted c=%d" % ring_c, im.ring, im.counter, im.resp, ref)
    und = {tuple(p) for p in ref["cand"][pr.undecided(ref)].tolist()}
    for name, want in expect.items():
        if want is not None:
            assert im.at[name] not in und and bool((pixels == np.array(im.at[name])).all(axis=1).any()) == want, name


def test_empty_and_capacity_images(engine):
    im = pi.Image()
    rows, _ = _check(engine, "empty", im.ring, im.counter, im.resp)
    assert len(rows) == 0
    im = pi.capacity()
    rows, pixels = _check(engine, "capacity", im.ring, im.counter, im.resp)
    assert len(rows) == pr.PLANAR_MAX
    yy, xx = np.mgrid[8:56, 8:1784]
    assert np.array_equal(pixels, np.c_[yy.ravel(), xx.ravel()])
    assert np.array_equal(rows[:, 3:6], np.tile(np.array([0, 0, 1], np.float32), (len(rows), 1)))


@pytest.fixture(scope="module")
def frames(engine, orc, scans):
    """frame 0 of both scenes, mm-quantised: ring and counter from the oracle's projection, the response from the device"""
    out = {}
    for kind in ("boxes", "clutter"):
        ring, cnt = orc.ProjectPC2SphericalRing(scans(0, quantum=1e-3, scene_kind=kind))
        resp = engine.respond(torch.from_numpy(ring).to(engine.device)).cpu().numpy()
        out[kind] = (ring, cnt, resp)
    return out


@pytest.mark.parametrize("kind", ["boxes", "clutter"])
def test_synthetic_frames(engine, frames, kind):
    ring, cnt, resp = frames[kind]
    ref = pr.planar_points(ring, cnt, resp)
    assert len(ref["cand"]) > 3000 and len(ref["rows"]) > 2000
    _check(engine, "frame 0 %s" % kind, ring, cnt, resp, ref, max_undecided=0.005)


def test_same_bytes_on_every_run_and_nothing_behind_n(engine, frames):
    """Two calls on the same input give identical bytes (no atomic decides a position), and the entry point leaves the rows from n
    on as it found them."""
    ring, cnt, resp = (torch.from_numpy(a).to(engine.device) for a in frames["boxes"])
    a = [t.cpu().numpy().tobytes() for t in engine.planar_points(ring, cnt, resp)]
    b = [t.cpu().numpy().tobytes() for t in engine.planar_points(ring, cnt, resp)]
    assert a == b
    planar = torch.full((pr.PLANAR_MAX, 6), 7.0, dtype=torch.float32, device=engine.device)
    pixels = torch.full((pr.PLANAR_MAX, 2), -7, dtype=torch.int32, device=engine.device)
    n = torch.full((1,), -1, dtype=torch.int32, device=engine.device)
    ws = torch.empty(int(engine.lib.caelo_planar_ws_bytes()), dtype=torch.uint8, device=engine.device)   # no initialisation needed
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    for px in (pixels, None):
        rc = engine.lib.caelo_planar_points(engine.ctx, ptr(ring), ring.shape[1], ring.shape[2], ptr(cnt), cnt.shape[1], ptr(resp), ptr(ws),
                                            ptr(planar), ptr(px) if px is not None else None, ptr(n), engine.stream)
        assert rc == 0
        k = int(n.item())
        assert 2000 < k < pr.PLANAR_MAX
        assert planar[:k].cpu().numpy().tobytes() == a[0][:k * 24] and pixels[:k].cpu().numpy().tobytes() == a[1][:k * 8]
        assert bool((planar[k:] == 7.0).all()) and bool((pixels[k:] == -7).all())


def test_icp_does_not_depend_on_the_normals_sign(engine):
    """GetPlanarPtsInliners (MyICP.py:104-107) multiplies by the normal twice: with every normal of both sets flipped, Engine.icp
    gives the same result record byte for byte, under both neighbour searches."""
    pc0, pc1, planar0, planar1 = ic.clouds("planar")
    flip = np.array([1, 1, 1, -1, -1, -1], np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(engine.device)   # noqa: E731
    for nn in ("brute", "grid"):
        res = [engine.icp(up(pc0), up(pc1), up(planar0 * s), up(planar1 * s), nn=nn, **ic.device_kw("planar")).cpu().numpy().tobytes() for s in (1, flip)]
        assert res[0] == res[1], nn
        r = engine.icp_result(torch.from_numpy(np.frombuffer(res[0], np.uint8).copy()))
        assert r.success and r.n_inliers_planar >= 200


def test_api_functions(engine, frames):
    from caelo import api
    ring, cnt, resp = frames["boxes"]
    planar, _, k = _device(engine, ring, cnt, resp)
    got = api.GetPlanarPts(ring, cnt, resp)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == planar[:k].tobytes()
    kpts, kpix, third = api.GetKeyPtsByAE(ring, cnt, resp, planar=True)
    assert third.tobytes() == got.tobytes()
    kpts0, kpix0, empty = api.GetKeyPtsByAE(ring, cnt, resp)
    assert empty.shape == (0,) and empty.dtype == np.float32 and np.array_equal(kpix0, kpix) and kpts0.tobytes() == kpts.tobytes()
    on_device = api.GetPlanarPts(*(torch.from_numpy(a).to(engine.device) for a in (ring, cnt, resp)))
    assert isinstance(on_device, torch.Tensor) and on_device.cpu().numpy().tobytes() == got.tobytes()
