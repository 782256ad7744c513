"""caelo_scan_context and caelo_loop_search on the device (k_sc_build, k_sc_prepare, k_loop_search, k_loop_merge; csrc/loopclose.hip,
DESIGN.md 9n) through Engine.scan_context / Engine.loop_search: the clouds and images of tests/test_loops_host.py, every output equal
to the host twins' BYTE FOR BYTE -- SC, u, valid, the dense distances and shifts, the k best.  For the search that is the claim
that v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, tested directly.  Also: two calls give the same bytes, a query range equals its
slice, and nothing outside the outputs is written."""
import ctypes as C

import numpy as np
import pytest
import torch

import loops_cases as lc

pytestmark = pytest.mark.gpu


def _up(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _valid_dev(engine, valid):
    return _up(engine, np.asarray(valid, np.uint64).view(np.int64))


def _search(engine, u, valid, **kw):
    return [t.cpu().numpy() for t in engine.loop_search(_up(engine, u), _valid_dev(engine, valid), **kw)]


@pytest.mark.parametrize("name", sorted(lc.descriptor_batches()))
def test_descriptor_equals_the_host_twin_byte_for_byte(engine, name):
    pts, n_pts = lc.descriptor_batches()[name]
    sc, u, valid = (t.cpu().numpy() for t in engine.scan_context(_up(engine, pts), _up(engine, n_pts)))
    sc_h, u_h, valid_h = lc.host_scan_context(pts, n_pts)
    assert sc.tobytes() == sc_h.tobytes() and u.tobytes() == u_h.tobytes() and valid.tobytes() == valid_h.tobytes(), name
    if name.startswith("crafted"):
        assert sc[0].tobytes() == lc.crafted_expected().tobytes()


@pytest.mark.parametrize("name", sorted(lc.search_cases()))
def test_search_equals_the_host_twin_byte_for_byte(engine, name):
    u, valid, _, _, kw = lc.search_cases()[name]
    got = _search(engine, u, valid, dense=True, **kw)
    want = lc.host_loop_search(u, valid, dense=True, **kw)
    for what, a, b in zip(("cand", "dist", "shift", "dense dist", "dense shift"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, what)
    plain = _search(engine, u, valid, **kw)                              # without the dense images: the same k best
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, want[:3])), name


def test_ties_and_the_query_range(engine):
    for make, kw in ((lc.identical_frames, dict(min_gap=1, k=4)), (lc.period_30, dict(min_gap=1, k=1))):
        u, valid, _, _ = make()
        got, want = _search(engine, u, valid, dense=True, **kw), lc.host_loop_search(u, valid, dense=True, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), make.__name__
    _, u, valid, _, _ = lc.search_images()
    full = lc.host_loop_search(u, valid, min_gap=3, k=4, dense=True)
    for q0, q1 in ((20, 37), (0, 16), (69, 70), (33, 33)):
        part = _search(engine, u, valid, min_gap=3, k=4, dense=True, queries=(q0, q1))
        assert all(a[q0:q1].tobytes() == b.tobytes() for a, b in zip(full, part)), (q0, q1)


def test_same_bytes_on_every_run_and_nothing_outside_the_outputs(engine):
    """Two calls on the same input give identical bytes (no atomic decides a result; the bins' maxima do not depend on the order), the
    workspaces need no initialisation, and the entry points leave what lies behind their outputs as they found it."""
    pts, n_pts = lc.descriptor_batches()["one empty of three"]
    dpts, dn = _up(engine, pts), _up(engine, n_pts)
    a = [t.cpu().numpy().tobytes() for t in engine.scan_context(dpts, dn)]
    b = [t.cpu().numpy().tobytes() for t in engine.scan_context(dpts, dn)]
    assert a == b
    lib, ptr = engine.lib, lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    f = len(pts)
    sc = torch.full((f + 1, 1200), 7.0, dtype=torch.float32, device=engine.device)
    u = torch.full((f + 1, 1200), 7.0, dtype=torch.float32, device=engine.device)
    valid = torch.full((f + 1,), -7, dtype=torch.int64, device=engine.device)
    ws = torch.full((int(lib.caelo_sc_ws_bytes(f)),), 0xA5, dtype=torch.uint8, device=engine.device)
    assert lib.caelo_scan_context(engine.ctx, ptr(dpts), pts.shape[1], pts.shape[2], ptr(dn), f, ptr(sc), ptr(u), ptr(valid), ptr(ws), engine.stream) == 0
    assert sc[:f].cpu().numpy().tobytes() == a[0] and u[:f].cpu().numpy().tobytes() == a[1] and valid[:f].cpu().numpy().tobytes() == a[2]
    assert bool((sc[f] == 7.0).all()) and bool((u[f] == 7.0).all()) and int(valid[f]) == -7

    _, uu, vv, _, _ = lc.search_images()
    du, dv = _up(engine, uu), _valid_dev(engine, vv)
    n, k, q0, q1 = len(uu), 3, 5, 70
    first = [t.cpu().numpy().tobytes() for t in engine.loop_search(du, dv, min_gap=3, k=k, queries=(q0, q1), dense=True)]
    again = [t.cpu().numpy().tobytes() for t in engine.loop_search(du, dv, min_gap=3, k=k, queries=(q0, q1), dense=True)]
    assert first == again
    nq = q1 - q0
    cand = torch.full((nq + 1, k), -7, dtype=torch.int32, device=engine.device)
    dist = torch.full((nq + 1, k), -7.0, dtype=torch.float32, device=engine.device)
    shift = torch.full((nq + 1, k), -7, dtype=torch.int32, device=engine.device)
    dd = torch.full((nq + 1, n), -7.0, dtype=torch.float32, device=engine.device)
    ds = torch.full((nq + 1, n), -7, dtype=torch.int8, device=engine.device)
    ws = torch.full((int(lib.caelo_loop_search_ws_bytes(n, q0, q1, 3, k)),), 0xA5, dtype=torch.uint8, device=engine.device)
    assert lib.caelo_loop_search(engine.ctx, ptr(du), ptr(dv), n, q0, q1, 3, k, float("inf"), 1, ptr(cand), ptr(dist), ptr(shift), ptr(dd), ptr(ds),
                                 ptr(ws), engine.stream) == 0
    for t, want in zip((cand, dist, shift, dd, ds), first):
        assert t[:nq].cpu().numpy().tobytes() == want
        assert bool((t[nq] == -7).all())
