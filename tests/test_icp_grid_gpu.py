"""caelo_icp_grid (csrc/icp.hip: k_grid_count, k_grid_scan_chunks, k_grid_scan_add, k_grid_scatter, k_icp_nn_grid) against the all-pairs
walk of caelo_icp: the grid has to return the same pairs in every iteration, so the result record and the moved clouds are compared
byte for byte, the pair arrays of the last evaluated iteration entry by entry (the index only where the mask is set: behind a zero
mask the grid cannot know the global nearest neighbour and nothing reads it), and the pair counts of every iteration with the oracle's.

Cell edges: threshold 0.5 -> 0.5 m, 1.0 -> 1.0 m, 5.0 -> 8.0 m; the cell of x is floor(x / edge)."""
import ctypes as C

import numpy as np
import pytest

import icp_clouds

pytestmark = pytest.mark.gpu


def _below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def _above(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def _run(engine, arrays, nn, **kw):
    """Engine.icp on copies -> (record bytes, record, moved arrays, idx [n1] of the point pairs, mask [n1])."""
    import torch
    dev = [torch.from_numpy(np.array(a)).to(engine.device) for a in arrays]
    r = engine.icp_result(engine.icp(*dev, nn=nn, **kw))
    n1 = arrays[1].shape[0]
    m1 = arrays[3].shape[0] if len(arrays) == 4 else 0
    ws = engine._ws("icp_grid" if nn == "grid" else "icp_loop", 0).cpu().numpy()   # state record | idx_p | idx_q | mask_p | mask_q
    idx = ws[512:512 + 8 * n1].view(np.int64).copy()
    mask = ws[512 + 8 * (n1 + m1):512 + 8 * (n1 + m1) + n1].copy()
    return bytes(r), r, [t.cpu().numpy() for t in dev], idx, mask


def _same(engine, arrays, **kw):
    """Both searches on the same input: equal bytes.  -> (record, idx, mask) of the grid's run."""
    b = _run(engine, arrays, "brute", **kw)
    g = _run(engine, arrays, "grid", **kw)
    assert g[0] == b[0], (g[1].iterations, b[1].iterations, g[1].n_inliers_pts, b[1].n_inliers_pts)
    for x, y in zip(g[2], b[2]):
        assert x.tobytes() == y.tobytes()
    assert g[4].tobytes() == b[4].tobytes()
    assert (g[3][g[4] == 1] == b[3][b[4] == 1]).all()
    return g[1], g[3], g[4]


@pytest.fixture(scope="module")
def oracle_steps(orc):
    return {name: icp_clouds.run_oracle(orc, name)[3] for name in icp_clouds.CASES}


@pytest.mark.parametrize("name", sorted(icp_clouds.CASES))
def test_cases_equal_the_brute_walk_and_the_oracles_counts(engine, oracle_steps, name):
    arrays = icp_clouds.clouds(name)
    planar = len(arrays) == 4
    steps = oracle_steps[name]
    r, _, _ = _same(engine, arrays, **icp_clouds.device_kw(name))
    assert (r.iterations, int(r.success)) == (steps[-1]["iterations"], int(steps[-1]["success"]))
    for k in range(1, len(steps) + 1):   # the state after k iterations: the pairs that iteration k - 1 found
        rk = _run(engine, arrays, "grid", **icp_clouds.device_kw(name, maxIterTimes=k))[1]
        assert (rk.n_inliers_pts, rk.n_inliers_planar if planar else 0) == (steps[k - 1]["n_pts"], steps[k - 1]["n_planar"]), (name, k)
    for k in (1, 2, len(steps) // 2):
        _same(engine, arrays, **icp_clouds.device_kw(name, maxIterTimes=k))


def test_gate_clouds(engine):
    """A pair exactly on its threshold is out, its twin a float32 step inside is in (0.5 m, 5.0 m with 8 m cells: the planar twin at
    y = 16 lies across a cell face from its neighbour at y = 12)."""
    arrays = icp_clouds.gate_clouds()
    base = icp_clouds.clouds("planar")
    r, _, _ = _same(engine, arrays[:4], **icp_clouds.device_kw("planar", maxIterTimes=1))
    r0 = _run(engine, base, "grid", **icp_clouds.device_kw("planar", maxIterTimes=1))[1]
    assert (r.n_inliers_pts - r0.n_inliers_pts, r.n_inliers_planar - r0.n_inliers_planar) == arrays[4]


@pytest.mark.parametrize("n0", icp_clouds.SHAPE_N0)
def test_shapes(engine, n0):
    for n1 in icp_clouds.SHAPE_N1:
        pc0, pc1, src = icp_clouds.shape_clouds(n0, n1)
        r, idx, mask = _same(engine, (pc0, pc1), threshold0=0.5, max_iter=1, min_pairs=4)
        assert r.n_inliers_pts == n1 and mask.all() and (idx == src).all()


def _background(n0=300, n1=120):
    pc0, pc1, _ = icp_clouds.shape_clouds(n0, n1)   # inside +-10 m, every pair inside a 0.5 m gate
    return pc0, pc1


def _with(extra0, extra1):
    pc0, pc1 = _background()
    return (np.ascontiguousarray(np.r_[pc0, np.array(extra0, np.float32)]), np.ascontiguousarray(np.r_[pc1, np.array(extra1, np.float32)]),
            pc0.shape[0], pc1.shape[0])


def test_points_on_cell_faces_edges_and_corners(engine):
    """Frame-0 points exactly on a face, an edge and a corner of the 0.5 m cells (they belong to the cell above), each with its
    query in the cell diagonally below, on the positive and on the negative side of the origin."""
    extra0 = [[20.0, 20.25, 20.25], [24.0, 24.0, 24.25], [28.0, 28.0, 28.0],
              [-20.0, -20.25, -20.25], [-24.0, -24.0, -24.25], [-28.0, -28.0, -28.0]]
    extra1 = [[19.95, 19.95, 19.95], [23.9, 23.9, 23.9], [27.9, 27.9, 27.9],
              [-20.05, -20.55, -20.55], [-24.1, -24.1, -24.6], [-28.1, -28.1, -28.1]]
    pc0, pc1, b0, b1 = _with(extra0, extra1)
    c0 = np.floor(pc0[b0:].astype(np.float64) / 0.5)
    c1 = np.floor(pc1[b1:].astype(np.float64) / 0.5)
    assert (c0 - c1 == 1).all()   # diagonal neighbours in all three axes
    assert (np.linalg.norm(pc0[b0:].astype(np.float64) - pc1[b1:], axis=1) < 0.5).all()
    r, idx, mask = _same(engine, (pc0, pc1), threshold0=0.5, max_iter=1, min_pairs=4)
    assert mask[b1:].all() and (idx[b1:] == b0 + np.arange(6)).all() and r.n_inliers_pts == pc1.shape[0]
    _same(engine, (pc0, pc1), threshold0=0.5, max_iter=3, min_iter=2, min_pairs=4)


def test_neighbour_exactly_at_the_threshold_across_a_cell_face(engine):
    """Distance exactly 0.5 across the face x = 20 (out), one float32 step inside (in); the same at 1.0 with 1.0 m cells."""
    for thr in (0.5, 1.0):
        extra0 = [[20.0, 3.0, 0.0], [20.0, -3.0, 0.0], [-20.0, 3.0, 0.0], [-20.0, -3.0, 0.0]]
        extra1 = [[20.0 - thr, 3.0, 0.0], [_above(20.0 - thr), -3.0, 0.0], [-20.0 + thr, 3.0, 0.0], [_below(-20.0 + thr), -3.0, 0.0]]
        pc0, pc1, b0, b1 = _with(extra0, extra1)
        r, idx, mask = _same(engine, (pc0, pc1), threshold0=thr, max_iter=1, min_pairs=4)
        assert mask[b1:].tolist() == [0, 1, 0, 1]
        assert idx[b1 + 1] == b0 + 1 and idx[b1 + 3] == b0 + 3


def test_duplicates_and_ties_take_the_lowest_index(engine):
    """Duplicated frame-0 coordinates, and two different frame-0 points at the same distance from a query (in one cell and in two,
    the lower index in the cell that is visited later): the lowest index wins, as in the walk's strict <."""
    extra0 = [[21.0, 0.0, 0.0], [20.0, 0.0, 0.0],            # tie across two 1 m cells; index b0 has the larger x
              [30.75, 5.0, 0.0], [30.25, 5.0, 0.0],          # tie inside one cell
              [40.0, 7.0, 1.0], [40.0, 7.0, 1.0], [40.0, 7.0, 1.0],   # duplicates
              [-21.0, 0.0, 0.0], [-20.0, 0.0, 0.0]]
    extra1 = [[20.5, 0.0, 0.0], [30.5, 5.0, 0.0], [40.125, 7.0, 1.0], [-20.5, 0.0, 0.0]]
    pc0, pc1, b0, b1 = _with(extra0, extra1)
    d = np.linalg.norm(pc0[b0:, None, :].astype(np.float64) - pc1[None, b1:, :], axis=2)
    assert d[0, 0] == d[1, 0] and d[2, 1] == d[3, 1] and d[7, 3] == d[8, 3]
    r, idx, mask = _same(engine, (pc0, pc1), threshold0=1.0, max_iter=1, min_pairs=4)
    assert mask[b1:].all() and (idx[b1:] - b0).tolist() == [0, 2, 4, 7]


def test_all_points_in_one_cell(engine):
    rng = np.random.RandomState(5)
    pc0 = (20.0 + rng.uniform(0.0, 0.499, (2049, 3))).astype(np.float32)
    src = rng.permutation(2049)[:150]
    pc1 = (pc0[src] + rng.uniform(-0.002, 0.002, (150, 3))).astype(np.float32)
    assert len(np.unique(np.floor(pc0.astype(np.float64) / 0.5), axis=0)) == 1
    r, idx, mask = _same(engine, (pc0, pc1), threshold0=0.5, max_iter=2, min_iter=1, min_pairs=4)
    assert r.n_inliers_pts == 150


def test_single_row_of_cells(engine):
    rng = np.random.RandomState(6)
    pc0 = np.c_[rng.uniform(-30, 30, 700), rng.uniform(0.0, 0.499, 700), rng.uniform(-0.5, -0.001, 700)].astype(np.float32)
    src = rng.permutation(700)[:200]
    pc1 = (pc0[src] + rng.uniform(-0.004, 0.004, (200, 3))).astype(np.float32)   # some leave the row: clamped back into it
    cells = np.unique(np.floor(pc0.astype(np.float64) / 0.5)[:, 1:], axis=0)
    assert len(cells) == 1
    r, idx, mask = _same(engine, (pc0, pc1), threshold0=0.5, max_iter=2, min_iter=1, min_pairs=4)
    assert r.n_inliers_pts == 200


def test_one_query_point(engine):
    pc0, pc1 = _background()
    r, idx, mask = _same(engine, (pc0, pc1[7:8].copy()), threshold0=0.5, max_iter=2, min_iter=1, min_pairs=1)
    assert r.n_inliers_pts == 1 and r.success == 1


def test_points_far_outside_the_box(engine):
    """Frame-0 points at +-200 m stretch the extent to 800^3 cells of 0.5 m, far above the table: the box shrinks and what lies
    outside is clamped into its edge cells, where it must still be found."""
    far0 = [[200.0, 200.0, 200.0], [-200.0, -200.0, -200.0], [200.0, -200.0, 0.0], [0.25, 200.0, -200.0]]
    far1 = [[200.1, 200.1, 199.9], [-200.1, -199.9, -200.1], [199.9, -200.1, 0.1], [0.3, 199.9, -199.9], [150.0, 150.0, 150.0]]
    pc0, pc1, b0, b1 = _with(far0, far1)
    r, idx, mask = _same(engine, (pc0, pc1), threshold0=0.5, max_iter=1, min_pairs=4)
    assert mask[b1:].tolist() == [1, 1, 1, 1, 0] and (idx[b1:b1 + 4] == b0 + np.arange(4)).all()
    _same(engine, (pc0, pc1), threshold0=0.5, max_iter=3, min_iter=2, min_pairs=4)


def test_threshold_decays_below_the_next_cell_size(engine):
    """Threshold 1.0 (1 m cells) decaying every iteration to below 0.5: the grid stays the one of the first iteration."""
    arrays = icp_clouds.clouds("points")
    r, _, _ = _same(engine, arrays, threshold0=1.0, decay0=0.9, small_shift=1.0e3, ep=0.0, max_iter=10, min_iter=9, min_pairs=100)
    assert r.iterations == 10 and r.threshold0 < 0.5
    for k in (3, 7, 8):
        _same(engine, arrays, threshold0=1.0, decay0=0.9, small_shift=1.0e3, ep=0.0, max_iter=k, min_iter=9, min_pairs=100)


def test_planar_set_with_its_8_m_cells(engine):
    """The planar clouds plus planar points on a corner of the 8 m cells with queries in the diagonal cell, and the planar
    threshold decaying from 5.0."""
    pc0, pc1, planar0, planar1 = icp_clouds.clouds("planar")
    z = [0.0, 0.0, 1.0]
    planar0 = np.ascontiguousarray(np.r_[planar0, np.array([[16.0, 16.0, 16.0] + z, [-16.0, -16.0, -16.0] + z], np.float32)])
    planar1 = np.ascontiguousarray(np.r_[planar1, np.array([[15.0, 14.0, 15.75] + z, [-17.0, -18.0, -16.25] + z], np.float32)])
    kw = dict(icp_clouds.device_kw("planar"), small_shift=1.0e3, ep=0.0)
    for k in (1, 4, 12):
        r, _, _ = _same(engine, (pc0, pc1, planar0, planar1), **dict(kw, max_iter=k))
    assert r.iterations == 12 and r.threshold1 < 2.0
    r1 = _run(engine, (pc0, pc1, planar0, planar1), "grid", **dict(kw, max_iter=1))[1]
    r0 = _run(engine, icp_clouds.clouds("planar"), "grid", **dict(kw, max_iter=1))[1]
    assert r1.n_inliers_planar - r0.n_inliers_planar == 2


@pytest.mark.parametrize("what", ["decay0", "decay1", "nan_pc0", "nan_pc1", "inf_planar1"])
def test_refusals_leave_the_outputs_untouched(engine, what):
    import torch
    from caelo import _ffi
    arrays = [np.array(a) for a in icp_clouds.clouds("planar")]
    kw = icp_clouds.device_kw("planar")
    if what.startswith("decay"):
        kw[what] = 1.0 + 2.0 ** -40
    elif what == "nan_pc0":
        arrays[0][17, 1] = np.nan
    elif what == "nan_pc1":
        arrays[1][3, 2] = np.nan
    else:
        arrays[3][5, 0] = np.inf
    dev = [torch.from_numpy(a).to(engine.device) for a in arrays]
    res = torch.full((C.sizeof(_ffi.IcpResult),), 0xAB, dtype=torch.uint8, device=engine.device)
    prm = _ffi.IcpParams(use_planar=1, reserved=0, **kw)
    lay = (C.c_int64 * 8)()
    assert engine.lib.caelo_icp_grid_ws_layout(arrays[0].shape[0], arrays[1].shape[0], arrays[2].shape[0], arrays[3].shape[0], C.cast(lay, C.c_void_p)) == 0
    ws = engine._ws("icp_grid", int(lay[7]))
    rc = engine.lib.caelo_icp_grid(engine.ctx, C.c_void_p(dev[0].data_ptr()), arrays[0].shape[0], C.c_void_p(dev[1].data_ptr()), arrays[1].shape[0],
                                   C.c_void_p(dev[2].data_ptr()), arrays[2].shape[0], C.c_void_p(dev[3].data_ptr()), arrays[3].shape[0],
                                   C.byref(prm), C.c_void_p(res.data_ptr()), C.c_void_p(ws.data_ptr()), engine.stream)
    torch.cuda.synchronize()
    assert rc == -1 and engine.lib.caelo_last_error()   # CAELO_ERR_ARG
    assert (res.cpu().numpy() == 0xAB).all()
    for t, a in zip(dev, arrays):
        assert t.cpu().numpy().tobytes() == a.tobytes()
    with pytest.raises(_ffi.CaeloError):
        engine.icp(*dev, nn="grid", **kw)
    if what.startswith("decay"):   # the all-pairs walk has no such limit
        assert engine.icp_result(engine.icp(*[t.clone() for t in dev], nn="brute", **kw)).iterations >= 1
