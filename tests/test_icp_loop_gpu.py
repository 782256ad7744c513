"""The device-resident ICP loops (csrc/icp.hip: k_icp_nn2, k_icp_update, caelo_icp; k_icp_nn, k_icp_fit_apply, caelo_icp_step) iteration by iteration
against the oracle's loops on the crafted clouds of tests/icp_clouds.py, and against what the reference itself returned
on them (tests/golden/icp_loop.npz).

No distance of these clouds comes within 1e-4 m of a gate in the oracle's runs (tests/test_icp_loop_host.py asserts it), so
the device has to select the same pairs: counts, iteration counts, success flags and thresholds are compared with ==.
What is left for R_star / T_star and for the moved clouds is float32 rounding -- NumPy's float32 SolveRT against the
device's float64 fit, sgemm against explicit multiplies and adds in the move.  BARS holds, per case, four times the worst
absolute difference measured on an MI355X (profiles/icp_loop_errors.txt), never above the 1e-4 (R) and 5e-4 (T) of the
older ICP tests; a wrong pair set, a dropped move or a wrong branch moves these numbers by orders of magnitude."""
import os

import numpy as np
import pytest

import icp_clouds

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# case -> bars on |R_star - oracle|, |T_star - oracle| and |moved cloud - (R_star input + T_star)|, all absolute: 4 x the
# figures of profiles/icp_loop_errors.txt
BARS = {
    "points": (1.43e-06, 1.47e-06, 1.37e-05),
    "points_102": (5.00e-06, 8.01e-06, 1.21e-05),
    "late_fail": (4.71e-07, 2.31e-06, 1.61e-05),
    "planar": (6.65e-07, 5.27e-06, 2.83e-05),
    "planar_late_stop": (3.45e-07, 1.81e-06, 1.64e-05),
    "planar_103": (4.30e-06, 4.06e-05, 5.82e-05),
    "gates": (1.53e-07, 9.09e-07, 5.29e-06),
    "shapes": (3.14e-07, 1.85e-06, 6.56e-06),
    "step": (1.06e-07, 6.26e-07, 5.35e-06),
}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (case, kind), v in sorted(WORST.items()):
        print("icp_loop_errors %-18s %-5s worst %.3e  bar %.3e" % (case, kind, v, BARS[case]["R T move".split().index(kind)]))


@pytest.fixture(scope="module")
def oracle_runs(orc):
    cache = {}

    def get(name, **over):
        key = (name, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = icp_clouds.run_oracle(orc, name, **over)
        return cache[key]
    return get


def _within(case, kind, got, want):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    WORST[(case, kind)] = max(WORST.get((case, kind), 0.0), err)
    bar = BARS[case]["R T move".split().index(kind)]
    assert err <= bar, "%s %s: %.3e above %.3e" % (case, kind, err, bar)


def _run(engine, arrays, **kw):
    """Engine.icp on copies of the arrays -> (caelo_icp_result, the arrays as the device left them)."""
    import torch
    dev = [torch.from_numpy(np.array(a)).to(engine.device) for a in arrays]
    r = engine.icp_result(engine.icp(*dev, **kw))
    return r, [t.cpu().numpy() for t in dev]


def _pose(r):
    return np.array(r.R_star, np.float64).reshape(3, 3), np.array(r.T_star, np.float64)


def _check_state(case, r, step, planar):
    """The loop's state against one record of the oracle's ``steps``."""
    got = (r.iterations, r.success, r.n_inliers_pts, r.n_inliers_planar if planar else 0, r.threshold0, r.threshold1 if planar else 0.0)
    want = (step["iterations"], int(step["success"]), step["n_pts"], step["n_planar"], step["thr0"], step["thr1"])
    assert got == want, (case, got, want)
    R, T = _pose(r)
    _within(case, "R", R, step["R_star"])
    _within(case, "T", T, step["T_star"])


def _check_move(case, r, arrays, moved):
    """pc1 (and planar1's xyz) = R_star input + T_star evaluated in float64; planar1's normals and frame 0 untouched."""
    R, T = _pose(r)
    for i in range(1, len(arrays), 2):
        _within(case, "move", moved[i][:, 0:3], arrays[i][:, 0:3].astype(np.float64) @ R.T + T)
        assert moved[i][:, 3:].tobytes() == arrays[i][:, 3:].tobytes()
        assert moved[i - 1].tobytes() == arrays[i - 1].tobytes()


@pytest.mark.parametrize("name", ["points", "planar", "late_fail"])
def test_state_after_every_iteration(engine, oracle_runs, name):
    """caelo_icp with max_iter = k leaves exactly the state after k iterations: every k up to the oracle's last iteration,
    the one that finds too few pairs included (there nothing moves: the clouds equal those of the iteration before)."""
    steps = oracle_runs(name)[3]
    arrays = icp_clouds.clouds(name)
    planar = len(arrays) == 4
    before = None
    for k in range(1, len(steps) + 1):
        r, moved = _run(engine, arrays, **icp_clouds.device_kw(name, maxIterTimes=k))
        _check_state(name, r, steps[k - 1], planar)
        _check_move(name, r, arrays, moved)
        if not steps[k - 1]["moved"]:
            assert k > 1 and all(a.tobytes() == b.tobytes() for a, b in zip(moved, before))
        before = moved
    assert name != "late_fail" or not steps[-1]["moved"]


@pytest.mark.parametrize("name", ["points", "planar", "late_fail", "planar_late_stop"])
def test_loop_stops_where_the_oracle_stops(engine, oracle_runs, name):
    """max_iter = 50: convergence at min_iter + 1 iterations, or too few pairs late in the loop -- a failure that keeps
    R_star in ICP, a success in ICP_Pt2PtAndPt2Plane."""
    R, T, ok, steps = oracle_runs(name)
    assert len(steps) < 50
    arrays = icp_clouds.clouds(name)
    r, moved = _run(engine, arrays, **icp_clouds.device_kw(name))
    _check_state(name, r, steps[-1], len(arrays) == 4)
    _check_move(name, r, arrays, moved)
    assert bool(r.success) == ok
    if name == "late_fail":
        assert r.success == 0 and np.abs(_pose(r)[0] - np.eye(3)).max() > 1e-3
    if name == "planar_late_stop":
        assert r.success == 1 and 1 <= r.iterations == steps[-1]["iterations"] and not steps[-1]["moved"]
        short, moved_short = _run(engine, arrays, **icp_clouds.device_kw(name, maxIterTimes=r.iterations))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(moved, moved_short))


def test_min_iter_and_max_iter(engine, oracle_runs):
    """min_iter other than 19: the stop rule applies from iteration min_iter on, not one later.  max_iter below the
    converging iteration: the loop ends there, moved and decayed."""
    arrays = icp_clouds.clouds("points")
    steps = oracle_runs("points", minIterTimes=3)[3]
    assert 4 <= len(steps) < 19
    r, moved = _run(engine, arrays, **icp_clouds.device_kw("points", minIterTimes=3))
    _check_state("points", r, steps[-1], False)
    _check_move("points", r, arrays, moved)
    steps = oracle_runs("points", maxIterTimes=7)[3]
    assert len(steps) == 7 and steps[-1]["thr0"] < 0.5
    r, moved = _run(engine, arrays, **icp_clouds.device_kw("points", maxIterTimes=7))
    _check_state("points", r, steps[-1], False)
    _check_move("points", r, arrays, moved)


@pytest.mark.parametrize("name", ["planar_103", "points_102"])
def test_past_iteration_100_vs_reference(engine, oracle_runs, name):
    """MyICP.py:147-153: from iteration 100 on ICP_Pt2PtAndPt2Plane fits the planar pairs of iteration 99 again and again --
    the count it prints stays that of iteration 99, the point pairs are still counted.  MyICP.ICP has no such branch.
    Against the reference's own result; a loop that goes on fitting fresh pairs misses T_star by centimetres."""
    g = np.load(os.path.join(GOLDEN, "icp_loop.npz"))
    arrays = icp_clouds.clouds(name)
    assert [icp_clouds.sha(a) for a in arrays] == g[name + "_sha256"].tolist()
    planar = len(arrays) == 4
    r, moved = _run(engine, arrays, **icp_clouds.device_kw(name))
    assert (r.iterations, r.success) == (int(g[name + "_moves"]), int(g[name + "_success"])) and r.iterations > 100
    assert [r.n_inliers_pts, r.n_inliers_planar if planar else 0] == g[name + "_counts"].tolist()
    R, T = _pose(r)
    _within(name, "R", R, g[name + "_R_star"])
    _within(name, "T", T, g[name + "_T_star"])
    _check_move(name, r, arrays, moved)
    _check_state(name, r, oracle_runs(name)[3][-1], planar)
    # ... and iteration by iteration across the branch
    steps = oracle_runs(name)[3]
    for k in (99, 100, 101):
        r, moved = _run(engine, arrays, **icp_clouds.device_kw(name, maxIterTimes=k))
        _check_state(name, r, steps[k - 1], planar)


def test_pairs_exactly_on_a_gate(engine, orc):
    """Every gate is a strict <: a point exactly 0.5 m from its neighbour, a planar point whose neighbour is exactly 5.0 m
    away and a planar pair whose pedal distance is exactly 0.5 are out; their twins one float32 step inside are in."""
    arrays = icp_clouds.gate_clouds()[:4]
    steps = []
    orc.ICP_Pt2PtAndPt2Plane(*arrays, steps=steps, **dict(icp_clouds.loop_kw("planar"), maxIterTimes=1))
    assert steps[0]["margin"] == 0.0
    r, moved = _run(engine, arrays, **icp_clouds.device_kw("planar", maxIterTimes=1))
    _check_state("gates", r, steps[0], True)
    _check_move("gates", r, arrays, moved)


@pytest.mark.parametrize("n0", icp_clouds.SHAPE_N0)
def test_tile_and_block_edges(engine, orc, n0):
    """n0 around the 1024-point tile of k_icp_nn2 x n1 around its 256-thread block, one iteration: the neighbours include
    the last point of the first tile, the first of the second and the last of all."""
    for n1 in icp_clouds.SHAPE_N1:
        pc0, pc1, src = icp_clouds.shape_clouds(n0, n1)
        d, idx = orc.nearest_neighbours(pc0, pc1)
        assert {i for i in (1023, 1024, n0 - 1) if i < n0} <= set(idx.tolist()) and (d < 0.5).all()
        R, T, _ = orc.SolveRT(pc0[idx], pc1)
        r, moved = _run(engine, (pc0, pc1), threshold0=0.5, max_iter=1, min_pairs=4)
        assert (r.iterations, r.success, r.n_inliers_pts) == (1, 1, n1), (n0, n1)
        _within("shapes", "R", _pose(r)[0], R)
        _within("shapes", "T", _pose(r)[1], T.ravel())
        _check_move("shapes", r, (pc0, pc1), moved)


def test_workspace_reuse_after_an_early_end(engine):
    """One engine, one workspace: a run that failed early, a full run, a run past iteration 100 (which leaves its stale
    sums in the state record), the full run again -- both full runs byte for byte."""
    def run(name):
        r, moved = _run(engine, icp_clouds.clouds(name), **icp_clouds.device_kw(name))
        return bytes(r) + b"".join(m.tobytes() for m in moved), r
    assert run("late_fail")[1].success == 0
    first, r = run("points")
    assert r.success == 1 and r.iterations == 20
    assert run("planar_103")[1].iterations == 103
    assert run("points")[0] == first


def test_icp_step_vs_one_oracle_iteration(engine, oracle_runs):
    """caelo_icp_step on the point cloud: pair count, (R | T) and the moved pc1 against the oracle's first iteration."""
    import torch
    step = oracle_runs("points", maxIterTimes=1)[3][0]
    pc0, pc1 = icp_clouds.clouds("points")
    d1 = torch.from_numpy(pc1.copy()).to(engine.device)
    rt, n_in = engine.icp_step(torch.from_numpy(pc0).to(engine.device), d1, 0.5)
    rt = rt.cpu().numpy().astype(np.float64)
    assert int(n_in.item()) == step["n_pts"]
    _within("step", "R", rt[:9].reshape(3, 3), step["R_star"])
    _within("step", "T", rt[9:], step["T_star"])
    _within("step", "move", d1.cpu().numpy(), pc1.astype(np.float64) @ rt[:9].reshape(3, 3).T + rt[9:])


@pytest.mark.parametrize("case", ["points", "edges"])
def test_icp_step_is_the_loops_first_iteration(engine, case):
    """Without planar points caelo_icp with max_iter = 1 and caelo_icp_step are the same computation -- one walk, one fit, one
    move (icp_nn_walk; RigidSums, rigid_from_sums, rigid_move of csrc/caelo_rigid.h) -- so pose, pair count and the moved
    cloud agree exactly: the loop multiplies the step's float32 pose into the identity in float64, which is exact.  On the
    `points` clouds and on those of test_tile_and_block_edges with n0 one past the LDS tile and n1 one past a workgroup."""
    import torch
    pc0, pc1 = icp_clouds.clouds("points") if case == "points" else icp_clouds.shape_clouds(1025, 257)[:2]
    least = 100 if case == "points" else 4
    r, moved = _run(engine, (pc0, pc1), threshold0=0.5, max_iter=1, min_pairs=least)
    d1 = torch.from_numpy(pc1.copy()).to(engine.device)
    rt, n_in = engine.icp_step(torch.from_numpy(pc0).to(engine.device), d1, 0.5, min_inliers=least)
    rt = rt.cpu().numpy()
    assert (r.iterations, r.success) == (1, 1) and int(n_in.item()) >= least
    assert (np.array(r.R_star) == rt[:9].astype(np.float64)).all()
    assert (np.array(r.T_star) == rt[9:12].astype(np.float64)).all()
    assert r.n_inliers_pts == int(n_in.item())
    assert moved[1].tobytes() == d1.cpu().numpy().tobytes() and moved[1].tobytes() != pc1.tobytes()
