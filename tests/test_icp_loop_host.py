"""The oracle's ICP loops (oracle.ICP, oracle.ICP_Pt2PtAndPt2Plane) on the crafted clouds of tests/icp_clouds.py against
what the reference's own loops returned on them (tests/golden/icp_loop.npz, written by tools/make_goldens.py), and the
conditions that the GPU tests of tests/test_icp_loop_gpu.py rest on.  No GPU."""
import json
import os

import numpy as np
import pytest

import icp_clouds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(icp_clouds.CASES)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "icp_loop.npz"))


@pytest.fixture(scope="module")
def runs(orc):
    return {name: icp_clouds.run_oracle(orc, name) for name in CASES}


def test_golden_covers_the_cases(golden):
    assert sorted(golden["cases"].tolist()) == CASES
    for name in CASES:
        assert json.loads(str(golden[name + "_kw"])) == icp_clouds.loop_kw(name)


@pytest.mark.parametrize("name", CASES)
def test_generator_reproduces_the_hashed_inputs(golden, name):
    arrays = icp_clouds.clouds(name)
    assert [icp_clouds.sha(a) for a in arrays] == golden[name + "_sha256"].tolist()
    for a in arrays:
        assert a.dtype == np.float32 and a.flags.c_contiguous and np.abs(a[:, 0:3]).max() <= 16.0
    assert arrays[0].shape == (1300, 3)           # one full 1024-point tile of the device's neighbour search plus 276
    for a in arrays[2:]:
        assert np.abs(np.linalg.norm(a[:, 3:6].astype(np.float64), axis=1) - 1.0).max() < 1e-6


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference(golden, runs, name):
    """The iteration count and what the reference printed with ==; R_star / T_star within a float32 budget.

    tools/make_goldens.py asserts R to 1e-7 and T to 1e-6 where oracle and reference share one NumPy.  Here the NumPy may be
    another: every iteration rounds its (R, T) to float32 afresh (SVD, sgemm), and two LAPACK / BLAS builds may differ in
    the last bit of each.  With the same pairs (test_no_distance_near_a_gate) nothing else differs, and without counting
    on the loop to contract the differences add up: one float32 ulp of 1.0 per iteration for R, twice that for T (R's
    error on a lever arm of up to 2 m, the centroids' distance from the origin, plus T's own rounding)."""
    R, T, ok, steps = runs[name]
    last = steps[-1]
    assert ok == bool(golden[name + "_success"])
    assert len(steps) == int(golden[name + "_iters"]) and last["iterations"] == int(golden[name + "_moves"])
    assert [last["n_pts"], last["n_planar"]] == golden[name + "_counts"].tolist()
    assert [round(last["thr0"], 5), round(last["thr1"], 5)] == golden[name + "_thr"].tolist()
    ulp = len(steps) * 2.0 ** -23
    assert np.abs(R - golden[name + "_R_star"]).max() <= ulp and np.abs(T.ravel() - golden[name + "_T_star"]).max() <= 2 * ulp
    assert np.array_equal(last["R_star"], R) and np.array_equal(last["T_star"], T.ravel())


@pytest.mark.parametrize("name", CASES)
def test_no_distance_near_a_gate(runs, name):
    """The condition under which pair counts may be compared with ==: in every iteration every distance is at least
    GATE_MARGIN from the threshold it is compared with."""
    margins = [s["margin"] for s in runs[name][3]]
    assert min(margins) >= icp_clouds.GATE_MARGIN, (int(np.argmin(margins)), min(margins))


def test_cases_take_the_paths_they_are_built_for(runs):
    pts = [s["n_pts"] for s in runs["points"][3]]
    assert runs["points"][2] and len(pts) == 20 and len(set(pts)) >= 4 and pts[-1] == 300    # every decay and both displaced groups matter
    assert np.abs(runs["points"][1].ravel() - np.array(icp_clouds.MOTION_T)).max() < 1e-4    # ... and the loop finds the motion
    R, T, ok, steps = runs["late_fail"]
    assert not ok and steps[-1]["iterations"] >= 10 and not steps[-1]["moved"] and steps[-1]["n_pts"] < 100
    assert np.abs(R - np.eye(3)).max() > 1e-3                                                # R_star so far is kept
    R, T, ok, steps = runs["planar"]
    assert ok and len(steps) == 20 and steps[-1]["n_planar"] == 390
    R, T, ok, steps = runs["planar_late_stop"]
    assert ok and steps[-1]["iterations"] >= 1 and not steps[-1]["moved"] and steps[-1]["n_pts"] + steps[-1]["n_planar"] < 200
    assert runs["points_102"][2] and [s["n_pts"] for s in runs["points_102"][3][1:]] == [540] * 101
    steps = runs["planar_103"][3]
    assert len(steps) == 103 and all(s["moved"] for s in steps)
    # from iteration 100 on the same (R, T) is applied: T_star - R T_star' is constant, and the planar count is stale
    d = [np.linalg.norm(steps[k]["T_star"] - steps[k - 1]["T_star"]) for k in (100, 101, 102)]
    assert max(d) - min(d) < 1e-6 and min(d) > 1e-5


def test_iteration_100_branch_is_observable(orc, golden):
    """After 100 joint fits the loop is at rest (a further joint fit moves the pose by micrometres), while the three stale
    fits of MyICP.py:151-153 that the reference does instead carry it centimetres away: a loop without that branch
    cannot pass the 103-iteration case."""
    arrays = icp_clouds.clouds("planar_103")
    kw = dict(icp_clouds.loop_kw("planar_103"), maxIterTimes=100)
    steps = []
    R, T, ok = orc.ICP_Pt2PtAndPt2Plane(*arrays, steps=steps, **kw)
    assert np.abs(steps[-1]["T_star"] - steps[-2]["T_star"]).max() < 1e-4
    assert np.abs(T.ravel() - golden["planar_103_T_star"]).max() > 5e-3


def test_gate_clouds_sit_on_the_gates(orc):
    pc0, pc1, planar0, planar1, extra = icp_clouds.gate_clouds()
    base = icp_clouds.clouds("planar")
    kw = dict(icp_clouds.loop_kw("planar"), maxIterTimes=1)
    a, b = [], []
    orc.ICP_Pt2PtAndPt2Plane(pc0, pc1, planar0, planar1, steps=a, **kw)
    orc.ICP_Pt2PtAndPt2Plane(*base, steps=b, **kw)
    assert (a[0]["n_pts"] - b[0]["n_pts"], a[0]["n_planar"] - b[0]["n_planar"]) == extra
    assert a[0]["margin"] == 0.0                              # some pair is exactly on its gate
    d, _ = orc.nearest_neighbours(pc0, pc1[-2:])
    assert d[0] == 0.5 and 0.5 - 1e-6 < d[1] < 0.5
    d, i = orc.nearest_neighbours(planar0[:, 0:3], planar1[-4:, 0:3])
    assert d[0] == 5.0 and 5.0 - 1e-6 < d[1] < 5.0 and i.tolist() == list(range(len(planar0) - 4, len(planar0)))
    assert d[2] == 0.5 and 0.5 - 1e-6 < d[3] < 0.5            # along the normal: these are the pedal distances


@pytest.mark.parametrize("n0", icp_clouds.SHAPE_N0)
@pytest.mark.parametrize("n1", icp_clouds.SHAPE_N1)
def test_shape_clouds_reach_the_tile_edges(orc, n0, n1):
    pc0, pc1, src = icp_clouds.shape_clouds(n0, n1)
    assert pc0.shape == (n0, 3) and pc1.shape == (n1, 3)
    d, idx = orc.nearest_neighbours(pc0, pc1)
    assert np.array_equal(idx, src) and d.max() < 0.5 - icp_clouds.GATE_MARGIN
    assert {i for i in (1023, 1024, n0 - 1) if i < n0} <= set(idx.tolist())
