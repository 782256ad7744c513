"""caelo.correct.correct_pc_host -- the float32 restatement of the reference's CorrectPC in the device's order -- against
tests/golden/correct_pc.npz, which the reference's own Transformations.CorrectPC wrote (tools/make_goldens_correct_pc.py), and the
argument checks of api.CorrectPC.  No GPU."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

from caelo import correct  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "correct_pc.npz")
ANGLES = [0.22, 0.205, -0.3, 0.0, 45.0]


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_golden_file_is_what_the_issue_describes(g):
    pts = g["points"]
    assert pts.shape == (4096, 3) and pts.dtype == np.float32 and g["angles"].tolist() == ANGLES
    assert g["out"].shape == (5, 4096, 3) and g["out"].dtype == np.float32
    assert g["R"].shape == (5, 256, 3, 3) and g["R"].dtype == np.float32 and g["R_index"].shape == (256,)
    assert int(str(g["numpy_version"]).split(".")[0]) >= 2            # the NEP 50 arithmetic is the contract
    x, y, z = pts.T
    axis = (x == 0) & (y == 0)
    assert axis.sum() >= 9 and ((x == 0) & (y == 0) & (z == 0)).any()  # >= 8 points on the z axis and the origin
    assert ((x == 0) & (y != 0)).any() and ((y == 0) & (x != 0)).any() and (z < 0).any() and ((z == 0) & ~axis).any()
    assert np.abs(pts).max() <= 120.0 and np.abs(pts).max() > 119.0
    assert np.array_equal(pts, (np.round(pts.astype(np.float64) * 1000) / 1000).astype(np.float32))   # mm-quantised
    r2 = x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2
    assert ((r2 == 0) | (np.maximum(np.abs(x), np.abs(y)) >= 2.0 ** -60)).all()
    assert np.isin(np.flatnonzero(axis), g["R_index"]).all()          # the subset holds every axis point


@pytest.mark.parametrize("ai", range(5))
def test_host_restatement_against_the_reference(g, ai):
    """R: the reference's bits on the subset.  NaN exactly where the golden has it -- the axis points and the origin, at every angle,
    0 included.  Elsewhere |out - golden| <= 6 * 2^-24 * (|x| + |y| + |z|) per component: gamma_3 for each of the two summation orders
    of a 3-term dot product with |R_ij| <= 1 (the reference's last step is its BLAS's sgemv, the restatement's is (R_i0 x + R_i1 y) +
    R_i2 z).  Largest observed ratio to that bound: 0.16, 0.10, 0.16, 0 and 0.29 for the five angles."""
    pts, angle = g["points"], float(g["angles"][ai])
    R = correct.rotation_matrices(pts, angle)[g["R_index"]]
    want_R = g["R"][ai]
    nan_R = np.isnan(want_R)
    assert np.array_equal(np.isnan(R), nan_R)
    assert np.array_equal(bits(R)[~nan_R], bits(want_R)[~nan_R]), "%d matrix entries differ" % int((bits(R)[~nan_R] != bits(want_R)[~nan_R]).sum())
    out, want = correct.correct_pc_host(pts, angle), g["out"][ai]
    assert out.dtype == np.float32 and out.shape == want.shape
    axis = (pts[:, 0] == 0) & (pts[:, 1] == 0)
    assert np.array_equal(np.isnan(want), np.repeat(axis[:, None], 3, axis=1))
    assert np.array_equal(np.isnan(out), np.isnan(want))
    ok = ~axis
    bound = 6 * 2.0 ** -24 * np.abs(pts[ok].astype(np.float64)).sum(axis=1, keepdims=True)
    d = np.abs(out[ok].astype(np.float64) - want[ok].astype(np.float64))
    print("angle %g: largest |out - golden| / bound = %.3f (%.1f %% of the values differ, by at most %.3g)"
          % (angle, (d / bound).max(), 100.0 * (d > 0).mean(), d.max()))
    assert (d <= bound).all()


def test_angle_zero_returns_the_input_bits(g):
    """Angle 0: R is the identity and every non-axis point comes back with its own bits -- and with the reference's, whose golden
    output at angle 0 this equals bit for bit.  One IEEE fact sits in between: a coordinate that is -0.0 (five of the golden's) comes
    back +0.0, from the reference too, because (1 * -0 + 0 * y) + 0 * z = +0."""
    pts = g["points"]
    out = correct.correct_pc_host(pts, 0.0)
    ok = ~((pts[:, 0] == 0) & (pts[:, 1] == 0))
    assert np.array_equal(bits(out[ok]), bits(g["out"][3][ok]))
    assert np.array_equal(out[ok], pts[ok])
    neg_zero = bits(pts) == 0x80000000
    assert np.array_equal(bits(out)[ok[:, None] & ~neg_zero], bits(pts)[ok[:, None] & ~neg_zero])
    assert (bits(out)[ok[:, None] & neg_zero] == 0).all() and (ok[:, None] & neg_zero).sum() == 5
    assert np.isnan(out[~ok]).all()


def test_fourth_column_and_input_are_kept(g):
    pts = g["points"][:300]
    inten = np.arange(300, dtype=np.uint32) * np.uint32(0x01F35A7B) + np.uint32(0x7FC00001)   # arbitrary bits, NaN patterns among them
    pc = np.concatenate([pts, inten.view(np.float32)[:, None]], axis=1)
    before = pc.copy()
    out = correct.correct_pc_host(pc, 0.22)
    assert out.shape == (300, 4) and np.array_equal(bits(out[:, 3]), inten)
    assert np.array_equal(bits(pc), bits(before))
    want = correct.correct_pc_host(pts, 0.22)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out[:, :3]), nan) and np.array_equal(bits(out[:, :3])[~nan], bits(want)[~nan])


def test_api_correctpc_rejects_bad_arguments():
    """Before any device work: no GPU is needed to be refused."""
    from caelo import api
    good = np.ones((5, 3), dtype=np.float32)
    for bad in (good.astype(np.float64), good.astype(np.int32), [[1.0, 2.0, 3.0]]):
        with pytest.raises(ValueError):
            api.CorrectPC(bad, 0.22)
    for bad in (np.ones((5, 4), np.float32), np.ones((5, 2), np.float32), np.ones((15,), np.float32), np.ones((5, 3, 1), np.float32)):
        with pytest.raises(ValueError):
            api.CorrectPC(bad, 0.22)
    for bad in (float("nan"), float("inf"), -float("inf"), None, "x"):
        with pytest.raises(ValueError):
            api.CorrectPC(good, bad)
        with pytest.raises(ValueError):
            correct.correct_pc_host(good, bad)
