"""detect_loops.py end to end on the device (caelo.loops): the 16-frame synthetic revisit sequence of tests/loops_seq.py --
frame 8 + k revisits frame k at a heading 0.7 k + 0.3 rad away.  Exactly the 8 loops are reported, each with the shift of its yaw,
all verified inside the reference's success bounds (RRE < 1 degree, RTE < 0.5 m as sums of absolute components,
EvaluationOnRegistration.py:22-23) after the turn to frame j's heading; evaluate.py loops reports recall 1 and precision 1; frame j's rows
from a features directory, and the search alone, give the same answers.

Measured on the CPU with the host twins (min_gap 4): the revisits are the best candidates at distances 0.207 - 0.331, the nearest
impostor over all queries lies at 0.576; the shifts are 3, 10, 16, 23, 30, 36, 43, 50."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import loops_seq as ls

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "cae-lo_amd") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

pytestmark = pytest.mark.gpu
COMMON = ["--min-gap", "4", "--max-dist", "0.45"]


@pytest.fixture(scope="module")
def detected(engine, tmp_path_factory):
    """-> (folder, loops file, rows) of the plain run"""
    import detect_loops
    folder = tmp_path_factory.mktemp("loops")
    out = str(folder / "loops.txt")
    rows = detect_loops.run(COMMON + ["--out", out], scans=ls.scans())
    return folder, out, rows


def test_exactly_the_eight_loops_with_their_shifts(detected):
    _, out, rows = detected
    from caelo import loops as lp
    back = lp.read_loops(out)
    assert back.shape == (ls.N_LOOPS, lp.LOOP_COLUMNS) and np.array_equal(back[:, 0:2], rows[:, 0:2])
    assert back[:, 0].tolist() == list(range(8, 16)) and back[:, 1].tolist() == list(range(8))
    for i, _, d, s in back[:, 0:4]:
        off = (s * 6.0 - math.degrees(ls.yaw_of(int(i))) + 180.0) % 360.0 - 180.0
        print("loop %2d: distance %.4f shift %2d (yaw %.2f deg, off by %+.2f deg)" % (i, d, s, math.degrees(ls.yaw_of(int(i))), off))
        assert abs(off) <= 6.0 and 0.0 < d < 0.45


def test_all_loops_verify_inside_the_success_bounds(detected):
    folder, out, rows = detected
    import evaluate as ev_cli
    from caelo import evaluate as ev
    from caelo import loops as lp
    gt, calib = ls.write_ground_truth(folder)
    res = ev.loops(np.loadtxt(gt), ev.read_tr(calib), lp.read_loops(out), revisit_radius=4.0, min_gap=4)
    for k in range(len(res["RRE"])):
        print("loop %2d: %4d inliers at %.1f m, RRE %.4f deg, RTE %.4f m" % (rows[k, 0], rows[k, 5], rows[k, 6], res["RRE"][k], res["RTE"][k]))
    assert (rows[:, 4] == 1).all() and res["n_verified"] == ls.N_LOOPS
    assert (res["RRE"] < 1.0).all() and (res["RTE"] < 0.5).all() and res["success"].all()
    assert res["n_revisit_queries"] == ls.N_LOOPS and res["recall"] == 1.0 and res["precision"] == 1.0 and res["precision_verified"] == 1.0
    for k, (i, j) in enumerate(rows[:, 0:2].astype(int)):                # the reported motion maps frame i into frame j
        R, T = ls.true_motion(i, j)
        assert np.abs(rows[k, 7:16].reshape(3, 3) - R).max() < 0.02 and np.abs(rows[k, 16:19] - T).max() < 0.5


def test_evaluate_cli_reports_recall_and_precision_one(detected, capsys):
    folder, out, _ = detected
    import evaluate as ev_cli
    gt, calib = ls.write_ground_truth(folder)
    assert ev_cli.main(["loops", "--gt", gt, "--calib", calib, "--loops", out, "--revisit-radius", "4", "--min-gap", "4"]) == 0
    text = capsys.readouterr().out
    assert "recall 1  precision 1  precision of verified 1" in text and "success 8 of 8" in text


def test_features_from_and_no_verify_give_the_same_answers(engine, detected):
    folder, out, rows = detected
    import detect_loops
    from caelo import keysources
    for f in range(ls.N_LOOPS):                                          # frame j's artefacts, as run_sequence.py --save-artifacts leaves them
        ff = engine.extract(torch.from_numpy(ls.scans()[f]).to(engine.device))
        k = int(ff.n_key.item())
        keysources.save_features(str(folder / "velodyne" / ("%06d.bin" % f)), ff.key_pts[:k].cpu().numpy(), ff.features[:k].cpu().numpy())
    other = str(folder / "loops_from_features.txt")
    detect_loops.run(COMMON + ["--features-from", str(folder / "Features"), "--out", other], scans=ls.scans())
    assert open(other, "rb").read() == open(out, "rb").read()
    plain = str(folder / "loops_no_verify.txt")
    cands = detect_loops.run(COMMON + ["--no-verify", "--out", plain], scans=ls.scans())
    assert np.array_equal(cands[:, 0:4], rows[:, 0:4]) and not cands[:, 4:7].any()
    assert np.array_equal(np.loadtxt(plain)[:, 0:4], np.loadtxt(out)[:, 0:4])
