"""CorrectPC on the device (csrc/correct.hip): the staged entry point against the host restatement (caelo/correct.py, itself pinned to
the reference by tests/test_correct_pc_host.py), the fused mode bit of caelo_extract and of the frame pipeline against the staged call,
and the two command-line tools.  "Bit for bit" below: NaN at the same positions, every other value the same 32 bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

from caelo import correct  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(REPO, "tests", "golden")
ANGLE = 0.22
GUARD = 0x5AFEC0DE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.fixture(scope="module")
def cloud():
    """4097 points [n,4]: the golden's 4096 and one more, with arbitrary bit patterns (NaNs among them) in the intensity column."""
    pts = np.load(os.path.join(GOLDEN, "correct_pc.npz"))["points"]
    pts = np.concatenate([pts, pts[17:18]], axis=0)
    inten = np.arange(pts.shape[0], dtype=np.uint32) * np.uint32(0x01F35A7B) + np.uint32(0x7FC00001)
    return np.ascontiguousarray(np.concatenate([pts, inten.view(np.float32)[:, None]], axis=1))


@pytest.fixture(scope="module")
def host(cloud):
    """The yardstick, computed once per angle."""
    return {a: correct.correct_pc_host(cloud, a) for a in (ANGLE, 0.0, 45.0)}


def ff_equal(a, b):
    """Two FrameFeatures: status, n_key, and the rows, key pixels and flags below n_key."""
    sa, sb = a.status.cpu().numpy(), b.status.cpu().numpy()
    k = int(a.n_key.item())
    return (np.array_equal(sa, sb) and k == int(b.n_key.item())
            and np.array_equal(bits(a.rows[:k].cpu().numpy()), bits(b.rows[:k].cpu().numpy()))
            and np.array_equal(a.key_pixels[:k].cpu().numpy(), b.key_pixels[:k].cpu().numpy())
            and np.array_equal(a.flags[:k].cpu().numpy(), b.flags[:k].cpu().numpy()))


@pytest.mark.parametrize("stride", (3, 4))
@pytest.mark.parametrize("n", (0, 1, 255, 256, 4097))
def test_staged_equals_the_host_restatement(engine, cloud, host, stride, n):
    for angle in (ANGLE, 45.0) if n == 4097 else (ANGLE,):
        src = np.ascontiguousarray(cloud[:n, :stride])
        pc = torch.from_numpy(src).to(engine.device)
        buf = torch.from_numpy(np.full(n * stride + 64, GUARD, dtype=np.uint32).view(np.float32)).to(engine.device)
        rc = engine.lib.caelo_correct_pc(engine.ctx, C.c_void_p(pc.data_ptr()), n, stride, angle, C.c_void_p(buf.data_ptr()), engine.stream)
        assert rc == 0, engine.lib.caelo_last_error()
        got = buf.cpu().numpy()
        assert (bits(got[n * stride:]) == GUARD).all(), "guard words after out[n] were written"
        want = host[angle][:n, :stride]
        assert same_bits(got[:n * stride].reshape(n, stride)[:, :3], want[:, :3])
        assert np.isnan(want[:, :3]).any() == (n >= 4096)            # (the golden's axis points sit at its end)
        if stride == 4:
            assert np.array_equal(bits(got[:n * stride].reshape(n, 4)[:, 3]), bits(src[:, 3]))
        assert np.array_equal(bits(pc.cpu().numpy()), bits(src)), "the input was written"
        if n:
            assert same_bits(engine.correct_pc(pc, angle).cpu().numpy()[:, :3], want[:, :3])


def test_staged_refuses_bad_arguments(engine, cloud):
    pc = torch.from_numpy(cloud[:64]).to(engine.device)
    out = torch.empty_like(pc)
    call = engine.lib.caelo_correct_pc
    p, o = C.c_void_p(pc.data_ptr()), C.c_void_p(out.data_ptr())
    assert call(engine.ctx, p, 64, 4, float("nan"), o, engine.stream) == -1
    assert call(engine.ctx, p, 64, 4, float("inf"), o, engine.stream) == -1
    assert call(engine.ctx, p, 64, 5, ANGLE, o, engine.stream) == -1
    assert call(engine.ctx, p, 64, 4, ANGLE, p, engine.stream) == -1                                  # out aliases pc
    assert call(engine.ctx, p, 64, 4, ANGLE, C.c_void_p(pc.data_ptr() + 16), engine.stream) == -1      # ... overlaps it
    assert call(engine.ctx, p, -1, 4, ANGLE, o, engine.stream) == -1
    assert engine.lib.caelo_set_calib_angle(engine.ctx, float("nan")) == -1
    with pytest.raises(ValueError):
        engine.correct_pc(pc, float("inf"))
    before = engine.get_calib_angle()
    engine.set_calib_angle(0.205)
    assert engine.get_calib_angle() == 0.205
    engine.set_calib_angle(before)


def test_api_correctpc_on_the_golden(engine, host, cloud):
    from caelo import api
    got = api.CorrectPC(np.ascontiguousarray(cloud[:, :3]), 45.0)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and same_bits(got, host[45.0][:, :3])
    assert api.CorrectPC(np.zeros((0, 3), np.float32), ANGLE).shape == (0, 3)


def test_fused_extract_equals_staged_then_extract(engine, scans):
    pc_h = scans(0)                                   # the scan of tests/golden/frame_0.npz
    pc = torch.from_numpy(pc_h).to(engine.device)
    fused = engine.extract(pc, calib_angle=ANGLE)
    assert engine.get_calib_angle() == ANGLE
    staged = engine.extract(engine.correct_pc(pc, ANGLE))
    plain = engine.extract(pc)
    assert int(fused.status[0].item()) == 0 and ff_equal(fused, staged)
    assert not ff_equal(fused, plain)
    assert np.array_equal(bits(pc.cpu().numpy()), bits(pc_h)), "the caller's scan was written"
    # the given key points of a frame are used as they are; only the scan is corrected
    kp = staged.key_pts[:300].contiguous()
    assert ff_equal(engine.extract(pc, key_pts=kp, calib_angle=ANGLE), engine.extract(engine.correct_pc(pc, ANGLE), key_pts=kp))


def test_pipeline_mixed_modes_and_a_nan_frame(engine, scans):
    """Batch 2, five jobs off | on on | on | off: a flush at each change of mode, one full and two partial batches."""
    s0, s1 = scans(0), scans(1)
    sz = s0.copy()
    sz[1234, 0:3] = (0.0, 0.0, -1.5)                  # one point on the z axis: NaN once corrected
    host_scans = [s0, s1, sz, s0, s1]
    calib = [None, ANGLE, ANGLE, ANGLE, None]
    dev = [torch.from_numpy(a).to(engine.device) for a in host_scans]
    pipe = engine.pipeline(batch=2)
    out = pipe.run(dev, pairs=False, calib_angle=calib)
    torch.cuda.synchronize()
    st = out.status[:, 0].cpu().numpy()
    from caelo.engine import ST_NONFINITE
    for i in (0, 1, 3, 4):
        single = engine.extract(dev[i], calib_angle=calib[i])
        assert st[i] == 0 and ff_equal(out.frame(i), single), "frame %d differs from its single fused call" % i
    assert st[2] & ST_NONFINITE and int(engine.extract(dev[2], calib_angle=ANGLE).status[0].item()) & ST_NONFINITE
    assert int(engine.extract(dev[2]).status[0].item()) == 0          # uncorrected, the same scan is a normal frame
    assert not ff_equal(out.frame(1), out.frame(4)) and not ff_equal(out.frame(0), out.frame(3))
    for t, a in zip(dev, host_scans):
        assert np.array_equal(bits(t.cpu().numpy()), bits(a)), "a caller's scan was written"
    # a run with one angle for every frame, and the refusals
    out2 = pipe.run(dev[:2], pairs=False, calib_angle=ANGLE)
    torch.cuda.synchronize()
    assert ff_equal(out2.frame(1), out.frame(1)) and ff_equal(out2.frame(0), out.frame(3))
    with pytest.raises(ValueError):
        pipe.run(dev[:2], pairs=False, calib_angle=[0.22, 0.205])


RUN_SEQUENCE = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")


def _run(args):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def cli_seq(engine, tmp_path_factory):
    """Six synthetic scans as raw files and as files corrected beforehand through api.CorrectPC, and the pose file of the run on the
    corrected ones: the reference of the two command-line tests below, computed once."""
    from caelo import api, synth
    base = tmp_path_factory.mktemp("calib_cli")
    raw, cor = base / "raw" / "velodyne", base / "cor" / "velodyne"
    raw.mkdir(parents=True)
    cor.mkdir(parents=True)
    for i in range(6):
        pc = synth.make_scan(i, trajectory="circuit").astype(np.float32)    # (run_sequence.py's default law)
        pc.tofile(str(raw / ("%06d.bin" % i)))
        np.c_[api.CorrectPC(np.ascontiguousarray(pc[:, 0:3]), ANGLE), pc[:, 3]].astype(np.float32).tofile(str(cor / ("%06d.bin" % i)))
    _run([RUN_SEQUENCE, "--scans", str(cor), "--out", str(base / "ref.txt")])
    want = open(str(base / "ref.txt"), "rb").read()
    assert len(want.splitlines()) == 6
    return raw, want


def test_cli_calib_angle_on_synthetic_scans(cli_seq, tmp_path):
    """run_sequence.py --synthetic 6 --calib-angle 0.22 (Python loader threads, Pipeline.run_uploading): the pose file of the same run
    on scans corrected beforehand, byte for byte."""
    out = str(tmp_path / "a.txt")
    _run([RUN_SEQUENCE, "--synthetic", "6", "--calib-angle", str(ANGLE), "--out", out])
    assert open(out, "rb").read() == cli_seq[1]


def test_cli_calib_angle_on_raw_files(cli_seq, tmp_path):
    """... and --scans <raw files> --calib-angle 0.22 through the native loader (Pipeline.run_loaded: the correction reads the device slot
    after the batch's copy has landed)."""
    out = str(tmp_path / "c.txt")
    _run([RUN_SEQUENCE, "--scans", str(cli_seq[0]), "--calib-angle", str(ANGLE), "--out", out])
    assert open(out, "rb").read() == cli_seq[1]


def test_cli_without_the_flag_is_unchanged(tmp_path):
    """No --calib-angle: the poses of the reference's golden sequence, as before (tests/test_gpu_parity.py holds run_sequence.py's loop
    to the same bound)."""
    g = np.load(os.path.join(GOLDEN, "sequence_20.npz"))
    out = str(tmp_path / "p.txt")
    _run([RUN_SEQUENCE, "--synthetic", "6", "--trajectory", "line", "--seed-base", str(int(g["seed_base"])), "--out", out])
    poses = np.loadtxt(out)
    want = g["poses_identity"].reshape(-1, 12)[:6]
    assert poses.shape == (6, 12) and np.abs(poses - want).max() <= 20 * 1e-4 * np.abs(want).max()


def test_correct_scans_round_trip(engine, cloud, host, tmp_path):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    sizes = (4097, 300, 1)
    for i, n in enumerate(sizes):
        cloud[:n].tofile(str(src / ("%06d.bin" % i)))
    _run([os.path.join(REPO, "cae-lo_amd", "correct_scans.py"), "--scans", str(src), "--out", str(dst), "--calib-angle", str(ANGLE)])
    for i, n in enumerate(sizes):
        got = np.fromfile(str(dst / ("%06d.bin" % i)), dtype=np.float32).reshape(-1, 4)
        assert same_bits(got[:, :3], host[ANGLE][:n, :3]) and np.array_equal(bits(got[:, 3]), bits(cloud[:n, 3]))
        assert np.array_equal(np.fromfile(str(src / ("%06d.bin" % i)), dtype=np.uint32), bits(cloud[:n]).ravel())
