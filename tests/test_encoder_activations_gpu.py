"""The HIP encoder under its two activation sets (hidden tanh | relu, code tanh | linear) against the float64 network of
tests/netref64_act.py: the reference's trained relu / linear model (the fixture of tests/golden/autoencoder_encoder_half.md) and seeded families under
activations they were not made for, on both stage-1 kernels; the exact points of relu; the derived tables across a change of
activations; the fused path, the pipeline, the refusals, ``api.load_model`` and ``run_sequence.py --encoder-h5``.

The engine of these tests is private (the session's shared engine keeps the shipped model), except where ``api.load_model`` -- which
serves the default engine -- is the thing under test.

Bars.  Descriptors: the project's own, ``_assert_descriptors`` (1e-4 relative, element-wise, floor 0.1).  Every model here was first
run through the plain float32 NumPy restatement on the CPU on the same 582 patches and kept only if that stays within a quarter of
the bar; all six did (fixture 4.0e-6, glorot0 1.2e-6, biased 3.5e-6, shipped_b1 4.1e-6, biased relu/tanh 3.5e-6, biased tanh/linear
7.3e-6), none was dropped, and the test asserts it again.  P2, F3 and the hidden vector: 4 x the float32 restatement's own maximum
error against float64 at that layer on these patches, computed here -- no constant taken from the device (the factor covers 2^-22
split products against 2^-24 roundings and another summation order)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import netref64 as nr
import netref64_act as na
from conftest import REPO
from test_gpu_parity import _assert_descriptors

pytestmark = pytest.mark.gpu

LAYERS = ("P2", "F3", "hidden", "descriptors")
F32_QUALIFIES = 2.5e-5      # a quarter of the descriptor bar
LAYER_FACTOR = 4.0


@pytest.fixture(scope="module")
def fixdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fixture"))


@functools.lru_cache(maxsize=None)
def _reference(name, directory):
    """(weights, activations, float64 layers, float32-restatement layers, float64 pre-activations of P2) of one model on the 582
    test patches: computed once, read-only."""
    ws, acts = na.model(name, directory)
    bits = na.test_patches()
    ref, pre2 = na.encoder_layers(ws, bits, acts)
    f32, _ = na.encoder_layers(ws, bits, acts, np.float32)
    for a in ref + f32 + (pre2,):
        a.setflags(write=False)
    return ws, acts, ref, f32, pre2


def _fresh(**kw):
    from caelo.engine import Engine
    return Engine(device=0, **kw)


@pytest.fixture(scope="module")
def eng(engine):   # (the session fixture first: it skips without a GPU)
    e = _fresh()
    yield e
    e.set_encoder_reference(False)


@pytest.fixture(scope="module")
def patches(eng):
    import torch
    return torch.from_numpy(na.test_patches().view(np.int64)).to(eng.device)


@pytest.fixture(scope="module")
def scan0(eng, scans):
    import torch
    return torch.from_numpy(scans(0)).to(eng.device)


def _layers(e, t, bd1, hidden):
    """encode_layers as float64-comparable arrays: P2, F3, H(Dense(200) + bias), descriptors."""
    p2, f3, pre, out = (x.cpu().numpy() for x in e.encode_layers(t))
    return p2, f3, na.ACTS[hidden](pre.astype(np.float64) + np.asarray(bd1, np.float64)), out


# ---- 1. descriptors and layers against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m[0] for m in na.MODELS])
def test_layers_against_float64(eng, patches, fixdir, name):
    ws, acts, ref, f32, _ = _reference(name, fixdir)
    f32_rel = na.relative_error(f32[3], ref[3])
    f32_err = {k: float(np.abs(a.astype(np.float64) - r).max()) for k, a, r in zip(LAYERS, f32, ref)}
    print(name, acts, "float32 restatement: descriptors rel %.3e, layers %s" % (f32_rel, f32_err))
    assert f32_rel <= F32_QUALIFIES, (name, f32_rel)
    eng.set_encoder_weights(ws, activations=acts)
    assert eng.encoder_activations() == acts
    got = {}
    try:
        for kernel, reference in (("stage1x", False), ("stage1_f32", True)):
            eng.set_encoder_reference(reference)
            got[kernel] = _layers(eng, patches, ws[7], acts[0])
    finally:
        eng.set_encoder_reference(False)
    errs = {k: {n_: float(np.abs(g.astype(np.float64) - r).max()) for n_, g, r in zip(LAYERS, lay, ref)} for k, lay in got.items()}
    rels = {k: na.relative_error(lay[3], ref[3]) for k, lay in got.items()}
    print(name, "device:", errs, "descriptors rel", rels)
    for kernel, lay in got.items():
        assert all(np.isfinite(x).all() for x in lay), (name, kernel)
        if acts[1] == "tanh":
            assert np.abs(lay[3]).max() <= 1.0
        if acts[0] == "relu":
            assert lay[0].min() >= 0.0 and lay[1].min() >= 0.0 and not np.signbit(lay[0]).any() and not np.signbit(lay[1]).any()
        _assert_descriptors(lay[3], ref[3])
        for layer in LAYERS[:3]:
            assert errs[kernel][layer] <= LAYER_FACTOR * f32_err[layer], (name, kernel, layer, errs[kernel][layer], f32_err[layer])
    assert (ref[3].max(axis=0) - ref[3].min(axis=0)).min() > 1e-3      # every descriptor column moves: not a constant any kernel would pass
    assert eng.lane_faults() == 0


# ---- 2. exact points under relu -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_relu_exact_points(eng, sign):
    """shipped_b1 with b1 := -|b1| (the background act(b1) is exactly 0 in every channel) and b1 := +|b1| (it is b1 itself), under
    relu / linear: every P2 element whose float64 pre-activation lies below -1e-4 is exactly +0.0 on the device, on both stage-1
    kernels; the empty patch's descriptor is the same bits from group 1 and group 3, at any batch position and in a batch of 67."""
    import torch
    ws = nr.encoder_family("shipped_b1")
    ws[1] = (sign * np.abs(ws[1])).astype(np.float32)
    bits = nr.edge_patches(70)
    t = torch.from_numpy(bits.view(np.int64)).to(eng.device)
    ref, pre2 = na.encoder_layers(ws, bits, ("relu", "linear"))
    dead = pre2 < -1e-4
    assert dead.mean() > 0.05 and (pre2 > 1e-4).mean() > 0.05
    eng.set_encoder_weights(ws, activations=("relu", "linear"))
    try:
        for reference in (False, True):
            eng.set_encoder_reference(reference)
            p2 = eng.encode_layers(t)[0].cpu().numpy()
            assert np.array_equal(p2[dead].view(np.uint32), np.zeros(int(dead.sum()), np.uint32)), (sign, reference)   # +0.0, bit for bit
            assert p2.min() >= 0.0 and np.abs(p2.astype(np.float64) - ref[0]).max() <= 1e-4
    finally:
        eng.set_encoder_reference(False)
    f = eng.encode(t, group=1)
    assert torch.equal(eng.encode(t[:69].contiguous(), group=3).reshape(69, 20), f[:69])
    perm = torch.from_numpy(np.random.RandomState(5).permutation(70)).to(eng.device)
    assert torch.equal(eng.encode(t[perm].contiguous(), group=1), f[perm])
    empties = torch.zeros((67, 64), dtype=torch.int64, device=eng.device)
    assert torch.equal(eng.encode(empties, group=1), f[0:1].expand(67, 20))
    _assert_descriptors(f.cpu().numpy(), ref[3])
    assert eng.lane_faults() == 0


# ---- 3. round trip of the derived tables -----------------------------------------------------------------------------------------
def test_activation_round_trip_restores_the_tanh_bits(eng, patches, scan0):
    """One context: biased weights as tanh / tanh -> relu / linear -> tanh / tanh.  The C0 table, its background-output tail and the
    background vector depend on the hidden activation; after the way back the context gives the bits of a context that never left tanh."""
    ws = nr.encoder_family("biased")

    def results(e):
        out = [x.cpu().numpy() for x in e.encode_layers(patches)] + [e.extract(scan0).rows[:, :63].cpu().numpy()]
        e.set_encoder_reference(True)
        out.append(e.encode_layers(patches)[0].cpu().numpy())
        e.set_encoder_reference(False)
        return out

    never = _fresh()
    never.set_encoder_weights(ws)
    assert never.encoder_activations() == ("tanh", "tanh")
    want = results(never)
    del never
    eng.set_encoder_weights(ws, activations=("relu", "linear"))
    away = results(eng)
    assert np.abs(away[3] - want[3]).max() > 1e-2
    eng.set_encoder_weights(ws)                                   # activations=None keeps the current pair
    assert eng.encoder_activations() == ("relu", "linear") and all(np.array_equal(a, b) for a, b in zip(results(eng), away))
    eng.set_encoder_weights(ws, activations=("tanh", "tanh"))
    for i, (g, w) in enumerate(zip(results(eng), want)):
        assert np.array_equal(g, w), i
    assert eng.lane_faults() == 0


# ---- 4. fused path ----------------------------------------------------------------------------------------------------------------
def test_fused_extract_equals_encode_of_its_own_patches(eng, scan0, fixdir):
    import torch
    ws, acts = na.model("fixture", fixdir)
    eng.set_encoder_weights(ws, activations=acts)
    a = eng.extract(scan0)
    b = eng.extract(scan0, dedup=False)
    k = int(a.n_key.item())
    assert k == 1024 and int(a.status[0].item()) == 0 and int(b.status[0].item()) == 0
    assert torch.equal(a.rows[:, :63], b.rows[:, :63]) and torch.equal(a.key_pixels, b.key_pixels)
    vm, st = eng.voxelize_fast(scan0, eng.voxmap(slot=5))
    bits, _ = eng.patches(vm, a.key_pts.contiguous())
    assert int(st.item()) == 0 and len(np.unique(bits.cpu().numpy().reshape(3072, 64), axis=0)) < 3072
    assert torch.equal(eng.encode(bits, group=3), a.features[:k])
    assert a.features.abs().max().item() > 1.0      # a linear code: not confined to [-1, 1]
    assert eng.lane_faults() == 0


# ---- 5. pipeline ------------------------------------------------------------------------------------------------------------------
def test_pipeline_three_frames_on_the_fixture_model(eng, scans, fixdir):
    import torch
    from caelo.engine import Pipeline, ransac_draws
    ws, acts = na.model("fixture", fixdir)
    eng.set_encoder_weights(ws, activations=acts)
    pcs = [torch.from_numpy(scans(i)).to(eng.device) for i in range(3)]
    rnd = [torch.from_numpy(ransac_draws(40 + i)).to(eng.device) for i in range(3)]
    ref = [eng.extract(pc) for pc in pcs]
    out = Pipeline(eng, 2, 3).run(pcs, rnd)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(out.rows[i], ref[i].rows), i
    for i in (1, 2):
        k0, k1 = int(ref[i - 1].n_key.item()), int(ref[i].n_key.item())
        f0 = ref[i - 1].features[:k0].cpu().numpy().astype(np.float64)
        f1 = ref[i].features[:k1].cpu().numpy().astype(np.float64)
        d2 = ((f1[:, None, :] - f0[None, :, :]) ** 2).sum(axis=2)          # [k1, k0]
        assert np.array_equal(out.pair_idx[i][:k1].cpu().numpy(), d2.argmin(axis=1)), i
        r = eng.pose_result(out.result[i])
        assert r.success and np.isfinite(np.array(r.R)).all() and np.isfinite(np.array(r.T)).all() and r.n_inliers > 50
    assert eng.lane_faults() == 0


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was(eng, patches, scan0, fixdir):
    import torch
    from caelo._ffi import CaeloError
    ws, acts = na.model("fixture", fixdir)
    eng.set_encoder_weights(ws, activations=acts)
    before = eng.encode(patches, group=1).clone()
    over = nr.encoder_family("glorot0")
    over[2] = over[2] * np.float32(1e4)
    with pytest.raises(CaeloError, match="conv3d_2"):
        eng.set_encoder_weights(over, activations=("relu", "linear"))
    assert eng.encoder_activations() == acts and torch.equal(eng.encode(patches, group=1), before)
    with pytest.raises(ValueError):
        eng.set_encoder_weights(ws, activations=("relu", "relu"))
    with pytest.raises(ValueError):
        eng.set_encoder_weights(ws, activations=("sigmoid", "tanh"))
    assert eng.encoder_activations() == acts
    # the 32^3 path is tanh / tanh only: refused before any launch under every other model
    eng.set_encoder32_dense(*eng.seeded_dense1_32())
    ff = eng.extract(scan0)
    vmap, _ = eng.voxelize(scan0)
    for bad in (("relu", "linear"), ("relu", "tanh"), ("tanh", "linear")):
        eng.set_encoder_weights(ws, activations=bad)
        with pytest.raises(CaeloError, match="tanh / tanh"):
            eng.patches32(vmap, ff.key_pts[::64].contiguous())
        with pytest.raises(CaeloError, match="tanh / tanh"):
            eng.encode32(torch.zeros((4, 512), dtype=torch.int64, device=eng.device))
    torch.cuda.synchronize()
    eng.set_encoder_weights(ws, activations=("tanh", "tanh"))
    assert eng.encode32(torch.zeros((4, 512), dtype=torch.int64, device=eng.device)).shape == (4, 20)
    assert eng.lane_faults() == 0


# ---- 7. api.load_model ------------------------------------------------------------------------------------------------------------
def test_api_load_model_predicts_with_the_files_activations(engine, fixdir):
    from caelo import api
    from caelo.engine import ENCODER_H5, default_engine
    ws, acts, ref, _, _ = _reference("fixture", fixdir)
    sel = slice(0, 96)
    dense = nr.unpack(na.test_patches()[sel]).astype(np.float32)                 # [96,16,16,16,1] like GetPatchesList
    try:
        model = api.load_model(na.fixture_h5(fixdir))
        assert default_engine().encoder_activations() == ("relu", "linear")
        got = model.predict(dense)
        assert got.shape == (96, 20) and got.dtype == np.float32
        _assert_descriptors(got, ref[3][sel])
    finally:
        api.load_model(ENCODER_H5)
    assert default_engine().encoder_activations() == ("tanh", "tanh")


# ---- 8. run_sequence.py -----------------------------------------------------------------------------------------------------------
def test_run_sequence_with_an_encoder_file(eng, fixdir, tmp_path):
    """run_sequence.py --synthetic 3 --encoder-h5 <fixture>: three finite pose rows, equal to the rows chained from Engine calls
    (extract, the exact match + RANSAC) on the same scans with the same seeds."""
    import torch
    from caelo import _ffi, stageio, synth
    from caelo.engine import ransac_draws
    h5 = na.fixture_h5(fixdir)
    out = tmp_path / "poses_" / "00.txt"
    subprocess.run([sys.executable, os.path.join(REPO, "cae-lo_amd", "run_sequence.py"), "--synthetic", "3", "--encoder-h5", h5,
                    "--out", str(out)], check=True, capture_output=True, timeout=300)
    rows = np.loadtxt(str(out))
    assert rows.shape == (3, 12) and np.isfinite(rows).all()
    ws, acts = na.model("fixture", fixdir)
    eng.set_encoder_weights(ws, activations=acts)
    feats = [eng.extract(torch.from_numpy(synth.make_scan(i, trajectory="circuit")).to(eng.device)) for i in range(3)]
    rel = []
    for i in (1, 2):
        draws = ransac_draws(1000 + i - 1)
        r = _ffi.PoseResult.from_buffer_copy(eng.match_pose_exact(feats[i - 1], feats[i], torch.from_numpy(draws).to(eng.device), draws)[0].tobytes())
        assert r.success
        rel.append(np.r_[np.array(r.R, np.float32), np.array(r.T, np.float32)])
    mine = tmp_path / "mine.txt"
    stageio.write_poses(str(mine), stageio.chain_poses(np.array(rel), None))
    assert open(str(out)).read() == open(str(mine)).read()
    # a file of the other network, or a stack the kernels do not implement, is refused before any device work
    from caelo.engine import RESPOND_H5
    r = subprocess.run([sys.executable, os.path.join(REPO, "cae-lo_amd", "run_sequence.py"), "--synthetic", "3", "--encoder-h5", RESPOND_H5,
                        "--out", str(tmp_path / "no.txt")], capture_output=True, timeout=120)
    assert r.returncode == 2 and b"--encoder-h5" in r.stderr and not (tmp_path / "no.txt").exists()
