"""The HIP decoder (csrc/decoder.hip) against the float64 network of tests/netref64_dec.py: the reference's trained autoencoder (the
fixtures of tests/golden/autoencoder_encoder_half.md and autoencoder_decoder_half.md) and two seeded families, layer by layer; the
thresholded voxels and the counts; launch shapes; exact points that pin the Reshape order, the up-sampling orientation and the zero
border; the refusals; that nothing else of the engine moves; ``api.load_autoencoder`` and ``evaluate.py reconstruction``.

The engines of these tests are private (the session's shared engine keeps the shipped model), except where ``api.load_autoencoder``
-- which serves the default engine -- is the thing under test.

Bars.  Codes are the float64 encoder's codes cast to float32, so only the decoder is measured.  G4, z = logit(prob), prob and the
loss: 4 x the plain float32 NumPy restatement's own maximum error against float64 for that quantity on these patches, computed here --
no constant taken from the device (the factor covers another summation order and the two-accumulator MFMA chains).  z is compared where
the float32 sigmoid can carry it: z64 in [-80, 12] (below, prob is subnormal or 0; above, 1 - prob has no bits left), with the
restatement's error taken through the same logit(prob).  The loss is pinned to the float64 formula of netref64_dec.bce, not to Keras,
which cannot run here.  Thresholded voxels: a voxel is decided when |z64 - logit(threshold)| exceeds 4 x the
restatement's max |z32 - z64|; every decided voxel must equal the float64 decision and at most 1e-4 of the voxels may be undecided.
Thresholds: 0.1 (Voxel.VoxelModel2PC's) and 0.5 for the trained model; the families' logits lie within +-0.6, where 0.1 decides
nothing, so they are cut inside their range (0.48 / 0.52 and 0.4 / 0.5; not 0.5 for the bias-free tanh family, whose empty patch has
z = 0 = logit(0.5) exactly in every voxel)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import netref64 as nr
import netref64_act as na
import netref64_dec as nd
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

FACTOR = 4.0
UNDECIDED_MAX = 1e-4
TILE = 64            # rows per workgroup of k_dec_dense
THRESHOLDS = [("fixture", 0.1), ("fixture", 0.5), ("glorot_tanh", 0.48), ("glorot_tanh", 0.52), ("biased_relu", 0.4), ("biased_relu", 0.5)]
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def fixdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fixture"))


def _fresh(**kw):
    from caelo.engine import Engine
    return Engine(device=0, **kw)


@pytest.fixture(scope="module")
def bare(engine):   # (the session fixture first: it skips without a GPU) -- an engine that never gets a decoder
    return _fresh()


@pytest.fixture(scope="module")
def eng(engine):
    return _fresh()


def _t(eng, a, dtype=None):
    import torch
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(eng.device)


def _set(eng, name, fixdir):
    R = nd.reference(name, fixdir)
    eng.set_decoder_weights(R["dws"], R["dact"])
    assert eng.decoder_activations() == R["dact"]
    return R


def _np(d):
    return tuple(None if x is None else x.cpu().numpy() for x in d)


def _logit(p):
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore"):
        return np.log(p) - np.log1p(-p)


def _raw_decode(eng, codes, n, group, ld, target, threshold, outs, ws=None):
    """caelo_decode through ctypes with the caller's output tensors (None = NULL) -> return code."""
    from caelo.engine import _ptr
    ws = eng._ws("decode", int(eng.lib.caelo_decode_ws_bytes(max(int(n), 0)))) if ws is None else ws
    return eng.lib.caelo_decode(eng.ctx, _ptr(codes), n, group, ld, _ptr(target), float(threshold), *[_ptr(o) for o in outs], _ptr(ws), eng.stream)


# ---- 0. an engine without a decoder ------------------------------------------------------------------------------------------------
def test_no_decoder_decode_is_refused_and_touches_nothing(bare):
    import torch
    from caelo._ffi import CaeloError
    codes = torch.zeros((4, 20), dtype=torch.float32, device=bare.device)
    with pytest.raises(CaeloError, match="no decoder model set"):
        bare.decode(codes)
    outs = [torch.full(s, SENTINEL, dtype=torch.uint8, device=bare.device) for s in ((4 * 4096 * 4,), (4 * 64 * 8,), (4 * 4,), (4 * 3 * 4,))]
    tgt = torch.zeros((4, 64), dtype=torch.int64, device=bare.device)
    assert _raw_decode(bare, codes, 4, 1, 20, tgt, 0.1, outs) == -1
    assert b"no decoder" in bare.lib.caelo_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)


def test_no_decoder_activations_are_an_error(bare):
    from caelo._ffi import CaeloError
    with pytest.raises(CaeloError, match="no decoder model set"):
        bare.decoder_activations()
    assert bare.encoder_activations() == ("tanh", "tanh")


def test_no_decoder_bad_models_are_refused_and_leave_none(bare):
    from caelo._ffi import CaeloError
    ws = nd.decoder_family("glorot")
    for acts in (("relu", "relu"), ("linear", "sigmoid"), ("sigmoid", "sigmoid"), ("relu",), None, ("relu", "tanh")):
        with pytest.raises(ValueError, match="decoder activations"):
            bare.set_decoder_weights(ws, acts)
    with pytest.raises(ValueError, match="decoder weights"):
        bare.set_decoder_weights(ws[:9], ("relu", "sigmoid"))
    with pytest.raises(ValueError, match="decoder weights"):
        bare.set_decoder_weights(ws[:8] + [np.zeros((3, 3, 3, 8, 2), np.float32), ws[9]], ("relu", "sigmoid"))
    p = [w.ctypes.data_as(C.c_void_p) for w in ws]
    assert bare.lib.caelo_set_decoder_model(bare.ctx, *(p + [2, 3])) == -1       # linear hidden
    assert bare.lib.caelo_set_decoder_model(bare.ctx, *(p + [1, 0])) == -1       # tanh output
    assert bare.lib.caelo_set_decoder_model(bare.ctx, *(p[:9] + [None] + [1, 3])) == -1
    with pytest.raises(CaeloError, match="no decoder model set"):
        bare.decoder_activations()
    # the engine still encodes
    bits = _t(bare, nr.edge_patches(8))
    assert np.isfinite(bare.encode(bits).cpu().numpy()).all()


# ---- 1. layers against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m[0] for m in nd.MODELS])
def test_layers_against_float64(eng, fixdir, name):
    R = _set(eng, name, fixdir)
    l64, l32, z64 = R["l64"], R["l32"], R["l64"][4]
    n = len(R["codes"])
    codes, target = _t(eng, R["codes"]), _t(eng, R["bits"])
    g4 = eng.decode_layers(codes).cpu().numpy()
    prob, bits, loss, counts = _np(eng.decode(codes, target=target, threshold=0.1, prob=True))
    assert g4.shape == (n, 2048) and prob.shape == (n, 4096) and prob.dtype == np.float32 and loss.shape == (n,) and loss.dtype == np.float32
    assert np.isfinite(g4).all() and np.isfinite(loss).all() and (prob >= 0).all() and (prob <= 1).all()
    if R["dact"][0] == "relu":
        assert g4.min() >= 0.0
    carried = (z64 >= -80.0) & (z64 <= 12.0)
    assert carried.mean() > 0.8          # (the trained model sends 15 % of its voxels below -80)
    bar = {"G4": float(np.abs(l32[1].astype(np.float64) - l64[1]).max()),
           "z": float(np.abs(_logit(R["p32"])[carried] - z64[carried]).max()),
           "prob": float(np.abs(R["p32"].astype(np.float64) - R["p64"]).max()),
           "loss": float(np.abs(R["loss32"].astype(np.float64) - R["loss64"]).max())}
    err = {"G4": float(np.abs(g4.astype(np.float64) - l64[1]).max()),
           "z": float(np.abs(_logit(prob)[carried] - z64[carried]).max()),
           "prob": float(np.abs(prob.astype(np.float64) - R["p64"]).max()),
           "loss": float(np.abs(loss.astype(np.float64) - R["loss64"]).max())}
    print(name, R["dact"], "n", n, "z64 range %.4g .. %.4g, carried share %.6f" % (z64.min(), z64.max(), carried.mean()))
    print(name, "float32 restatement:", bar)
    print(name, "device:             ", err, "loss range %.4g .. %.4g" % (R["loss64"].min(), R["loss64"].max()))
    for k in bar:
        assert err[k] <= FACTOR * bar[k], (name, k, err[k], bar[k])


# ---- 2. thresholded voxels and counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,threshold", THRESHOLDS)
def test_bits_and_counts(eng, fixdir, name, threshold):
    R = _set(eng, name, fixdir)
    z64 = R["l64"][4]
    margin = FACTOR * float(np.abs(R["l32"][4].astype(np.float64) - z64).max())
    cut = float(np.log(threshold / (1.0 - threshold)))
    decided = np.abs(z64 - cut) > margin
    share = 1.0 - decided.mean()
    codes, target = _t(eng, R["codes"]), _t(eng, R["bits"])
    _, bits, _, counts = _np(eng.decode(codes, target=target, threshold=threshold))
    got = nd.dense_target(bits.view(np.uint64)) > 0
    want = z64 > cut
    wrong = int((got != want)[decided].sum())
    print(name, "threshold", threshold, "margin %.3e, undecided share %.3e, set %d of %d, decided and wrong %d" % (margin, share, int(want.sum()), want.size, wrong))
    assert share <= UNDECIDED_MAX
    assert wrong == 0
    assert 0 < want.sum() < want.size                                   # the threshold cuts inside the model's range
    tb = R["bits"]
    assert np.array_equal(counts[:, 0], nd.popcount(tb)) and np.array_equal(counts[:, 1], nd.popcount(bits.view(np.uint64)))
    assert np.array_equal(counts[:, 2], nd.popcount(tb & bits.view(np.uint64)))


# ---- 3. launch shapes --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(eng, fixdir):
    """The trained model on its first 200 patches, every output: what every launch shape must reproduce bit for bit."""
    R = _set(eng, "fixture", fixdir)
    codes, target = _t(eng, R["codes"][:200]), _t(eng, R["bits"][:200])
    return codes, target, _np(eng.decode(codes, target=target, threshold=0.1, prob=True))


def _same(a, b, rows):
    return all(x[rows].tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1])
def test_launch_sizes_reproduce_the_bits(eng, fixdir, full, n):
    codes, target, want = full
    _set(eng, "fixture", fixdir)
    got = _np(eng.decode(codes[:n].contiguous(), target=target[:n].contiguous(), threshold=0.1, prob=True))
    assert _same(want, got, slice(0, n))


def test_a_patch_alone_or_inside_200(eng, fixdir, full):
    codes, target, want = full
    _set(eng, "fixture", fixdir)
    for i in (0, 5, TILE - 1, TILE, 137, 199):
        got = _np(eng.decode(codes[i:i + 1].contiguous(), target=target[i:i + 1].contiguous(), threshold=0.1, prob=True))
        assert _same(want, got, slice(i, i + 1)), i


def test_zero_patches_do_nothing(eng, fixdir):
    import torch
    _set(eng, "fixture", fixdir)
    d = eng.decode(torch.zeros((0, 20), dtype=torch.float32, device=eng.device), target=torch.zeros((0, 64), dtype=torch.int64, device=eng.device), prob=True)
    assert d.prob.shape == (0, 4096) and d.bits.shape == (0, 64) and d.loss.shape == (0,) and d.counts.shape == (0, 3)
    outs = [torch.full((64,), SENTINEL, dtype=torch.uint8, device=eng.device) for _ in range(4)]
    assert _raw_decode(eng, None, 0, 1, 20, None, 0.1, outs[:2] + [None, outs[3]]) == 0
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)


def test_descriptor_rows_equal_plain_codes(eng, fixdir, full):
    """group = 3, ld = 64 on [K,64] rows (descriptor 0:60 | xyz | valid, the pipeline's resident rows) against group = 1, ld = 20."""
    import torch
    codes, target, want = full
    _set(eng, "fixture", fixdir)
    k = 66
    rows = torch.full((k, 64), 7.5, dtype=torch.float32, device=eng.device)
    rows[:, :60] = codes[:3 * k].reshape(k, 60)
    got = _np(eng.decode(rows, group=3, target=target[:3 * k].contiguous(), threshold=0.1, prob=True))
    assert _same(want, got, slice(0, 3 * k))


def test_each_output_alone_gives_the_same_bits(eng, fixdir, full):
    codes, target, want = full
    _set(eng, "fixture", fixdir)
    n = 70
    c, t = codes[:n].contiguous(), target[:n].contiguous()
    alone = (eng.decode(c, prob=True, bits=False).prob, eng.decode(c).bits, eng.decode(c, target=t, bits=False, counts=False).loss,
             eng.decode(c, target=t, bits=False, loss=False).counts)
    for w, g in zip(want, alone):
        assert w[:n].tobytes() == g.cpu().numpy().tobytes()
    d = eng.decode(c, counts=True)                       # no target: the reconstruction's count only
    assert d.loss is None and np.array_equal(d.counts.cpu().numpy(), want[3][:n] * np.array([0, 1, 0], np.int32))


# ---- 4. exact points ---------------------------------------------------------------------------------------------------------------
def _zero_model():
    return [np.zeros(s, np.float32) for s in nd.DECODER_SHAPES]


@pytest.mark.parametrize("b6", [0.3, -2.0, 0.0, 9.0])
def test_zero_kernels_give_sigmoid_of_the_bias(eng, b6):
    ws = _zero_model()
    ws[9][0] = b6
    for hidden in ("relu", "tanh"):
        eng.set_decoder_weights(ws, (hidden, "sigmoid"))
        codes = _t(eng, np.random.RandomState(1).uniform(-3, 3, size=(3, 20)), np.float32)
        prob, bits, _, _ = _np(eng.decode(codes, prob=True, threshold=0.5))
        want = 1.0 / (1.0 + np.exp(-np.float64(np.float32(b6))))
        assert (prob == prob[0, 0]).all()
        assert abs(float(prob[0, 0]) - want) <= 3 * np.spacing(np.float32(want))     # expf, one addition, one division
        assert (bits == (-1 if want > 0.5 else 0)).all()                               # 0.5 > 0.5 is false: the test is strict


def _one_hot_model(cell, channel, taps):
    """G4 = the one-hot vector at (cell, channel) whatever the code; conv3d_4/5/6 single taps of weight 1 (conv3d_4 from ``channel``
    to channel 0): every activation is 0 or 1 and exact."""
    ws = _zero_model()
    ws[1][0] = 1.0                                                   # h3 = relu(b3) = e_0
    ws[2][0, ((cell[0] * 4 + cell[1]) * 4 + cell[2]) * 32 + channel] = 1.0     # Reshape: ((x*4+y)*4+z)*32+c
    ws[4][taps[0] + (channel, 0)] = 1.0
    ws[6][taps[1] + (0, 0)] = 1.0
    ws[8][taps[2] + (0, 0)] = 1.0
    return ws


@pytest.mark.parametrize("cell,channel,taps", [
    ((1, 2, 3), 5, ((1, 1, 1), (1, 1, 1), (1, 1, 1))),        # centre taps: cell (x,y,z) becomes the 4^3 block at (4x, 4y, 4z)
    ((3, 0, 2), 31, ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    ((0, 0, 0), 0, ((1, 1, 1), (1, 1, 1), (0, 0, 0))),        # conv3d_6 reads voxel u - 1: the block moves by +1, voxel (0,0,0) reads padding
    ((3, 3, 3), 0, ((1, 1, 1), (1, 1, 1), (2, 2, 2))),        # ... u + 1: voxel (15,15,15) reads padding
    ((3, 3, 3), 7, ((1, 1, 1), (0, 1, 2), (2, 0, 1))),        # a different tap per axis, through both folds
    ((0, 3, 1), 16, ((2, 1, 0), (2, 2, 0), (0, 2, 1))),
    ((2, 1, 0), 9, ((0, 0, 0), (0, 0, 0), (0, 0, 0))),
    ((1, 1, 2), 3, ((2, 2, 2), (2, 2, 2), (2, 2, 2))),
])
def test_one_hot_pins_reshape_upsampling_and_border(eng, cell, channel, taps):
    ws = _one_hot_model(cell, channel, taps)
    eng.set_decoder_weights(ws, ("relu", "sigmoid"))
    codes = np.zeros((2, 20), np.float32)
    z64 = nd.decoder_layers(ws, codes, ("relu", "sigmoid"))[4]
    assert set(np.unique(z64)) <= {0.0, 1.0}
    prob, bits, _, counts = _np(eng.decode(_t(eng, codes), prob=True, threshold=0.6, counts=True))
    want = z64 > 0.5
    assert np.array_equal(nd.dense_target(bits.view(np.uint64)) > 0, want)
    assert np.array_equal(counts[:, 1], want.sum(axis=1))
    s1 = 1.0 / (1.0 + np.exp(-1.0))
    assert np.abs(prob[want] - s1).max() <= 3 * np.spacing(np.float32(s1)) if want.any() else True
    assert (prob[~want] == 0.5).all()
    vol = want[0].reshape(16, 16, 16)
    if taps == ((1, 1, 1), (1, 1, 1), (1, 1, 1)):
        lo = [4 * c for c in cell]
        block = np.zeros((16, 16, 16), bool)
        block[lo[0]:lo[0] + 4, lo[1]:lo[1] + 4, lo[2]:lo[2] + 4] = True
        assert np.array_equal(vol, block)
    if cell == (0, 0, 0) and taps[2] == (0, 0, 0):
        assert not vol[0, 0, 0] and vol[1, 1, 1] and vol[4, 4, 4] and not vol[5, 5, 5] and vol.sum() == 64
    if cell == (3, 3, 3) and taps[2] == (2, 2, 2) and taps[1] == (1, 1, 1):
        assert not vol[15, 15, 15] and vol[14, 14, 14] and vol[11, 11, 11] and not vol[10, 10, 10] and vol.sum() == 64


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_touch_nothing_and_leave_the_engine_usable(eng, fixdir, full):
    import torch
    from caelo._ffi import CaeloError
    codes, target, want = full
    _set(eng, "fixture", fixdir)
    n = 8
    c, t = codes[:n].contiguous(), target[:n].contiguous()
    sizes = (n * 4096 * 4, n * 64 * 8, n * 4, n * 3 * 4)
    outs = [torch.full((s,), SENTINEL, dtype=torch.uint8, device=eng.device) for s in sizes]
    rows = torch.zeros((n, 64), dtype=torch.float32, device=eng.device)
    cases = [("loss without a target", (c, n, 1, 20, None, 0.1, outs)),
             ("threshold 0", (c, n, 1, 20, t, 0.0, outs)), ("threshold 1", (c, n, 1, 20, t, 1.0, outs)),
             ("threshold below 0", (c, n, 1, 20, t, -0.1, outs)), ("threshold nan", (c, n, 1, 20, t, float("nan"), outs)),
             ("threshold inf", (c, n, 1, 20, t, float("inf"), outs)),
             ("group * 20 > ld", (rows, n, 4, 64, t, 0.1, outs)), ("group 2 on ld 20", (c, n, 2, 20, t, 0.1, outs)),
             ("group 0", (c, n, 0, 20, t, 0.1, outs)), ("negative n", (c, -1, 1, 20, t, 0.1, outs)),
             ("no output", (c, n, 1, 20, t, 0.1, [None] * 4)), ("null codes", (None, n, 1, 20, t, 0.1, outs))]
    for what, args in cases:
        assert _raw_decode(eng, *args) == -1, what
        assert eng.lib.caelo_last_error(), what
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    with pytest.raises(CaeloError, match="threshold"):
        eng.decode(c, threshold=1.5)
    with pytest.raises(CaeloError, match="target"):
        eng.decode(c, loss=True)
    with pytest.raises(CaeloError, match="no output"):
        eng.decode(c, bits=False)
    got = _np(eng.decode(c, target=t, threshold=0.1, prob=True))
    assert _same(want, got, slice(0, n))


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------------
def test_encoder_bits_do_not_move_and_no_lane_faults(engine, fixdir):
    e = _fresh()
    g = np.load(os.path.join(GOLDEN, "frame_0.npz"))["patch_bits"]
    bits = _t(e, np.ascontiguousarray(g.reshape(-1, 64)))
    before = e.encode(bits, group=3).cpu().numpy()
    R = nd.reference("fixture", fixdir)
    e.set_decoder_weights(R["dws"], R["dact"])
    after = e.encode(bits, group=3).cpu().numpy()
    assert before.tobytes() == after.tobytes() and e.encoder_activations() == ("tanh", "tanh")
    d = e.decode(_t(e, after), group=3, target=bits)
    assert np.isfinite(d.loss.cpu().numpy()).all()
    assert e.encode(bits, group=3).cpu().numpy().tobytes() == before.tobytes()
    assert e.lane_faults() == 0


# ---- 7. api ------------------------------------------------------------------------------------------------------------------------
def test_api_load_autoencoder_predict(engine, fixdir):
    from caelo import api
    from caelo.engine import ENCODER_H5, default_engine
    R = nd.reference("fixture", fixdir)
    sel = slice(0, 96)
    dense = nr.unpack(R["bits"][sel]).astype(np.float32)                 # [96,16,16,16,1] like GetPatchesList
    # the float32 restatement of the whole autoencoder, and the float64 one
    c32 = na.encoder_layers(R["ews"], R["bits"][sel], R["eact"], np.float32)[0][3]
    c64 = na.encoder_layers(R["ews"], R["bits"][sel], R["eact"])[0][3]
    p32 = nd.sigmoid(nd.decoder_layers(R["dws"], c32, R["dact"], np.float32)[4])
    p64 = nd.sigmoid(nd.decoder_layers(R["dws"], c64, R["dact"])[4])
    bar = float(np.abs(p32.astype(np.float64) - p64).max())
    e = default_engine()
    try:
        model = api.load_autoencoder(nd.fixture_h5(fixdir), encoder_h5=na.fixture_h5(fixdir))
        assert e.encoder_activations() == ("relu", "linear") and e.decoder_activations() == ("relu", "sigmoid")
        got = model.predict(dense)
        assert got.shape == (96, 16, 16, 16, 1) and got.dtype == np.float32
        bits = _t(e, R["bits"][sel])
        mine = e.decode(e.encode(bits), prob=True, bits=False).prob.cpu().numpy()
        assert got.tobytes() == mine.tobytes()
        err = float(np.abs(got.reshape(96, 4096).astype(np.float64) - p64).max())
        print("autoencoder.predict: float32 restatement %.3e, device %.3e" % (bar, err))
        assert err <= FACTOR * bar
        loss, counts = api.ReconstructionLoss(model, [dense[:32], dense[32:64], dense[64:96]])
        assert loss.shape == (32, 3) and loss.dtype == np.float32 and counts.shape == (32, 3, 3) and counts.dtype == np.int32
        d = e.decode(e.encode(bits), target=bits, threshold=0.1)
        assert np.array_equal(loss, d.loss.cpu().numpy().reshape(3, 32).T) and np.array_equal(counts, d.counts.cpu().numpy().reshape(3, 32, 3).transpose(1, 0, 2))
        with pytest.raises(ValueError, match="no encoder weights"):
            api.load_autoencoder(nd.fixture_h5(fixdir))
        with pytest.raises(ValueError, match="no decoder weights"):
            api.load_autoencoder(na.fixture_h5(fixdir))
        assert api.load_model(na.fixture_h5(fixdir)).kind == "encoder"      # load_model keeps returning the encoder
    finally:
        api.load_model(ENCODER_H5)
    assert e.encoder_activations() == ("tanh", "tanh")


# ---- 7b. the patches of the last extract line up with its descriptor rows ------------------------------------------------------------
def test_extract_patch_bits_line_up_with_the_descriptor_rows(engine, scans, fixdir):
    """What evaluate.reconstruction relies on: ``extract_patch_bits()[k, s]`` is the patch behind columns 20 s .. 20 s + 20 of row k.
    decode of the resident rows (group 3) against those patches gives the losses of decode(encode(patches)) against themselves, and
    a target shifted by one patch does not."""
    import torch
    e = _fresh()
    R = nd.reference("fixture", fixdir)
    e.set_encoder_weights(R["ews"], activations=R["eact"])
    e.set_decoder_weights(R["dws"], R["dact"])
    ff = e.extract(torch.from_numpy(scans(0)).to(e.device), dedup=False)
    bits = e.extract_patch_bits()
    k = int(ff.n_key.item())
    assert k > 50 and bits.shape == (1024, 3, 64)
    tgt = bits[:k].contiguous()
    rows = e.decode(ff.rows[:k].contiguous(), group=3, target=tgt)
    codes = e.encode(tgt.view(-1, 64))
    assert codes.cpu().numpy().tobytes() == ff.features[:k].contiguous().cpu().numpy().tobytes()
    own = e.decode(codes, target=tgt.view(-1, 64))
    assert rows.loss.cpu().numpy().tobytes() == own.loss.cpu().numpy().tobytes()
    assert rows.counts.cpu().numpy().tobytes() == own.counts.cpu().numpy().tobytes()
    shifted = e.decode(ff.rows[:k].contiguous(), group=3, target=torch.roll(tgt.view(-1, 64), 1, dims=0).contiguous())
    assert float(shifted.loss.double().mean().item()) > 1.5 * float(rows.loss.double().mean().item())
    from caelo import evaluate as ev
    res = ev.reconstruction(e, [scans(0)])
    assert np.array_equal(res["patch_loss"], rows.loss.cpu().numpy().reshape(k, 3)) and res["n_key"].tolist() == [k]


# ---- 8. evaluate.py reconstruction -------------------------------------------------------------------------------------------------
def test_evaluate_reconstruction_on_the_fixture(engine, fixdir, tmp_path):
    from scipy import io
    out = tmp_path / "recon.mat"
    r = subprocess.run([sys.executable, os.path.join(REPO, "cae-lo_amd", "evaluate.py"), "reconstruction", "--autoencoder-h5", nd.fixture_h5(fixdir),
                        "--encoder-h5", na.fixture_h5(fixdir), "--synthetic", "3", "--out", str(out)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert b"reconstruction: 3 frames" in r.stdout
    m = io.loadmat(str(out))
    k = m["n_key"].ravel()
    assert k.shape == (3,) and (k > 50).all() and m["loss"].shape == (3, 3) and m["iou"].shape == (3, 3)
    pl = m["patch_loss"]
    assert pl.shape == (int(k.sum()), 3) and np.isfinite(pl).all() and (pl > 0).all() and np.isfinite(m["loss"]).all()
    assert abs(float(m["mean_loss"].item()) - float(pl.mean(dtype=np.float64))) <= 1e-12
    assert np.allclose(m["loss"][0], pl[:k[0]].mean(axis=0, dtype=np.float64), rtol=1e-6)
    iou = m["iou"]
    assert ((iou >= 0) & (iou <= 1)).all()
    assert float(m["threshold"].item()) == 0.1
