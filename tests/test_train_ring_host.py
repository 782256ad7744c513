"""CPU: what training the ring autoencoder rests on besides the kernels -- the torch reference checks itself against central
differences, ``keras_config.read_ring_autoencoder`` and ``write_ring_models_like`` on the fixture and the shipped response-layer file,
``train_ring.fit``'s shuffling and batching with a stub trainer, Adam's float32 restatement against its float64 twin, and the
parameter layout of the C ABI."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import netref64_ring as nr

REPO = os.path.dirname(nr.HERE)
RESPOND_H5 = os.path.join(REPO, "weights", "SphericalRingPCRespondLayer.h5")
ENCODER_H5 = os.path.join(REPO, "weights", "EncoderModel4VoxelPatch.h5")


# ---- the reference checks itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nr.MODELS)
def test_reference_gradient_matches_central_difference(name):
    h, cd, gd = nr.self_check(name, tol=1e-6)
    print("%s: h %.0e, central difference %.12g, g.d %.12g, relative %.3g" % (name, h, cd, gd, abs(cd - gd) / abs(gd)))


def test_parameter_count_and_layout():
    from caelo import _ffi, keras_config, train_ring
    sizes = [int(np.prod(s)) for s in nr.SHAPES]
    assert sizes == [864, 32, 256, 8, 1152, 16, 2304, 16, 1152, 8, 24, 3] and sum(sizes) == 5835 == nr.N_PARAMS == train_ring.N_PARAMS
    assert [tuple(s) for s in keras_config.RING_AE_SHAPES] == nr.SHAPES
    lay = train_ring.param_layout()
    assert [c for _, c in lay] == sizes and [o for o, _ in lay] == list(np.cumsum([0] + sizes[:-1]))
    lib = _ffi.load()
    assert lib.caelo_ring_train_param_layout(None) == -1
    for h, w, chunk in ((0, 8, 1), (8, 0, 1), (6, 8, 1), (8, 10, 1), (-4, 8, 1), (8, 8, 0), (8, 8, 4097)):
        assert lib.caelo_ring_train_ws_bytes(h, w, chunk) == 0, (h, w, chunk)
    # the saved activations and their gradients alone are 118 floats per pixel
    assert lib.caelo_ring_train_ws_bytes(64, 1792, 2) > 2 * 64 * 1792 * 118 * 4
    out = (C.c_int64 * 4)()
    assert lib.caelo_ring_train_ws_layout(8, 16, 2, C.cast(out, C.c_void_p)) == 0
    assert len(set(out)) == 4 and all(0 < o < lib.caelo_ring_train_ws_bytes(8, 16, 2) for o in out)
    assert lib.caelo_ring_train_ws_layout(8, 18, 2, C.cast(out, C.c_void_p)) == -1 and b"multiple of 4" in lib.caelo_last_error()
    assert (train_ring.LR, train_ring.BETA_1, train_ring.BETA_2, train_ring.EPSILON) == (nr.LR, nr.BETA_1, nr.BETA_2, nr.EPSILON)
    for t in (1, 2, 1000):
        assert train_ring.adam_lr_t(t) == np.float32(nr.adam_lr_t(t))


# ---- the reader --------------------------------------------------------------------------------------------------------------------
def test_read_ring_autoencoder_on_the_fixture():
    from caelo import keras_config
    ws = keras_config.read_ring_autoencoder(nr.FIXTURE)
    assert [w.shape for w in ws] == nr.SHAPES and all(w.dtype == np.float32 and np.isfinite(w).all() for w in ws)
    # its first two layers are the shipped response layer, bit for bit
    kind, rws, _ = keras_config.read_model(RESPOND_H5)
    assert kind == "respond" and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ws[:4], rws))
    # kind_of / read_model are unchanged: a file with Conv2D layers is "respond", and the full autoencoder fails check there
    assert keras_config.kind_of(keras_config.layers(nr.FIXTURE)) == "respond"
    with pytest.raises(ValueError, match="unsupported respond layer stack"):
        keras_config.read_model(nr.FIXTURE)


def _patched(tmp_path, name, old, new):
    raw = open(nr.FIXTURE, "rb").read()
    assert len(old) == len(new) and raw.count(old) >= 1, (old, raw.count(old))
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(raw.replace(old, new, 1))
    return path


def test_read_ring_autoencoder_refuses_everything_else(tmp_path):
    from caelo import keras_config
    with pytest.raises(ValueError, match="layer stack"):
        keras_config.read_ring_autoencoder(RESPOND_H5)
    with pytest.raises(ValueError, match="layer stack"):
        keras_config.read_ring_autoencoder(ENCODER_H5)
    # one field changed in a patched copy of the JSON: conv2d_1's activation, a pooling's padding, conv2d_6's filters
    for name, old, new, field in (("act.h5", b'"activation": "relu"', b'"activation": "tanh"', "activation"),
                                  ("pad.h5", b'"pool_size": [2, 2], "padding": "same"', b'"pool_size": [2, 2], "padding": "full"', "padding"),
                                  ("filters.h5", b'"filters": 3,', b'"filters": 4,', "filters")):
        with pytest.raises(ValueError, match=field):
            keras_config.read_ring_autoencoder(_patched(tmp_path, name, old, new))


# ---- the writers -------------------------------------------------------------------------------------------------------------------
def _new_weights(seed):
    rs = np.random.RandomState(seed)
    return [rs.standard_normal(s).astype(np.float32) for s in nr.SHAPES]


def _spans(path, n):
    from caelo import h5lite
    h = h5lite.H5File(path)
    inside = np.zeros(len(h.buf), bool)
    for i in range(1, n + 1):
        for what in ("kernel", "bias"):
            off, nbytes = h5lite.dataset_span(h, "/model_weights/conv2d_%d/conv2d_%d/%s:0" % (i, i, what))
            assert not inside[off:off + nbytes].any()
            inside[off:off + nbytes] = True
    return inside


def test_written_files_read_back_bit_for_bit_and_change_nothing_else(tmp_path):
    from caelo import keras_config
    ws = _new_weights(7)
    ae, rl = str(tmp_path / "ae.h5"), str(tmp_path / "rl.h5")
    assert keras_config.write_ring_models_like(nr.FIXTURE, ae, ws, out_respond_h5=rl) == (ae, rl)     # the response template: the shipped file
    got = keras_config.read_ring_autoencoder(ae)
    assert all(g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, ws))
    kind, rws, acts = keras_config.read_model(rl)
    assert kind == "respond" and acts is None and all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(rws, ws[:4]))
    for tpl, out, layers, floats in ((nr.FIXTURE, ae, 6, 5835), (RESPOND_H5, rl, 2, 1160)):
        a, b = np.frombuffer(open(tpl, "rb").read(), np.uint8), np.frombuffer(open(out, "rb").read(), np.uint8)
        inside = _spans(tpl, layers)
        assert a.size == b.size and inside.sum() == 4 * floats
        assert np.array_equal(a[~inside], b[~inside]) and not np.array_equal(a[inside], b[inside])
    # the autoencoder alone; flat arrays are taken too
    ae2 = str(tmp_path / "ae2.h5")
    assert keras_config.write_ring_models_like(nr.FIXTURE, ae2, [w.ravel() for w in ws]) == (ae2, None)
    assert open(ae2, "rb").read() == open(ae, "rb").read()


def test_writer_refusals_leave_no_file_behind(tmp_path):
    from caelo import keras_config
    ws = _new_weights(8)
    ae, rl = str(tmp_path / "never_ae.h5"), str(tmp_path / "never_rl.h5")
    with pytest.raises(ValueError, match="12 arrays"):
        keras_config.write_ring_models_like(nr.FIXTURE, ae, ws[:11], out_respond_h5=rl)
    with pytest.raises(ValueError, match="shape"):
        keras_config.write_ring_models_like(nr.FIXTURE, ae, ws[:11] + [np.zeros(4, np.float32)], out_respond_h5=rl)
    with pytest.raises(ValueError, match="shape"):      # a bad array among the four that go into both files
        keras_config.write_ring_models_like(nr.FIXTURE, ae, [np.zeros((3, 3, 3, 31), np.float32)] + ws[1:], out_respond_h5=rl)
    with pytest.raises(ValueError, match="layer stack"):    # templates swapped, or of another network
        keras_config.write_ring_models_like(RESPOND_H5, ae, ws, out_respond_h5=rl)
    with pytest.raises(ValueError, match="layer stack"):
        keras_config.write_ring_models_like(nr.FIXTURE, ae, ws, template_respond_h5=nr.FIXTURE, out_respond_h5=rl)
    with pytest.raises(ValueError):
        keras_config.write_ring_models_like(nr.FIXTURE, ae, ws, template_respond_h5=ENCODER_H5, out_respond_h5=rl)
    with pytest.raises(ValueError, match="activation"):
        keras_config.write_ring_models_like(_patched(tmp_path, "act.h5", b'"activation": "relu"', b'"activation": "tanh"'), ae, ws)
    # a template whose conv2d_4 kernel is stored as [3, 3, 16, 8] x 2: the dataspace's last dimensions changed in the object header
    import struct
    raw = open(nr.FIXTURE, "rb").read()
    pat = struct.pack("<QQQQ", 3, 3, 16, 16)
    assert raw.count(pat) >= 1
    bad = str(tmp_path / "bad_shape.h5")
    with open(bad, "wb") as f:
        f.write(raw.replace(pat, struct.pack("<QQQQ", 3, 3, 32, 8)))
    with pytest.raises(ValueError, match="shape"):
        keras_config.write_ring_models_like(bad, ae, ws, out_respond_h5=rl)
    assert not os.path.exists(ae) and not os.path.exists(rl)


# ---- fit ---------------------------------------------------------------------------------------------------------------------------
class _StubTrainer:
    """Counts what ``fit`` feeds it: ``eng.project`` marks each ring with its scan's id."""

    def __init__(self):
        self.steps, self.evals = [], []
        self.eng = types.SimpleNamespace(device=torch.device("cpu"), project=self._project,
                                         zeros=lambda shape, dtype: torch.zeros(shape, dtype=dtype))

    @staticmethod
    def _project(pc):
        ring = torch.zeros((69, 1800, 5), dtype=torch.float32)
        ring[0, 0, 0] = pc[0, 0]
        return ring, None, torch.zeros(1, dtype=torch.int32)

    def step(self, images, sync=True):
        self.steps.append([int(v) for v in images[:, 0, 0, 0]])
        return torch.tensor([float(len(self.steps))])

    def loss(self, images):
        self.evals.append([int(v) for v in images[:, 0, 0, 0]])
        return 0.5


def _scans(n):
    return [lambda i=i: np.full((3, 4), float(i), np.float32) for i in range(n)]


@pytest.mark.parametrize("files,steps", [(1, 1), (33, 1), (65, 2)])
def test_fit_takes_the_references_steps_per_pass(files, steps):
    """YieldBatchData's strict bound: L training files give (L - 1) // 32 steps per pass, at least one here."""
    from caelo import train_ring
    tr = _StubTrainer()
    hist = train_ring.fit(tr, _scans(files), epochs=2, files_per_step=32, seed=3, train_ratio=1.0, log=None)
    assert len(tr.steps) == 2 * steps and not tr.evals
    assert np.isnan(hist["val_loss"]).all() and hist["val_loss"].shape == (2,)
    order = list(range(files))
    np.random.RandomState(3).shuffle(order)
    for s in range(steps):
        assert tr.steps[s] == order[32 * s:32 * (s + 1)] == tr.steps[steps + s]       # shuffled once, the same pass every epoch
    want = [np.mean(np.arange(e * steps, (e + 1) * steps) + 1.0) for e in range(2)]
    assert np.array_equal(hist["loss"], want)


def test_fit_splits_train_and_validation_and_refuses_an_empty_training_list():
    from caelo import train_ring
    tr = _StubTrainer()
    hist = train_ring.fit(tr, _scans(70), epochs=1, files_per_step=32, seed=0, log=None)
    order = list(range(70))
    np.random.RandomState(0).shuffle(order)
    assert tr.steps == [order[0:32]] and tr.evals == [order[63:70]]        # 63 train: (63 - 1) // 32 = 1 step; 7 validate: one step
    assert hist["val_loss"][0] == 0.5
    with pytest.raises(ValueError, match="no training scans"):
        train_ring.fit(_StubTrainer(), _scans(1), epochs=1, log=None)


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
def test_adam_float32_restatement_follows_its_float64_twin():
    rs = np.random.RandomState(5)
    p64 = rs.standard_normal(nr.N_PARAMS)
    m64, v64 = np.zeros_like(p64), np.zeros_like(p64)
    p32, m32, v32 = p64.astype(np.float32), m64.astype(np.float32), v64.astype(np.float32)
    p64 = p32.astype(np.float64)
    for t in range(1, 11):
        g = (rs.standard_normal(nr.N_PARAMS) * 10.0 ** rs.uniform(-4, 1, size=nr.N_PARAMS)).astype(np.float32)
        p64, m64, v64 = nr.adam_step(p64, g.astype(np.float64), m64, v64, t)
        p32, m32, v32 = nr.adam_step(p32, g, m32, v32, t)
        assert p32.dtype == np.float32
        for what, a, b in (("p", p32, p64), ("m", m32, m64), ("v", v32, v64)):
            rel = np.abs(a - b).max() / np.abs(b).max()
            print("step %d %s: relative %.3g" % (t, what, rel))
            assert rel <= 1e-6
    # the first step moves every parameter by lr against its gradient's sign (m / sqrt(v) = sign(g) before epsilon matters)
    p, m, v = nr.adam_step(np.zeros(4), np.array([3.0, -2.0, 1e-3, -50.0]), np.zeros(4), np.zeros(4), 1)
    assert np.allclose(p, [-1e-3, 1e-3, -1e-3, 1e-3], rtol=1e-2)         # (epsilon costs 0.3 % at |g| = 1e-3)
