"""CPU: the encoder's two activation sets, everything that needs no device -- which layer stacks ``keras_config`` accepts and
refuses, the fixture model (the reference's trained relu / linear autoencoder, encoder half: tests/golden/autoencoder_encoder_half.md) through the
project's loader, the range guard ``caelo_host_encoder_range`` against the float64 recurrence restated here, and the guard's
translation unit linked into a stand-alone program."""
import copy
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import netref64 as nr
import netref64_act as na
from conftest import GOLDEN, REPO, WEIGHTS

SHIPPED = os.path.join(WEIGHTS, "EncoderModel4VoxelPatch.h5")


@pytest.fixture(scope="module")
def fixture_path(tmp_path_factory):
    return na.fixture_h5(tmp_path_factory.mktemp("fixture"))


@pytest.fixture(scope="module")
def shipped_layers():
    from caelo import keras_config
    return keras_config.layers(SHIPPED)


def _with_activations(lys, hidden, code):
    """A copy of a bare encoder stack with ``hidden`` (one name, or four) on the hidden layers and ``code`` on dense_2."""
    mod = copy.deepcopy(lys)
    idx = [i for i, (c, _) in enumerate(mod) if c in ("Conv3D", "Dense")]
    hidden = [hidden] * 4 if isinstance(hidden, str) else list(hidden)
    for i, a in zip(idx, hidden + [code]):
        mod[i][1]["activation"] = a
    return mod


# ---- what keras_config accepts --------------------------------------------------------------------------------------------------
def test_shipped_file_is_tanh_tanh(shipped_layers):
    from caelo import keras_config
    assert keras_config.encoder_model(shipped_layers) == (len(shipped_layers), ("tanh", "tanh"))
    assert keras_config.check(shipped_layers) == "encoder"      # the strict form still names the shipped stack


def test_fixture_is_relu_linear_cut_at_dense_2(fixture_path):
    from caelo import keras_config
    lys = keras_config.layers(fixture_path)
    assert len(lys) == 17
    cut, acts = keras_config.encoder_model(lys)
    assert acts == ("relu", "linear") and cut == 9 and lys[cut - 1][1]["name"] == "dense_2" and lys[cut][1]["name"] == "dense_3"


@pytest.mark.parametrize("hidden,code", na.COMBINATIONS)
def test_hand_built_stacks_of_all_four_combinations(shipped_layers, hidden, code):
    from caelo import keras_config
    mod = _with_activations(shipped_layers, hidden, code)
    assert keras_config.encoder_model(mod) == (len(mod), (hidden, code))
    decoder = [("Dense", dict(name="dense_3", units=200, activation=hidden, use_bias=True))]
    assert keras_config.encoder_model(mod + decoder) == (len(mod), (hidden, code))      # ... and with something behind the code


# ---- what it refuses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,code,word", [
    (["relu", "tanh", "relu", "relu"], "linear", "conv3d_2"), (["tanh", "tanh", "tanh", "relu"], "tanh", "dense_1"),
    ("sigmoid", "tanh", "sigmoid"), ("elu", "linear", "elu"), ("linear", "linear", "linear"),
    ("relu", "sigmoid", "sigmoid"), ("relu", "relu", "dense_2"), ("tanh", "elu", "elu")])
def test_other_activations_are_refused(shipped_layers, hidden, code, word):
    from caelo import keras_config
    with pytest.raises(ValueError, match=word):
        keras_config.encoder_model(_with_activations(shipped_layers, hidden, code))


def test_other_stacks_are_refused(shipped_layers, fixture_path):
    from caelo import keras_config
    lys = copy.deepcopy(shipped_layers)
    lys[-1][1]["units"] = 19                                            # a 19-unit code: no Dense(20) behind Flatten
    with pytest.raises(ValueError, match="unsupported encoder layer stack"):
        keras_config.encoder_model(lys)
    full = keras_config.layers(fixture_path)
    with pytest.raises(ValueError, match="unsupported encoder layer stack"):
        keras_config.encoder_model(full[9:])                            # the decoder alone (it has Conv3D layers, and no Flatten)
    with pytest.raises(ValueError, match="unsupported encoder layer stack"):
        keras_config.encoder_model(full[:1] + full[9:])
    for key, bad in (("kernel_size", [5, 5, 5]), ("kernel_size", [1, 1, 1]), ("filters", 7)):
        mod = copy.deepcopy(full)
        mod[3][1][key] = bad
        with pytest.raises(ValueError, match="conv3d_2.*%s" % key):
            keras_config.encoder_model(mod)
    with pytest.raises(ValueError):                                     # the 2D autoencoder's kind of stack: no Conv3D at all
        keras_config.encoder_model([("InputLayer", {}), ("Conv2D", dict(activation="relu")), ("Dense", dict(units=20, activation="linear"))])


def test_a_stack_that_is_not_linear_is_refused(fixture_path, tmp_path):
    """A functional model whose layer consumes something other than its predecessor: refused by ``layers`` before any check.  The
    model_config of the fixture is edited in memory (dense_2 fed by flatten_1) and parsed through the same code path."""
    import json
    from caelo import keras_config
    from caelo.h5lite import H5File
    h = H5File(fixture_path)
    cfg = json.loads(h.attrs("/")["model_config"].decode("utf8"))
    lys = cfg["config"]["layers"]
    assert lys[8]["config"]["name"] == "dense_2" and lys[8]["inbound_nodes"][0][0][0] == "dense_1"
    lys[8]["inbound_nodes"][0][0][0] = "flatten_1"

    class Edited(H5File):
        def __init__(self):
            pass

        def attrs(self, path="/"):
            return {"model_config": json.dumps(cfg).encode("utf8")}

    with pytest.raises(ValueError, match="not a linear stack"):
        keras_config.layers(Edited())


def test_shipped_file_padding_and_stride_errors_read_as_before(shipped_layers):
    """The messages of the strict check and of the encoder description are the same words for a wrong padding or stride."""
    from caelo import keras_config
    for key, bad, text in (("padding", "valid", "unsupported encoder: Conv3D(conv3d_1).padding = 'valid', the kernels implement 'same'"),
                           ("strides", [3, 3, 3], "unsupported encoder: Conv3D(conv3d_1).strides = [3, 3, 3], the kernels implement [1, 1, 1]")):
        mod = copy.deepcopy(shipped_layers)
        assert mod[1][1]["name"] == "conv3d_1"
        mod[1][1][key] = bad
        for fn in (keras_config.check, keras_config.encoder_model):
            with pytest.raises(ValueError) as e:
                fn(mod)
            assert str(e.value) == text


def test_the_2d_autoencoder_stays_refused():
    """AE4SphericalRingPC.h5 is a Conv2D autoencoder whose first two layers are the response layer; taking a prefix is the encoder's
    rule only.  Its class list and filters are restated here (the file itself is not a fixture)."""
    from caelo import keras_config
    conv = dict(padding="same", data_format="channels_last", use_bias=True, strides=[1, 1], dilation_rate=[1, 1], activation="relu")
    stack = [("Conv2D", 32, 3), ("Conv2D", 8, 1), ("MaxPooling2D", 0, 0), ("Conv2D", 16, 3), ("MaxPooling2D", 0, 0), ("Conv2D", 16, 3),
             ("UpSampling2D", 0, 0), ("Conv2D", 8, 3), ("UpSampling2D", 0, 0), ("Conv2D", 3, 1)]
    lys = [("InputLayer", dict(batch_input_shape=[None, 64, 1792, 3]))]
    lys += [(c, dict(conv, filters=f, kernel_size=[k, k]) if c == "Conv2D" else {}) for c, f, k in stack]
    assert keras_config.kind_of(lys) == "respond"
    with pytest.raises(ValueError, match="unsupported respond layer stack"):
        keras_config.check(lys)
    with pytest.raises(ValueError):
        keras_config.encoder_model(lys)


# ---- the fixture through the loader ---------------------------------------------------------------------------------------------
def test_fixture_weights_have_the_recorded_hashes(fixture_path):
    from caelo import keras_config
    kind, ws, acts = keras_config.read_model(fixture_path)
    assert kind == "encoder" and acts == ("relu", "linear") and len(ws) == 10
    assert [w.shape for w in ws] == nr.ENCODER_SHAPES and all(w.dtype == np.float32 for w in ws)
    assert [hashlib.sha256(w.tobytes()).hexdigest() for w in ws] == na.FIXTURE_SHA256
    readme = open(os.path.join(GOLDEN, "autoencoder_encoder_half.md")).read()
    assert all(h in readme for h in na.FIXTURE_SHA256) and na.FIXTURE_FILE_SHA256 in readme
    kind, ws, acts = keras_config.read_model(SHIPPED)
    assert kind == "encoder" and acts == ("tanh", "tanh") and all(np.array_equal(a, b) for a, b in zip(ws, nr.encoder_family("shipped")))


def test_fixture_descriptors_discriminate(fixture_path):
    """The model is trained: distinct patches get distinct descriptors with a spread of order 1 per dimension, and float32 arithmetic
    stays a long way inside the descriptor bar (the premise of the GPU test's 1e-4)."""
    from caelo import keras_config
    ws = keras_config.read_model(fixture_path)[1]
    g = np.load(os.path.join(GOLDEN, "frame_0.npz"))
    bits = np.unique(g["patch_bits"].reshape(-1, 64), axis=0)[::6]
    (_, _, _, out), _ = na.encoder_layers(ws, bits, ("relu", "linear"))
    assert len(np.unique(np.round(out, 6), axis=0)) == len(bits) and out.std(axis=0).min() > 0.1
    (_, _, _, out32), _ = na.encoder_layers(ws, bits, ("relu", "linear"), np.float32)
    assert na.relative_error(out32, out) <= 2.5e-5


# ---- the range guard --------------------------------------------------------------------------------------------------------------
def _range(ws, acts):
    """caelo_host_encoder_range through ctypes, without a device."""
    import ctypes as C
    from caelo import _ffi
    from caelo.engine import ACTIVATION_CODES
    ws = [np.ascontiguousarray(w, np.float32) for w in ws]
    out = (C.c_double * 5)()
    rc = _ffi.load().caelo_host_encoder_range(*([w.ctypes.data_as(C.c_void_p) for w in ws] + [ACTIVATION_CODES[acts[0]], ACTIVATION_CODES[acts[1]], C.cast(out, C.c_void_p)]))
    return rc, np.array(out, np.float64)


def test_range_of_the_fixture_equals_the_float64_recurrence(fixture_path):
    from caelo import keras_config
    from caelo.engine import Engine
    ws = keras_config.read_model(fixture_path)[1]
    rc, got = _range(ws, ("relu", "linear"))
    want = na.range_bounds(ws, ("relu", "linear"))
    print(got)
    assert rc == 0 and np.all(np.abs(got - want) <= 1e-12 * want)
    assert np.allclose(got, [2.85, 31.8, 510.0, 23190.0, 437269.0], rtol=2e-3)      # the figures of DESIGN.md 9d
    assert got[:3].max() < 65504 / 100                                               # the bounds that bind: two decades to spare
    bounds, over = Engine.encoder_range(ws, ("relu", "linear"))
    assert over is None and np.array_equal(bounds, got)
    for acts in (("relu", "tanh"), ("tanh", "linear"), ("tanh", "tanh")):
        rc, got = _range(ws, acts)
        want = na.range_bounds(ws, acts)
        assert rc == 0 and np.all(np.abs(got - want) <= 1e-12 * want)


@pytest.mark.parametrize("family", nr.ENCODER_FAMILIES)
def test_a_tanh_hidden_stack_is_never_refused(family):
    ws = nr.encoder_family(family)
    rc, got = _range(ws, ("tanh", "tanh"))
    assert rc == 0 and np.array_equal(got, np.ones(5))
    rc, got = _range(ws, ("tanh", "linear"))
    assert rc == 0 and np.array_equal(got[:4], np.ones(4)) and abs(got[4] - na.range_bounds(ws, ("tanh", "linear"))[4]) <= 1e-12 * got[4]


def over_range_family():
    """glorot0 with conv3d_2's kernel scaled by 1e4: sum |w2| per output channel is ~1e5, so P2 can exceed the f16 range under relu."""
    ws = nr.encoder_family("glorot0")
    ws[2] = ws[2] * np.float32(1e4)
    return ws


def test_an_over_range_relu_family_is_reported():
    from caelo import _ffi
    from caelo.engine import Engine
    ws = over_range_family()
    rc, got = _range(ws, ("relu", "linear"))
    want = na.range_bounds(ws, ("relu", "linear"))
    assert rc == 2 and got[0] <= 65504 < got[1] and np.all(np.abs(got - want) <= 1e-12 * want)
    msg = _ffi.load().caelo_last_error().decode()
    assert "conv3d_2" in msg and "65504" in msg
    assert Engine.encoder_range(ws, ("relu", "tanh"))[1] == "conv3d_2"
    assert _range(ws, ("tanh", "tanh"))[0] == 0 and _range(ws, ("tanh", "linear"))[0] == 0
    with pytest.raises(ValueError):
        Engine.encoder_range(ws, ("linear", "tanh"))
    with pytest.raises(ValueError):
        Engine.encoder_range(ws, ("relu", "relu"))


def test_guard_unit_links_and_runs_alone(tmp_path):
    """csrc/enc_range.hip is plain C++ and needs nothing of the library: compiled with tools/micro/enc_range_main.cpp into a
    stand-alone program and run once (nothing is loaded into Python).  The same two files built with -fsanitize=address,undefined
    are the guard's sanitizer run (the command is in the program's header)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "enc_range_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-x", "c++", os.path.join(REPO, "tools", "micro", "enc_range_main.cpp"),
                           os.path.join(REPO, "cae-lo_amd", "csrc", "enc_range.hip"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0 and b"enc_range ok" in r.stdout, r.stdout.decode()
