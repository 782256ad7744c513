"""The decoder half without a GPU: the layer stack ``keras_config.decoder_model`` accepts and what it refuses, the decoder fixture
(the reference's trained autoencoder, decoder half: tests/golden/autoencoder_decoder_half.md) through ``read_autoencoder``, the weight
fold of UpSampling3D(2) + Conv3D (caelo_host_decoder_fold) against its float64 restatement, and the command line's argument checks.
Two tests check the reference itself (the fold identity and the loss formula's two forms in float64): they run no code of the
library and say so."""
import copy
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import netref64_act as na
import netref64_dec as nd
from conftest import REPO


@pytest.fixture(scope="module")
def fixdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fixture"))


@pytest.fixture(scope="module")
def stack(fixdir):
    from caelo import keras_config
    return keras_config.layers(nd.fixture_h5(fixdir))


def _with(stack, index, **fields):
    lys = copy.deepcopy(stack)
    lys[index][1].update(fields)
    return lys


# ---- the layer stack ----------------------------------------------------------------------------------------------------------------
def test_decoder_model_accepts_both_fixtures_stacks(fixdir, stack):
    """Both fixture files carry the reference file's ``model_config`` bit for bit (17 layers): the decoder starts behind dense_2."""
    from caelo import keras_config
    assert len(stack) == 17 and [c for c, _ in stack[9:]] == [c for c, _ in keras_config.DECODER_SPEC]
    assert keras_config.decoder_model(stack) == (9, ("relu", "sigmoid"))
    assert keras_config.decoder_model(keras_config.layers(na.fixture_h5(fixdir))) == (9, ("relu", "sigmoid"))
    tanh = copy.deepcopy(stack)
    for i in (9, 10, 12, 14):
        tanh[i][1]["activation"] = "tanh"
    assert keras_config.decoder_model(tanh) == (9, ("tanh", "sigmoid"))
    # the encoder's reading of the same stack is what it was
    assert keras_config.encoder_model(stack) == (9, ("relu", "linear"))


@pytest.mark.parametrize("index,fields,words", [
    (16, dict(activation="linear"), ("conv3d_6", "activation", "sigmoid")),
    (16, dict(activation="relu"), ("conv3d_6", "activation", "sigmoid")),
    (12, dict(activation="tanh"), ("conv3d_4", "activation", "all four hidden layers")),
    (10, dict(activation="sigmoid"), ("dense_4", "activation")),
    (13, dict(size=[2, 2, 1]), ("up_sampling3d_1", "size", "[2, 2, 2]")),
    (15, dict(size=[3, 3, 3]), ("up_sampling3d_2", "size")),
    (11, dict(target_shape=[4, 4, 32, 4]), ("reshape_1", "target_shape", "[4, 4, 4, 32]")),
    (11, dict(target_shape=[8, 8, 8, 4]), ("reshape_1", "target_shape")),
    (12, dict(kernel_size=[5, 5, 5]), ("conv3d_4", "kernel_size")),
    (14, dict(strides=[2, 2, 2]), ("conv3d_5", "strides")),
    (14, dict(padding="valid"), ("conv3d_5", "padding")),
    (16, dict(use_bias=False), ("conv3d_6", "use_bias")),
    (16, dict(data_format="channels_first"), ("conv3d_6", "data_format")),
    (9, dict(units=100), ("dense_3", "units")),
    (10, dict(units=1024), ("dense_4", "units")),
    (14, dict(filters=4), ("conv3d_5", "filters")),
])
def test_decoder_model_refuses_and_names_the_field(stack, index, fields, words):
    from caelo import keras_config
    with pytest.raises(ValueError) as e:
        keras_config.decoder_model(_with(stack, index, **fields))
    assert "unsupported decoder" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)


def test_decoder_model_refuses_other_stacks(stack):
    from caelo import keras_config
    with pytest.raises(ValueError, match="bare encoder"):
        keras_config.decoder_model(stack[:9])
    with pytest.raises(ValueError, match="unsupported decoder layer stack"):
        keras_config.decoder_model(stack[:16])
    with pytest.raises(ValueError, match="unsupported decoder layer stack"):
        keras_config.decoder_model(stack[:13] + stack[14:])          # an UpSampling3D missing
    with pytest.raises(ValueError, match="unsupported encoder"):
        keras_config.decoder_model(stack[9:])                        # no encoder in front


def test_read_autoencoder_returns_the_recorded_arrays(fixdir):
    from caelo import keras_config
    enc, eact, dec, dact = keras_config.read_autoencoder(nd.fixture_h5(fixdir))
    assert enc is None and eact == ("relu", "linear") and dact == ("relu", "sigmoid")
    assert [w.shape for w in dec] == nd.DECODER_SHAPES and all(w.dtype == np.float32 for w in dec)
    assert [hashlib.sha256(w.tobytes()).hexdigest() for w in dec] == nd.FIXTURE_SHA256
    enc, eact, dec, dact = keras_config.read_autoencoder(na.fixture_h5(fixdir))
    assert dec is None and eact == ("relu", "linear") and dact == ("relu", "sigmoid")
    assert [hashlib.sha256(w.tobytes()).hexdigest() for w in enc] == na.FIXTURE_SHA256
    # read_model keeps giving the encoder of an autoencoder file, and says so when that half was cut out
    kind, ws, acts = keras_config.read_model(na.fixture_h5(fixdir))
    assert kind == "encoder" and acts == ("relu", "linear") and all(a.tobytes() == b.tobytes() for a, b in zip(ws, enc))
    with pytest.raises(ValueError, match="do not match the encoder architecture"):
        keras_config.read_model(nd.fixture_h5(fixdir))
    from caelo.engine import ENCODER_H5
    with pytest.raises(ValueError, match="bare encoder"):
        keras_config.read_autoencoder(ENCODER_H5)


# ---- the fold -----------------------------------------------------------------------------------------------------------------------
def _fold(w, cin, cout):
    from caelo import _ffi
    w = np.ascontiguousarray(w, np.float32)
    out = np.full((8, 8, cin, cout), np.nan, np.float32)
    rc = _ffi.load().caelo_host_decoder_fold(w.ctypes.data_as(C.c_void_p), cin, cout, out.ctypes.data_as(C.c_void_p))
    return rc, out


@pytest.mark.parametrize("cin,cout,index", [(16, 8, 6), (8, 1, 8)])
def test_host_fold_equals_the_float64_fold_rounded_once(fixdir, cin, cout, index):
    from caelo import keras_config
    dec = keras_config.read_autoencoder(nd.fixture_h5(fixdir))[2]
    for w in (dec[index], nd.decoder_family("biased")[index]):
        rc, got = _fold(w, cin, cout)
        assert rc == 0 and got.tobytes() == nd.fold64(w).astype(np.float32).tobytes()


def test_fold_identity_in_float64():
    """A check of the REFERENCE (tests/netref64_dec.py only, no code of the library): UpSampling3D(2) + Conv3D(3^3, same) == the eight folded 2^3 convolutions on the zero-padded source, borders included."""
    rs = np.random.RandomState(5)
    for size, cin, cout in ((4, 16, 8), (8, 8, 1)):
        x = rs.uniform(-1, 1, size=(3, size, size, size, cin))
        w, b = rs.uniform(-1, 1, size=(3, 3, 3, cin, cout)), rs.uniform(-1, 1, size=cout)
        want = nd._conv(nd.upsample2(x), w, b, np.float64)
        got = nd.folded_upconv(x, nd.fold64(w), b)
        assert np.abs(got - want).max() <= 1e-12


def test_host_fold_argument_errors():
    from caelo import _ffi
    lib = _ffi.load()
    w, out = np.ones(27, np.float32), np.zeros(64, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.caelo_host_decoder_fold(None, 1, 1, p(out)) == -1 and b"caelo_host_decoder_fold" in lib.caelo_last_error()
    assert lib.caelo_host_decoder_fold(p(w), 1, 1, None) == -1
    assert lib.caelo_host_decoder_fold(p(w), 0, 1, p(out)) == -1 and lib.caelo_host_decoder_fold(p(w), 1, 0, p(out)) == -1
    assert not out.any()


def test_fold_unit_links_and_runs_alone(tmp_path):
    """csrc/dec_fold.hip is plain C++ and needs nothing of the library: compiled with tools/micro/dec_fold_main.cpp into a
    stand-alone program and run once (nothing is loaded into Python).  The same two files built with -fsanitize=address,undefined
    are the fold's sanitizer run (the command is in the program's header)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "dec_fold_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-x", "c++", os.path.join(REPO, "tools", "micro", "dec_fold_main.cpp"),
                           os.path.join(REPO, "cae-lo_amd", "csrc", "dec_fold.hip"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0 and b"dec_fold ok" in r.stdout, r.stdout.decode()


# ---- the loss -----------------------------------------------------------------------------------------------------------------------
def test_loss_formula_equals_softplus_of_the_clipped_logit():
    """A check of the REFERENCE and of the kernel's formula on paper (tests/netref64_dec.py only, no code of the library): Keras clips the probability to [1e-7, 1 - 1e-7]; the sigmoid is monotone, so that is a clip of the logit to +-logit(1 - 1e-7),
    and -log p = softplus(-z), -log(1 - p) = softplus(z): the form the kernel evaluates, here in float64 against the pinned formula."""
    rs = np.random.RandomState(9)
    z = np.concatenate([rs.uniform(-140, 30, size=(7, 4096)), np.zeros((1, 4096))])
    y = (rs.uniform(size=z.shape) < 0.3).astype(np.float64)
    zc = np.clip(z, -nd.LOGIT_CLIP, nd.LOGIT_CLIP)
    t = np.where(y > 0, -zc, zc)
    soft = (np.maximum(t, 0) + np.log1p(np.exp(-np.abs(t)))).mean(axis=1)
    want = nd.bce(nd.sigmoid(z), y)
    assert np.abs(soft - want).max() <= 1e-9 * want.max()
    assert abs(nd.LOGIT_CLIP - 16.11809555) < 1e-7


# ---- the command line ---------------------------------------------------------------------------------------------------------------
_CLI = ["reconstruction", "--autoencoder-h5", "x.h5", "--out", "o.mat"]


@pytest.mark.parametrize("argv,message", [
    (_CLI + ["--synthetic", "3", "--threshold", "1.0"], "--threshold must lie in (0, 1)"),
    (_CLI + ["--synthetic", "3", "--threshold", "nan"], "--threshold must lie in (0, 1)"),
    (_CLI + ["--synthetic", "3", "--every", "0"], "--every and --synthetic must be >= 1"),
    (_CLI + ["--synthetic", "0"], "--every and --synthetic must be >= 1"),
    (_CLI, "one of the arguments --scans --synthetic is required"),
    (_CLI + ["--synthetic", "3", "--scans", "d"], "not allowed with argument --synthetic"),
    (["reconstruction", "--synthetic", "3", "--out", "o.mat"], "--autoencoder-h5"),
])
def test_reconstruction_arguments_are_checked_before_any_device_work(argv, message, capsys):
    """Each refusal by its own message (an unknown subcommand would exit with the same status)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("caelo_evaluate_cli", os.path.join(REPO, "cae-lo_amd", "evaluate.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and message in err and "invalid choice" not in err, err
