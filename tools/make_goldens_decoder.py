#!/usr/bin/env python3
"""Write tests/golden/autoencoder_decoder_half.h5 (as two parts): the reference's trained AUTOENCODER file with the ENCODER's weights
dropped -- the counterpart of tools/make_goldens_activations.py, made the same way.

Needs h5py and the reference's file (make_goldens_activations.SRC); run with an interpreter that has h5py:
    PYTHONDONTWRITEBYTECODE=1 python3 tools/make_goldens_decoder.py
(the tests read the result with caelo.h5lite and need neither.)  The copy keeps, bit for bit,
  * the root attributes ``model_config``, ``keras_version``, ``backend``,
  * ``/model_weights``' attributes, ``layer_names`` among them (all 17 layers),
  * the groups and datasets of the five decoder layers that own weights: dense_3, dense_4, conv3d_4, conv3d_5, conv3d_6;
the five encoder layers conv3d_1 .. conv3d_3, dense_1, dense_2 keep their group with an EMPTY ``weight_names``.  Before anything is
written the project's loader (caelo.keras_config.read_autoencoder) must return identical decoder arrays and activations from the
unmodified source and from the copy.

A committed file may not exceed 1 MiB and Dense(2048)'s kernel alone is 1.6 MB, so the copy is stored as its first PART_BYTES bytes
(``autoencoder_decoder_half.h5.part0``) and the rest (``.part1``); tests/netref64_dec.py::fixture_h5 joins them again and checks the
SHA-256 of the whole file.  The hashes (file, and each of the ten arrays) go into tests/golden/autoencoder_decoder_half.md.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_goldens_activations import SRC, GOLDEN, PART_BYTES, ENCODER_LAYERS, _copy_attrs  # noqa: E402

NAME = "autoencoder_decoder_half.h5"
DECODER_LAYERS = ("dense_3", "dense_4", "conv3d_4", "conv3d_5", "conv3d_6")
ARRAY_NAMES = [l + "/" + k for l in DECODER_LAYERS for k in ("kernel", "bias")]
DECODER_SHAPES = [(20, 200), (200,), (200, 2048), (2048,), (3, 3, 3, 32, 16), (16,), (3, 3, 3, 16, 8), (8,), (3, 3, 3, 8, 1), (1,)]


def write_copy(path):
    import h5py
    with h5py.File(SRC, "r") as s, h5py.File(path, "w", libver="earliest") as d:
        _copy_attrs(s, d)
        mw = d.create_group("model_weights")
        _copy_attrs(s["model_weights"], mw)
        for ln in s["model_weights"].attrs["layer_names"]:
            ln = ln.decode()
            g = s["model_weights"][ln]
            if ln in ENCODER_LAYERS:
                _copy_attrs(g, mw.create_group(ln), empty=("weight_names",))
            else:
                s.copy(g, mw, name=ln)
        for key in ("model_config", "keras_version", "backend"):
            assert d.attrs[key] == s.attrs[key], key
        assert np.array_equal(mw.attrs["layer_names"], s["model_weights"].attrs["layer_names"])
        for ln in DECODER_LAYERS:
            for k in ("kernel:0", "bias:0"):
                a, b = s["model_weights"][ln][ln][k], mw[ln][ln][k]
                assert a.dtype == b.dtype and a[...].tobytes() == b[...].tobytes(), (ln, k)


def main():
    sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
    from caelo import keras_config
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, NAME)
        write_copy(path)
        enc0, eact0, dec0, dact0 = keras_config.read_autoencoder(SRC)
        enc1, eact1, dec1, dact1 = keras_config.read_autoencoder(path)
        assert enc0 is not None and enc1 is None and eact0 == eact1 == ("relu", "linear") and dact0 == dact1 == ("relu", "sigmoid")
        assert len(dec0) == len(dec1) == 10 and all(a.dtype == np.float32 and a.tobytes() == b.tobytes() for a, b in zip(dec0, dec1))
        assert [w.shape for w in dec1] == DECODER_SHAPES
        assert len(keras_config.layers(path)) == 17
        blob = open(path, "rb").read()
    assert PART_BYTES < len(blob) < 2 * PART_BYTES and len(blob) - PART_BYTES <= 1 << 20
    for i, part in enumerate((blob[:PART_BYTES], blob[PART_BYTES:])):
        with open(os.path.join(GOLDEN, "%s.part%d" % (NAME, i)), "wb") as f:
            f.write(part)
    print("%s: %d bytes, sha256 %s" % (NAME, len(blob), hashlib.sha256(blob).hexdigest()))
    for name, w in zip(ARRAY_NAMES, dec1):
        print("  %-16s %-18s %s" % (name, w.shape, hashlib.sha256(w.tobytes()).hexdigest()))


if __name__ == "__main__":
    main()
