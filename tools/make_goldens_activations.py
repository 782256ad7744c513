#!/opt/conda/bin/python3.9
"""Write tests/golden/autoencoder_encoder_half.h5 (as two parts): the reference's trained AUTOENCODER file with the decoder's
weights dropped -- a relu / relu / relu / relu / linear encoder inside a 17-layer ``model_config``, the kind of file the reference's
training script (AE4VoxelPatch.py:177-197) leaves behind.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tools/make_goldens_activations.py

(h5py lives in that interpreter; the tests read the result with caelo.h5lite.)  The copy keeps, bit for bit,
  * the root attributes ``model_config``, ``keras_version``, ``backend``,
  * ``/model_weights``' attributes, ``layer_names`` among them (all 17 layers),
  * the groups and datasets of the five encoder layers conv3d_1, conv3d_2, conv3d_3, dense_1, dense_2;
the six decoder layers that own weights (dense_3, dense_4, conv3d_4 .. conv3d_6) keep their group with an EMPTY ``weight_names``.
Before anything is written the project's loader (caelo.keras_config.read_model) must return identical arrays and activations from
the unmodified source and from the copy.

A committed file may not exceed 1 MiB and Dense(200)'s kernel alone is 1.6 MB, so the copy is stored as its first PART_BYTES bytes
(``autoencoder_encoder_half.h5.part0``) and the rest (``.part1``); tests/netref64_act.py::fixture_h5 joins them again and checks the
SHA-256 of the whole file.  The hashes (file, and each of the ten arrays) go into tests/golden/autoencoder_encoder_half.md.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "/root/reference/TrainedModels/AutoencoderModel4VoxelPatch.h5"
GOLDEN = os.path.join(REPO, "tests", "golden")
NAME = "autoencoder_encoder_half.h5"
PART_BYTES = 900000
ENCODER_LAYERS = ("conv3d_1", "conv3d_2", "conv3d_3", "dense_1", "dense_2")
ARRAY_NAMES = [l + "/" + k for l in ENCODER_LAYERS for k in ("kernel", "bias")]


def _copy_attrs(src, dst, empty=()):
    import h5py
    for name in src.attrs:
        aid = h5py.h5a.open(src.id, name.encode())
        raw = src.attrs[name]
        if name in empty:
            dst.attrs.create(name, data=np.zeros((0,), dtype=raw.dtype), dtype=raw.dtype)
        else:
            dst.attrs.create(name, data=raw, dtype=aid.dtype if not isinstance(raw, np.ndarray) else raw.dtype)


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
                s.copy(g, mw, name=ln)
            else:
                _copy_attrs(g, mw.create_group(ln), empty=("weight_names",))
        for key in ("model_config", "keras_version", "backend"):
            assert d.attrs[key] == s.attrs[key], key
        assert np.array_equal(mw.attrs["layer_names"], s["model_weights"].attrs["layer_names"])
        for ln in ENCODER_LAYERS:
            for k in ("kernel:0", "bias:0"):
                a, b = s["model_weights"][ln][ln][k], mw[ln][ln][k]
                assert a.dtype == b.dtype and a[...].tobytes() == b[...].tobytes(), (ln, k)


def main():
    sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
    from caelo import keras_config
    read_keras_model = keras_config.read_model     # (what caelo.engine.read_keras_model calls; needs no torch)
    ENCODER_SHAPES = [(3, 3, 3, 1, 8), (8,), (3, 3, 3, 8, 16), (16,), (3, 3, 3, 16, 32), (32,), (2048, 200), (200,), (200, 20), (20,)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, NAME)
        write_copy(path)
        kind0, ws0, act0 = read_keras_model(SRC)
        kind1, ws1, act1 = read_keras_model(path)
        assert kind0 == kind1 == "encoder" and act0 == act1 == ("relu", "linear"), (kind0, act0, kind1, act1)
        assert len(ws0) == len(ws1) == 10 and all(a.dtype == np.float32 and a.tobytes() == b.tobytes() for a, b in zip(ws0, ws1))
        assert [w.shape for w in ws1] == ENCODER_SHAPES
        assert len(keras_config.layers(path)) == 17
        blob = open(path, "rb").read()
    assert PART_BYTES < len(blob) < 2 * PART_BYTES and len(blob) - PART_BYTES <= 1 << 20
    for i, part in enumerate((blob[:PART_BYTES], blob[PART_BYTES:])):
        with open(os.path.join(GOLDEN, "%s.part%d" % (NAME, i)), "wb") as f:
            f.write(part)
    print("%s: %d bytes, sha256 %s" % (NAME, len(blob), hashlib.sha256(blob).hexdigest()))
    for name, w in zip(ARRAY_NAMES, ws1):
        print("  %-16s %-18s %s" % (name, w.shape, hashlib.sha256(w.tobytes()).hexdigest()))


if __name__ == "__main__":
    main()
