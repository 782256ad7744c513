"""The layer stack recorded in a Keras ``.h5`` (root attribute ``model_config``) -- parsed, never assumed.

The reference obtains its two networks with ``keras.models.load_model(path)`` (Dirs.py:29-30, Match.py:313,324), which
rebuilds the layers from this JSON.  ``check`` compares every semantic field of every layer (kernel size, strides, padding,
dilation, data format, activation, bias, pooling, units, input shape) with the stack the shipped files hold and refuses
anything else, so a different ``.h5`` can never be run silently through the wrong arithmetic.

The encoder kernels implement that one stack with two activation sets (``encoder_model``): a hidden activation H in
{tanh, relu} on conv3d_1..3 and dense_1 alike, and a code activation C in {tanh, linear} on dense_2.  The shipped
EncoderModel4VoxelPatch.h5 is (tanh, tanh); the reference's training script (AE4VoxelPatch.py:177-197) builds (relu, linear).
A file may be the bare encoder or a full autoencoder whose first layers, up to the first Dense(20) behind Flatten, are it.
"""
import json

import numpy as np

from .h5lite import H5File

# what ring.hip::k_respond and encoder.hip / config5.hip implement
_CONV = dict(padding="same", data_format="channels_last", use_bias=True)
RESPOND_SPEC = [
    ("InputLayer", dict(batch_input_shape=[None, 64, 1792, 3])),
    ("Conv2D", dict(_CONV, filters=32, kernel_size=[3, 3], strides=[1, 1], dilation_rate=[1, 1], activation="relu")),
    ("Conv2D", dict(_CONV, filters=8, kernel_size=[1, 1], strides=[1, 1], dilation_rate=[1, 1], activation="relu")),
]
_C3 = dict(_CONV, kernel_size=[3, 3, 3], strides=[1, 1, 1], dilation_rate=[1, 1, 1], activation="tanh")
_POOL = dict(pool_size=[2, 2, 2], strides=[2, 2, 2], padding="same", data_format="channels_last")
ENCODER_SPEC = [
    ("InputLayer", dict(batch_input_shape=[None, 16, 16, 16, 1])),
    ("Conv3D", dict(_C3, filters=8)), ("MaxPooling3D", _POOL),
    ("Conv3D", dict(_C3, filters=16)), ("MaxPooling3D", _POOL),
    ("Conv3D", dict(_C3, filters=32)),
    ("Flatten", dict(data_format="channels_last")),
    ("Dense", dict(units=200, activation="tanh", use_bias=True)),
    ("Dense", dict(units=20, activation="tanh", use_bias=True)),
]


# what decoder.hip implements: the suffix of an autoencoder behind the encoder's Dense(20) (AE4VoxelPatch.py:199-211)
_UP = dict(size=[2, 2, 2], data_format="channels_last")
DECODER_SPEC = [
    ("Dense", dict(units=200, activation="relu", use_bias=True)),
    ("Dense", dict(units=2048, activation="relu", use_bias=True)),
    ("Reshape", dict(target_shape=[4, 4, 4, 32])),
    ("Conv3D", dict(_C3, filters=16, activation="relu")), ("UpSampling3D", _UP),
    ("Conv3D", dict(_C3, filters=8, activation="relu")), ("UpSampling3D", _UP),
    ("Conv3D", dict(_C3, filters=1, activation="sigmoid")),
]
DECODER_OUT_ACTIVATIONS = ("sigmoid",)    # conv3d_6
_DEC_ACTIVATED = [i for i, (c, _) in enumerate(DECODER_SPEC) if c in ("Conv3D", "Dense")]
DECODER_SIZES = [4000, 200, 409600, 2048, 13824, 16, 3456, 8, 216, 1]   # dense_3, dense_4, conv3d_4 .. conv3d_6: kernel, bias


HIDDEN_ACTIVATIONS = ("tanh", "relu")     # conv3d_1, conv3d_2, conv3d_3, dense_1: one of these, the same on all four
CODE_ACTIVATIONS = ("tanh", "linear")     # dense_2
_ACTIVATED = [i for i, (c, _) in enumerate(ENCODER_SPEC) if c in ("Conv3D", "Dense")]


def _norm(v):
    return list(v) if isinstance(v, (list, tuple)) else v


def layers(path_or_h5):
    """-> [(class_name, config dict)] of a Keras Model / Sequential ``.h5`` in execution order (linear stacks only)."""
    h = path_or_h5 if isinstance(path_or_h5, H5File) else H5File(path_or_h5)
    cfg = json.loads(h.attrs("/")["model_config"].decode("utf8"))
    lys = cfg["config"]["layers"] if isinstance(cfg["config"], dict) else cfg["config"]
    out = []
    for i, l in enumerate(lys):
        inbound = l.get("inbound_nodes") or []
        if i > 0 and inbound:   # functional Model: every layer must consume exactly its predecessor
            srcs = [n[0] for n in inbound[0]]
            if srcs != [lys[i - 1]["config"]["name"]]:
                raise ValueError("model_config is not a linear stack at layer %s" % l["config"].get("name"))
        out.append((l["class_name"], l["config"]))
    return out


def kind_of(lys):
    classes = [c for c, _ in lys]
    if "Conv2D" in classes:
        return "respond"
    if "Conv3D" in classes:
        return "encoder"
    raise ValueError("not one of the two CAE-LO inference models (layers: %s)" % classes)


def check(lys, kind=None):
    """Raise ValueError unless the stack is exactly the one the kernels implement; returns 'respond' | 'encoder'."""
    kind = kind or kind_of(lys)
    spec = RESPOND_SPEC if kind == "respond" else ENCODER_SPEC
    if [c for c, _ in lys] != [c for c, _ in spec]:
        raise ValueError("unsupported %s layer stack %s (kernels implement %s)" % (kind, [c for c, _ in lys], [c for c, _ in spec]))
    for (cls, cfg), (_, want) in zip(lys, spec):
        for key, val in want.items():
            # Keras 2.2 writes Flatten.data_format / InputLayer shapes; an absent optional field means the Keras default
            got = cfg.get(key, "channels_last" if key == "data_format" else None)
            if _norm(got) != _norm(val):
                raise ValueError("unsupported %s: %s(%s).%s = %r, the kernels implement %r" % (kind, cls, cfg.get("name"), key, got, val))
    return kind


def encoder_model(lys):
    """The encoder inside a linear Conv3D stack -> (number of leading layers that are the encoder, (H, C)).

    ``lys`` is a bare encoder (every layer is used) or a full autoencoder: then the prefix up to and including the first
    ``Dense(20)`` behind ``Flatten`` must be the encoder stack and the rest (the decoder) is ignored.  ValueError, in ``check``'s
    words, for everything the kernels do not implement: hidden activations that differ from each other, any activation outside
    ``HIDDEN_ACTIVATIONS`` / ``CODE_ACTIVATIONS``, other kernel sizes, strides, paddings, units."""
    classes = [c for c, _ in lys]
    if "Conv3D" not in classes:
        raise ValueError("not a voxel-patch encoder (layers: %s)" % classes)
    cut = None
    if "Flatten" in classes:
        for i in range(classes.index("Flatten") + 1, len(lys)):
            if classes[i] == "Dense" and lys[i][1].get("units") == 20:
                cut = i + 1
                break
    want = [c for c, _ in ENCODER_SPEC]
    if cut is None or classes[:cut] != want:
        raise ValueError("unsupported encoder layer stack %s (kernels implement %s, alone or followed by a decoder)" % (classes, want))
    head = lys[:cut]
    acts = [head[i][1].get("activation") for i in _ACTIVATED]
    hidden, code = acts[0], acts[-1]
    for i, a in zip(_ACTIVATED[:-1], acts[:-1]):
        if a not in HIDDEN_ACTIVATIONS or a != hidden:
            raise ValueError("unsupported encoder: %s(%s).activation = %r, the kernels implement one of %r on all four hidden layers (%s has %r)"
                             % (head[i][0], head[i][1].get("name"), a, HIDDEN_ACTIVATIONS, head[_ACTIVATED[0]][1].get("name"), hidden))
    if code not in CODE_ACTIVATIONS:
        raise ValueError("unsupported encoder: Dense(%s).activation = %r, the kernels implement one of %r for the code"
                         % (head[-1][1].get("name"), code, CODE_ACTIVATIONS))
    for (cls, cfg), (_, spec) in zip(head, ENCODER_SPEC):
        for key, val in spec.items():
            if key == "activation":
                continue
            got = cfg.get(key, "channels_last" if key == "data_format" else None)
            if _norm(got) != _norm(val):
                raise ValueError("unsupported encoder: %s(%s).%s = %r, the kernels implement %r" % (cls, cfg.get("name"), key, got, val))
    return cut, (hidden, code)


def decoder_model(lys):
    """The decoder inside a full autoencoder -> (index of its first layer, (hidden, out)).

    ``lys`` is a linear Conv3D stack whose prefix is the encoder (``encoder_model``); the layers that follow its ``Dense(20)`` must be
    ``Dense(200)``, ``Dense(2048)``, ``Reshape([4,4,4,32])``, ``Conv3D(16)``, ``UpSampling3D([2,2,2])``, ``Conv3D(8)``,
    ``UpSampling3D([2,2,2])``, ``Conv3D(1)``.  ValueError, in ``check``'s words, for everything the kernels do not implement: a bare
    encoder, hidden activations that differ from each other or lie outside ``HIDDEN_ACTIVATIONS``, an output activation outside
    ``DECODER_OUT_ACTIVATIONS``, other kernel sizes, strides, paddings, units, up-sampling sizes or target shapes."""
    cut, _ = encoder_model(lys)
    tail = lys[cut:]
    classes, want = [c for c, _ in tail], [c for c, _ in DECODER_SPEC]
    if not tail:
        raise ValueError("unsupported decoder: the file holds a bare encoder (layers: %s), the kernels implement %s behind it"
                         % ([c for c, _ in lys], want))
    if classes != want:
        raise ValueError("unsupported decoder layer stack %s (kernels implement %s)" % (classes, want))
    acts = [tail[i][1].get("activation") for i in _DEC_ACTIVATED]
    hidden, out = acts[0], acts[-1]
    for i, a in zip(_DEC_ACTIVATED[:-1], acts[:-1]):
        if a not in HIDDEN_ACTIVATIONS or a != hidden:
            raise ValueError("unsupported decoder: %s(%s).activation = %r, the kernels implement one of %r on all four hidden layers (%s has %r)"
                             % (tail[i][0], tail[i][1].get("name"), a, HIDDEN_ACTIVATIONS, tail[_DEC_ACTIVATED[0]][1].get("name"), hidden))
    if out not in DECODER_OUT_ACTIVATIONS:
        raise ValueError("unsupported decoder: Conv3D(%s).activation = %r, the kernels implement %r for the output"
                         % (tail[-1][1].get("name"), out, DECODER_OUT_ACTIVATIONS[0]))
    for (cls, cfg), (_, spec) in zip(tail, DECODER_SPEC):
        for key, val in spec.items():
            if key == "activation":
                continue
            got = cfg.get(key, "channels_last" if key == "data_format" else None)
            if _norm(got) != _norm(val):
                raise ValueError("unsupported decoder: %s(%s).%s = %r, the kernels implement %r" % (cls, cfg.get("name"), key, got, val))
    return cut, (hidden, out)


def _layer_weights(h, names, keep):
    ws = []
    for ln in names:
        if ln not in keep:
            continue
        for wn in h.attrs("/model_weights/" + ln).get("weight_names", []):
            ws.append(np.ascontiguousarray(h.dataset("/model_weights/%s/%s" % (ln, wn.decode())), np.float32))
    return ws


def read_autoencoder(path):
    """-> (encoder ws [10], (H, C), decoder ws [10], (hidden, out)) from a Keras 2.2 autoencoder .h5.  Both halves of the layer stack
    are compared field by field with what the kernels implement (``encoder_model``, ``decoder_model``) before a weight is read.
    A half whose layers are all stored with an empty ``weight_names`` (a file cut down to the other half, as the test fixtures are)
    comes back as None; a half that is there in part, or in other shapes, is a ValueError."""
    h = H5File(path)
    lys = layers(h)
    cut, enc_acts = encoder_model(lys)
    _, dec_acts = decoder_model(lys)
    names = [n.decode() for n in h.attrs("/model_weights")["layer_names"]]
    enc = _layer_weights(h, names, {cfg["name"] for _, cfg in lys[:cut]}) or None
    dec = _layer_weights(h, names, {cfg["name"] for _, cfg in lys[cut:]}) or None
    if enc is not None and [w.size for w in enc] != [216, 8, 3456, 16, 13824, 32, 409600, 200, 4000, 20]:
        raise ValueError("%s: weight shapes %s do not match the encoder architecture" % (path, [w.shape for w in enc]))
    if dec is not None and [w.size for w in dec] != DECODER_SIZES:
        raise ValueError("%s: weight shapes %s do not match the decoder architecture" % (path, [w.shape for w in dec]))
    return enc, enc_acts, dec, dec_acts


def read_model(path):
    """-> ("respond", [w1,b1,w2,b2], None) or ("encoder", [10 arrays], (H, C)) from a Keras 2.2 .h5 file.  The layer stack is read
    from the file's ``model_config`` and compared field by field with what the kernels implement: the response layer exactly
    (``check``), the encoder up to its two activation sets (``encoder_model``; a full autoencoder gives its encoder half, and only
    those five layers' datasets are read).  Any other activation / padding / stride / data format / shape is refused before a
    weight is read."""
    h = H5File(path)
    lys = layers(h)
    kind = kind_of(lys)
    activations, keep = None, None
    if kind == "respond":
        check(lys, kind)
    else:
        cut, activations = encoder_model(lys)
        keep = {cfg["name"] for _, cfg in lys[:cut]}
    names = [n.decode() for n in h.attrs("/model_weights")["layer_names"]]
    ws = []
    for ln in names:
        if keep is not None and ln not in keep:
            continue
        for wn in h.attrs("/model_weights/" + ln).get("weight_names", []):
            ws.append(np.ascontiguousarray(h.dataset("/model_weights/%s/%s" % (ln, wn.decode())), np.float32))
    want = [864, 32, 256, 8] if kind == "respond" else [216, 8, 3456, 16, 13824, 32, 409600, 200, 4000, 20]
    if [w.size for w in ws] != want:
        raise ValueError("%s: weight shapes %s do not match the %s architecture" % (path, [w.shape for w in ws], kind))
    return kind, ws, activations


def _weight_paths(h, keep=None):
    """The dataset path of every weight of the layers named in ``keep`` (None: all of them), in the file's ``layer_names`` x
    ``weight_names`` order."""
    for ln in [n.decode() for n in h.attrs("/model_weights")["layer_names"]]:
        if keep is None or ln in keep:
            for wn in h.attrs("/model_weights/" + ln).get("weight_names", []):
                yield "/model_weights/%s/%s" % (ln, wn.decode())


def _weight_datasets(h, keep):
    """-> [(dataset path, (offset, nbytes), shape)] of ``_weight_paths(h, keep)``: what a writer needs.  H5Error for storage that is
    not contiguous little-endian float32 (``dataset_span``); the writers turn it into their ValueError."""
    from .h5lite import dataset_span
    return [(p, dataset_span(h, p), tuple(h.dataset_info(p)[0])) for p in _weight_paths(h, keep)]


def _patched(h, sets, ws):
    """-> the bytes of ``h``'s file with the datasets ``sets`` overwritten by the arrays ``ws`` (their shapes or flat); ValueError for an
    array of another shape.  Nothing is written."""
    buf = bytearray(h.buf)
    for (p, (off, nbytes), s), w in zip(sets, ws):
        a = np.ascontiguousarray(w, dtype="<f4")
        if a.shape != s and a.shape != (int(np.prod(s)),):
            raise ValueError("%s: array of shape %s for a dataset of shape %s" % (p, a.shape, s))
        raw = a.tobytes()
        assert len(raw) == nbytes
        buf[off:off + nbytes] = raw
    return bytes(buf)


def autoencoder_datasets(h):
    """-> ([(dataset path, (offset, nbytes), shape)] of the encoder half, the same of the decoder half) of an autoencoder ``H5File``, in
    ``read_autoencoder``'s order; a half stored with empty ``weight_names`` gives an empty list."""
    lys = layers(h)
    cut, _ = encoder_model(lys)
    decoder_model(lys)
    return [_weight_datasets(h, {cfg["name"] for _, cfg in half}) for half in (lys[:cut], lys[cut:])]


def write_autoencoder_like(template_h5, out_h5, ews, dws, activations=None):
    """Write trained weights as a Keras file without an HDF5 writer: ``out_h5`` is a byte copy of ``template_h5`` with the values of its
    weight datasets overwritten in place -- the 10 encoder arrays ``ews`` and the 10 decoder arrays ``dws`` (Keras shapes or flat; the
    20 tensors of the network).  Nothing else in the file changes: layer names, ``model_config`` -- so the activations are the
    template's, and a trainer's activation set must equal its template's -- and ``training_config``; the ``optimizer_weights`` group
    of the template, if it has one, stays as it is and is STALE for the new weights (Keras reads it only to resume training).  A
    template that was cut down to one half (empty ``weight_names`` on the other: the test fixtures) takes that half only, and the other
    argument may be None.  Refused with ValueError BEFORE anything is written: a dataset that is not contiguous little-endian float32
    with allocated storage, a dataset or an array of another shape, a half given for which the template has no datasets, and --
    ``activations`` = ((H, C), (hidden, out)) of the model the weights were trained as -- a template whose ``model_config`` says
    otherwise."""
    from .h5lite import H5Error
    h = H5File(template_h5)
    try:
        enc, dec = autoencoder_datasets(h)
    except H5Error as e:
        raise ValueError("%s: %s" % (template_h5, e))
    if activations is not None:
        lys = layers(h)
        have = (encoder_model(lys)[1], decoder_model(lys)[1])
        if tuple(tuple(a) for a in activations) != have:
            raise ValueError("%s: the template's activations are %r, the weights were trained with %r" % (template_h5, have, activations))
    from .engine import DECODER_SHAPES, ENCODER_SHAPES
    all_sets, all_ws = [], []
    for what, sets, ws, shapes in (("encoder", enc, ews, ENCODER_SHAPES), ("decoder", dec, dws, DECODER_SHAPES)):
        if not sets and ws is None:
            continue
        if not sets or ws is None:
            raise ValueError("%s: the template holds %s %s datasets and %s given" % (template_h5, "no" if not sets else len(sets), what,
                                                                                      "no arrays are" if ws is None else "arrays are"))
        # Keras stores a Conv3D kernel [3,3,3,cin,cout]; ENCODER_SHAPES / DECODER_SHAPES name those shapes
        if [s for _, _, s in sets] != [tuple(s) for s in shapes]:
            raise ValueError("%s: %s dataset shapes %s, the architecture has %s" % (template_h5, what, [s for _, _, s in sets], list(shapes)))
        if len(ws) != len(shapes):
            raise ValueError("%s weights: %d arrays wanted, got %d" % (what, len(shapes), len(ws)))
        all_sets += sets
        all_ws += list(ws)
    if not all_sets:
        raise ValueError("%s holds no weight datasets" % template_h5)
    raw = _patched(h, all_sets, all_ws)
    with open(out_h5, "wb") as f:
        f.write(raw)
    return out_h5


# ---- the spherical-ring autoencoder (AE4SphericalRingPC.py:129-144), whose first two layers are the response layer -----------------
_C2 = dict(_CONV, strides=[1, 1], dilation_rate=[1, 1], activation="relu")
_POOL2 = dict(pool_size=[2, 2], strides=[2, 2], padding="same", data_format="channels_last")
_UP2 = dict(size=[2, 2], data_format="channels_last")
RING_AE_SPEC = [
    ("InputLayer", dict(batch_input_shape=[None, 64, 1792, 3])),    # (or [None, None, None, 3]: the network is fully convolutional)
    ("Conv2D", dict(_C2, filters=32, kernel_size=[3, 3])),
    ("Conv2D", dict(_C2, filters=8, kernel_size=[1, 1])),
    ("MaxPooling2D", _POOL2),
    ("Conv2D", dict(_C2, filters=16, kernel_size=[3, 3])),
    ("MaxPooling2D", _POOL2),
    ("Conv2D", dict(_C2, filters=16, kernel_size=[3, 3])),
    ("UpSampling2D", _UP2),
    ("Conv2D", dict(_C2, filters=8, kernel_size=[3, 3])),
    ("UpSampling2D", _UP2),
    ("Conv2D", dict(_C2, filters=3, kernel_size=[1, 1], activation="linear")),
]
RING_AE_INPUT_SHAPES = ([None, 64, 1792, 3], [None, None, None, 3])   # what the shipped file records; what its script's Input() says
RING_AE_SHAPES = [(3, 3, 3, 32), (32,), (1, 1, 32, 8), (8,), (3, 3, 8, 16), (16,), (3, 3, 16, 16), (16,), (3, 3, 16, 8), (8,), (1, 1, 8, 3), (3,)]


def check_ring_autoencoder(lys):
    """Raise ValueError unless the stack is exactly ``RING_AE_SPEC``, compared field by field as ``check`` does."""
    if [c for c, _ in lys] != [c for c, _ in RING_AE_SPEC]:
        raise ValueError("unsupported ring autoencoder layer stack %s (the training kernels implement %s)"
                         % ([c for c, _ in lys], [c for c, _ in RING_AE_SPEC]))
    for (cls, cfg), (_, want) in zip(lys, RING_AE_SPEC):
        for key, val in want.items():
            got = cfg.get(key, "channels_last" if key == "data_format" else None)
            ok = _norm(got) in RING_AE_INPUT_SHAPES if key == "batch_input_shape" else _norm(got) == _norm(val)
            if not ok:
                raise ValueError("unsupported ring autoencoder: %s(%s).%s = %r, the training kernels implement %r" % (cls, cfg.get("name"), key, got, val))
        if cls == "UpSampling2D" and cfg.get("interpolation", "nearest") != "nearest":
            raise ValueError("unsupported ring autoencoder: UpSampling2D(%s).interpolation = %r, the training kernels implement 'nearest'"
                             % (cfg.get("name"), cfg.get("interpolation")))


def _conv2d_datasets(h, lys, spec_shapes, what, path):
    """-> ``_weight_datasets`` of the stack's layers; ValueError for storage that is not contiguous little-endian float32 or for other
    shapes than ``spec_shapes``."""
    from .h5lite import H5Error
    try:
        sets = _weight_datasets(h, {cfg["name"] for _, cfg in lys})
    except H5Error as e:
        raise ValueError("%s: %s" % (path, e))
    if [s for _, _, s in sets] != [tuple(s) for s in spec_shapes]:
        raise ValueError("%s: %s dataset shapes %s, the architecture has %s" % (path, what, [s for _, _, s in sets], list(spec_shapes)))
    return sets


def read_ring_autoencoder(path):
    """-> the 12 arrays (conv2d_1 .. conv2d_6, kernel then bias, Keras shapes ``RING_AE_SHAPES``) of an AE4SphericalRingPC.h5.  The
    layer stack is compared field by field with ``RING_AE_SPEC`` before a weight is read; anything else -- the response-layer file,
    an encoder, one changed field -- is a ValueError."""
    h = H5File(path)
    check_ring_autoencoder(layers(h))
    ws = [np.ascontiguousarray(h.dataset(p), np.float32) for p in _weight_paths(h)]
    if [w.shape for w in ws] != RING_AE_SHAPES:
        raise ValueError("%s: weight shapes %s do not match the ring autoencoder's %s" % (path, [w.shape for w in ws], RING_AE_SHAPES))
    return ws


def _default_respond_h5():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "weights", "SphericalRingPCRespondLayer.h5")


def write_ring_models_like(template_ae_h5, out_ae_h5, ws12, template_respond_h5=None, out_respond_h5=None):
    """Write a trained ring autoencoder as the reference saves it (AE4SphericalRingPC.py:169-170) without an HDF5 writer: ``out_ae_h5`` is
    a byte copy of ``template_ae_h5`` with its 12 weight datasets overwritten in place by ``ws12`` (Keras shapes or flat), and -- when
    ``out_respond_h5`` is given -- ``out_respond_h5`` a byte copy of ``template_respond_h5`` (default: the shipped
    weights/SphericalRingPCRespondLayer.h5) with its four datasets overwritten by the first four arrays.  Nothing else in either file
    changes.  Refused with ValueError BEFORE anything is written: a template of another layer stack, a dataset that is not contiguous
    little-endian float32 with allocated storage, a dataset or an array of another shape, another number of arrays."""
    ws12 = list(ws12)
    if len(ws12) != 12:
        raise ValueError("ring autoencoder weights: 12 arrays wanted, got %d" % len(ws12))
    todo = []
    h = H5File(template_ae_h5)
    lys = layers(h)
    check_ring_autoencoder(lys)
    todo.append((h, _conv2d_datasets(h, lys, RING_AE_SHAPES, "ring autoencoder", template_ae_h5), ws12, out_ae_h5))
    if out_respond_h5 is not None:
        template_respond_h5 = template_respond_h5 or _default_respond_h5()
        hr = H5File(template_respond_h5)
        lr = layers(hr)
        if kind_of(lr) != "respond":
            raise ValueError("%s is not a response-layer file" % template_respond_h5)
        check(lr, "respond")
        todo.append((hr, _conv2d_datasets(hr, lr, RING_AE_SHAPES[:4], "response layer", template_respond_h5), ws12[:4], out_respond_h5))
    elif template_respond_h5 is not None:
        raise ValueError("template_respond_h5 given without out_respond_h5")
    for out, raw in [(out, _patched(hh, sets, ws)) for hh, sets, ws, out in todo]:    # both refused or both written
        with open(out, "wb") as f:
            f.write(raw)
    return out_ae_h5, out_respond_h5
