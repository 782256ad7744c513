"""The decoder half of the voxel-patch autoencoder (AE4VoxelPatch.py:199-211) in float64 (the exact network) and in plain NumPy
float32 (what float32 arithmetic itself costs: the yardstick the device's per-layer errors are held against) -- a helper module, not a
conftest, the counterpart of tests/netref64_act.py:

    code [20] -> Dense(200) -> Dense(2048) -> Reshape(4,4,4,32) -> Conv3D(16) -> UpSampling3D(2) -> Conv3D(8) -> UpSampling3D(2)
    -> Conv3D(1, sigmoid)

hidden activation in {relu, tanh} on the four hidden layers, sigmoid on the output.  Also Keras's ``binary_crossentropy`` as the
float64 formula the loss is pinned to (Keras itself is not available: SURVEY.md 8c), the float64 fold of UpSampling3D(2) + Conv3D into
eight parity classes of 2^3 taps, seeded weight families, and the fixture model: tests/golden/autoencoder_decoder_half.h5 is stored
in two parts (a committed file may not exceed 1 MiB); ``fixture_h5`` joins them and checks the whole file's SHA-256, ``FIXTURE_SHA256``
are the ten arrays' (tests/golden/autoencoder_decoder_half.md).
"""
import hashlib
import os

import numpy as np

import netref64 as nr
import netref64_act as na

GOLDEN = na.GOLDEN
FIXTURE_NAME = "autoencoder_decoder_half.h5"
FIXTURE_FILE_SHA256 = "67b2a241b2760112ad809247c78f151f9a1e4846445aac8025dda84c636fabf4"
FIXTURE_SHA256 = [   # dense_3, dense_4, conv3d_4 .. conv3d_6: kernel, bias
    "0dd254c7cc136cdff3d765a131fd5feb8ebe9912810c2ad78fc79f3bf07ff229", "9a8f1559afa26601ef3389493830df6872ea4402dc6ba8257f6e8be454cbc690",
    "31e25223f7dd67dbd30b32827bf75512a5ce21ab99b730575be68cc0043dbf87", "7fd5ec9156b37f97715116c6a5ebd4440f875b22905bb1ae40a2facbf4ef2786",
    "c51aff0f876ece33bc7c1fc8c04495936385ff6ace27a9c5fd2307313f8b1078", "4b6175267eaacf9ecfdf4c6b468fdab659771dd25b4a09db4d123d7a9c7d8dc3",
    "434f8bdc691579d833d2dbc3cf1db1efb36aa3997356c4680facb9a9e6227c06", "ec7ee35c3ad16c9923fc804b1537dd6bdb57fd43bd0fee75d86cafa0a7046076",
    "61e155203b120b38a8537385186fb5096d4bafddd2bfb6ce2083f39387005b1b", "9da9289cddc0de8e8f3a20661ca29f60919edcbf65354c7979a107a2c7d73ef4",
]
DECODER_SHAPES = [(20, 200), (200,), (200, 2048), (2048,), (3, 3, 3, 32, 16), (16,), (3, 3, 3, 16, 8), (8,), (3, 3, 3, 8, 1), (1,)]
ACTS = na.ACTS
EPS = 1e-7                                         # Keras backend epsilon: binary_crossentropy clips p to [EPS, 1 - EPS]
LOGIT_CLIP = float(np.log((1 - EPS) / EPS))        # the same clip on the logit


def fixture_h5(directory):
    """Join the decoder fixture's two parts into ``directory`` -> the path of the .h5 (written once per directory)."""
    path = os.path.join(str(directory), FIXTURE_NAME)
    if not os.path.exists(path):
        blob = b"".join(open(os.path.join(GOLDEN, "%s.part%d" % (FIXTURE_NAME, i)), "rb").read() for i in (0, 1))
        assert hashlib.sha256(blob).hexdigest() == FIXTURE_FILE_SHA256
        with open(path, "wb") as f:
            f.write(blob)
    return path


# ---- layers -------------------------------------------------------------------------------------------------------------------
def _conv(x, w, b, dtype, chunk=64):
    """Conv3D 3^3, stride 1, zero 'same' padding, channels last, in ``dtype``: float64 as one matrix product over (tap, input
    channel), float32 tap by tap in the kernel's order (netref64_act.encoder_layers' two forms), ``chunk`` patches at a time."""
    out = np.empty(x.shape[:-1] + (w.shape[-1],), dtype)
    sp = x.shape[1:4]
    for i in range(0, len(x), chunk):
        xp = np.pad(x[i:i + chunk], [(0, 0), (1, 1), (1, 1), (1, 1), (0, 0)])
        wins = [xp[(slice(None),) + tuple(slice(t, t + s) for t, s in zip(tap, sp))] for tap in np.ndindex(3, 3, 3)]
        if dtype == np.float64:
            out[i:i + chunk] = np.concatenate(wins, axis=-1) @ w.reshape(-1, w.shape[-1]) + b
        else:
            acc = np.zeros(xp.shape[:1] + sp + (w.shape[-1],), dtype)
            for win, tap in zip(wins, np.ndindex(3, 3, 3)):
                acc += win @ w[tap]
            out[i:i + chunk] = acc + b
    return out


def upsample2(x):
    """UpSampling3D(2), channels last: nearest neighbour, voxel u of the result = voxel u >> 1 of the source."""
    return x.repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)


def sigmoid(z):
    """1 / (1 + exp(-z)) in z's dtype (exp may overflow to inf for z < -88 in float32: the quotient is then 0, as on the device)."""
    with np.errstate(over="ignore"):
        return (1 / (1 + np.exp(-z))).astype(z.dtype)


def decoder_layers(ws, codes, activations, dtype=np.float64):
    """codes [n,20] -> (h3 [n,200], G4 [n,2048], Y4 [n,1024] (4^3 x 16), Y5 [n,4096] (8^3 x 8), z [n,4096] (16^3 logits, x, y, z order)),
    the four hidden layers activated, in ``dtype`` arithmetic (float32: every product, sum and activation in float32, NumPy's order)."""
    assert activations[1] == "sigmoid"
    h = ACTS[activations[0]]
    k = [np.asarray(w, dtype).reshape(s) for w, s in zip(ws, DECODER_SHAPES)]
    x = np.asarray(codes, dtype)
    n = len(x)
    h3 = h(x @ k[0] + k[1])
    g4 = h(h3 @ k[2] + k[3])
    y4 = h(_conv(g4.reshape(n, 4, 4, 4, 32), k[4], k[5], dtype))
    y5 = h(_conv(upsample2(y4), k[6], k[7], dtype))
    z = _conv(upsample2(y5), k[8], k[9], dtype)
    assert z.dtype == dtype
    return h3, g4, y4.reshape(n, -1), y5.reshape(n, -1), z.reshape(n, -1)


def bce(p, target):
    """Keras binary_crossentropy on a sigmoid output, per patch, in p's dtype: mean over the voxels of -(y log p^ + (1 - y) log(1 - p^)),
    p^ = clip(p, 1e-7, 1 - 1e-7).  p, target [n,4096]."""
    dt = p.dtype.type
    ph = np.clip(p, dt(EPS), dt(1) - dt(EPS))
    y = np.asarray(target, p.dtype)
    return (-(y * np.log(ph) + (dt(1) - y) * np.log(dt(1) - ph))).mean(axis=1, dtype=p.dtype)


def dense_target(bits):
    """[n,64] u64 -> [n,4096] f64 in (x, y, z) order."""
    return nr.unpack(bits).reshape(len(bits), -1)


def pack(dense):
    """bool [n,4096] in (x, y, z) order -> [n,64] u64 (netref64.unpack's layout)."""
    return np.packbits(np.asarray(dense, bool).reshape(len(dense), -1), axis=1, bitorder="little").view("<u8").reshape(len(dense), 64)


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8).reshape(len(words), -1), axis=1).sum(axis=1).astype(np.int64)


# ---- the fold -----------------------------------------------------------------------------------------------------------------
def fold64(w):
    """w [3,3,3,cin,cout] -> [8,8,cin,cout] f64: class p (x*4+y*2+z) of output voxel 2s + p, offset o: source cell s + o + p - 1; the taps t
    with ((p + t - 1) >> 1) - (p - 1) == o per axis summed in float64, ascending."""
    w = np.asarray(w, np.float64).reshape(3, 3, 3, *np.shape(w)[-2:])
    out = np.zeros((8, 8) + w.shape[3:], np.float64)
    for p in range(8):
        pa = (p >> 2, (p >> 1) & 1, p & 1)
        for t in np.ndindex(3, 3, 3):
            oa = [((pp + tt - 1) >> 1) - (pp - 1) for pp, tt in zip(pa, t)]
            out[p, oa[0] * 4 + oa[1] * 2 + oa[2]] += w[t]
    return out


def folded_upconv(x, folded, b):
    """UpSampling3D(2) + Conv3D(3^3, same) of x [n,s,s,s,cin] through the fold -> [n,2s,2s,2s,cout] PRE-activations, f64."""
    n, s = x.shape[0], x.shape[1]
    xp = np.pad(np.asarray(x, np.float64), [(0, 0), (1, 1), (1, 1), (1, 1), (0, 0)])
    out = np.zeros((n, 2 * s, 2 * s, 2 * s, folded.shape[-1]), np.float64)
    for p in range(8):
        pa = (p >> 2, (p >> 1) & 1, p & 1)
        acc = 0.0
        for o in range(8):
            oa = (o >> 2, (o >> 1) & 1, o & 1)
            sl = tuple(slice(oo + pp, oo + pp + s) for oo, pp in zip(oa, pa))    # cell s + o + p - 1, +1 for the padding
            acc = acc + xp[(slice(None),) + sl] @ folded[p, o]
        out[:, pa[0]::2, pa[1]::2, pa[2]::2] = acc
    return out + np.asarray(b, np.float64)


# ---- the models of the tests --------------------------------------------------------------------------------------------------
def decoder_family(name):
    """-> the ten float32 arrays of a decoder (Keras shapes, kernel then bias per layer): ``glorot`` glorot_uniform kernels, all biases 0;
    ``biased`` glorot_uniform kernels, every bias U(-0.5, 0.5)."""
    return nr._glorot_set(DECODER_SHAPES, {"glorot": 301, "biased": 302}[name], {"glorot": 0.0, "biased": 0.5}[name])


# (name, encoder weights, encoder activations, decoder weights, decoder activations)
MODELS = (("fixture", "fixture", ("relu", "linear"), "fixture", ("relu", "sigmoid")),
          ("glorot_tanh", "glorot0", ("tanh", "tanh"), "glorot", ("tanh", "sigmoid")),
          ("biased_relu", "biased", ("relu", "linear"), "biased", ("relu", "sigmoid")))


def model(name, directory):
    """-> (encoder ws, encoder activations, decoder ws, decoder activations) of one of MODELS."""
    _, enc, eact, dec, dact = next(m for m in MODELS if m[0] == name)
    if enc == "fixture":
        from caelo import keras_config
        ews, e_acts, none, _ = keras_config.read_autoencoder(na.fixture_h5(directory))
        none2, _, dws, d_acts = keras_config.read_autoencoder(fixture_h5(directory))
        assert none is None and none2 is None and e_acts == eact and d_acts == dact
        return ews, eact, dws, dact
    return nr.encoder_family(enc), eact, decoder_family(dec), dact


def patches(name):
    """The patches a model is tested on: test_patches() (582) for the trained model, its 70 edge patches + 64 of the others for a family."""
    bits = na.test_patches()
    return bits if name == "fixture" else np.ascontiguousarray(np.concatenate([bits[:70], bits[70::8][:64]]))


_cache = {}


def reference(name, directory):
    """Computed once per model and shared (callers must not modify it): dict with bits [n,64], codes [n,20] f32 (the float64 encoder's
    codes, cast), target [n,4096] f64, ``l64`` / ``l32`` = decoder_layers in float64 / float32, ``p64`` / ``p32`` = sigmoid of their
    logits, ``loss64`` / ``loss32`` = bce of those."""
    if name not in _cache:
        ews, eact, dws, dact = model(name, directory)
        bits = patches(name)
        codes = na.encoder_layers(ews, bits, eact)[0][3].astype(np.float32)
        l64, l32 = decoder_layers(dws, codes, dact), decoder_layers(dws, codes, dact, np.float32)
        tgt = dense_target(bits)
        p64, p32 = sigmoid(l64[4]), sigmoid(l32[4])
        _cache[name] = dict(bits=bits, codes=codes, target=tgt, l64=l64, l32=l32, p64=p64, p32=p32, loss64=bce(p64, tgt), loss32=bce(p32, tgt),
                            ews=ews, eact=eact, dws=dws, dact=dact)
    return _cache[name]
