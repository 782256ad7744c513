"""The encoder of tests/netref64.py with its two activations as parameters (a helper module, not a conftest): hidden activation H in
{tanh, relu} on conv3d_1..3 and dense_1, code activation C in {tanh, linear} on dense_2 -- in float64 (the exact network) and in
plain NumPy float32 (what float32 arithmetic itself costs: the yardstick the device's per-layer errors are held against).

Also the fixture model: tests/golden/autoencoder_encoder_half.h5 is stored in two parts (a committed file may not exceed 1 MiB);
``fixture_h5`` joins them and checks the whole file's SHA-256, ``FIXTURE_SHA256`` are the ten arrays' (tests/golden/autoencoder_encoder_half.md).
"""
import hashlib
import os

import numpy as np

import netref64 as nr

GOLDEN = os.path.join(nr.REPO, "tests", "golden")
FIXTURE_NAME = "autoencoder_encoder_half.h5"
FIXTURE_FILE_SHA256 = "afb4a8e54c234ef0a18124428be8d7e930e150c2135b67252e2c41bde40edfc3"
FIXTURE_SHA256 = [   # conv3d_1 .. dense_2: kernel, bias
    "e335f7a6c5673f2f40d17a95e93fc28219a09f5b8279e17efbc9922c7995254c", "a8a42adb6eca9b94212c0899c9845d7e2e214c37c249713360406cb64ff6f796",
    "76089555f7f1be094eadfa335ddfb43c18c878445e2ce174d760f55be6f69c5d", "0c52fcc811cfd896dd81edb14c87adfc40e448bef6a1adf956351e817168f079",
    "3293bef27352a0d0f36eea7085d0e1965784965f2deb9579f6292f07df2b1642", "f6629e75342e0a4f9029435cde021149549ff192aac27858f5d54b438eef38e4",
    "ea70098178b174d7403391824a96ba34fdca7666d95b16ee6db4e533f1603b35", "767c63a681d37e12f8c8a72b2eabb04fdee696058e1b64e9bf2610853eb32bfb",
    "5b0b709158de5627abe025dd263f19a261ba5caa61c2b5ddc00306fa27fe9a58", "da3d40c4564a373d62cb7c56828d0de8fc411d8506d1878c53f65d3d9afc42c2",
]
ACTS = {"tanh": np.tanh, "relu": lambda x: np.maximum(x, 0), "linear": lambda x: x}
COMBINATIONS = (("tanh", "tanh"), ("relu", "linear"), ("relu", "tanh"), ("tanh", "linear"))


def fixture_h5(directory):
    """Join the fixture's two parts into ``directory`` -> the path of the .h5 (written once per directory)."""
    path = os.path.join(str(directory), FIXTURE_NAME)
    if not os.path.exists(path):
        blob = b"".join(open(os.path.join(GOLDEN, "%s.part%d" % (FIXTURE_NAME, i)), "rb").read() for i in (0, 1))
        assert hashlib.sha256(blob).hexdigest() == FIXTURE_FILE_SHA256
        with open(path, "wb") as f:
            f.write(blob)
    return path


def encoder_layers(ws, bits, activations, dtype=np.float64):
    """Bit-packed 16^3 patches [n,64] u64 -> (P2 [n,1024], F3 [n,2048], hidden [n,200], out [n,20]) and, second, the float64
    PRE-activations of P2 (pooled) -- in ``dtype`` arithmetic: float64 is the exact network, float32 evaluates every product, sum and
    activation in float32 (NumPy's order of summation)."""
    h, c = ACTS[activations[0]], ACTS[activations[1]]
    k = [np.asarray(w, dtype) for w in nr._kernels(ws)]
    n = len(bits)

    def conv(x, w, b):   # nr.conv_same in ``dtype``
        sp = x.shape[1:4]
        xp = np.pad(x, [(0, 0), (1, 1), (1, 1), (1, 1), (0, 0)])
        wins = [xp[(slice(None),) + tuple(slice(t, t + s) for t, s in zip(tap, sp))] for tap in np.ndindex(3, 3, 3)]
        if dtype == np.float64:   # exact to ~1e-16 in any order: ONE matrix product over (tap, input channel), several times faster
            return np.concatenate(wins, axis=-1) @ w.reshape(-1, w.shape[-1]) + b
        out = np.zeros(x.shape[:-1] + (w.shape[-1],), dtype)   # float32: tap by tap in the kernel's order, like netref64.conv_same
        for win, tap in zip(wins, np.ndindex(3, 3, 3)):
            out += win @ w[tap]
        return out + b

    p1 = nr.pool2(h(conv(nr.unpack(bits).astype(dtype), k[0], k[1])))
    pre2 = nr.pool2(conv(p1, k[2], k[3]))
    p2 = h(pre2)
    f3 = h(conv(p2, k[4], k[5])).reshape(n, -1)
    hidden = h(f3 @ k[6].reshape(2048, 200) + k[7])
    out = c(hidden @ k[8].reshape(200, 20) + k[9])
    assert out.dtype == dtype
    return (p2.reshape(n, -1), f3, hidden, out), pre2.reshape(n, -1)


def range_bounds(ws, activations):
    """The range guard's recurrence in float64, per channel: b_1[c] = sum |w1[..., c]| + |b1[c]|, b_l[c] = sum_k |w_l[k, c]|
    b_{l-1}[channel of k] + |b_l[c]| (1 behind a tanh layer) -> B_l = max_c b_l[c], l = 1 .. 5."""
    out, prev = [], np.ones(1)
    for l in range(5):
        act = activations[0] if l < 4 else activations[1]
        w, b = np.asarray(ws[2 * l], np.float64), np.asarray(ws[2 * l + 1], np.float64)
        w = np.abs(w).reshape(-1, len(prev), w.shape[-1])        # [positions or taps, input channel, output channel]
        prev = np.ones(len(b)) if act == "tanh" else np.einsum("pkc,k->c", w, prev) + np.abs(b)
        out.append(float(prev.max()))
    return np.array(out)


def relative_error(got, want, floor=0.1):
    """The descriptor criterion of test_gpu_parity._assert_descriptors as a number: max |got - want| / max(|want|, floor)."""
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), floor)).max())


# ---- the models of the GPU tests ------------------------------------------------------------------------------------------------
# (name, weights, activations): the fixture model, and seeded families of netref64 under activations they were not made for.
# Between them every new kernel instantiation runs: relu stage 1 / conv3 with a zero, a positive and a mixed-sign background, and
# the three new (hidden, code) heads.
MODELS = (("fixture", "fixture", ("relu", "linear")), ("glorot0", "glorot0", ("relu", "linear")), ("biased", "biased", ("relu", "linear")),
          ("shipped_b1", "shipped_b1", ("relu", "linear")), ("biased_relu_tanh", "biased", ("relu", "tanh")),
          ("biased_tanh_linear", "biased", ("tanh", "linear")))


def model(name, directory):
    """-> (ten float32 arrays, (H, C)) of one of MODELS; ``directory``: where the fixture's parts are joined."""
    _, family, acts = next(m for m in MODELS if m[0] == name)
    if family == "fixture":
        from caelo import keras_config
        kind, ws, file_acts = keras_config.read_model(fixture_h5(directory))
        assert kind == "encoder" and file_acts == acts
        return ws, acts
    return nr.encoder_family(family), acts


def test_patches():
    """The 70 edge patches of netref64 (empty, full, the two corner voxels, fills of 0.002 / 0.02 / 0.2) and every sixth patch of
    golden frame 0 -> [582, 64] u64."""
    g = np.load(os.path.join(GOLDEN, "frame_0.npz"))["patch_bits"].reshape(-1, 64)
    return np.ascontiguousarray(np.concatenate([nr.edge_patches(70), g[::6]]))
