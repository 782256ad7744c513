"""float64 restatement of the two networks, and seeded weight families for them (a helper module, not a conftest).

Written from the layer stacks of ``oracle._ENCODER_STACK`` / ``oracle._RESPOND_STACK`` and SURVEY.md 8a-3 / 8a-6 in plain NumPy,
independent of the C oracle and of the HIP kernels: Keras channels-last, zero 'same' padding, cross-correlation, MaxPooling 2,
Flatten in (x, y, z, c) order.  Every sum is a float64 sum of float64 products of the float32 weights, so against a float32
evaluation of at most a few thousand terms this is the exact network.

Nothing here is stored in files: weights and patches come from fixed seeds (or from the shipped .h5 files).
"""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = os.path.join(REPO, "weights")

ENCODER_SHAPES = [(3, 3, 3, 1, 8), (8,), (3, 3, 3, 8, 16), (16,), (3, 3, 3, 16, 32), (32,), (2048, 200), (200,), (200, 20), (20,)]
RESPOND_SHAPES = [(3, 3, 3, 32), (32,), (1, 1, 32, 8), (8,)]
ENCODER_FAMILIES = ("shipped", "glorot0", "biased", "shipped_b1", "shipped_w1neg", "sat_conv1")
RESPOND_FAMILIES = ("shipped", "glorot0", "biased", "dead", "wide")
BACKGROUND_FAMILIES = ("biased", "shipped_b1", "shipped_w1neg")   # |tanh(b1)| is material


# ---- layers ---------------------------------------------------------------------------------------------------------------
def unpack(bits, size=16):
    """[n, size^3 / 64] u64 -> [n, size, size, size, 1] f64; voxel (x, y, z) = bit lin & 63 of word lin >> 6, lin = (x * size + y) * size + z."""
    b = np.ascontiguousarray(bits, dtype="<u8").view(np.uint8).reshape(len(bits), size ** 3 // 8)
    return np.unpackbits(b, axis=1, bitorder="little").reshape(len(bits), size, size, size, 1).astype(np.float64)


def conv_same(x, w, b):
    """Conv2D / Conv3D, 3^d or 1^d kernel, stride 1, zero 'same' padding, channels last: the PRE-activations, f64."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    nd = w.ndim - 2
    sp = x.shape[1:1 + nd]
    pads = [k // 2 for k in w.shape[:nd]]
    xp = np.pad(x, [(0, 0)] + [(p, p) for p in pads] + [(0, 0)])
    out = np.zeros(x.shape[:-1] + (w.shape[-1],), np.float64)
    for tap in np.ndindex(*w.shape[:nd]):
        win = xp[(slice(None),) + tuple(slice(t, t + s) for t, s in zip(tap, sp))]
        out += win @ w[tap]
    return out + b


def abs_conv_same(x, w, b):
    """Sum of |products| + |bias| of the same convolution: the magnitude a floating-point error bound scales with."""
    return conv_same(np.abs(x), np.abs(w), np.abs(b))


def pool2(x):
    """MaxPooling3D(2), channels last."""
    n, d = x.shape[0], x.shape[1] // 2
    return x.reshape(n, d, 2, d, 2, d, 2, x.shape[-1]).max(axis=(2, 4, 6))


def _kernels(ws):
    ws = [np.asarray(w, np.float64) for w in ws]
    return [ws[0].reshape(3, 3, 3, 1, 8), ws[1], ws[2].reshape(3, 3, 3, 8, 16), ws[3], ws[4].reshape(3, 3, 3, 16, 32), ws[5]] + ws[6:]


def conv1_preact(ws, bits, size=16):
    """conv3d_1's pre-activations [n, size, size, size, 8]."""
    k = _kernels(ws)
    return conv_same(unpack(bits, size), k[0], k[1])


def pooled1(ws, bits, size=16):
    """P1 = MaxPool(tanh(conv3d_1)) [n, size/2, size/2, size/2, 8]."""
    return pool2(np.tanh(conv1_preact(ws, bits, size)))


def occupied_cells(bits, size=16):
    """bool [n, size/2, size/2, size/2]: pooled cells whose 4^3 receptive field (two conv positions, one voxel of halo each side)
    holds a set voxel -- the cells stage 1 evaluates instead of taking the background for granted."""
    v = unpack(bits, size)[..., 0]
    near = conv_same(v[..., None], np.ones((3, 3, 3, 1, 1)), np.zeros(1)) > 0     # conv positions with a voxel in their 3^3 field
    return pool2(near.astype(np.float64))[..., 0] > 0


def _encoder(ws, dense1, bias1, bits, size):
    k = _kernels(ws)
    n = len(bits)
    p1 = pool2(np.tanh(conv_same(unpack(bits, size), k[0], k[1])))
    p2 = pool2(np.tanh(conv_same(p1, k[2], k[3])))
    f3 = np.tanh(conv_same(p2, k[4], k[5])).reshape(n, -1)        # Flatten: (x, y, z, c) == memory order
    hidden = np.tanh(f3 @ np.asarray(dense1, np.float64).reshape(f3.shape[1], 200) + np.asarray(bias1, np.float64))
    out = np.tanh(hidden @ k[8].reshape(200, 20) + k[9])
    return p1, p2.reshape(n, -1), f3, hidden, out


def encoder_layers(ws, bits):
    """Bit-packed 16^3 patches [n,64] u64 -> (P2 [n,1024] after the second pooling, F3 [n,2048] after conv3d_3's tanh, hidden [n,200]
    after Dense(200)'s tanh, out [n,20]), all f64."""
    return _encoder(ws, ws[6], ws[7], bits, 16)[1:]


def encoder32(ws, dense1, bias1, bits):
    """The same stack on bit-packed 32^3 patches [n,512] u64 with ``dense1`` [16384,200] / ``bias1`` [200] as the first dense
    layer -> descriptors [n,20] f64."""
    return _encoder(ws, dense1, bias1, bits, 32)[4]


def encoder32_layers(ws, dense1, bias1, bits):
    """encoder32 with every layer -> (P1 [n,16,16,16,8] after the first pooling, P2 [n,8192], F3 [n,16384], hidden [n,200], out [n,20]),
    all f64."""
    return _encoder(ws, dense1, bias1, bits, 32)


def dense1_32(seed=5):
    """The stand-in dense_1 of the 32^3 encoder WITH a bias: N(0, 1/16384) [16384,200] f32 (the same draw as
    Engine.seeded_dense1_32) and, from the same stream, a bias U(-0.5, 0.5) [200] f32."""
    rs = np.random.RandomState(seed)
    wd1 = (rs.standard_normal((16384, 200)) / 128.0).astype(np.float32)
    return wd1, rs.uniform(-0.5, 0.5, 200).astype(np.float32)


def respond(ws, img, with_magnitude=False):
    """Response layer on one image [64,1792,3]: Conv2D 3x3 same relu 3->32, Conv2D 1x1 relu 32->8 -> [64,1792,8] f64.
    ``with_magnitude``: also M [64,1792,8] = |b2| + sum_c |W2[c,k]| (|b1[c]| + sum |x W1|), the sum of |products| + |bias| through
    both layers (relu is 1-Lipschitz): an f32 evaluation with 27 + 32 = 59 accumulations per output, in any order, fused or
    not, lies within 59 u M (1 + O(u)) of the exact value, u = 2^-24."""
    w1, b1 = np.asarray(ws[0], np.float64).reshape(3, 3, 3, 32), np.asarray(ws[1], np.float64)
    w2, b2 = np.asarray(ws[2], np.float64).reshape(1, 1, 32, 8), np.asarray(ws[3], np.float64)
    x = np.asarray(img, np.float64)[None]
    h = np.maximum(conv_same(x, w1, b1), 0.0)
    out = np.maximum(conv_same(h, w2, b2), 0.0)[0]
    if not with_magnitude:
        return out
    return out, abs_conv_same(abs_conv_same(x, w1, b1), w2, b2)[0]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def edge_patches(n):
    """[n,64] u64, the recipe of test_encoder_edge_patches_and_batch_independence: empty, full, the single voxels at [0,0,0] and
    [15,15,15], then random fill at 0.002 / 0.02 / 0.2 (seed 3)."""
    assert n >= 4
    rs = np.random.RandomState(3)
    bits = np.zeros((n, 64), np.uint64)
    bits[1] = ~np.uint64(0)
    bits[2, 0] = 1
    bits[3, 63] = np.uint64(1) << np.uint64(63)
    for i in range(4, n):
        dense = rs.uniform(size=4096) < rs.choice([0.002, 0.02, 0.2])
        bits[i] = np.packbits(dense, bitorder="little").view(np.uint64)
    return bits


def random_patches32(n, seed=11):
    """[n,512] u64: the empty and the full 32^3 patch, then random fill at 0.002 / 0.02 / 0.2."""
    rs = np.random.RandomState(seed)
    bits = np.zeros((n, 512), np.uint64)
    bits[1] = ~np.uint64(0)
    for i in range(2, n):
        dense = rs.uniform(size=32768) < (0.002, 0.02, 0.2)[i % 3]
        bits[i] = np.packbits(dense, bitorder="little").view(np.uint64)
    return bits


def pack32(dense):
    """bool [n,32,32,32] -> [n,512] u64 (the layout of ``unpack(bits, 32)``)."""
    dense = np.asarray(dense, bool)
    return np.packbits(dense.reshape(len(dense), 32768), axis=1, bitorder="little").view(np.uint64)


def edge_patches32(n):
    """[n,512] u64, n >= 16, deterministic: 0 the empty patch, 1 the full patch, 2 / 3 the single voxels at (0,0,0) / (31,31,31), 4 the
    pair (0,31,0) + (31,0,31), 5..10 the full face planes x = 0, x = 31, y = 0, y = 31, z = 0, z = 31, 11 the full cube minus its outer
    shell, 12 the single voxel at (15,16,16), then random fill at 0.002 / 0.02 / 0.2 in turn (seed 13)."""
    assert n >= 16
    d = np.zeros((n, 32, 32, 32), bool)
    d[1] = True
    d[2, 0, 0, 0] = True
    d[3, 31, 31, 31] = True
    d[4, 0, 31, 0] = d[4, 31, 0, 31] = True
    d[5, 0], d[6, 31] = True, True
    d[7, :, 0], d[8, :, 31] = True, True
    d[9, :, :, 0], d[10, :, :, 31] = True, True
    d[11, 1:31, 1:31, 1:31] = True
    d[12, 15, 16, 16] = True
    rs = np.random.RandomState(13)
    for i in range(13, n):
        d[i] = rs.uniform(size=(32, 32, 32)) < (0.002, 0.02, 0.2)[(i - 13) % 3]
    return pack32(d)


# ---- weight families ------------------------------------------------------------------------------------------------------
def _glorot(rs, shape):
    """Keras glorot_uniform: U(-l, l), l = sqrt(6 / (fan_in + fan_out)), fans = receptive field x channels."""
    field = int(np.prod(shape[:-2]))
    lim = np.sqrt(6.0 / (field * shape[-2] + field * shape[-1]))
    return rs.uniform(-lim, lim, size=shape).astype(np.float32)


def _glorot_set(shapes, seed, bias_range):
    rs = np.random.RandomState(seed)
    ws = []
    for s in shapes:
        if len(s) > 1:
            ws.append(_glorot(rs, s))
        elif bias_range:
            ws.append(rs.uniform(-bias_range, bias_range, size=s).astype(np.float32))
        else:
            ws.append(np.zeros(s, np.float32))
    return ws


_shipped = {}


def _shipped_weights():
    if not _shipped:
        import oracle
        r, e = oracle.load_models(os.path.join(WEIGHTS, "SphericalRingPCRespondLayer.h5"), os.path.join(WEIGHTS, "EncoderModel4VoxelPatch.h5"))
        _shipped["encoder"] = [np.array(w, np.float32).reshape(s) for w, s in zip(e.w, ENCODER_SHAPES)]
        _shipped["respond"] = [np.array(w, np.float32).reshape(s) for w, s in zip((r.w1, r.b1, r.w2, r.b2), RESPOND_SHAPES)]
    return _shipped


def encoder_family(name):
    """-> the ten float32 arrays of an encoder (Keras shapes, kernel then bias per layer).
      shipped        the .h5
      glorot0        glorot_uniform kernels, all biases 0: background exactly 0, an untrained net
      biased         glorot_uniform kernels, every bias U(-0.5, 0.5): material background, 27 distinct C0 border classes
      shipped_b1     shipped with b1 := U(-0.5, 0.5): a trained net's sensitivity with a material background
      shipped_w1neg  shipped with w1 := -|w1|, b1 := 0.4: occupied cells whose pooled value is still the background
      sat_conv1      biased with w1[..., c] = +4 (even c) / -4 (odd c): conv1 pre-activations of +-108 inside the full patch"""
    if name == "shipped":
        return [w.copy() for w in _shipped_weights()["encoder"]]
    if name == "glorot0":
        return _glorot_set(ENCODER_SHAPES, 101, 0.0)
    if name == "biased":
        return _glorot_set(ENCODER_SHAPES, 102, 0.5)
    if name == "shipped_b1":
        ws = encoder_family("shipped")
        ws[1] = np.random.RandomState(103).uniform(-0.5, 0.5, size=8).astype(np.float32)
        return ws
    if name == "shipped_w1neg":
        ws = encoder_family("shipped")
        ws[0] = -np.abs(ws[0])
        ws[1] = np.full(8, 0.4, np.float32)
        return ws
    if name == "sat_conv1":
        ws = encoder_family("biased")
        ws[0][...] = np.where(np.arange(8) % 2 == 0, 4.0, -4.0).astype(np.float32)
        return ws
    raise KeyError(name)


def respond_family(name):
    """-> [w1, b1, w2, b2] float32 of a response layer.
      shipped / glorot0 / biased   as for the encoder
      dead    biased with b1 = -10 and the kernel of conv 1 scaled by 2^-3 (ring images hold metres, up to 70 here: at glorot's
              scale 27 taps reach +41, at an eighth of it +5.2 < 10): every hidden unit is zero, out = relu(b2) everywhere
      wide    biased with output channel c of conv 1 (kernel and bias) scaled by 2^(c - 16): partial sums 31 binades apart"""
    if name == "shipped":
        return [w.copy() for w in _shipped_weights()["respond"]]
    if name == "glorot0":
        return _glorot_set(RESPOND_SHAPES, 201, 0.0)
    if name == "biased":
        return _glorot_set(RESPOND_SHAPES, 202, 0.5)
    if name == "dead":
        ws = respond_family("biased")
        ws[0] = ws[0] * np.float32(0.125)
        ws[1] = np.full(32, -10.0, np.float32)
        return ws
    if name == "wide":
        ws = respond_family("biased")
        scale = np.exp2(np.arange(32) - 16.0).astype(np.float32)
        ws[0] = ws[0] * scale
        ws[1] = ws[1] * scale
        return ws
    raise KeyError(name)
