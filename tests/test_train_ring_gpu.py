"""The ring autoencoder's training kernels (csrc/train_ring.hip) against the torch-CPU autograd network of tests/netref64_ring.py: loss
and gradient on the three models of netref64_ring.MODELS, the full-size image read in place from projected rings, strides,
determinism and chunking, the pooling rule, the Adam kernel bit for bit, ten optimizer steps, the round trip into the key-point
detector and two .h5 files, the refusals.

Bars (DESIGN 9f's, derived here, not fixed).  Keras cannot run here, so everything is pinned to the float64 torch network.  Per tensor
t, max |g_dev - g64| / max |g64| <= 4 x max(e32_t, E): e32_t the float32 torch network's own error on that tensor and batch, E the
median of e32_t over the tensors that have a scale (a tensor whose float64 gradient is identically zero must be zero exactly and
stays out of the median).  Loss: relative error <= 4 x max(e32, 2e-6), 2e-6 being 32 float32 ulps; the reconstruction and the
response layer's output A2: max abs error / max |.| <= 4 x max(e32, 2e-6) with their own e32.  The engine of these tests is private.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import netref64_ring as nr

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOOR = 2e-6
SENTINEL = 0x5A
REPO = os.path.dirname(nr.HERE)
RESPOND_H5 = os.path.join(REPO, "weights", "SphericalRingPCRespondLayer.h5")
SHAPES = [(4, 4, 1, 1), (4, 8, 3, 2), (8, 16, 5, 2), (12, 20, 4, 3), (16, 36, 4, 4), (16, 36, 5, 2)]


@pytest.fixture(scope="module")
def eng(engine):   # (the session fixture first: it skips without a GPU)
    from caelo.engine import Engine
    return Engine(device=0)


def _rel(g, g64):
    """max |g - g64| / max |g64|; a tensor whose float64 gradient is zero everywhere must be zero exactly: 0 when it is, inf when not."""
    top = np.abs(g64).max()
    if top == 0:
        return 0.0 if not np.any(g) else np.inf
    return float(np.abs(np.asarray(g, np.float64) - g64).max() / top)


def _median(e32, g64):
    return float(np.median([e for e, g in zip(e32, g64) if np.any(g)]))


_refs = {}


def _ref(name, key, x):
    """The float64 and float32 torch networks' loss, gradients and tensors on batch ``x``: computed once per (model, key), shared."""
    if (name, key) not in _refs:
        ws = nr.model(name)
        l64, g64, x64 = nr.loss_and_grads(ws, x)
        l32, g32, x32 = nr.loss_and_grads(ws, x, torch.float32)
        e32 = np.array([_rel(a, b) for a, b in zip(g32, g64)])
        _refs[(name, key)] = dict(ws=ws, x=x, l64=l64, g64=g64, x64=x64, e32=e32, E=_median(e32, g64), l32=abs(l32 - l64) / l64,
                                  r32=_rel(x32["r"], x64["r"]), a32=_rel(x32["a2"], x64["a2"]))
    return _refs[(name, key)]


def _trainer(eng, ws, chunk):
    from caelo.train_ring import RingTrainer
    return RingTrainer(eng, ws, chunk=chunk)


def _ws_tensors(eng, tr, h, w, rows):
    """What the last chunk left in the workspace -> (A2 [rows,h,w,8], r [rows,h,w,3], dL/dP1 [rows,h/2,w/2,8], dL/dr [rows,h,w,3]) f64."""
    lay = (C.c_int64 * 4)()
    assert eng.lib.caelo_ring_train_ws_layout(h, w, tr.chunk, C.cast(lay, C.c_void_p)) == 0
    ws = eng._ws("train_ring", tr.ws_bytes(h, w))
    shapes = ((rows, h, w, 8), (rows, h, w, 3), (rows, h // 2, w // 2, 8), (rows, h, w, 3))
    return tuple(ws[int(o):int(o) + 4 * int(np.prod(s))].view(torch.float32).view(s).cpu().numpy().astype(np.float64) for o, s in zip(lay, shapes))


def _check(R, loss, grads, what):
    rel = abs(loss - R["l64"]) / R["l64"]
    bar = FACTOR * max(R["l32"], FLOOR)
    print("%s: loss %.9g (f64 %.9g) relative %.3g, bar %.3g (f32 network %.3g)" % (what, loss, R["l64"], rel, bar, R["l32"]))
    worst = []
    for t, (g, g64) in enumerate(zip(grads, R["g64"])):
        err = _rel(g, g64)
        tb = FACTOR * max(R["e32"][t], R["E"])
        print("  tensor %2d %-14s error %.3g, bar %.3g (f32 network %.3g, median %.3g)" % (t, nr.SHAPES[t], err, tb, R["e32"][t], R["E"]))
        if not err <= tb:
            worst.append((t, err, tb))
    assert rel <= bar
    assert not worst, "%s: tensors beyond their bars (index, error, bar): %s" % (what, worst)


def _check_tensors(R, recon, a2, rows, what):
    """The reconstruction of the whole batch and the last chunk's A2 against the float64 network."""
    for name, got, want, f32 in (("recon", recon, R["x64"]["r"], R["r32"]), ("A2", a2, R["x64"]["a2"][len(R["x"]) - rows:], R["a32"])):
        err = np.abs(got - want).max() / np.abs(R["x64"]["r" if name == "recon" else "a2"]).max()
        bar = FACTOR * max(f32, FLOOR)
        print("%s %s: error %.3g, bar %.3g (f32 network %.3g)" % (what, name, err, bar, f32))
        assert err <= bar


# ---- gradient and loss parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,n,chunk", SHAPES)
@pytest.mark.parametrize("name", nr.MODELS)
def test_gradient_parity(eng, name, h, w, n, chunk):
    R = _ref(name, (h, w, n), nr.images(n, h, w, seed=h))
    tr = _trainer(eng, R["ws"], chunk)
    loss, grads = tr.grad(R["x"])
    rows = n - (n - 1) // chunk * chunk
    a2 = _ws_tensors(eng, tr, h, w, rows)[0]
    _check(R, loss, grads, "%s %dx%d n=%d chunk=%d" % (name, h, w, n, chunk))
    recon = tr.predict(R["x"]).cpu().numpy().astype(np.float64)
    _check_tensors(R, recon, a2, rows, name)


def test_gradient_parity_on_windows_of_a_projected_ring(eng):
    """Real geometry instead of noise: 16 x 36 windows of frame 0's and frame 1's ring, cut where the ring has returns."""
    from caelo import synth
    from caelo.train_ring import ring_batch
    rings = ring_batch(eng, [synth.make_scan(f, quantum=1e-3) for f in (0, 1)]).cpu().numpy()
    x = np.stack([nr.ring_window(r, 16, 36) for r in rings])
    R = _ref("shipped", "ring windows", x)
    loss, grads = _trainer(eng, R["ws"], 2).grad(x)
    _check(R, loss, grads, "shipped, ring windows")


# ---- full size, once ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rings(eng):
    from caelo import synth
    from caelo.train_ring import ring_batch
    return ring_batch(eng, [synth.make_scan(f, quantum=1e-3) for f in (0, 1)])


def test_full_size_rings_read_in_place(eng, rings):
    x = np.ascontiguousarray(rings[:, :64, :1792, :3].cpu().numpy())
    R = _ref("shipped", "full", x)
    bits = []
    for chunk in (1, 2):
        tr = _trainer(eng, R["ws"], chunk)
        loss, grads = tr.grad(rings)                 # [2, 69, 1800, 5]: read through the strides, no crop copy
        a2 = _ws_tensors(eng, tr, 64, 1792, chunk)[0]
        _check(R, loss, grads, "shipped 64x1792 n=2 chunk=%d" % chunk)
        _check_tensors(R, tr.predict(rings).cpu().numpy().astype(np.float64), a2, chunk, "chunk=%d" % chunk)
        bits.append(np.float32(loss).tobytes())
    assert bits[0] == bits[1]


# ---- strides -----------------------------------------------------------------------------------------------------------------------
def _raw_grad(eng, tr, t, n, h, w, strides):
    from caelo.engine import _ptr
    ws = eng._ws("train_ring", tr.ws_bytes(h, w))
    assert eng.lib.caelo_ring_autoencoder_grad(eng.ctx, _ptr(tr.params), _ptr(t), n, h, w, strides[0], strides[1], strides[2], tr.chunk,
                                               _ptr(tr.grads), _ptr(tr._loss), None, _ptr(ws), eng.stream) == 0
    return tr._loss.cpu().numpy().copy(), tr.grads.cpu().numpy().copy()


def test_a_window_of_a_larger_tensor_gives_the_bits_of_the_contiguous_batch(eng):
    x = nr.images(3, 8, 16, seed=8)
    big = np.full((3, 11, 24, 5), 777.0, np.float32)          # what lies outside the window must never be read into a sum
    big[:, :8, :16, :3] = x
    tr = _trainer(eng, nr.model("biased"), 2)
    l0, g0 = _raw_grad(eng, tr, torch.from_numpy(x).to(eng.device), 3, 8, 16, (8 * 16 * 3, 16 * 3, 3))
    l1, g1 = _raw_grad(eng, tr, torch.from_numpy(big).to(eng.device), 3, 8, 16, (11 * 24 * 5, 24 * 5, 5))
    assert l0.tobytes() == l1.tobytes() and np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    l2, g2 = tr.grad(x)
    assert np.float32(l2).tobytes() == l0.tobytes() and np.array_equal(np.concatenate([g.ravel() for g in g2]).view(np.uint32), g0.view(np.uint32))


# ---- determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nr.MODELS)
def test_same_call_same_bits_and_chunks_agree(eng, name):
    R = _ref(name, (8, 16, 5), nr.images(5, 8, 16, seed=8))
    tr = _trainer(eng, R["ws"], 2)
    l0, g0 = tr.grad(R["x"])
    l1, g1 = tr.grad(R["x"])
    assert np.float32(l0).tobytes() == np.float32(l1).tobytes()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(g0, g1))
    assert np.float32(tr.loss(R["x"])).tobytes() == np.float32(l0).tobytes()       # forward only: the loss bits of the full call
    l5, g5 = _trainer(eng, R["ws"], 5).grad(R["x"])
    _check(R, l5, g5, "%s 8x16 n=5 chunk=5" % name)
    assert np.float32(l5).tobytes() == np.float32(l0).tobytes()                    # the loss bits depend on (n, h, w) alone
    print("gradient bits equal across chunk 2 / 5: %s" % [bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))) for a, b in zip(g0, g5)])


# ---- the pooling rule --------------------------------------------------------------------------------------------------------------
def _tie_model_and_batch():
    """conv2d_1's channel 0 copies the input's channel 0 (centre tap), conv2d_2's channel 0 copies that: A2[..., 0] = relu(x[..., 0]).
    The input's channel 0 has period 2, positive, with equal maxima inside every pooling window: image 0 tied along x in the odd rows
    (first maximum (1, 0)), image 1 tied along y in the odd columns ((0, 1)), image 2 constant ((0, 0)), image 3 tied on the diagonal
    ((0, 0) before (1, 1)).  The other 31 channels of conv2d_1 see the noise of channels 1 and 2, so A1 differs between the tied cells
    and conv2d_2's kernel gradient depends on which of them the gradient went to."""
    ws = [w.copy() for w in nr.model("biased")]
    ws[0][:, :, :, 0] = 0.0
    ws[0][1, 1, 0, 0] = 1.0
    ws[1][0] = 0.0
    ws[2][0, 0, :, 0] = 0.0
    ws[2][0, 0, 0, 0] = 1.0
    ws[3][0] = 0.0
    x = nr.images(4, 8, 12, seed=3)
    x[:, :, :, 1:][x[:, :, :, 1:] == 0] = 1.5       # (no empty pixels here: every A1 value differs between neighbours)
    yy, xx = np.meshgrid(np.arange(8), np.arange(12), indexing="ij")
    x[0, :, :, 0] = 3.0 + (yy % 2)
    x[1, :, :, 0] = 3.0 + (xx % 2)
    x[2, :, :, 0] = 4.0
    x[3, :, :, 0] = np.where((yy % 2) == (xx % 2), 5.0, 2.0)
    return ws, x


def _route(a2, dp1, last=False):
    """dL/dA2 [n,h,w,c] from A2 and dL/dP1 by the rule under test in NumPy: the window's first (``last``: last) maximum in ascending
    (dy, dx) order takes the gradient, times relu'."""
    n, h, w, c = a2.shape
    win = a2.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    arg = 3 - np.argmax(win[..., ::-1], axis=-1) if last else np.argmax(win, axis=-1)
    out = np.zeros_like(win)
    np.put_along_axis(out, arg[..., None], (dp1 * (win.max(axis=-1) > 0))[..., None], axis=-1)
    return out.reshape(n, h // 2, w // 2, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)


def test_pooling_gradient_goes_to_the_first_maximum(eng):
    ws, x = _tie_model_and_batch()
    l64, g64, x64 = nr.loss_and_grads(ws, x)
    l32, g32, x32 = nr.loss_and_grads(ws, x, torch.float32)
    a2 = x64["a2"]
    win = a2[..., 0].reshape(4, 4, 2, 6, 2).transpose(0, 1, 3, 2, 4).reshape(4, 4, 6, 4)
    ties = (win == win.max(axis=-1, keepdims=True)).sum(axis=-1)
    assert (win.max(axis=-1) > 0).all() and [int(t.min()) for t in ties] == [2, 2, 4, 2]      # the ties exist in the float64 network
    assert np.array_equal(_route(a2, x64["dp1"]) != 0, x64["da2"] != 0)                        # _route restates torch's rule
    e32 = np.array([_rel(a, b) for a, b in zip(g32, g64)])
    E = _median(e32, g64)
    tr = _trainer(eng, ws, 4)
    loss, grads = tr.grad(x)
    a2_dev, _, dp1_dev, _ = _ws_tensors(eng, tr, 8, 12, 4)
    f32 = _rel(x32["dp1"], x64["dp1"])
    err = _rel(dp1_dev, x64["dp1"])
    print("dL/dP1: error %.3g, bar %.3g (f32 network %.3g, median of the tensors %.3g)" % (err, FACTOR * max(f32, E), f32, E))
    assert err <= FACTOR * max(f32, E)
    # the device's dL/dP1 routed through the device's A2 by the rule lands on torch's cells
    assert np.array_equal(_route(a2_dev, dp1_dev) != 0, x64["da2"] != 0)
    # conv2d_2's kernel gradient is the sum of A1 x dL/dA2: routed to the LAST maximum instead it would differ by far more than the bar
    k0, k1 = (torch.tensor(w, dtype=torch.float64) for w in ws[:2])
    a1 = torch.relu(nr._conv(torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), k0, k1)).permute(0, 2, 3, 1).numpy()
    first = np.einsum("nyxk,nyxc->kc", a1, _route(a2, x64["dp1"]))
    last = np.einsum("nyxk,nyxc->kc", a1, _route(a2, x64["dp1"], last=True))
    assert _rel(first, g64[2][0, 0]) <= 1e-12
    bar = FACTOR * max(e32[2], E)
    print("conv2d_2 kernel gradient: device error %.3g, bar %.3g; the last-maximum rule would be off by %.3g" % (_rel(grads[2], g64[2]), bar, _rel(last, g64[2][0, 0])))
    assert _rel(last, g64[2][0, 0]) > 100 * bar
    for t, (g, w) in enumerate(zip(grads, g64)):
        assert _rel(g, w) <= FACTOR * max(e32[t], E), t


# ---- the Adam kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_kernel_is_bit_equal_to_the_float32_restatement(eng, t):
    from caelo.engine import _ptr
    n = nr.N_PARAMS
    rs = np.random.RandomState(40 + t)
    p = rs.standard_normal(n).astype(np.float32)
    g = (rs.standard_normal(n) * 10.0 ** rs.uniform(-8, 2, size=n)).astype(np.float32)
    m = (rs.standard_normal(n) * 10.0 ** rs.uniform(-8, 2, size=n)).astype(np.float32)
    v = (10.0 ** rs.uniform(-16, 4, size=n)).astype(np.float32)
    g[0::7] = 0.0
    v[0::14] = 0.0             # g = 0 and v = 0: the quotient is (lr_t beta_1 m) / (0 + eps)
    m[0::28] = 0.0             # ... and 0 / (0 + eps)
    v[3::11] = 0.0
    g[5::13] = 1e10
    g[6::17] = -1e-20
    dev = [torch.from_numpy(a.copy()).to(eng.device) for a in (p, g, m, v)]
    lr_t = float(np.float32(nr.adam_lr_t(t)))
    assert eng.lib.caelo_adam_step(eng.ctx, _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), n, lr_t, nr.BETA_1, nr.BETA_2, nr.EPSILON, eng.stream) == 0
    want = nr.adam_step(p, g, m, v, t)
    for what, host, d in zip(("params", "m", "v"), want, (dev[0], dev[2], dev[3])):
        got = d.cpu().numpy()
        same = got.view(np.uint32) == host.view(np.uint32)
        assert same.all(), "t %d %s: %d of %d differ, first at %d: %r vs %r" % (t, what, (~same).sum(), n, np.flatnonzero(~same)[0], got[~same][0], host[~same][0])
    assert np.array_equal(dev[1].cpu().numpy().view(np.uint32), g.view(np.uint32))


# ---- ten steps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shipped", "glorot7"])
def test_ten_adam_steps_follow_the_float64_trajectory(eng, name):
    ws, x = nr.model(name), nr.images(4, 16, 36, seed=16)
    l64, _ = nr.trajectory(ws, x, 10, torch.float64)
    l32, _ = nr.trajectory(ws, x, 10, torch.float32)
    d32 = float((np.abs(l32 - l64) / l64).max())
    tr = _trainer(eng, ws, 4)
    dev = np.array([tr.step(x) for _ in range(10)])
    bar = FACTOR * max(d32, FLOOR)
    for s in range(10):
        print("%s step %d: device %.9g, f64 %.9g, relative %.3g, bar %.3g (f32 trajectory's worst %.3g)" % (name, s, dev[s], l64[s], abs(dev[s] - l64[s]) / l64[s], bar, d32))
    assert d32 <= 1e-5                                   # an ill-conditioned batch may not widen the bar unnoticed
    assert l64[-1] < l64[0]                              # the reference itself falls
    assert all(abs(dev[s] - l64[s]) / l64[s] <= bar for s in range(10))
    assert dev[-1] < dev[0] and tr.t == 10


# ---- the round trip ----------------------------------------------------------------------------------------------------------------
def _a2_cpu(ws, x, dtype):
    k = [torch.tensor(np.asarray(w), dtype=dtype) for w in ws[:4]]
    with torch.no_grad():
        a1 = torch.relu(nr._conv(torch.tensor(x, dtype=dtype).permute(0, 3, 1, 2), k[0], k[1]))
        return torch.relu(nr._conv(a1, k[2], k[3])).permute(0, 2, 3, 1).double().numpy()


def test_trained_response_layer_runs_in_the_detector_and_through_two_h5_files(eng, rings, tmp_path):
    from caelo import keras_config, synth
    pc = torch.from_numpy(synth.make_scan(0, quantum=1e-3)).to(eng.device)
    before = eng.extract(pc)
    before = [t.clone() for t in (before.rows, before.key_pixels, before.n_key, before.status)]
    tr = _trainer(eng, nr.model("shipped"), 2)
    losses = [tr.step(rings) for _ in range(10)]
    print("ten full-size steps: loss %.6f -> %.6f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all()       # (from a trained model Adam's first steps overshoot, in float64 as well: no fall is asked here)
    # a trainer that was created and stepped, not installed, changes nothing the engine computes
    after = eng.extract(pc)
    assert all(bool(torch.equal(a, b)) for a, b in zip(before, (after.rows, after.key_pixels, after.n_key, after.status)))
    try:
        ws = tr.weights()
        x0 = np.ascontiguousarray(rings[:1, :64, :1792, :3].cpu().numpy())
        a64 = _a2_cpu(ws, x0, torch.float64)
        a32 = _rel(_a2_cpu(ws, x0, torch.float32), a64)
        bar = FACTOR * max(a32, FLOOR)
        tr.loss(rings[:1])
        a2_dev = _ws_tensors(eng, tr, 64, 1792, 1)[0]
        tr.install()
        resp = eng.respond(rings[0].contiguous())
        r0 = resp.cpu().numpy().astype(np.float64)[None]
        print("A2 after ten steps: trainer %.3g, Engine.respond %.3g, between them %.3g; bar %.3g (f32 network %.3g)"
              % (_rel(a2_dev, a64), _rel(r0, a64), np.abs(r0 - a2_dev).max() / np.abs(a64).max(), bar, a32))
        assert _rel(a2_dev, a64) <= bar and _rel(r0, a64) <= bar
        assert np.abs(r0 - a2_dev).max() / np.abs(a64).max() <= bar
        ae, rl = str(tmp_path / "ae.h5"), str(tmp_path / "respond.h5")
        keras_config.write_ring_models_like(nr.FIXTURE, ae, ws, out_respond_h5=rl)
        eng.load_weights(RESPOND_H5)
        assert not torch.equal(eng.respond(rings[0].contiguous()), resp)          # (the shipped layer answers otherwise)
        assert eng.load_weights(rl) == "respond"
        assert torch.equal(eng.respond(rings[0].contiguous()), resp)
        back = keras_config.read_ring_autoencoder(ae)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(back, ws))
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(tr.respond_weights(), ws[:4]))
    finally:
        eng.load_weights(RESPOND_H5)
    again = eng.extract(pc)
    assert all(bool(torch.equal(a, b)) for a, b in zip(before, (again.rows, again.key_pixels, again.n_key, again.status)))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(eng):
    from caelo.engine import _ptr
    tr = _trainer(eng, nr.model("glorot7"), 2)
    x = torch.from_numpy(nr.images(3, 8, 16, seed=8)).to(eng.device)
    ws = eng._ws("train_ring", tr.ws_bytes(8, 16))
    grads = torch.full((nr.N_PARAMS * 4,), SENTINEL, dtype=torch.uint8, device=eng.device)
    loss = torch.full((4,), SENTINEL, dtype=torch.uint8, device=eng.device)
    recon = torch.full((3 * 8 * 16 * 3 * 4,), SENTINEL, dtype=torch.uint8, device=eng.device)
    params = tr.params.clone()

    def call(ctx=eng.ctx, p=tr.params, im=x, n=3, h=8, w=16, st=(8 * 16 * 3, 16 * 3, 3), chunk=2, g=grads, l=loss, w_=ws):
        return eng.lib.caelo_ring_autoencoder_grad(ctx, _ptr(p), _ptr(im), n, h, w, st[0], st[1], st[2], chunk, _ptr(g), _ptr(l), _ptr(recon), _ptr(w_), eng.stream)

    cases = [dict(n=-1), dict(h=0), dict(w=0), dict(h=-8), dict(h=6), dict(w=18), dict(h=7, w=15),
             dict(st=(8 * 16 * 3, 16 * 3, 2)), dict(st=(8 * 16 * 3, 16 * 3 - 1, 3)), dict(st=(8 * 16 * 3 - 1, 16 * 3, 3)),
             dict(chunk=0), dict(chunk=-2), dict(chunk=4097), dict(p=None), dict(l=None), dict(w_=None), dict(im=None), dict(ctx=None)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert eng.lib.caelo_last_error()
        if "h" in kw or "w" in kw:
            assert b"multiples of 4" in eng.lib.caelo_last_error() and b"not built" in eng.lib.caelo_last_error()
    torch.cuda.synchronize()
    assert bool((grads == SENTINEL).all()) and bool((loss == SENTINEL).all()) and bool((recon == SENTINEL).all()) and bool(torch.equal(params, tr.params))
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((loss == SENTINEL).all())
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(c=None), dict(count=-1)):
        arg = dict(c=eng.ctx, p=tr.params, g=tr.grads, m=tr.m, v=tr.v, count=16)
        arg.update(kw)
        rc = eng.lib.caelo_adam_step(arg["c"], _ptr(arg["p"]), _ptr(arg["g"]), _ptr(arg["m"]), _ptr(arg["v"]), arg["count"], 1e-3, 0.9, 0.999, 1e-7, eng.stream)
        assert rc == -1 and bool(torch.equal(params, tr.params)), kw
    from caelo.train_ring import RingTrainer
    with pytest.raises(ValueError, match="chunk"):
        RingTrainer(eng, nr.model("glorot7"), chunk=0)
    with pytest.raises(ValueError, match="ring autoencoder weights"):
        RingTrainer(eng, nr.model("glorot7")[:11])
    with pytest.raises(ValueError, match="multiples of 4"):
        tr.loss(np.zeros((1, 6, 8, 3), np.float32))
    with pytest.raises(ValueError, match="images"):
        tr.loss(np.zeros((1, 8, 8, 4), np.float32))


def test_no_images_give_loss_zero_and_zero_gradients(eng):
    tr = _trainer(eng, nr.model("biased"), 2)
    tr.grads.fill_(3.0)
    tr._loss.fill_(3.0)
    loss, grads = tr.grad(np.zeros((0, 8, 16, 3), np.float32))
    assert loss == 0.0 and all(not g.any() for g in grads)
    tr._loss.fill_(3.0)
    assert tr.loss(np.zeros((0, 8, 16, 3), np.float32)) == 0.0


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_command_line_trains_one_epoch_on_synthetic_scans_and_writes_readable_files(engine, tmp_path):
    """train_ring_autoencoder.py in this process: three synthetic scans (two train, one validates), one epoch of one full-size step from
    the fixture; both written files load, keep their templates' sizes, and the log holds finite losses."""
    from scipy import io
    import train_ring_autoencoder
    from caelo import keras_config
    ae, rl, log = str(tmp_path / "ae.h5"), str(tmp_path / "respond.h5"), str(tmp_path / "loss.mat")
    assert train_ring_autoencoder.main(["--synthetic", "3", "--init", nr.FIXTURE, "--epochs", "1", "--chunk", "2", "--out", ae, "--out-respond", rl,
                                        "--log", log, "--seed", "4"]) == 0
    hist = io.loadmat(log)
    assert hist["loss"].size == 1 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all() and hist["loss"].ravel()[0] > 0
    new, old = keras_config.read_ring_autoencoder(ae), keras_config.read_ring_autoencoder(nr.FIXTURE)
    assert all(np.isfinite(w).all() for w in new) and any(not np.array_equal(a, b) for a, b in zip(new, old))
    kind, rws, _ = keras_config.read_model(rl)
    assert kind == "respond" and all(np.array_equal(a, b) for a, b in zip(rws, new[:4]))
    assert os.path.getsize(ae) == os.path.getsize(nr.FIXTURE) and os.path.getsize(rl) == os.path.getsize(RESPOND_H5)
