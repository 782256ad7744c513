"""The training kernels (csrc/train.hip) against the torch-CPU autograd network of tests/netref64_train.py: loss and gradient of the
whole autoencoder on the three models of netref64_dec.MODELS, determinism and chunking, the pooling rule, the Adadelta kernel bit for
bit, ten optimizer steps, the round trip into the inference paths and an .h5, the refusals.

Bars.  Keras cannot run here, so everything is pinned to the float64 torch network.  Per tensor t, max |g_dev - g64| / max |g64| <=
4 x max(e32_t, E): e32_t the float32 torch network's own error on that tensor and batch, E the median of e32_t over the model's 20
tensors (a single tensor's float32 error can be luckily small; tensors whose float64 gradient is identically zero must be zero
exactly and stay out of the median: _rel, _median), both computed here; 4 is the project's usual margin over the float32
restatement.  Loss: relative error <= 4 x max(e32, 2e-6), 2e-6 being 32 float32 ulps.  The engines of these tests are private.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import netref64_dec as nd
import netref64_train as nt

pytestmark = pytest.mark.gpu

FACTOR = 4.0
LOSS_FLOOR = 2e-6
CHUNK = 8
NAMES = [m[0] for m in nd.MODELS]
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def fixdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fixture"))


@pytest.fixture(scope="module")
def eng(engine):   # (the session fixture first: it skips without a GPU)
    from caelo.engine import Engine
    return Engine(device=0)


_refs = {}


def _ref(name, n, fixdir):
    """The float64 and float32 torch networks' loss and gradients on the first n patches of the model's set: computed once, shared."""
    if (name, n) not in _refs:
        ews, eact, dws, dact = nd.model(name, fixdir)
        bits = nd.patches(name)[:n]
        l64, g64, x64 = nt.loss_and_grads(ews, eact, dws, dact, bits)
        l32, g32, _ = nt.loss_and_grads(ews, eact, dws, dact, bits, torch.float32)
        e32 = np.array([_rel(a, b) for a, b in zip(g32, g64)])
        _refs[(name, n)] = dict(model=(ews, eact, dws, dact), bits=bits, l64=l64, g64=g64, x64=x64, e32=e32, E=_median(e32, g64),
                                l32=abs(l32 - l64) / l64)
    return _refs[(name, n)]


def _rel(g, g64):
    """max |g - g64| / max |g64|.  A tensor whose float64 gradient is zero everywhere (conv3d_1's kernel on an empty patch: every input
    is 0) has no scale: there the gradient must be zero exactly -- 0 when it is, inf when it is not."""
    top = np.abs(g64).max()
    if top == 0:
        return 0.0 if not np.any(g) else np.inf
    return float(np.abs(np.asarray(g, np.float64) - g64).max() / top)


def _median(e32, g64):
    """E: the median of e32_t over the tensors that have a scale.  A tensor whose float64 gradient is zero everywhere has e32 = 0 for no
    merit of float32 arithmetic (on the empty patch alone that is every kernel of the bias-free model: half the tensors), and would
    pull the floor, which is there to tell what float32 costs on this batch, to 0."""
    return float(np.median([e for e, g in zip(e32, g64) if np.any(g)]))


def _trainer(eng, name, fixdir, chunk=CHUNK):
    from caelo.train import Trainer
    ews, eact, dws, dact = nd.model(name, fixdir)
    return Trainer(eng, ews, eact, dws, dact, chunk=chunk)


def _check(R, loss, grads, what):
    rel = abs(loss - R["l64"]) / R["l64"]
    bar = FACTOR * max(R["l32"], LOSS_FLOOR)
    print("%s: loss %.9g (f64 %.9g) relative %.3g, bar %.3g (f32 network %.3g)" % (what, loss, R["l64"], rel, bar, R["l32"]))
    worst = []
    for t, (g, g64) in enumerate(zip(grads, R["g64"])):
        err = _rel(g, g64)
        tb = FACTOR * max(R["e32"][t], R["E"])
        print("  tensor %2d %-18s error %.3g, bar %.3g (f32 network %.3g, median %.3g)" % (t, nt.SHAPES[t], err, tb, R["e32"][t], R["E"]))
        if not err <= tb:
            worst.append((t, err, tb))
    assert rel <= bar
    assert not worst, "%s: tensors beyond their bars (index, error, bar): %s" % (what, worst)


# ---- 6. gradient parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("name", NAMES)
def test_gradient_parity(eng, name, n, fixdir):
    R = _ref(name, n, fixdir)
    loss, grads = _trainer(eng, name, fixdir).grad(R["bits"])
    _check(R, loss, grads, "%s n=%d chunk=%d" % (name, n, CHUNK))


def test_gradient_parity_chunk_64_n_134(eng, fixdir):
    R = _ref("biased_relu", 134, fixdir)
    loss, grads = _trainer(eng, "biased_relu", fixdir, chunk=64).grad(R["bits"])
    _check(R, loss, grads, "biased_relu n=134 chunk=64")


# ---- 7. determinism and chunk behaviour ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_same_call_same_bits_and_chunks_agree(eng, name, fixdir):
    R = _ref(name, 17, fixdir)
    tr = _trainer(eng, name, fixdir)
    l0, g0 = tr.grad(R["bits"])
    l1, g1 = tr.grad(R["bits"])
    assert np.float32(l0).tobytes() == np.float32(l1).tobytes()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(g0, g1))
    fwd = tr.loss(R["bits"])
    assert np.float32(fwd).tobytes() == np.float32(l0).tobytes()        # forward only: the loss bits of the full call
    l17, g17 = _trainer(eng, name, fixdir, chunk=17).grad(R["bits"])
    _check(R, l17, g17, "%s n=17 chunk=17" % name)
    assert np.float32(l17).tobytes() == np.float32(l0).tobytes()        # the loss is summed patch by patch: its bits depend on n alone
    print("gradient bits equal across chunk 8 / 17: %s" % [bool(np.array_equal(a.view(np.uint32), b.view(np.uint32))) for a, b in zip(g0, g17)])


# ---- 8. the pooling rule -------------------------------------------------------------------------------------------------------------
def _period2_batch():
    """Four patches: occupancy of period 2 along x, along y, along z (every interior pooling window of conv3d_1's output then holds
    equal maxima: the window's cells along the other two axes see equal neighbourhoods), and the all-set patch."""
    dense = np.zeros((4, 16, 16, 16), bool)
    dense[0, ::2, :, :] = True
    dense[1, :, ::2, :] = True
    dense[2, :, :, ::2] = True
    dense[3] = True
    return nd.pack(dense.reshape(4, -1))


def _ws_tensors(eng, tr, rows):
    lay = (C.c_int64 * 3)()
    assert eng.lib.caelo_train_ws_layout(tr.chunk, C.cast(lay, C.c_void_p)) == 0
    ws = eng._ws("train", int(eng.lib.caelo_train_ws_bytes(tr.chunk)))
    take = lambda off, per: ws[off:off + rows * per * 4].view(torch.float32).view(rows, per).cpu().numpy().astype(np.float64)
    return take(int(lay[0]), 4096), take(int(lay[1]), 20), take(int(lay[2]), 4096)


@pytest.mark.parametrize("name", NAMES)
def test_pooling_gradient_goes_to_the_first_maximum(eng, name, fixdir):
    ews, eact, dws, dact = nd.model(name, fixdir)
    bits = _period2_batch()
    l64, g64, x64 = nt.loss_and_grads(ews, eact, dws, dact, bits)
    l32, g32, x32 = nt.loss_and_grads(ews, eact, dws, dact, bits, torch.float32)
    e32 = np.array([_rel(a, b) for a, b in zip(g32, g64)])
    E = _median(e32, g64)
    tr = _trainer(eng, name, fixdir)
    loss, grads = tr.grad(bits)
    dz, dcode, dp1 = _ws_tensors(eng, tr, 4)
    for what, got, key in (("dL/dz", dz, "dz"), ("dL/dcode", dcode, "dcode"), ("dL/dP1", dp1, "dp1")):
        want = x64[key]
        err = np.abs(got - want).max() / np.abs(want).max()
        f32 = np.abs(x32[key] - want).max() / np.abs(want).max()
        print("%s %s: error %.3g, bar %.3g (f32 network %.3g, median of the tensors %.3g)" % (name, what, err, FACTOR * max(f32, E), f32, E))
        assert err <= FACTOR * max(f32, E)
    # where dL/dP1 is non-zero is decided by which cell of each tied window of the second pooling the gradient went to
    assert np.array_equal(dp1 != 0, x64["dp1"] != 0)
    for t, (g, w) in enumerate(zip(grads, g64)):
        assert _rel(g, w) <= FACTOR * max(e32[t], E), t


# ---- 9. the Adadelta kernel ------------------------------------------------------------------------------------------------------------
def test_adadelta_kernel_is_bit_equal_to_the_float32_restatement(eng):
    from caelo.engine import _ptr
    n = 1000003
    rs = np.random.RandomState(9)
    p = rs.standard_normal(n).astype(np.float32)
    a, d = np.zeros(n, np.float32), np.zeros(n, np.float32)
    dev = [torch.from_numpy(x.copy()).to(eng.device) for x in (p, a, d)]
    for step in range(3):
        g = (rs.standard_normal(n) * 10.0 ** rs.uniform(-8, 2, size=n)).astype(np.float32)
        g[step::7] = 0.0
        g[3 + step::11] = 1e-20
        g[5 + step::13] = 1e10
        g[6 + step::17] = -1e10
        p, a, d = nt.adadelta_step(p, g, a, d)
        gd = torch.from_numpy(g).to(eng.device)
        assert eng.lib.caelo_adadelta_step(eng.ctx, _ptr(dev[0]), _ptr(gd), _ptr(dev[1]), _ptr(dev[2]), n, 1.0, 0.95, 1e-7, eng.stream) == 0
        for what, host, t in zip(("params", "acc_g", "acc_d"), (p, a, d), dev):
            got = t.cpu().numpy()
            same = got.view(np.uint32) == host.view(np.uint32)
            assert same.all(), "step %d %s: %d of %d differ, first at %d: %r vs %r" % (step, what, (~same).sum(), n, np.flatnonzero(~same)[0],
                                                                                      got[~same][0], host[~same][0])


# ---- 10, 11. ten steps, then the round trip -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(eng, fixdir):
    """name -> (trainer after 10 steps on the first 64 patches, device losses, bits, f64 losses, f32 deviations, f64 final weights)."""
    out = {}
    for name in ("glorot_tanh", "biased_relu"):
        ews, eact, dws, dact = nd.model(name, fixdir)
        bits = nd.patches(name)[:64]
        l64, w64 = nt.trajectory(ews, eact, dws, dact, bits, 10, torch.float64)
        l32, _ = nt.trajectory(ews, eact, dws, dact, bits, 10, torch.float32)
        tr = _trainer(eng, name, fixdir)
        out[name] = (tr, np.array([tr.step(bits) for _ in range(10)]), bits, l64, np.abs(l32 - l64) / l64, w64)
    return out


@pytest.mark.parametrize("name", ["glorot_tanh", "biased_relu"])
def test_ten_adadelta_steps_follow_the_float64_trajectory(trained, name):
    _, dev, _, l64, d32, _ = trained[name]
    for s in range(10):
        print("%s step %d: device %.9g, f64 %.9g, relative %.3g, bar %.3g (f32 trajectory %.3g)"
              % (name, s, dev[s], l64[s], abs(dev[s] - l64[s]) / l64[s], FACTOR * max(d32[s], LOSS_FLOOR), d32[s]))
    assert np.all(np.diff(l64[1:]) < 0) and l64[-1] < 0.6 * l64[0]          # the reference itself: falls after step 1, to below 0.6 x
    assert all(abs(dev[s] - l64[s]) / l64[s] <= FACTOR * max(d32[s], LOSS_FLOOR) for s in range(10))
    assert dev[-1] < 0.6 * dev[0]


@pytest.mark.parametrize("name", ["glorot_tanh", "biased_relu"])
def test_trained_weights_run_in_the_inference_paths_and_through_an_h5(eng, trained, name, fixdir, tmp_path):
    from caelo import keras_config
    tr, _, bits, _, _, _ = trained[name]
    ews, dws = tr.weights()
    # the loss bar of test_decoder_gpu: 4 x the float32 restatement's largest per-patch error on these patches
    want = nt.patch_losses(ews + dws, tr.eact, tr.dact, bits)
    bar = FACTOR * float(np.abs(nt.patch_losses(ews + dws, tr.eact, tr.dact, bits, torch.float32) - want).max())
    t_loss = tr.loss(bits)
    tr.install()
    assert eng.encoder_activations() == tr.eact and eng.decoder_activations() == tr.dact
    b = torch.from_numpy(bits.view(np.int64)).to(eng.device)
    d0 = eng.decode(eng.encode(b), target=b, bits=False).loss.cpu().numpy()
    i_err = float(np.abs(d0.astype(np.float64) - want).max())
    print("%s: Trainer.loss %.9g (f64 %.9g, error %.3g), encode + decode per patch: largest error %.3g; bar %.3g"
          % (name, t_loss, want.mean(), abs(t_loss - want.mean()), i_err, bar))
    assert abs(t_loss - want.mean()) <= bar      # (a mean's error is at most the largest per-patch error)
    assert i_err <= bar
    # through files: each fixture template holds one half
    enc_tpl, dec_tpl = nt.templates(fixdir)
    e_out, d_out = str(tmp_path / "enc.h5"), str(tmp_path / "dec.h5")
    if (tr.eact, tr.dact) != (("relu", "linear"), ("relu", "sigmoid")):    # the templates' model_config would contradict the trainer
        with pytest.raises(ValueError, match="activations"):
            keras_config.write_autoencoder_like(enc_tpl, e_out, ews, None, activations=(tr.eact, tr.dact))
        assert not os.path.exists(e_out)
        return
    keras_config.write_autoencoder_like(enc_tpl, e_out, ews, None, activations=(tr.eact, tr.dact))
    keras_config.write_autoencoder_like(dec_tpl, d_out, None, dws, activations=(tr.eact, tr.dact))
    assert eng.load_autoencoder(d_out, encoder_h5=e_out) == (tr.eact, tr.dact)
    d1 = eng.decode(eng.encode(b), target=b, bits=False).loss.cpu().numpy()
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(eng, fixdir):
    from caelo.engine import _ptr
    tr = _trainer(eng, "glorot_tanh", fixdir)
    bits = torch.from_numpy(nd.patches("glorot_tanh")[:4].view(np.int64)).to(eng.device)
    ws = eng._ws("train", int(eng.lib.caelo_train_ws_bytes(CHUNK)))
    grads = torch.full((nt.N_PARAMS * 4,), SENTINEL, dtype=torch.uint8, device=eng.device)
    loss = torch.full((4,), SENTINEL, dtype=torch.uint8, device=eng.device)

    def call(ctx=eng.ctx, params=tr.params, acts=(0, 0, 0), b=bits, n=4, chunk=CHUNK, g=grads, l=loss, w=ws):
        return eng.lib.caelo_autoencoder_grad(ctx, _ptr(params), acts[0], acts[1], acts[2], _ptr(b), n, chunk, _ptr(g), _ptr(l), _ptr(w), eng.stream)

    cases = [dict(n=-1), dict(chunk=0), dict(chunk=-3), dict(params=None), dict(b=None), dict(l=None), dict(w=None), dict(ctx=None),
             dict(acts=(2, 0, 0)), dict(acts=(3, 0, 0)), dict(acts=(0, 1, 0)), dict(acts=(0, 3, 0)), dict(acts=(0, 0, 2)), dict(acts=(0, 0, 3)),
             dict(acts=(-1, 0, 0)), dict(acts=(0, 0, 7))]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert eng.lib.caelo_last_error()
    torch.cuda.synchronize()
    assert bool((grads == SENTINEL).all()) and bool((loss == SENTINEL).all())
    for kw in (dict(p=None), dict(g=None), dict(a=None), dict(d=None), dict(c=None), dict(count=-1)):
        arg = dict(c=eng.ctx, p=tr.params, g=tr.grads, a=tr.acc_g, d=tr.acc_d, count=16)
        arg.update(kw)
        before = tr.params.clone()
        rc = eng.lib.caelo_adadelta_step(arg["c"], _ptr(arg["p"]), _ptr(arg["g"]), _ptr(arg["a"]), _ptr(arg["d"]), arg["count"], 1.0, 0.95, 1e-7, eng.stream)
        assert rc == -1 and bool(torch.equal(before, tr.params)), kw


def test_no_patches_give_loss_zero_and_zero_gradients(eng, fixdir):
    tr = _trainer(eng, "biased_relu", fixdir)
    tr.grads.fill_(3.0)
    tr._loss.fill_(3.0)
    loss, grads = tr.grad(np.zeros((0, 64), np.uint64))
    assert loss == 0.0 and all(not g.any() for g in grads)
    tr._loss.fill_(3.0)
    assert tr.loss(np.zeros((0, 64), np.uint64)) == 0.0


def test_trainer_refuses_activations_the_kernels_do_not_implement(eng, fixdir):
    from caelo.train import Trainer
    ews, eact, dws, dact = nd.model("biased_relu", fixdir)
    for bad_e, bad_d in ((("sigmoid", "linear"), dact), (("relu", "relu"), dact), (eact, ("linear", "sigmoid")), (eact, ("relu", "tanh")), (None, dact)):
        with pytest.raises(ValueError, match="activations"):
            Trainer(eng, ews, bad_e, dws, bad_d)
    with pytest.raises(ValueError, match="chunk"):
        Trainer(eng, ews, eact, dws, dact, chunk=0)
    with pytest.raises(ValueError, match="encoder weights"):
        Trainer(eng, ews[:9], eact, dws, dact)


# ---- the epoch loop and the command line ---------------------------------------------------------------------------------------------
def test_command_line_trains_one_epoch_on_synthetic_scans_and_writes_readable_files(engine, fixdir, tmp_path):
    """train_autoencoder.py in this process: three synthetic scans (two train, one validates), one epoch of one 1 536-patch step, from
    the fixture model; the two written halves load, differ from the templates in the weight datasets only, and the log holds finite losses."""
    from scipy import io
    import train_autoencoder
    from caelo import keras_config
    enc_tpl, dec_tpl = nt.templates(fixdir)
    e_out, d_out, log = str(tmp_path / "enc.h5"), str(tmp_path / "dec.h5"), str(tmp_path / "loss.mat")
    assert train_autoencoder.main(["--synthetic", "3", "--init", dec_tpl, "--init-encoder", enc_tpl, "--epochs", "1", "--chunk", "128",
                                   "--out", d_out, "--out-encoder", e_out, "--log", log, "--seed", "4"]) == 0
    hist = io.loadmat(log)
    assert hist["loss"].size == 1 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all() and 0 < hist["loss"].ravel()[0] < 1
    new_e, eacts, _, _ = keras_config.read_autoencoder(e_out)
    _, _, new_d, dacts = keras_config.read_autoencoder(d_out)
    old_e, _, _, _ = keras_config.read_autoencoder(enc_tpl)
    _, _, old_d, _ = keras_config.read_autoencoder(dec_tpl)
    assert (eacts, dacts) == (("relu", "linear"), ("relu", "sigmoid"))
    assert all(np.isfinite(w).all() for w in new_e + new_d)
    assert all(not np.array_equal(a, b) for a, b in zip(new_e + new_d, old_e + old_d))     # Adadelta moves every tensor in its first step
    assert os.path.getsize(e_out) == os.path.getsize(enc_tpl) and os.path.getsize(d_out) == os.path.getsize(dec_tpl)
