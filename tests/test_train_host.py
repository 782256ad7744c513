"""CPU: what training rests on besides the kernels -- the torch reference checks itself against finite differences, Adadelta's NumPy
restatement against torch.optim.Adadelta, ``keras_config.write_autoencoder_like`` on the fixture files, ``sample_training_points``
against the literal loop, the parameter layout of the C ABI, and ``train.fit``'s shuffling, batching and generator with a stub trainer."""
import ctypes as C
import os
import struct
import types

import numpy as np
import pytest
import torch

import netref64_dec as nd
import netref64_train as nt


@pytest.fixture(scope="module")
def fixdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fixture"))


# ---- 1. the reference checks itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m[0] for m in nd.MODELS])
def test_reference_gradient_matches_central_difference(name, fixdir):
    """f64, 16 patches: (L(w + h d) - L(w - h d)) / 2h against g . d to 1e-6 relative.  d = (g / |g| + r / |r|) / sqrt 2 with r a seeded
    normal direction over all 20 tensors (the share along g keeps g . d far above the difference's rounding error); h is the decade at
    which two neighbouring step sizes agree best, among the steps at which no relu output changes sign and no pooling window changes
    its argmax between the two evaluations (the loss is piecewise smooth: across a kink the difference quotient measures something
    else); a direction without two such neighbouring steps is passed over.  A bias-free model sits ON such kinks: in its empty
    regions every pooling window holds exact ties, which any step along the biases of conv3d_1 / conv3d_2 breaks one way for +h and
    the other way for -h (border cells sum fewer taps), and there autograd's gradient is one of the subgradients.  So every other
    direction has no component along those two biases, and g . d is taken over the same components."""
    ews, eact, dws, dact = nd.model(name, fixdir)
    bits = nd.patches(name)[:16]
    _, g, _ = nt.loss_and_grads(ews, eact, dws, dact, bits)
    base = [np.asarray(w, np.float64).reshape(s) for w, s in zip(list(ews) + list(dws), nt.SHAPES)]
    gn = np.sqrt(sum(float((x * x).sum()) for x in g))

    def at(d, h):
        with torch.no_grad():
            l, t = nt.forward([torch.tensor(w + h * x, dtype=torch.float64) for w, x in zip(base, d)], bits, eact, dact)
        return float(l.item()), t

    for seed in range(20):
        rs = np.random.RandomState(1000 + seed)
        r = [rs.standard_normal(s) for s in nt.SHAPES]
        gs = g
        if seed % 2:    # every other direction leaves the biases in front of the two poolings alone (see the docstring)
            r = [np.zeros_like(x) if t in (1, 3) else x for t, x in enumerate(r)]
            gs = [np.zeros_like(x) if t in (1, 3) else x for t, x in enumerate(g)]
        rn = np.sqrt(sum(float((x * x).sum()) for x in r))
        d = [(x / gn + y / rn) / np.sqrt(2.0) for x, y in zip(gs, r)]
        gd = sum(float((x * y).sum()) for x, y in zip(g, d))
        hs = [10.0 ** -k for k in range(2, 9)]
        ev = [(at(d, h), at(d, -h)) for h in hs]
        cd = [(p[0] - m[0]) / (2 * h) for (p, m), h in zip(ev, hs)]
        same = [nt.same_branch(p[1], m[1]) for p, m in ev]
        pairs = [i for i in range(len(hs) - 1) if same[i] and same[i + 1]]
        if not pairs:
            print("%s seed %d: a kink is crossed at every pair of neighbouring steps (kink-free steps: %s)" % (name, seed, [h for h, s in zip(hs, same) if s]))
            continue
        best = min(pairs, key=lambda i: abs(cd[i] - cd[i + 1]))
        print("%s seed %d: h %.0e, central difference %.12g, g.d %.12g, relative %.3g" % (name, seed, hs[best], cd[best], gd, abs(cd[best] - gd) / abs(gd)))
        assert abs(cd[best] - gd) <= 1e-6 * abs(gd)
        return
    pytest.fail("no direction among 20 left every relu sign and pooling argmax unchanged at two neighbouring steps")


# ---- 2. Adadelta -------------------------------------------------------------------------------------------------------------------
def test_adadelta_restatement_equals_torch():
    rs = np.random.RandomState(5)
    p = rs.standard_normal(1000)
    a, d = np.zeros_like(p), np.zeros_like(p)
    tp = torch.tensor(p.copy(), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adadelta([tp], lr=1.0, rho=0.95, eps=1e-7)
    for _ in range(5):
        g = rs.standard_normal(1000) * 10.0 ** rs.uniform(-6, 2, size=1000)
        p, a, d = nt.adadelta_step(p, g, a, d)
        tp.grad = torch.tensor(g)
        opt.step()
        assert np.abs(tp.detach().numpy() - p).max() <= 1e-12


# ---- 3. write_autoencoder_like -----------------------------------------------------------------------------------------------------
def _new_weights(seed):
    rs = np.random.RandomState(seed)
    return [rs.standard_normal(s).astype(np.float32) for s in nt.SHAPES]


def test_written_file_reads_back_bit_for_bit_and_changes_nothing_else(fixdir, tmp_path):
    from caelo import h5lite, keras_config
    ws = _new_weights(7)
    for tpl, half, kw in zip(nt.templates(fixdir), (0, 1), (dict(ews=ws[:10], dws=None), dict(ews=None, dws=ws[10:]))):
        out = str(tmp_path / ("out%d.h5" % half))
        assert keras_config.write_autoencoder_like(tpl, out, **kw) == out
        enc, eacts, dec, dacts = keras_config.read_autoencoder(out)
        t_enc, t_eacts, t_dec, t_dacts = keras_config.read_autoencoder(tpl)
        assert (eacts, dacts) == (t_eacts, t_dacts)
        got, other = (enc, dec) if half == 0 else (dec, enc)
        assert other is None and len(got) == 10
        for g, w in zip(got, ws[:10] if half == 0 else ws[10:]):
            assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32).ravel(), w.view(np.uint32).ravel())
        a, b = np.frombuffer(open(tpl, "rb").read(), np.uint8), np.frombuffer(open(out, "rb").read(), np.uint8)
        assert a.size == b.size
        inside = np.zeros(a.size, bool)
        h = h5lite.H5File(tpl)
        for path, (off, nbytes), shape in keras_config.autoencoder_datasets(h)[half]:
            assert h5lite.dataset_span(tpl, path) == (off, nbytes) and nbytes == 4 * int(np.prod(shape))
            assert not inside[off:off + nbytes].any()
            inside[off:off + nbytes] = True
        assert inside.sum() == 4 * sum(int(np.prod(s)) for s in (nt.SHAPES[:10] if half == 0 else nt.SHAPES[10:]))
        assert np.array_equal(a[~inside], b[~inside]) and not np.array_equal(a[inside], b[inside])


def test_wrong_templates_and_arrays_are_refused_and_no_file_appears(fixdir, tmp_path):
    from caelo import keras_config
    ws = _new_weights(8)
    enc_tpl, dec_tpl = nt.templates(fixdir)
    out = str(tmp_path / "never.h5")
    # a template whose dense_4 kernel is stored as [2048, 200]: the dataspace's dimensions swapped in the object header
    raw = open(dec_tpl, "rb").read()
    pat = struct.pack("<QQ", 200, 2048)
    assert raw.count(pat) >= 1
    bad = str(tmp_path / "bad_shape.h5")
    open(bad, "wb").write(raw.replace(pat, struct.pack("<QQ", 2048, 200)))
    with pytest.raises(ValueError, match="shape"):
        keras_config.write_autoencoder_like(bad, out, None, ws[10:])
    # an array of another shape, too few arrays, a half the template does not hold
    with pytest.raises(ValueError, match="shape"):
        keras_config.write_autoencoder_like(dec_tpl, out, None, ws[10:19] + [np.zeros(2, np.float32)])
    with pytest.raises(ValueError, match="arrays wanted"):
        keras_config.write_autoencoder_like(dec_tpl, out, None, ws[10:19])
    with pytest.raises(ValueError, match="encoder"):    # the decoder-half template has no encoder datasets
        keras_config.write_autoencoder_like(dec_tpl, out, ws[:10], ws[10:])
    with pytest.raises(ValueError, match="decoder"):
        keras_config.write_autoencoder_like(enc_tpl, out, ws[:10], ws[10:])
    assert not os.path.exists(out)


def test_dataset_span_refuses_what_is_not_contiguous_float32(fixdir):
    from caelo import h5lite
    _, dec_tpl = nt.templates(fixdir)
    with pytest.raises(h5lite.H5Error):
        h5lite.dataset_span(dec_tpl, "/model_weights")            # a group
    with pytest.raises(KeyError):
        h5lite.dataset_span(dec_tpl, "/model_weights/nothing")


# ---- 4. sample_training_points -----------------------------------------------------------------------------------------------------
def _key_points(seed, k, inside):
    """Seeded key points: a share inside the cropped grid (|x|, |y| < 94.72, |z| < 9.6), the rest in the cropped blocks or beyond."""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-1, 1, size=(k, 3)) * np.array([94.0, 94.0, 9.5])
    out = rs.uniform(size=k) >= inside
    axis = rs.randint(0, 3, size=k)
    far = np.array([97.0, 97.0, 12.0])[axis] * rs.choice([-1.0, 1.0], size=k)
    pts[out, axis[out]] = far[out]
    return pts.astype(np.float32)


@pytest.mark.parametrize("seed,k,inside,n_groups", [(1, 600, 0.9, 256), (2, 300, 0.3, 64), (3, 52, 0.6, 16), (4, 1024, 1.0, 256)])
def test_sampled_points_equal_the_literal_loop(seed, k, inside, n_groups):
    from caelo import train
    kp = _key_points(seed, k, inside)
    want, drawn = nt.sample_points_loop(kp, n_groups, np.random.RandomState(seed))
    got = train.sample_training_points(kp, n_groups, np.random.RandomState(seed))
    assert got.dtype == np.float32 and got.shape == (n_groups, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert drawn.min() >= 1 and drawn.max() <= k - 1           # index 0 is never drawn
    assert len(np.unique(drawn)) < len(drawn)                  # repeats are allowed (10 n_groups draws)
    if inside < 1.0:                                           # a dropped point never comes back
        assert np.abs(got[:, :2]).max() < 94.72 and np.abs(got[:, 2]).max() < 9.6


def test_sampling_constants_are_the_references():
    from caelo import train
    assert (train.BLOCK_SIZE, train.CROP_BLOCKS, train.N_BLOCKS) == (64, 4, (156, 156, 23))
    assert np.allclose(train.VISIBLE_RANGE, [[99.84, 99.84, 14.72]])


def test_too_few_survivors_is_a_value_error():
    from caelo import train
    kp = _key_points(9, 400, 0.01)
    with pytest.raises(AssertionError):
        nt.sample_points_loop(kp, 64, np.random.RandomState(0))
    with pytest.raises(ValueError, match="cropped grid"):
        train.sample_training_points(kp, 64, np.random.RandomState(0))


def test_glorot_uniform_shapes_and_limits():
    from caelo import train
    ws = train.glorot_uniform(nt.SHAPES, np.random.RandomState(3))
    assert [w.shape for w in ws] == [tuple(s) for s in nt.SHAPES] and all(w.dtype == np.float32 for w in ws)
    for w, s in zip(ws, nt.SHAPES):
        if len(s) == 1:
            assert not w.any()
        else:
            field = int(np.prod(s[:-2]))
            lim = np.sqrt(6.0 / (field * (s[-2] + s[-1])))
            assert np.abs(w).max() <= lim and np.abs(w).max() > 0.9 * lim


# ---- 5. the parameter layout -------------------------------------------------------------------------------------------------------
def test_param_layout_is_the_shapes_cumulative_sizes():
    from caelo import _ffi, train
    lay = train.param_layout()
    sizes = [int(np.prod(s)) for s in nt.SHAPES]
    assert [c for _, c in lay] == sizes and [o for o, _ in lay] == list(np.cumsum([0] + sizes[:-1]))
    assert lay[-1][0] + lay[-1][1] == 864741 == nt.N_PARAMS == train.N_PARAMS
    lib = _ffi.load()
    assert lib.caelo_train_param_layout(None) == -1
    assert lib.caelo_train_ws_bytes(0) == 0 and lib.caelo_train_ws_bytes(8) > 8 * 480000
    out = (C.c_int64 * 3)()
    assert lib.caelo_train_ws_layout(8, C.cast(out, C.c_void_p)) == 0 and 0 < out[0] < out[1] < out[2] < lib.caelo_train_ws_bytes(8)
    assert lib.caelo_train_ws_layout(0, C.cast(out, C.c_void_p)) == -1


# ---- 6. fit ------------------------------------------------------------------------------------------------------------------------
class _StubTrainer:
    """Counts what ``fit`` feeds it: the stubbed ``training_patches`` marks each scan's three patches with the scan's id."""

    def __init__(self):
        self.steps, self.evals = [], []
        self.eng = types.SimpleNamespace(device=torch.device("cpu"))

    def step(self, bits, sync=True):
        self.steps.append([int(v) for v in bits[:, 0]])
        return torch.tensor([float(len(self.steps))])

    def loss(self, bits):
        self.evals.append([int(v) for v in bits[:, 0]])
        return 0.5


# the first number the shuffling generator gives a step's batch builder, recorded on the commit before the epoch loop was shared
FIRST_DRAW = {1: 0.5507979025745755, 3: 0.7081478226181048, 5: 0.2909047389129443}


@pytest.mark.parametrize("files,steps", [(1, 1), (3, 1), (5, 2)])
def test_fit_takes_the_references_steps_per_pass(files, steps, monkeypatch):
    """YieldBatchData's strict bound: L training files give (L - 1) // 2 steps per pass, at least one here; and the generator that
    shuffled the scans is the one every step's ``training_patches`` draws from, in the state the shuffle left it in."""
    from caelo import train
    seen = []

    def patches(eng, pc, n_groups, rng):
        seen.append((rng, float(rng.random_sample())))
        return torch.full((n_groups, 64), int(pc[0, 0]), dtype=torch.int64)

    monkeypatch.setattr(train, "training_patches", patches)
    tr = _StubTrainer()
    hist = train.fit(tr, [lambda i=i: np.full((3, 4), float(i), np.float32) for i in range(files)], epochs=2, files_per_step=2, points_per_file=3,
                     seed=3, train_ratio=1.0, log=None)
    assert len(tr.steps) == 2 * steps and not tr.evals
    assert np.isnan(hist["val_loss"]).all() and hist["val_loss"].shape == (2,)
    rs = np.random.RandomState(3)
    order = list(range(files))
    rs.shuffle(order)
    for s in range(steps):
        want = [i for i in order[2 * s:2 * (s + 1)] for _ in range(3)]
        assert tr.steps[s] == want == tr.steps[steps + s]          # shuffled once, the same pass every epoch
    assert np.array_equal(hist["loss"], [np.mean(np.arange(e * steps, (e + 1) * steps) + 1.0) for e in range(2)])
    assert all(r is seen[0][0] for r, _ in seen) and len(seen) == sum(len(b) // 3 for b in tr.steps)
    assert seen[0][1] == FIRST_DRAW[files]
    assert [d for _, d in seen] == [float(rs.random_sample()) for _ in seen]      # one generator: the shuffle, then every draw in turn
