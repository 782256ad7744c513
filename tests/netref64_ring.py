"""The spherical-ring autoencoder (AE4SphericalRingPC.py:129-144) as a torch-CPU autograd network built from Keras-layout weights -- the
reference the device's loss and gradients (csrc/train_ring.hip) are pinned to, in float64 (the reference) and float32 (the yardstick
for what float32 arithmetic itself costs).  A helper module, not a conftest, beside netref64_train.py.

Keras cannot run here, so this is a restatement: Conv2D kernels ``permute(3, 2, 0, 1)`` (cross-correlation, zero 'same'
padding), MaxPooling2D(2) = ``max_pool2d`` on (N, C, y, x) (whose gradient goes to a window's first maximum in ascending (dy, dx)
order; TensorFlow's rule is unpinned), UpSampling2D(2) = ``repeat_interleave``, the loss = ``mse_loss`` against the input (the mean
over all n h w 3 elements).  Also Keras 2.2.4's Adam in NumPy -- in float32 with every operation rounded on its own, and its float64
twin --, the seeded inputs and the three models.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ring_autoencoder.h5")
SHAPES = [(3, 3, 3, 32), (32,), (1, 1, 32, 8), (8,), (3, 3, 8, 16), (16,), (3, 3, 16, 16), (16,), (3, 3, 16, 8), (8,), (1, 1, 8, 3), (3,)]
N_PARAMS = int(sum(int(np.prod(s)) for s in SHAPES))
MODELS = ("shipped", "glorot7", "biased")
LR, BETA_1, BETA_2, EPSILON = 0.001, 0.9, 0.999, 1e-7    # Keras 2.2.4 Adam defaults; epsilon = K.epsilon()


# ---- models and inputs ---------------------------------------------------------------------------------------------------------
def model(name):
    """-> the 12 float32 arrays: ``shipped`` the fixture; ``glorot7`` glorot_uniform, seed 7, zero biases; ``biased`` glorot, seed 11,
    biases U(0.05, 0.5), so that few relus are dead."""
    from caelo import keras_config, train
    if name == "shipped":
        return keras_config.read_ring_autoencoder(FIXTURE)
    if name == "glorot7":
        return train.glorot_uniform(SHAPES, np.random.RandomState(7))
    assert name == "biased"
    rs = np.random.RandomState(11)
    ws = train.glorot_uniform(SHAPES, rs)
    return [w if w.ndim > 1 else rs.uniform(0.05, 0.5, size=w.shape).astype(np.float32) for w in ws]


def images(n, h, w, seed=0):
    """[n, h, w, 3] float32 from one seeded RandomState: xyz = 10 N(0, 1), 30 % of the pixels exactly 0 in all three channels (empty
    ring cells)."""
    rs = np.random.RandomState(1000 + seed)
    x = (10.0 * rs.standard_normal((n, h, w, 3))).astype(np.float32)
    x[rs.uniform(size=(n, h, w)) < 0.3] = 0.0
    return x


def ring_window(ring, h, w, min_fill=0.5):
    """A [h, w, 3] window of a projected ring [69, 1800, 5] (array) cut at the first columns, in steps of w, where at least ``min_fill``
    of the window's cells have returns -- rows (64 - h) // 2 onward."""
    ring = np.asarray(ring)
    y0 = (64 - h) // 2
    for x0 in range(0, 1792 - w + 1, w):
        win = ring[y0:y0 + h, x0:x0 + w, 0:3]
        if np.mean(np.any(win != 0, axis=2)) >= min_fill:
            return np.ascontiguousarray(win, dtype=np.float32)
    raise AssertionError("no %d x %d window of the ring has %g of its cells filled" % (h, w, min_fill))


# ---- the network ---------------------------------------------------------------------------------------------------------------
def to_params(ws, dtype=torch.float64):
    """The 12 arrays -> leaf tensors of ``dtype`` in Keras shapes that require a gradient."""
    return [torch.tensor(np.asarray(w, np.float32).reshape(s), dtype=dtype, requires_grad=True) for w, s in zip(ws, SHAPES)]


def _conv(x, w, b):   # x [N, Cin, y, x], w Keras [kh, kw, Cin, Cout]
    return F.conv2d(x, w.permute(3, 2, 0, 1), b, padding=w.shape[0] // 2)


def _up(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def forward(params, x, keep=False):
    """x [n, h, w, 3] array -> (loss, dict): ``r`` [n, 3, h, w], ``a2`` [n, 8, h, w] (the response layer's output), ``p1`` [n, 8, h/2,
    w/2], all (N, C, y, x); ``signs`` / ``pools`` as in netref64_train.forward (what a finite-difference step must not change).
    ``keep``: retain the gradients of r, a2 and p1."""
    k = params
    x = torch.tensor(np.asarray(x), dtype=k[0].dtype).permute(0, 3, 1, 2)
    assert x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0
    a1 = torch.relu(_conv(x, k[0], k[1]))
    a2 = torch.relu(_conv(a1, k[2], k[3]))
    p1, i1 = F.max_pool2d(a2, 2, return_indices=True)
    a3 = torch.relu(_conv(p1, k[4], k[5]))
    p2, i2 = F.max_pool2d(a3, 2, return_indices=True)
    y4 = torch.relu(_conv(p2, k[6], k[7]))
    y5 = torch.relu(_conv(_up(y4), k[8], k[9]))
    r = _conv(_up(y5), k[10], k[11])
    if keep:
        for t in (r, a2, p1):
            t.retain_grad()
    loss = F.mse_loss(r, x)
    return loss, dict(r=r, a2=a2, p1=p1, signs=[t > 0 for t in (a1, a2, a3, y4, y5)], pools=[(a2.detach(), i1), (a3.detach(), i2)])


def same_branch(t0, t1, tie=1e-12):
    """Two ``forward`` dicts took the same branch of every relu and every pooling window (netref64_train.same_branch)."""
    if not all(bool(torch.equal(a, b)) for a, b in zip(t0["signs"], t1["signs"])):
        return False
    for (a, i0), (_, i1) in zip(t0["pools"], t1["pools"]):
        flat = a.flatten(2)
        if float((flat.gather(2, i0.flatten(2)) - flat.gather(2, i1.flatten(2))).abs().max()) > tie:
            return False
    return True


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).double().numpy()


def loss_and_grads(ws, x, dtype=torch.float64):
    """-> (loss, [12 gradient arrays f64], dict of [n, h, w, c] f64 arrays: ``r``, ``a2``, ``dr``, ``da2`` (dL/dA2, behind relu'),
    ``dp1``)."""
    params = to_params(ws, dtype)
    loss, t = forward(params, x, keep=True)
    loss.backward()
    a2 = _nhwc(t["a2"])
    extra = dict(r=_nhwc(t["r"]), a2=a2, dr=_nhwc(t["r"].grad), da2=_nhwc(t["a2"].grad) * (a2 > 0), dp1=_nhwc(t["p1"].grad))
    return float(loss.item()), [p.grad.double().numpy() for p in params], extra


# ---- Keras 2.2.4 Adam ----------------------------------------------------------------------------------------------------------
def adam_lr_t(t, lr=LR, beta_1=BETA_1, beta_2=BETA_2):
    """lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t) in float64 (the caller's part of caelo_adam_step)."""
    return float(lr) * np.sqrt(1.0 - float(beta_2) ** int(t)) / (1.0 - float(beta_1) ** int(t))


def adam_step(p, g, m, v, t, lr=LR, beta_1=BETA_1, beta_2=BETA_2, eps=EPSILON):
    """Keras 2.2.4's Adam (optimizers.py: m_t = beta_1 m + (1. - beta_1) g; v_t = beta_2 v + (1. - beta_2) square(g); p_t = p - lr_t *
    m_t / (sqrt(v_t) + epsilon) -- Python's order: (lr_t m_t) / (...)) in the arrays' dtype, every operation rounded on its own ->
    (p, m, v) after step t >= 1.  lr_t is computed in float64 and rounded to the dtype once; epsilon sits OUTSIDE the bias correction
    (torch.optim.Adam's does not, so it is no yardstick).  The constants are Keras's float32 variables in either dtype -- beta_2 is
    float32(0.999), so 1 - beta_2 is 0.00099998713, not 0.001: the float64 twin differs from the float32 form in its roundings alone."""
    ty = p.dtype.type
    f32 = np.float32
    lr_t, b1, b2, eps = ty(f32(adam_lr_t(t, lr, beta_1, beta_2))), ty(f32(beta_1)), ty(f32(beta_2)), ty(f32(eps))
    one_b1, one_b2 = ty(1) - b1, ty(1) - b2
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g2 = g * g
        m = b1 * m + one_b1 * g
        v = b2 * v + one_b2 * g2
        num = lr_t * m
        den = np.sqrt(v) + eps
        p = p - num / den
    assert p.dtype == m.dtype == v.dtype == g.dtype
    return p, m, v


def trajectory(ws, x, steps, dtype):
    """``steps`` Adam steps on the fixed batch in torch ``dtype`` -> the losses before each step [steps] and the final 12 arrays."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    ws = [np.asarray(w, np.float32).reshape(s).astype(npd) for w, s in zip(ws, SHAPES)]
    ms = [np.zeros_like(w) for w in ws]
    vs = [np.zeros_like(w) for w in ws]
    losses = []
    for t in range(1, steps + 1):
        params = [torch.tensor(w, dtype=dtype, requires_grad=True) for w in ws]
        loss, _ = forward(params, x)
        loss.backward()
        losses.append(float(loss.item()))
        for i, p in enumerate(params):
            ws[i], ms[i], vs[i] = adam_step(ws[i], p.grad.numpy().astype(npd), ms[i], vs[i], t)
    return np.array(losses), ws


# ---- the reference checks itself -----------------------------------------------------------------------------------------------
def self_check(name, tol=1e-6):
    """float64, one 4 x 8 image: (L(w + h d) - L(w - h d)) / 2h against g . d to ``tol`` relative, d = (g / |g| + r / |r|) / sqrt 2 with
    r a seeded normal direction; h is the decade at which two neighbouring step sizes agree best among the steps that cross no relu
    or pooling kink (netref64_train's method).  A bias-free model sits ON kinks where the image is empty: a pixel whose 3 x 3
    neighbourhood holds no return has conv2d_1 = 0 exactly, and any step along a relu layer's bias moves it one way for +h and the other
    for -h.  So every other direction has no component along those five biases, and g . d is taken over the same components.
    -> (h, central difference, g . d)."""
    ws = model(name)
    x = images(1, 4, 8, seed=5)
    _, g, _ = loss_and_grads(ws, x)
    base = [np.asarray(w, np.float64).reshape(s) for w, s in zip(ws, SHAPES)]
    gn = np.sqrt(sum(float((a * a).sum()) for a in g))

    def at(d, h):
        with torch.no_grad():
            l, t = forward([torch.tensor(w + h * a, dtype=torch.float64) for w, a in zip(base, d)], x)
        return float(l.item()), t

    for seed in range(20):
        rs = np.random.RandomState(2000 + seed)
        r = [rs.standard_normal(s) for s in SHAPES]
        gs = g
        if seed % 2:    # every other direction leaves the relu layers' biases alone (see the docstring)
            r = [np.zeros_like(a) if t in (1, 3, 5, 7, 9) else a for t, a in enumerate(r)]
            gs = [np.zeros_like(a) if t in (1, 3, 5, 7, 9) else a for t, a in enumerate(g)]
        rn = np.sqrt(sum(float((a * a).sum()) for a in r))
        d = [(a / gn + b / rn) / np.sqrt(2.0) for a, b in zip(gs, r)]
        gd = sum(float((a * b).sum()) for a, b in zip(g, d))
        hs = [10.0 ** -k for k in range(2, 9)]
        ev = [(at(d, h), at(d, -h)) for h in hs]
        cd = [(p[0] - m[0]) / (2 * h) for (p, m), h in zip(ev, hs)]
        same = [same_branch(p[1], m[1]) for p, m in ev]
        pairs = [i for i in range(len(hs) - 1) if same[i] and same[i + 1]]
        if not pairs:
            continue
        best = min(pairs, key=lambda i: abs(cd[i] - cd[i + 1]))
        assert abs(cd[best] - gd) <= tol * abs(gd), (name, seed, hs[best], cd[best], gd)
        return hs[best], cd[best], gd
    raise AssertionError("no direction among 20 left every relu sign and pooling argmax unchanged at two neighbouring steps")
