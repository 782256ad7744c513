"""The whole voxel-patch autoencoder (AE4VoxelPatch.py:186-213) as a torch-CPU autograd network built from Keras-layout weights -- the
reference the device's loss and gradients (csrc/train.hip) are pinned to, in float64 (the reference) and float32 (the yardstick for
what float32 arithmetic itself costs).  A helper module, not a conftest, beside netref64_dec.py.

Keras cannot run here, so this is a restatement: Conv3D kernels ``permute(4,3,0,1,2)`` (cross-correlation, zero 'same'
padding), MaxPooling3D(2) = ``max_pool3d`` (whose gradient goes to a window's first maximum in ascending (dx, dy, dz) order;
TensorFlow's rule is unpinned), Flatten and Reshape in (x, y, z, c) order, UpSampling3D(2) = ``repeat_interleave``, the loss =
``binary_cross_entropy_with_logits`` of the logit clamped to +-logit(1 - 1e-7) -- Keras's clip of the probability, whose gradient is 0
beyond the clip.  Also Adadelta (Keras 2.3) in NumPy, the literal loop of BatchInputData's point selection, and the joined fixture.
"""
import numpy as np
import torch
import torch.nn.functional as F

import netref64 as nr
import netref64_dec as nd

SHAPES = list(nr.ENCODER_SHAPES) + list(nd.DECODER_SHAPES)
N_PARAMS = int(sum(int(np.prod(s)) for s in SHAPES))
LOGIT_CLIP = nd.LOGIT_CLIP
_ACT = {"tanh": torch.tanh, "relu": torch.relu, "linear": lambda x: x}


def to_params(ews, dws, dtype=torch.float64):
    """The 20 arrays -> leaf tensors of ``dtype`` in Keras shapes that require a gradient."""
    return [torch.tensor(np.asarray(w, np.float32).reshape(s), dtype=dtype, requires_grad=True) for w, s in zip(list(ews) + list(dws), SHAPES)]


def _conv(x, w, b):   # x [N, Cin, X, Y, Z], w Keras [3,3,3,Cin,Cout]
    return F.conv3d(x, w.permute(4, 3, 0, 1, 2), b, padding=1)


def _up(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)


def forward(params, bits, eact, dact, keep=False):
    """-> (loss, dict).  The dict holds ``z`` [n,4096] logits in (x, y, z) order, ``code`` [n,20], ``p1`` [n,8,8,8,8] (N, C, x, y, z), and
    ``signs`` / ``pools``: the sign pattern of every relu layer's output, and every pooling's input with its argmaxes (what a
    finite-difference step must not change: ``same_branch``).  ``keep``: retain the gradients of z, code and p1."""
    k = params
    dt = k[0].dtype
    h, c, hd = _ACT[eact[0]], _ACT[eact[1]], _ACT[dact[0]]
    assert dact[1] == "sigmoid"
    n = len(bits)
    y = torch.tensor(nr.unpack(bits), dtype=dt).permute(0, 4, 1, 2, 3)
    a1 = h(_conv(y, k[0], k[1]))
    p1, i1 = F.max_pool3d(a1, 2, return_indices=True)
    a2 = h(_conv(p1, k[2], k[3]))
    p2, i2 = F.max_pool3d(a2, 2, return_indices=True)
    a3 = h(_conv(p2, k[4], k[5]))
    f3 = a3.permute(0, 2, 3, 4, 1).reshape(n, 2048)
    h1 = h(f3 @ k[6] + k[7])
    code = c(h1 @ k[8] + k[9])
    h3 = hd(code @ k[10] + k[11])
    g4 = hd(h3 @ k[12] + k[13])
    y4 = hd(_conv(g4.reshape(n, 4, 4, 4, 32).permute(0, 4, 1, 2, 3), k[14], k[15]))
    y5 = hd(_conv(_up(y4), k[16], k[17]))
    z = _conv(_up(y5), k[18], k[19])
    if keep:
        for t in (z, code, p1):
            t.retain_grad()
    loss = F.binary_cross_entropy_with_logits(torch.clamp(z, -LOGIT_CLIP, LOGIT_CLIP), y)
    signs = [t > 0 for t, a in ((a1, eact[0]), (a2, eact[0]), (a3, eact[0]), (h1, eact[0]), (h3, dact[0]), (g4, dact[0]), (y4, dact[0]),
                                (y5, dact[0])) if a == "relu"]
    return loss, dict(z=z, code=code, p1=p1, signs=signs, pools=[(a1.detach(), i1), (a2.detach(), i2)])


def same_branch(t0, t1, tie=1e-12):
    """Two ``forward`` dicts took the same branch of every relu and every pooling window: equal relu sign patterns, and equal pooling
    argmaxes except between cells whose values differ by at most ``tie`` (equal neighbourhoods of a binary patch give equal sums up to
    the summation order: moving the gradient among them is no kink of the loss)."""
    if not all(bool(torch.equal(a, b)) for a, b in zip(t0["signs"], t1["signs"])):
        return False
    for (a, i0), (_, i1) in zip(t0["pools"], t1["pools"]):
        flat = a.flatten(2)
        v0, v1 = flat.gather(2, i0.flatten(2)), flat.gather(2, i1.flatten(2))
        if float((v0 - v1).abs().max()) > tie:
            return False
    return True


def loss_and_grads(ews, eact, dws, dact, bits, dtype=torch.float64):
    """-> (loss, [20 gradient arrays f64], dict: ``dz`` [n,4096], ``dcode`` [n,20], ``dp1`` [n,4096] in (x, y, z, c) order)."""
    params = to_params(ews, dws, dtype)
    loss, t = forward(params, bits, eact, dact, keep=True)
    loss.backward()
    n = len(bits)
    extra = dict(dz=t["z"].grad.reshape(n, 4096).double().numpy(), dcode=t["code"].grad.double().numpy(),
                 dp1=t["p1"].grad.permute(0, 2, 3, 4, 1).reshape(n, 4096).double().numpy())
    return float(loss.item()), [p.grad.double().numpy() for p in params], extra


def patch_losses(ws, eact, dact, bits, dtype=torch.float64):
    """The 20 arrays' network, forward only -> every patch's loss [n] f64 (the batch loss is their mean)."""
    with torch.no_grad():
        z = forward([torch.tensor(np.asarray(w), dtype=dtype) for w in ws], bits, eact, dact)[1]["z"]
        y = torch.tensor(nr.unpack(bits), dtype=dtype).permute(0, 4, 1, 2, 3)
        l = F.binary_cross_entropy_with_logits(torch.clamp(z, -LOGIT_CLIP, LOGIT_CLIP), y, reduction="none")
        return l.reshape(len(bits), -1).mean(dim=1).double().numpy()


# ---- Adadelta -------------------------------------------------------------------------------------------------------------------
def adadelta_step(p, g, a, d, lr=1.0, rho=0.95, eps=1e-7):
    """Keras 2.3's Adadelta in the arrays' dtype, every operation rounded on its own -> (p, a, d) after the step:
    a = rho a + (1 - rho) g^2; u = g sqrt(d + eps) / sqrt(a + eps); p -= lr u; d = rho d + (1 - rho) u^2."""
    t = p.dtype.type
    lr, rho, eps = t(lr), t(rho), t(eps)
    one_rho = t(1) - rho
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g2 = g * g
        a = rho * a + one_rho * g2
        num = g * np.sqrt(d + eps)
        u = num / np.sqrt(a + eps)
        u2 = u * u
        p = p - lr * u
        d = rho * d + one_rho * u2
    assert p.dtype == a.dtype == d.dtype == g.dtype
    return p, a, d


def trajectory(ews, eact, dws, dact, bits, steps, dtype):
    """``steps`` Adadelta steps on the fixed batch in torch ``dtype`` -> the losses before each step [steps] and the final 20 arrays."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    ws = [np.asarray(w, np.float32).reshape(s).astype(npd) for w, s in zip(list(ews) + list(dws), SHAPES)]
    acc = [np.zeros_like(w) for w in ws]
    dlt = [np.zeros_like(w) for w in ws]
    losses = []
    for _ in range(steps):
        params = [torch.tensor(w, dtype=dtype, requires_grad=True) for w in ws]
        loss, _t = forward(params, bits, eact, dact)
        loss.backward()
        losses.append(float(loss.item()))
        for i, p in enumerate(params):
            ws[i], acc[i], dlt[i] = adadelta_step(ws[i], p.grad.numpy().astype(npd), acc[i], dlt[i])
    return np.array(losses), ws


# ---- BatchInputData's points (AE4VoxelPatch.py:93-126, RandDataSource = 1), a literal loop --------------------------------------
def sample_points_loop(key_pts, n_groups, rng):
    """AE4VoxelPatch.py trains at import and cannot be imported, so ``caelo.train.sample_training_points`` is pinned to this restatement
    only.  Constants: Voxel.py:15-52.  AssertionError where the reference asserts."""
    voxel_size, block_real = 0.02, 1.28
    block = int(block_real / voxel_size)
    crop = int(32 * int(16 / 2) / block)
    nb = [int(2 * 100 / block_real), int(2 * 100 / block_real), int(2 * 15 / block_real)]
    vis = np.array([nb[0] / 2 * block_real, nb[1] / 2 * block_real, nb[2] / 2 * block_real], dtype=np.float32).reshape(1, 3)
    rand = rng.random_sample((n_groups * 10,))
    rand = rand * (key_pts.shape[0] - 1) + 1
    rand = np.array(rand, dtype=int)
    cnt = 0
    valid = np.zeros((n_groups, 3), dtype=np.float32)
    for i in range(rand.shape[0]):
        pts = key_pts[rand[i], :]
        voxel0 = ((pts + vis) / voxel_size).reshape(3,)
        if voxel0[0] < crop * block or voxel0[0] >= (nb[0] - crop) * block or voxel0[1] < crop * block or voxel0[1] >= (nb[1] - crop) * block or \
                voxel0[2] < crop * block or voxel0[2] >= (nb[2] - crop) * block:
            continue
        valid[cnt, :] = (voxel0 * voxel_size).reshape(1, 3) - vis
        cnt += 1
        if cnt == n_groups:
            break
    assert cnt == n_groups
    return valid, rand


def templates(directory):
    """-> (encoder-half .h5, decoder-half .h5): the fixture autoencoder is stored as two files, each cut down to one half's weights."""
    import netref64_act as na
    return na.fixture_h5(directory), nd.fixture_h5(directory)
