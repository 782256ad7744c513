"""Training the voxel-patch autoencoder on the device (AE4VoxelPatch.py:58-233; csrc/train.hip).

``Trainer`` holds the 20 weight tensors as ONE flat float32 device buffer in Keras layout (``param_layout``), asks the library for the
loss and its gradient (caelo_autoencoder_grad) and takes Keras 2.3's Adadelta step (caelo_adadelta_step).  ``sample_training_points``
restates the reference's choice of training points, ``fit`` its epoch loop, ``glorot_uniform`` Keras's default initialiser.  The
result is written with ``keras_config.write_autoencoder_like``.  Single GPU: ``multi_gpu_model`` only splits a batch whose merged
gradient is the one computed here.  What caelo.train_ring shares lives here once: ``FlatTrainer`` (the flat buffers and loss / grad /
step / weights on them) and ``_fit`` (the epoch loop); what the two command lines share is caelo.train_cli.
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from .engine import ACTIVATION_CODES, DECODER_SHAPES, ENCODER_SHAPES, _ptr

SHAPES = list(ENCODER_SHAPES) + list(DECODER_SHAPES)
N_PARAMS = 864741
# Keras 2.3 Adadelta defaults (optimizer='adadelta', AE4VoxelPatch.py:213)
LR, RHO, EPSILON = 1.0, 0.95, 1e-7

# Voxel.py:15-52 -- the voxel grid the training points are cropped in
_VOXEL_SIZE, _BLOCK_REAL = 0.02, 1.28
BLOCK_SIZE = int(_BLOCK_REAL / _VOXEL_SIZE)
CROP_BLOCKS = int(32 * int(16 / 2) / BLOCK_SIZE)
N_BLOCKS = (int(2 * 100 / _BLOCK_REAL), int(2 * 100 / _BLOCK_REAL), int(2 * 15 / _BLOCK_REAL))
VISIBLE_RANGE = np.array([nb / 2 * _BLOCK_REAL for nb in N_BLOCKS], dtype=np.float32).reshape(1, 3)
RESERVE_RATIO = 10


def param_layout():
    """caelo_train_param_layout -> [(offset, count)] of the 20 tensors in the flat buffer, ``SHAPES`` order."""
    out = (C.c_int64 * 40)()
    _ffi.check(_ffi.load().caelo_train_param_layout(C.cast(out, C.c_void_p)))
    return [(int(out[2 * t]), int(out[2 * t + 1])) for t in range(20)]


def glorot_uniform(shapes, rng):
    """Keras's default initialisers for a fresh start: glorot_uniform kernels (U(-l, l), l = sqrt(6 / (fan_in + fan_out)), fans =
    receptive field x channels), zero biases -> float32 arrays of ``shapes``.  ``rng``: a numpy RandomState."""
    out = []
    for s in shapes:
        if len(s) == 1:
            out.append(np.zeros(s, np.float32))
            continue
        field = int(np.prod(s[:-2]))
        lim = np.sqrt(6.0 / (field * s[-2] + field * s[-1]))
        out.append(rng.uniform(-lim, lim, size=s).astype(np.float32))
    return out


def sample_training_points(key_pts, n_groups, rng):
    """BatchInputData's choice of training points with RandDataSource = 1 (AE4VoxelPatch.py:93-126), in its dtypes: 10 n_groups indices
    ``int(random() (K - 1) + 1)`` (index 0 is never drawn, repeats are allowed), the voxel ``(pt + range) / 0.02`` unrounded, points in
    the outer CropBlocks = 4 blocks of any axis dropped, the first ``n_groups`` survivors taken -> [n_groups, 3] float32.  ValueError
    where the reference asserts (fewer survivors).  ``rng``: a numpy RandomState (the reference draws from numpy's global one)."""
    key_pts = np.asarray(key_pts)
    idx = rng.random_sample((n_groups * RESERVE_RATIO,))
    idx = np.array(idx * (key_pts.shape[0] - 1) + 1, dtype=int)
    lo = CROP_BLOCKS * BLOCK_SIZE
    hi = [(nb - CROP_BLOCKS) * BLOCK_SIZE for nb in N_BLOCKS]
    out = np.zeros((n_groups, 3), dtype=np.float32)
    cnt = 0
    for i in idx:
        voxel0 = ((key_pts[i, :] + VISIBLE_RANGE) / _VOXEL_SIZE).reshape(3,)
        if any(voxel0[a] < lo or voxel0[a] >= hi[a] for a in range(3)):
            continue
        out[cnt, :] = (voxel0 * _VOXEL_SIZE).reshape(1, 3) - VISIBLE_RANGE
        cnt += 1
        if cnt == n_groups:
            break
    if cnt != n_groups:
        raise ValueError("only %d of %d drawn key points lie inside the cropped grid (the reference asserts cntValidPt == nPatchGroups)"
                         % (cnt, n_groups))
    return out


class FlatTrainer:
    """What the two trainers (``Trainer`` here, ``train_ring.RingTrainer``) share: the weight tensors ``ws`` of ``shapes`` as ONE flat
    float32 device buffer ``params`` in the library's ``layout`` of ``n_params`` floats, the gradient ``grads`` and the optimizer's two
    ``state`` buffers in the same layout.  A subclass supplies ``_call(batch, grads)`` -- the library's loss (and, with ``grads``,
    gradient) of a batch into ``_loss`` (and ``grads``) -- and ``_next_optimizer_step()`` -> (the step's C symbol, its hyperparameters),
    which ``step`` calls exactly once per step: it may count (Adam's t)."""

    def __init__(self, eng, ws, shapes, layout, n_params, chunk):
        self.eng, self.chunk, self.shapes, self.layout = eng, int(chunk), shapes, layout
        assert sum(c for _, c in layout) == n_params and [c for _, c in layout] == [w.size for w in ws]
        self.params = torch.from_numpy(np.concatenate([w.ravel() for w in ws])).to(eng.device)
        self.grads = eng.zeros((n_params,), torch.float32)
        self.state = (eng.zeros((n_params,), torch.float32), eng.zeros((n_params,), torch.float32))
        self._loss = eng.zeros((1,), torch.float32)

    def _split(self, flat):
        return [flat[o:o + c].reshape(s).copy() for (o, c), s in zip(self.layout, self.shapes)]

    def loss(self, batch):
        """The mean loss of the batch (forward only; ``Trainer``: binary_crossentropy, ``RingTrainer``: mean_squared_error against the
        batch itself) -> float.  Synchronises."""
        self._call(batch, False)
        return float(self._loss.item())

    def grad(self, batch):
        """-> (loss, the gradient arrays in ``shapes``).  Synchronises."""
        self._call(batch, True)
        return float(self._loss.item()), self._split(self.grads.cpu().numpy())

    def step(self, batch, sync=True):
        """One optimizer step (``Trainer``: Adadelta, ``RingTrainer``: Adam) on the batch -> its loss BEFORE the step (what Keras logs); ``sync=False`` returns the device scalar."""
        self._call(batch, True)
        eng = self.eng
        symbol, hyper = self._next_optimizer_step()    # once per step, here only: RingTrainer's advances t
        _ffi.check(getattr(eng.lib, symbol)(eng.ctx, _ptr(self.params), _ptr(self.grads), _ptr(self.state[0]), _ptr(self.state[1]),
                                            self.params.numel(), *hyper, eng.stream))
        return float(self._loss.item()) if sync else self._loss.clone()

    def weights(self):
        """-> the current weights, float32 arrays in Keras layout."""
        return self._split(self.params.cpu().numpy())


class Trainer(FlatTrainer):
    """The autoencoder's weights on ``eng``'s device, trainable with Keras 2.3's Adadelta (``acc_g``, ``acc_d``: its accumulators).
    ``ews`` / ``dws``: the ten encoder / decoder arrays in Keras layout, ``eact`` = (hidden, code), ``dact`` = (hidden, "sigmoid") -- the
    sets keras_config accepts, anything else is a ValueError before a weight is read.  ``chunk``: patches whose activations the
    workspace holds at once (about 480 KB each).  ``bits`` of every method: the batch's patches, [n, 64] int64 / uint64."""

    def __init__(self, eng, ews, eact, dws, dact, chunk=64):
        try:
            ok = (eact[0] in ("tanh", "relu") and eact[1] in ("tanh", "linear") and dact[0] in ("tanh", "relu") and dact[1] == "sigmoid"
                  and len(eact) == 2 and len(dact) == 2)
        except (TypeError, IndexError):
            ok = False
        if not ok:
            raise ValueError("activations: encoder (hidden, code) with hidden in ('tanh', 'relu') and code in ('tanh', 'linear'), decoder "
                             "(hidden, 'sigmoid'); got %r, %r" % (eact, dact))
        if int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        ws = eng._weight_arrays(list(ews), ENCODER_SHAPES, "encoder") + eng._weight_arrays(list(dws), DECODER_SHAPES, "decoder")
        super().__init__(eng, ws, SHAPES, param_layout(), N_PARAMS, chunk)
        self.eact, self.dact = tuple(eact), tuple(dact)
        self.acc_g, self.acc_d = self.state

    def _bits(self, bits):
        if not isinstance(bits, torch.Tensor):
            a = np.ascontiguousarray(bits)
            bits = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
        bits = bits.to(self.eng.device).contiguous()
        assert bits.dtype == torch.int64 and bits.numel() % 64 == 0, "patches: [n, 64] int64 / uint64"
        return bits, bits.numel() // 64

    def _call(self, bits, grads):
        eng = self.eng
        bits, n = self._bits(bits)
        ws = eng._ws("train", int(eng.lib.caelo_train_ws_bytes(self.chunk)))
        _ffi.check(eng.lib.caelo_autoencoder_grad(eng.ctx, _ptr(self.params), ACTIVATION_CODES[self.eact[0]], ACTIVATION_CODES[self.eact[1]],
                                                  ACTIVATION_CODES[self.dact[0]], _ptr(bits) if n else None, n, self.chunk,
                                                  _ptr(self.grads) if grads else None, _ptr(self._loss), _ptr(ws), eng.stream))

    def _next_optimizer_step(self):
        return "caelo_adadelta_step", (LR, RHO, EPSILON)

    def weights(self):
        """-> (ews, dws): the current weights as float32 arrays in Keras layout."""
        ws = super().weights()
        return ws[:10], ws[10:]

    def install(self):
        """Hand the current weights to the engine's inference paths (set_encoder_weights, set_decoder_weights): ``Engine.encode`` and
        ``Engine.decode`` then run the trained model.  A relu encoder that has left the f16 range of the inference operands is refused
        there (Engine.set_encoder_weights)."""
        ews, dws = self.weights()
        self.eng.set_encoder_weights(ews, activations=self.eact)
        self.eng.set_decoder_weights(dws, self.dact)


def training_patches(eng, pc, n_groups, rng):
    """One scan's training batch: the detector's key points, ``sample_training_points`` of them, the three scales' patches of those
    points -> [3 n_groups, 64] int64 on the device."""
    from .engine import raise_status
    pc = pc if isinstance(pc, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32))
    pc = pc.to(eng.device).contiguous()
    ff = eng.extract(pc)
    raise_status(int(ff.status[0].item()))
    k = int(ff.n_key.item())
    pts = sample_training_points(ff.rows[:k, 60:63].cpu().numpy(), n_groups, rng)
    ff = eng.extract(pc, key_pts=pts)
    bits = eng.extract_patch_bits()
    raise_status(int(ff.status[0].item()))
    return bits[:n_groups].reshape(3 * n_groups, 64).contiguous()


def fit(trainer, scans, epochs=10, files_per_step=2, points_per_file=256, seed=0, train_ratio=0.9, log=print):
    """The reference's epoch loop (AE4VoxelPatch.py:137-157, 223-232).  ``scans``: a list of callables, each returning one [N,4] f32
    cloud (files are read when their step comes).  The list is shuffled, the first ``train_ratio`` of it trains, the rest validates;
    a step takes ``files_per_step`` scans, ``points_per_file`` key points each, three patches per key point (YieldBatchData's
    strict bound: a list of L files gives (L - 1) // files_per_step steps, at least one here).  -> dict ``loss`` / ``val_loss``
    [epochs] f64, the epoch means (``val_loss`` is NaN without validation files)."""
    def batch_of(files, rng):    # the generator that shuffled the scans goes on to draw every step's training points
        return torch.cat([training_patches(trainer.eng, scans[i](), points_per_file, rng) for i in files])
    return _fit(trainer, scans, batch_of, epochs, files_per_step, seed, train_ratio, log)


def _fit(trainer, scans, batch_of, epochs, files_per_step, seed, train_ratio, log):
    """The epoch loop of both trainers (``fit`` here, ``train_ring.fit``).  ``batch_of(files, rng)``: the batch of one step, ``files``
    its scans' indices, ``rng`` the RandomState(seed) that shuffled the list."""
    rng = np.random.RandomState(seed)
    order = list(range(len(scans)))
    rng.shuffle(order)
    n_train = int(train_ratio * len(order))
    parts = (order[:n_train], order[n_train:])
    if not parts[0]:
        raise ValueError("no training scans (%d given, %g of them train)" % (len(scans), train_ratio))

    def batches(part):
        steps = max((len(part) - 1) // files_per_step, 1) if part else 0
        for s in range(steps):
            yield batch_of(part[s * files_per_step:(s + 1) * files_per_step], rng)

    hist = dict(loss=[], val_loss=[])
    for ep in range(epochs):
        tl = [trainer.step(b, sync=False) for b in batches(parts[0])]
        vl = [trainer.loss(b) for b in batches(parts[1])]
        hist["loss"].append(float(torch.cat(tl).double().mean().item()))
        hist["val_loss"].append(float(np.mean(vl)) if vl else float("nan"))
        if log:
            log("epoch %d/%d: loss %.6f, val_loss %.6f (%d + %d steps)" % (ep + 1, epochs, hist["loss"][-1], hist["val_loss"][-1], len(tl), len(vl)))
    return {k: np.asarray(v, np.float64) for k, v in hist.items()}
