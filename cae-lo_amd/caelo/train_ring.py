"""Training the spherical-ring autoencoder on the device (AE4SphericalRingPC.py:65-170; csrc/train_ring.hip) -- the network whose
first two layers are the response layer of the key-point detector.

``RingTrainer`` holds the 12 weight tensors as ONE flat float32 device buffer in Keras layout (``param_layout``), asks the library for
the mean-squared-error loss and its gradient (caelo_ring_autoencoder_grad) and takes Keras 2.2.4's Adam step (caelo_adam_step; the
bias-corrected step size lr_t is computed here in float64 and rounded once).  ``ring_batch`` projects scans into the rings the
reference trains on, ``fit`` restates its epoch loop; ``glorot_uniform`` is caelo.train's.  The result is written with
``keras_config.write_ring_models_like``.  Single GPU: ``multi_gpu_model`` only splits a batch whose merged gradient is the one
computed here.
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from .engine import NET_H, NET_W, RESPOND_SHAPES, RING_C, RING_H, RING_W, _ptr
from .keras_config import RING_AE_SHAPES
from .train import FlatTrainer, _fit, glorot_uniform  # noqa: F401  (glorot_uniform is shape-generic: glorot_uniform(RING_AE_SHAPES, rng))

N_PARAMS = 5835
# Keras 2.2.4 Adam defaults (optimizer='Adam', AE4SphericalRingPC.py:150); epsilon = K.epsilon()
LR, BETA_1, BETA_2, EPSILON = 0.001, 0.9, 0.999, 1e-7
assert [tuple(s) for s in RING_AE_SHAPES[:4]] == [tuple(s) for s in RESPOND_SHAPES]


def param_layout():
    """caelo_ring_train_param_layout -> [(offset, count)] of the 12 tensors in the flat buffer, ``RING_AE_SHAPES`` order."""
    out = (C.c_int64 * 24)()
    _ffi.check(_ffi.load().caelo_ring_train_param_layout(C.cast(out, C.c_void_p)))
    return [(int(out[2 * t]), int(out[2 * t + 1])) for t in range(12)]


def adam_lr_t(t, lr=LR, beta_1=BETA_1, beta_2=BETA_2):
    """Keras's lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t) of step t >= 1, in float64, rounded to float32 once."""
    return np.float32(float(lr) * np.sqrt(1.0 - float(beta_2) ** int(t)) / (1.0 - float(beta_1) ** int(t)))


class RingTrainer(FlatTrainer):
    """The ring autoencoder's weights on ``eng``'s device, trainable with Keras 2.2.4's Adam (``m``, ``v``: its moments, ``t``: the steps
    taken).  ``ws12``: the 12 arrays in Keras layout (``RING_AE_SHAPES`` or flat).  ``chunk``: images whose activations the workspace
    holds at once (54 MB each at 64 x 1792).  ``images`` of every method: a ``[n, h, w, 3]`` float32 tensor (h and w multiples of 4),
    or a ``[n, 69, 1800, 5]`` batch of projected rings, which is read in place at h = 64, w = 1792, channels 0..2, through the strides."""

    def __init__(self, eng, ws12, chunk=4):
        if not 1 <= int(chunk) <= 4096:
            raise ValueError("chunk must be in [1, 4096]")
        ws = eng._weight_arrays(list(ws12), [tuple(s) for s in RING_AE_SHAPES], "ring autoencoder")
        super().__init__(eng, ws, RING_AE_SHAPES, param_layout(), N_PARAMS, chunk)
        (self.m, self.v), self.t = self.state, 0

    def _images(self, images):
        if not isinstance(images, torch.Tensor):
            images = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32))
        images = images.to(self.eng.device).contiguous()
        if images.dtype != torch.float32 or images.dim() != 4:
            raise ValueError("images: a [n, h, w, 3] float32 tensor or a [n, %d, %d, %d] batch of rings" % (RING_H, RING_W, RING_C))
        n = int(images.shape[0])
        if tuple(images.shape[1:]) == (RING_H, RING_W, RING_C):
            return images, n, NET_H, NET_W, (RING_H * RING_W * RING_C, RING_W * RING_C, RING_C)
        if images.shape[3] != 3:
            raise ValueError("images: a [n, h, w, 3] float32 tensor or a [n, %d, %d, %d] batch of rings, got %s" % (RING_H, RING_W, RING_C, tuple(images.shape)))
        h, w = int(images.shape[1]), int(images.shape[2])
        return images, n, h, w, (h * w * 3, w * 3, 3)

    def ws_bytes(self, h, w):
        need = int(self.eng.lib.caelo_ring_train_ws_bytes(h, w, self.chunk))
        if need <= 0:
            raise ValueError("image size %d x %d: h and w must be positive multiples of 4 (Keras pads its 'same' poolings elsewhere; not built)" % (h, w))
        return need

    def _call(self, images, grads, recon=False):
        eng = self.eng
        images, n, h, w, strides = self._images(images)
        ws = eng._ws("train_ring", self.ws_bytes(h, w))
        out = eng.empty((n, h, w, 3), torch.float32) if recon else None
        _ffi.check(eng.lib.caelo_ring_autoencoder_grad(eng.ctx, _ptr(self.params), _ptr(images) if n else None, n, h, w, strides[0], strides[1], strides[2],
                                                       self.chunk, _ptr(self.grads) if grads else None, _ptr(self._loss), _ptr(out) if recon and n else None,
                                                       _ptr(ws), eng.stream))
        return out

    def _next_optimizer_step(self):
        self.t += 1
        return "caelo_adam_step", (float(adam_lr_t(self.t)), BETA_1, BETA_2, EPSILON)

    def predict(self, images):
        """autoencoder.predict -> [n, h, w, 3] float32 on the device."""
        return self._call(images, False, recon=True)

    def respond_weights(self):
        """-> conv2d_1 and conv2d_2 (kernel, bias each): the response layer the reference saves beside the autoencoder."""
        return self.weights()[:4]

    def install(self):
        """Hand the response layer to the engine's key-point detector (Engine.set_respond_weights)."""
        self.eng.set_respond_weights(self.respond_weights())


def ring_batch(eng, scans):
    """Each scan ([N, 4] float32, array or tensor) -> ``eng.project`` -> one [n, 69, 1800, 5] tensor of rings, which ``RingTrainer``
    reads in place (SphericalRing[0:64, 0:1792, 0:3], AE4SphericalRingPC.py:74)."""
    from .engine import raise_status
    rings = []
    for pc in scans:
        pc = pc if isinstance(pc, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32))
        ring, _, status = eng.project(pc.to(eng.device).contiguous())
        raise_status(int(status[0].item()))
        rings.append(ring)
    return torch.stack(rings) if rings else eng.zeros((0, RING_H, RING_W, RING_C), torch.float32)


def fit(trainer, scans, epochs=10, files_per_step=32, seed=0, train_ratio=0.9, log=print):
    """The reference's epoch loop (AE4SphericalRingPC.py:96-105, 81-89, 157-166).  ``scans``: a list of callables, each returning one
    [N, 4] f32 cloud (files are read when their step comes).  The list is shuffled, the first ``train_ratio`` of it trains, the rest
    validates; a step takes ``files_per_step`` scans (YieldBatchData's strict bound: a list of L files gives (L - 1) // files_per_step
    steps per pass, at least one here).  -> dict ``loss`` / ``val_loss`` [epochs] f64, the epoch means (``val_loss`` is NaN without
    validation files)."""
    return _fit(trainer, scans, lambda files, rng: ring_batch(trainer.eng, [scans[i]() for i in files]), epochs, files_per_step, seed, train_ratio, log)
