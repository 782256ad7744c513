#!/usr/bin/env python
"""train_ring_autoencoder.py -- AE4SphericalRingPC.py's training on this engine (caelo.train_ring): scans -> spherical rings -> loss,
gradient and Adam on the GPU -> the autoencoder .h5 and the response-layer .h5 that run_sequence.py --respond-h5 reads.

    python train_ring_autoencoder.py (--scans <seq>/velodyne | --synthetic N) --init AE4SphericalRingPC.h5 [--glorot SEED]
                                     [--calib-angle DEG] [--epochs 10] [--files-per-step 32] [--chunk 4] [--seed 0]
                                     --out new_AE.h5 --out-respond new_RespondLayer.h5 [--log loss.mat]

--init is the model to fine-tune and the template of --out: the result is a byte copy of it with the weight datasets overwritten
(keras_config.write_ring_models_like); --out-respond is the same of the shipped weights/SphericalRingPCRespondLayer.h5 with the first
two layers' weights.  --glorot SEED starts from fresh glorot_uniform weights instead and uses --init as the template only.
--calib-angle applies CorrectPC before the projection, as run_sequence.py does (the reference trains on corrected scans).  Each step
takes --files-per-step scans (the reference's 2 GPUs x 16), read in place at 64 x 1792 x 3; 90 % of the shuffled scans train, 10 %
validate; --log gets the per-epoch losses.  Single GPU: multi_gpu_model only splits a batch whose merged gradient is the one computed
here.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from caelo import train_cli as cli  # noqa: E402  (no torch, no library: --help stays cheap)


def main(argv=None):
    ap = argparse.ArgumentParser()
    cli.source(ap)
    ap.add_argument("--init", required=True, help="ring autoencoder .h5: the weights to fine-tune and the template of --out")
    cli.option(ap, "--glorot", help="start from fresh glorot_uniform weights (--init: the template only)")
    ap.add_argument("--calib-angle", type=float, metavar="DEG", help="CorrectPC's vertical-angle calibration, applied before the projection")
    cli.option(ap, "--epochs")
    cli.option(ap, "--files-per-step", default=32)
    ap.add_argument("--chunk", type=int, default=4, help="images whose activations are held at once (54 MB each)")
    cli.option(ap, "--seed", help="shuffles the scans")
    ap.add_argument("--out", required=True, help="the trained autoencoder .h5")
    ap.add_argument("--out-respond", required=True, help="the trained response layer's .h5 (run_sequence.py --respond-h5)")
    cli.option(ap, "--log")
    a = ap.parse_args(argv)
    cli.check(ap, a, 1 <= a.chunk <= 4096, "--epochs, --files-per-step and --synthetic must be >= 1, --chunk in [1, 4096]")
    if a.calib_angle is not None and not np.isfinite(a.calib_angle):
        ap.error("--calib-angle must be a finite number of degrees")
    import caelo
    from caelo import keras_config, train_ring
    from caelo.engine import Engine
    caelo.configure_runtime()
    ws = keras_config.read_ring_autoencoder(a.init)
    if a.glorot is not None:
        ws = train_ring.glorot_uniform(keras_config.RING_AE_SHAPES, np.random.RandomState(a.glorot))
    read = cli.scans(ap, a)
    eng = Engine()
    if a.calib_angle is not None:
        import torch
        scans = [lambda r=r: eng.correct_pc(torch.from_numpy(np.ascontiguousarray(r(), dtype=np.float32)).to(eng.device), a.calib_angle) for r in read]
    else:
        scans = read
    tr = train_ring.RingTrainer(eng, ws, chunk=a.chunk)
    hist = train_ring.fit(tr, scans, epochs=a.epochs, files_per_step=a.files_per_step, seed=a.seed)
    keras_config.write_ring_models_like(a.init, a.out, tr.weights(), out_respond_h5=a.out_respond)
    cli.finish(a, hist, a.out, a.out_respond)
    return 0


if __name__ == "__main__":
    sys.exit(main())
