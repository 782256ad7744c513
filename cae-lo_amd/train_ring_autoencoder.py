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
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--scans", help="directory of KITTI velodyne .bin files")
    src.add_argument("--synthetic", type=int, help="number of synthetic 64x2000 scans (caelo.synth)")
    ap.add_argument("--init", required=True, help="ring autoencoder .h5: the weights to fine-tune and the template of --out")
    ap.add_argument("--glorot", type=int, metavar="SEED", help="start from fresh glorot_uniform weights (--init: the template only)")
    ap.add_argument("--calib-angle", type=float, metavar="DEG", help="CorrectPC's vertical-angle calibration, applied before the projection")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--files-per-step", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=4, help="images whose activations are held at once (54 MB each)")
    ap.add_argument("--seed", type=int, default=0, help="shuffles the scans")
    ap.add_argument("--out", required=True, help="the trained autoencoder .h5")
    ap.add_argument("--out-respond", required=True, help="the trained response layer's .h5 (run_sequence.py --respond-h5)")
    ap.add_argument("--log", help="per-epoch losses (.mat: loss, val_loss)")
    a = ap.parse_args(argv)
    if a.epochs < 1 or a.files_per_step < 1 or not 1 <= a.chunk <= 4096 or (a.synthetic is not None and a.synthetic < 1):
        ap.error("--epochs, --files-per-step and --synthetic must be >= 1, --chunk in [1, 4096]")
    if a.calib_angle is not None and not np.isfinite(a.calib_angle):
        ap.error("--calib-angle must be a finite number of degrees")
    import caelo
    from caelo import keras_config, stageio, synth, train_ring
    from caelo.engine import Engine
    caelo.configure_runtime()
    ws = keras_config.read_ring_autoencoder(a.init)
    if a.glorot is not None:
        ws = train_ring.glorot_uniform(keras_config.RING_AE_SHAPES, np.random.RandomState(a.glorot))
    if a.scans:
        files = sorted(glob.glob(os.path.join(a.scans, "*.bin")))
        if not files:
            ap.error("no .bin files in %s" % a.scans)
        read = [lambda f=f: stageio.read_scan(f) for f in files]
    else:
        read = [lambda f=f: synth.make_scan(f, quantum=1e-3) for f in range(a.synthetic)]
    eng = Engine()
    if a.calib_angle is not None:
        import torch
        scans = [lambda r=r: eng.correct_pc(torch.from_numpy(np.ascontiguousarray(r(), dtype=np.float32)).to(eng.device), a.calib_angle) for r in read]
    else:
        scans = read
    tr = train_ring.RingTrainer(eng, ws, chunk=a.chunk)
    hist = train_ring.fit(tr, scans, epochs=a.epochs, files_per_step=a.files_per_step, seed=a.seed)
    keras_config.write_ring_models_like(a.init, a.out, tr.weights(), out_respond_h5=a.out_respond)
    if a.log:
        from scipy import io
        io.savemat(a.log, hist)
    print("trained %d epochs: loss %.6f -> %.6f, val_loss %.6f -> %s, %s" % (a.epochs, hist["loss"][0], hist["loss"][-1], hist["val_loss"][-1], a.out, a.out_respond))
    return 0


if __name__ == "__main__":
    sys.exit(main())
