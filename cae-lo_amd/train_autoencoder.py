#!/usr/bin/env python
"""train_autoencoder.py -- AE4VoxelPatch.py's training on this engine (caelo.train): scans -> key points -> patches -> loss, gradient
and Adadelta on the GPU -> an autoencoder .h5 that run_sequence.py --encoder-h5 and evaluate.py reconstruction read.

    python train_autoencoder.py (--scans <seq>/velodyne | --synthetic N) --init AutoencoderModel4VoxelPatch.h5 [--glorot SEED]
                                [--init-encoder encoder_half.h5] [--epochs 10] [--files-per-step 2] [--chunk 256] [--seed 0]
                                --out new.h5 [--out-encoder new_encoder_half.h5] [--log loss.mat]

--init is the model to fine-tune and the template of the output: the result is a byte copy of it with the weight datasets overwritten
(keras_config.write_autoencoder_like), so layer names and activations are the template's.  --glorot SEED starts from fresh
glorot_uniform weights instead and uses --init for shape and activations only.  --init-encoder / --out-encoder: the encoder's file
when --init was cut down to the decoder's weights.  Each step takes --files-per-step scans, 256 key points each, three patches per key
point (the reference's batch of 1 536); 90 % of the shuffled scans train, 10 % validate; --log gets the per-epoch losses.
Single GPU: multi_gpu_model only splits a batch whose merged gradient is the one computed here.
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
    ap.add_argument("--init", required=True, help="autoencoder .h5: the weights to fine-tune and the template of --out")
    ap.add_argument("--init-encoder", help="the encoder's .h5 when --init holds the decoder's weights only")
    cli.option(ap, "--glorot", help="start from fresh glorot_uniform weights (--init: shape and activations)")
    cli.option(ap, "--epochs")
    cli.option(ap, "--files-per-step", default=2)
    ap.add_argument("--chunk", type=int, default=256, help="patches whose activations are held at once (about 480 KB each)")
    cli.option(ap, "--seed", help="shuffles the scans and draws the training points")
    ap.add_argument("--out", required=True, help="the trained autoencoder .h5")
    ap.add_argument("--out-encoder", help="the trained encoder's .h5 (with --init-encoder)")
    cli.option(ap, "--log")
    a = ap.parse_args(argv)
    cli.check(ap, a, a.chunk >= 1, "--epochs, --files-per-step, --chunk and --synthetic must be >= 1")
    if bool(a.init_encoder) != bool(a.out_encoder):
        ap.error("--init-encoder and --out-encoder go together")
    import caelo
    from caelo import keras_config, train
    from caelo.engine import Engine
    caelo.configure_runtime()
    ews, eact, dws, dact = keras_config.read_autoencoder(a.init)
    if a.init_encoder:
        ews, eact, _, _ = keras_config.read_autoencoder(a.init_encoder)
    if ews is None or dws is None:
        ap.error("%s holds one half of the weights only (pass --init-encoder)" % a.init)
    if a.glorot is not None:
        fresh = train.glorot_uniform(train.SHAPES, np.random.RandomState(a.glorot))
        ews, dws = fresh[:10], fresh[10:]
    scans = cli.scans(ap, a)
    eng = Engine()
    tr = train.Trainer(eng, ews, eact, dws, dact, chunk=a.chunk)
    hist = train.fit(tr, scans, epochs=a.epochs, files_per_step=a.files_per_step, seed=a.seed)
    ews, dws = tr.weights()
    if a.out_encoder:
        keras_config.write_autoencoder_like(a.init_encoder, a.out_encoder, ews, None, activations=(eact, dact))
        keras_config.write_autoencoder_like(a.init, a.out, None, dws, activations=(eact, dact))
    else:
        keras_config.write_autoencoder_like(a.init, a.out, ews, dws, activations=(eact, dact))
    cli.finish(a, hist, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
