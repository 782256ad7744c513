"""What train_autoencoder.py and train_ring_autoencoder.py share: the scan source, the options both take, their range checks, the lazy
scan readers, the --log file and the closing line.  Nothing here imports torch or the library, so --help and a usage error cost what
argparse costs."""
import glob
import os

# the options both scripts take; a script adds them where its own --help lists them, with its own default and help text
_OPTIONS = {"--glorot": dict(type=int, metavar="SEED"), "--epochs": dict(type=int, default=10), "--files-per-step": dict(type=int),
            "--seed": dict(type=int, default=0), "--log": dict(help="per-epoch losses (.mat: loss, val_loss)")}


def source(ap):
    """The scan source: --scans or --synthetic, one of them required."""
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--scans", help="directory of KITTI velodyne .bin files")
    src.add_argument("--synthetic", type=int, help="number of synthetic 64x2000 scans (caelo.synth)")


def option(ap, name, **own):
    """One of the shared options, ``own``: the script's default or help text."""
    ap.add_argument(name, **dict(_OPTIONS[name], **own))


def check(ap, a, chunk_ok, message):
    """The range checks of the shared options and of a script's --chunk: ``ap.error(message)`` unless all hold."""
    if a.epochs < 1 or a.files_per_step < 1 or not chunk_ok or (a.synthetic is not None and a.synthetic < 1):
        ap.error(message)


def scans(ap, a):
    """-> one callable per scan (files are read, scans made, when their step comes); ``ap.error`` for a directory without .bin files."""
    from . import stageio, synth
    if not a.scans:
        return [lambda f=f: synth.make_scan(f, quantum=1e-3) for f in range(a.synthetic)]
    files = sorted(glob.glob(os.path.join(a.scans, "*.bin")))
    if not files:
        ap.error("no .bin files in %s" % a.scans)
    return [lambda f=f: stageio.read_scan(f) for f in files]


def finish(a, hist, *outs):
    """--log's file and the closing line."""
    if a.log:
        from scipy import io
        io.savemat(a.log, hist)
    print("trained %d epochs: loss %.6f -> %.6f, val_loss %.6f -> %s" % (a.epochs, hist["loss"][0], hist["loss"][-1], hist["val_loss"][-1], ", ".join(outs)))
