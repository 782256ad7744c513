"""caelo -- MI355X-native CAE-LO feature-and-matching engine (host side).

    caelo.api      the reference's function-level call surface (NumPy or torch-GPU arrays)
    caelo.engine   device engine: fused extract / match_pose hot path, one process per GPU
    caelo.dist     frame sharding + RCCL descriptor all-gather (torch.distributed)
    caelo.h5lite   minimal HDF5 reader for the Keras .h5 weights
    caelo.synth    seeded synthetic KITTI-shaped scans
    caelo._ffi     ctypes binding of libcaelo.so (include/caelo.h)

Sub-modules are imported lazily so that the light ones (h5lite, synth) work without torch.
"""
import importlib
import os

def configure_runtime(hw_queues=8):
    """Report whether the pipeline's fourth stream (voxel maps beside the key-point chain) has the hardware
    queues it needs.

    ROCclr deals HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and reads the variable once, when HIP
    initialises at the first device call.  The fourth stream only pays with >= 8 queues; with the default the pipeline runs
    three streams (same results, a few per cent less throughput).  The queue count is a setting of the device, which other
    processes share, so the package never raises it: whoever runs the process sets it before the first device call.
    Entry points that own their process (bench.py, run_sequence.py, the test session) still call this before touching the
    GPU.  Returns True when the variable is in effect with >= hw_queues, False otherwise (the pipeline reports what it runs
    with through caelo_pipeline_stats)."""
    cur = os.environ.get("GPU_MAX_HW_QUEUES")
    if cur is None:
        return False
    try:
        return int(cur.strip() or 0) >= hw_queues
    except ValueError:   # the runtime reads it with atoi: a value it would take for 0 leaves the default of four queues
        return False


__all__ = ["api", "engine", "dist", "h5lite", "synth", "_ffi", "hostblas", "hostexact", "configure_runtime"]


def __getattr__(name):
    if name in __all__ and name != "configure_runtime":
        return importlib.import_module("." + name, __name__)
    raise AttributeError(name)
