"""Host helpers of the SIFT3D key point detector (csrc/sift.hip, Engine.sift_octave / sift_keypoints, detect_keypoints.py): the
parameter checks and the scales of an octave.  The plumbing round the detector call (thinning, subsampling, ensure_keypoint_number)
is caelo.iss's, shared by all three detectors.  Importable without a GPU.  The detector itself runs on the device only; nothing here
computes a key point.
"""
import numpy as np

from .iss import MAX_POINTS, _finite, ensure_keypoint_number, subsample, voxel_downsample  # noqa: F401  (one copy for the detectors)

# PclKeyPts.py:55-58
DEFAULTS = dict(min_scale=0.5, n_octaves=4, n_scales_per_octave=8, min_contrast=0.1)
K = 25            # include/caelo.h CAELO_SIFT_K: the neighbourhood of the extremum rule, and the fewest points an octave runs on
MAX_SCALES = 19   # include/caelo.h CAELO_SIFT_MAX_SCALES = 16 + 3


def _integer_in(v, lo, hi):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and lo <= int(v) <= hi


def check_params(**params):
    """The parameters of Engine.sift_keypoints with the defaults filled in -> dict.  ValueError for an unknown name, a min_scale that
    is not finite and positive, n_octaves outside [1, 8], n_scales_per_octave outside [1, 16] (both integers), a min_contrast that is
    not finite or is negative."""
    unknown = sorted(set(params) - set(DEFAULTS))
    if unknown:
        raise ValueError("SIFT parameters are %s (got %s)" % (", ".join(DEFAULTS), ", ".join(unknown)))
    p = dict(DEFAULTS)
    p.update(params)
    if isinstance(p["min_scale"], bool) or not _finite(p["min_scale"]) or not float(p["min_scale"]) > 0.0:
        raise ValueError("SIFT min_scale must be finite and positive (got %r)" % (p["min_scale"],))
    if not _integer_in(p["n_octaves"], 1, 8):
        raise ValueError("SIFT n_octaves must be an integer in [1, 8] (got %r)" % (p["n_octaves"],))
    if not _integer_in(p["n_scales_per_octave"], 1, MAX_SCALES - 3):
        raise ValueError("SIFT n_scales_per_octave must be an integer in [1, %d] (got %r)" % (MAX_SCALES - 3, p["n_scales_per_octave"]))
    if isinstance(p["min_contrast"], bool) or not _finite(p["min_contrast"]) or float(p["min_contrast"]) < 0.0:
        raise ValueError("SIFT min_contrast must be finite and not negative (got %r)" % (p["min_contrast"],))
    p["min_scale"], p["min_contrast"] = float(p["min_scale"]), float(p["min_contrast"])
    p["n_octaves"], p["n_scales_per_octave"] = int(p["n_octaves"]), int(p["n_scales_per_octave"])
    return p


def octave_scales(scale, n_scales_per_octave):
    """The n_scales_per_octave + 3 scales of the octave whose base scale is ``scale``: sigma[s] = scale * 2.0 ** ((s - 1) /
    n_scales_per_octave), float64 (PCL's SIFTKeypoint::detectKeypointsForOctave).  The kernel is handed these numbers, so it and
    whoever restates it see the same bits."""
    if isinstance(scale, bool) or not _finite(scale) or not float(scale) > 0.0:
        raise ValueError("the octave's scale must be finite and positive (got %r)" % (scale,))
    if not _integer_in(n_scales_per_octave, 1, MAX_SCALES - 3):
        raise ValueError("n_scales_per_octave must be an integer in [1, %d] (got %r)" % (MAX_SCALES - 3, n_scales_per_octave))
    n = int(n_scales_per_octave)
    return np.array([float(scale) * 2.0 ** ((s - 1) / n) for s in range(n + 3)], dtype=np.float64)


def check_scales(sigma):
    """sigma -> float64 [S]; ValueError for what caelo_sift_octave refuses: S outside [3, 19], a scale that is not finite and positive,
    scales that do not increase."""
    try:
        s = np.array(sigma, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("SIFT sigma must be a list of numbers (got %r)" % (sigma,))
    if not 3 <= s.shape[0] <= MAX_SCALES:
        raise ValueError("SIFT takes 3 to %d scales (got %d)" % (MAX_SCALES, s.shape[0]))
    if not (np.isfinite(s).all() and (s > 0).all() and (np.diff(s) > 0).all()):
        raise ValueError("SIFT scales must be finite, positive and increasing (got %s)" % (s.tolist(),))
    return s
