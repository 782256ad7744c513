"""Host helpers of the Harris3D key point detector (csrc/harris.hip, Engine.harris_keypoints, detect_keypoints.py): the parameter
checks of the C ABI.  The plumbing round the detector call (thinning, subsampling, ensure_keypoint_number) is caelo.iss's, shared by
both detectors.  Importable without a GPU.  The detector itself runs on the device only; nothing here computes a key point.
"""
from .iss import MAX_POINTS, _finite, ensure_keypoint_number, subsample, voxel_downsample  # noqa: F401  (one copy for both detectors)

# PclKeyPts.py:50-51
DEFAULTS = dict(radius=1.0, threshold=0.001)


def check_params(**params):
    """The parameters of caelo_harris_keypoints with the defaults filled in -> dict.  ValueError for what the C ABI refuses: an unknown
    name, a radius that is not finite and positive, a threshold that is not finite or is negative."""
    unknown = sorted(set(params) - set(DEFAULTS))
    if unknown:
        raise ValueError("Harris parameters are %s (got %s)" % (", ".join(DEFAULTS), ", ".join(unknown)))
    p = dict(DEFAULTS)
    p.update(params)
    if isinstance(p["radius"], bool) or not _finite(p["radius"]) or not float(p["radius"]) > 0.0:
        raise ValueError("Harris radius must be finite and positive (got %r)" % (p["radius"],))
    if isinstance(p["threshold"], bool) or not _finite(p["threshold"]) or float(p["threshold"]) < 0.0:
        raise ValueError("Harris threshold must be finite and not negative (got %r)" % (p["threshold"],))
    p["radius"], p["threshold"] = float(p["radius"]), float(p["threshold"])
    return p
