#!/usr/bin/env python
"""Generate tests/golden/planar_pts.npz from the reference's own lines (a read-only reference tree, see make_goldens.py):

    python tools/make_goldens_planar.py <reference directory>

At run time the tool reads GetKeyPtsByAE from the reference's SphericalRing.py, un-comments its per-pixel loop in memory (lines 236-282;
both levels of `#` for the PCA block at 268-276), stands NumPy in for cupy, and runs the result on the crafted image of
tests/planar_images.py.  The loop writes its per-pixel minDiff into DiffImg, whose definition (line 121) stays commented out: the tool
hands it in as a global.  No reference text goes into this file or into the fixture; the fixture holds data only -- the image stored
sparsely (occupied pixels with their count, x/y/z and response vector), the PlanarPts the reference's lines returned, the minDiff they
recorded, and what tests/planar_ref.py makes of the same image (pixels, candidates, eigenvalues) for the comparison rule.

Left out of the golden image, because the reference's lines do something else there than the rule the library states
(include/caelo.h): a NaN response vector (the builtin min of line 253 skips a NaN unless it comes first; the library's stays a NaN)
and a non-finite coordinate (np.linalg.eig raises; the library writes no row).

The script exits non-zero if tests/planar_ref.py disagrees with what the reference's lines computed."""
import copy
import io as _io
import math
import os
import sys
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import planar_images as pi   # noqa: E402
import planar_ref as pr      # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "planar_pts.npz")
CONSTANTS = (27, 68)      # the module's geometry constants and pixel lists
FUNCTION = (113, 291)     # GetKeyPtsByAE
LOOP = (236, 282)         # its commented per-pixel loop
PCA = (268, 276)          # ... whose PCA block is commented once more


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = _io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def reference_function(ref_dir):
    """-> (GetKeyPtsByAE with its loop un-commented, the namespace it runs in)"""
    lines = open(os.path.join(ref_dir, "SphericalRing.py")).read().split("\n")

    def strip_hash(line):
        body = line.lstrip(" ")
        lead = line[:len(line) - len(body)]
        if body.startswith("# "):
            return lead + body[2:]
        return lead + body[1:] if body.startswith("#") else line
    for no in range(LOOP[0], LOOP[1] + 1):
        lines[no - 1] = strip_hash(lines[no - 1])
    for no in range(PCA[0], PCA[1] + 1):
        lines[no - 1] = strip_hash(lines[no - 1])
    numpy_as_cupy = types.ModuleType("cupy")
    numpy_as_cupy.__dict__.update({k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    numpy_as_cupy.asnumpy = np.asarray
    numpy_as_cupy.bool = bool
    ns = {"np": np, "cp": numpy_as_cupy, "LA": np.linalg, "copy": copy, "math": math, "__name__": "ref_SphericalRing"}
    text = "\n".join(lines[CONSTANTS[0] - 1:CONSTANTS[1]] + [""] + lines[FUNCTION[0] - 1:FUNCTION[1]]) + "\n"
    exec(compile(text, "SphericalRing.py (loop un-commented)", "exec"), ns)
    return ns["GetKeyPtsByAE"], ns


def golden_image():
    """The crafted image without its non-finite patches, plus a field of key points: the reference asserts more than 50 of them
    (pixels with minDiff > 0.2 at 10 m or more); theirs is 1 or more, far from PlanarThreshold."""
    im, expect = pi.crafted()
    for name in ("nan_neighbour", "nan_unoccupied", "inf_coordinate"):
        y, x = im.at.pop(name)
        expect.pop(name)
        im.ring[y - 3:y + 4, x - 3:x + 4] = 0
        im.counter[y - 3:y + 4, x - 3:x + 4] = 0
        im.resp[y - 3:y + 4, x - 3:x + 4] = 0
    k = 0
    for y in range(40, 48):
        for x in range(600, 612):
            r = np.zeros(8, np.float32)
            r[k % 8] = 1.0 + k
            im.put(y, x, (30.0 + 0.3 * (x - 600), 0.3 * (y - 40), -1.0 + 0.05 * ((7 * k) % 11)), r)
            k += 1
    return im, expect


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    fn, ns = reference_function(sys.argv[1])
    im, expect = golden_image()
    ns["DiffImg"] = np.zeros((im.ring.shape[0], im.ring.shape[1]), np.float32)
    key_pts, key_pixels, planar = fn(im.ring.copy(), im.counter.copy(), im.resp.copy())
    planar = np.asarray(planar, np.float32).reshape(-1, 6)
    diff_img = ns["DiffImg"]
    ref = pr.planar_points(im.ring, im.counter, im.resp)
    # ---- tests/planar_ref.py against the reference's lines ------------------------------------------------------------------------------
    bad = []
    if planar.shape != ref["rows"].shape:
        bad.append("PlanarPts: %s rows, planar_ref %s" % (planar.shape, ref["rows"].shape))
    else:
        signed = planar.copy()                      # LAPACK's sign -> the library's convention, n_z > 0
        down = signed[:, 5] < 0
        signed[down, 3:6] = -signed[down, 3:6]
        if signed[:, 0:3].tobytes() != ref["rows"][:, 0:3].tobytes():
            bad.append("PlanarPts: points differ")
        if not np.array_equal(signed[:, 3:6], ref["rows"][:, 3:6]):
            bad.append("PlanarPts: normals differ by %.3e" % np.abs(signed[:, 3:6] - ref["rows"][:, 3:6]).max())
    occ = np.argwhere(im.counter > 0)
    cy, cx = ref["cand"][:, 0], ref["cand"][:, 1]
    if not np.array_equal(diff_img[cy, cx], ref["min_diff"][cy, cx]):
        bad.append("minDiff differs at %d candidates" % (diff_img[cy, cx] != ref["min_diff"][cy, cx]).sum())
    for name, want in expect.items():
        if want is not None and bool((ref["pixels"] == np.array(im.at[name])).all(axis=1).any()) != want:
            bad.append("patch %s: expected %s" % (name, want))
    if bad:
        print("\n".join(bad))
        return 1
    py, px = occ[:, 0], occ[:, 1]
    arrays = dict(pix=occ.astype(np.int16), cnt=im.counter[py, px].astype(np.int32), xyz=im.ring[py, px, 0:3], resp=im.resp[py, px],
                  planar_reference=planar, min_diff_reference=diff_img[py, px].astype(np.float32), n_key_reference=np.int32(len(key_pts)),
                  pixels=ref["pixels"], cand=ref["cand"], eig=ref["eig"], absnz=ref["absnz"],
                  patch_names=np.array(sorted(im.at)), patch_at=np.array([im.at[k] for k in sorted(im.at)], np.int32),
                  patch_expect=np.array([{True: 1, False: 0, None: -1}[expect.get(k)] for k in sorted(im.at)], np.int8))
    save_npz(OUT, arrays)
    print("%s: %d occupied pixels, %d candidates, %d planar points, %d key points, %d bytes"
          % (OUT, len(occ), len(ref["cand"]), len(planar), len(key_pts), os.path.getsize(OUT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
