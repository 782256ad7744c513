"""The 32^3 patch gather as a set-membership rule in NumPy, and the hand-made voxel sets and key points it is asked about (a helper
module, not a conftest).

The rule (csrc/config5.hip, oracle orc_patches32; GetPatchesList, Voxel.py:177-216, at PatchSize = 32 without the 496-nearest cap):
key voxel = int32((float64(pts) + Visible) / size), window [-16, 16)^3 around it, voxel at offset d placed at index d mod 32.

Nothing here is stored in files or drawn at run time from anything but fixed seeds."""
import functools

import numpy as np

VISIBLE = np.array([99.84, 99.84, 14.72])
SIZES = (0.02, 0.02 * 8, 0.02 * 32)                      # Voxel.py:31 (the products as the C code forms them)
GRID = ((9984, 9984, 1472), (1248, 1248, 184), (312, 312, 46))


def key_voxels(pts, scale):
    """[k, >= 3] f32 -> int32 [k, 3]: float64 sum, float64 division, truncation toward zero."""
    p = np.asarray(pts, np.float32)[:, 0:3].astype(np.float64)
    return np.int32((p + VISIBLE) / SIZES[scale])


def patches32(pts, vox, scale):
    """pts [k, >= 3] f32, vox [n, 3] integer voxel list of ``scale`` -> bit-packed patches [k, 512] u64: voxel (ix, iy, iz) of the
    patch at bit lin & 63 of word lin >> 6, lin = (ix * 32 + iy) * 32 + iz."""
    keys = key_voxels(pts, scale).astype(np.int64)
    vox = np.asarray(vox).astype(np.int64).reshape(-1, 3)
    dense = np.zeros((len(keys), 32 * 32 * 32), bool)
    for p, key in enumerate(keys):
        d = vox - key
        d = d[((d >= -16) & (d < 16)).all(axis=1)]
        i = d % 32                                             # Python's mod: -16 -> 16, -1 -> 31
        dense[p, (i[:, 0] * 32 + i[:, 1]) * 32 + i[:, 2]] = True
    return np.packbits(dense, axis=1, bitorder="little").view(np.uint64)


def centre(voxels, scale):
    """float32 points at the centres of ``voxels`` [k, 3] of ``scale``: half a voxel from every face, so that no rounding of the
    point or of the index arithmetic can move it to a neighbour."""
    return ((np.asarray(voxels, np.float64) + 0.5) * SIZES[scale] - VISIBLE).astype(np.float32)


# ---- the hand-made case -----------------------------------------------------------------------------------------------------------
# Every structure is laid out in voxel INDICES, the same recipe at each scale (the grid is 9984 x 9984 x 1472, 1248 x 1248 x 184 and
# 312 x 312 x 46 voxels), so the x bands below hold at the narrowest grid:
#   [0, 40)         sparse voxels in the grid's low corner (windows that reach below index 0)
#   [40, 88)        a solid block, 48 voxels wide (46 tall at scale 2: the whole height of the grid)
#   [95, 130), [177, 211), [219, 253)   single isolated voxels, one per site (x column = axis, y row = offset)
#   centre +- 20    sparse voxels around the sensor origin, where the key voxel quotient can be an exact integer
#   [top - 40, top) sparse voxels in the grid's high corner (windows that reach above the grid)
OFFSETS = (-17, -16, -1, 0, 15, 16)       # of a single voxel from the key voxel; -17 and +16 lie outside the window
SITE_X = (112, 194, 236)
FAR_POINT = (-40.0, 70.0, 0.0)


def _block_z(scale):
    return (0, 46) if scale == 2 else (40, 88)


def _site(axis, j, scale):
    return np.array([SITE_X[axis], 20 + 36 * j, 20 if scale == 2 else 100])


def _face_coordinate(vis, m0):
    """The smallest float32 p (a multiple of the float64 spacing at ``vis``, so that p + vis is exact) whose scale-0 quotient
    (float64(p) + vis) / 0.02 reaches m0 = vis / 0.02, and the one a spacing below it.  Around p = 0 the quotients of neighbouring
    sums lie closer together than the float64 numbers around m0, so the first of them IS m0: a point exactly on a voxel face."""
    step = np.spacing(vis)
    j = 0
    while (j * step + vis) / SIZES[0] >= m0:
        j -= 1
    while (j * step + vis) / SIZES[0] < m0:
        j += 1
    hit, low = np.float32(j * step), np.float32((j - 1) * step)
    assert float(hit) == j * step and float(low) == (j - 1) * step and abs(j) < 64
    return hit, low


@functools.lru_cache(maxsize=None)
def gather_case():
    """-> (lists, pts, tags): three int16 voxel lists [n_s, 3] in shuffled order, key points [k, 3] f32 and, per key point, a tag
    (kind, scale it was made for, detail).  Read-only."""
    rs = np.random.RandomState(17)
    lists = []
    for s in range(3):
        g = np.array(GRID[s])
        z0, z1 = _block_z(s)
        bx, by, bz = np.meshgrid(np.arange(40, 88), np.arange(40, 88), np.arange(z0, z1), indexing="ij")
        parts = [np.stack([bx.ravel(), by.ravel(), bz.ravel()], 1)]
        for lo in (np.zeros(3, int), g // 2 - 20, g - 40):                       # low corner, centre, high corner
            cell = np.argwhere(rs.uniform(size=(40, 40, 40)) < 0.05) + lo
            parts.append(cell[(cell < g).all(axis=1) & (cell >= 0).all(axis=1)])
        for axis in range(3):
            for j, off in enumerate(OFFSETS):
                v = _site(axis, j, s)
                v[axis] += off
                parts.append(v[None])
        vox = np.unique(np.concatenate(parts), axis=0)
        assert vox.min() >= 0 and (vox < g).all()
        lists.append(np.ascontiguousarray(vox[rs.permutation(len(vox))].astype(np.int16)))
    pts, tags = [], []

    def add(p, kind, scale, detail=None):
        pts.append(np.asarray(p, np.float32).reshape(3))
        tags.append((kind, scale, detail))

    for s in range(3):
        g = np.array(GRID[s])
        z0 = _block_z(s)[0] + 16
        for i in range(8):                                                        # inside the solid block, every brick phase on every axis
            add(centre([56 + i, 56 + (3 * i) % 8, z0 + (5 * i) % 8], s), "solid", s)
        for k in ([3, 20, 20], [20, 5, 20], [20, 20, 2], [1, 2, 3]):              # below index 0: x, y, z, all three
            add(centre(k, s), "below", s, tuple(k))
        for k in ([-5, -20, -20], [-20, -3, -20], [-20, -20, -2], [-1, -1, -1]):  # above the top: x, y, z, all three
            add(centre(g + np.array(k), s), "above", s)
        for axis in range(3):
            for j, off in enumerate(OFFSETS):
                add(centre(_site(axis, j, s), s), "single", s, (axis, off))
    hit, low = zip(*[_face_coordinate(VISIBLE[a], (4992, 4992, 736)[a]) for a in range(3)])
    add(hit, "face", None, "hit")
    for a in range(3):
        add([low[b] if b == a else hit[b] for b in range(3)], "face", None, "low%d" % a)
    add(low, "face", None, "low")
    add(np.nextafter(np.array(hit, np.float32), np.float32(-np.inf)), "face", None, "next")     # one float32 step below the face
    add(FAR_POINT, "far", None)
    pts = np.ascontiguousarray(np.stack(pts))
    pts.setflags(write=False)
    for a in lists:
        a.setflags(write=False)
    return tuple(lists), pts, tuple(tags)


@functools.lru_cache(maxsize=None)
def gather_reference():
    """patches32 of the case at the three scales: u64 [k, 3, 512], read-only."""
    lists, pts, _ = gather_case()
    ref = np.ascontiguousarray(np.stack([patches32(pts, lists[s], s) for s in range(3)], axis=1))
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def both_ways_case():
    """A voxel set for the two builders: scale-0 voxels around the sensor origin -> (points at their centres [n, 4] f32, the three
    lists a voxelisation of those points gives (the coarser scales are the scale-0 indices >> 3 and >> 5), key points [8, 3])."""
    rs = np.random.RandomState(19)
    v0 = np.unique(rs.randint(-24, 24, size=(3000, 3)) + np.array([4992, 4992, 736]), axis=0)
    v0 = v0[rs.permutation(len(v0))]
    pc = np.zeros((len(v0), 4), np.float32)
    pc[:, 0:3] = centre(v0, 0)
    lists = tuple(np.ascontiguousarray(np.unique(v0 >> sh, axis=0).astype(np.int16)) for sh in (0, 3, 5))
    keys = centre(v0[:8], 0)
    return pc, lists, keys
