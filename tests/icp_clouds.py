"""Crafted clouds for the ICP loops (csrc/icp.hip, oracle.ICP / oracle.ICP_Pt2PtAndPt2Plane), shared by the host and the
GPU tests and by tools/make_goldens.py.  Everything is rebuilt from a seed; tests/golden/icp_loop.npz stores only the
SHA-256 of each array and the results of the reference's own loops on them.

Every coordinate stays within +-16 m.  Frame 0 is a jittered lattice, so nearest neighbours are unambiguous; frame 1 holds
copies of frame-0 points (exact, or displaced by a fixed distance so that they leave the pair set when the threshold
decays past it), moved by the inverse of a known motion, so the loops have something to find.

The seeds are chosen so that in the oracle's run no distance comes within GATE_MARGIN of the threshold it is compared
with, in any iteration (tests/test_icp_loop_host.py asserts it): the device then has to select the same pairs, and the
pair counts are compared with ==."""
import hashlib

import numpy as np

GATE_MARGIN = 1e-4          # metres: about 100 float32 ulps at 16 m
MOTION_AXIS = (0.2, -0.3, 1.0)
MOTION_DEG = 1.5
MOTION_T = (0.12, -0.08, 0.05)

# keyword arguments of the reference's loops.  ICP: its defaults.  ICP_Pt2PtAndPt2Plane: RefinementCore's call (RefinePoses.py:290-293)
ICP_KW = dict(maxIterTimes=50, minIterTimes=19, inlierThreshold=0.5, smallShiftThreshold=0.05, decay_rate=0.9, ep=0.001)
P2P_KW = dict(maxIterTimes=50, minIterTimes=19, inlierThreshold0=0.5, decay_rate0=0.9, inlierThreshold1=5.0, decay_rate1=0.9,
              smallShiftThreshold=0.1, ep=0.001)

# name -> (clouds: builder name and its arguments, loop: "icp" | "p2p", overrides of the loop's keyword arguments)
CASES = {
    "points": (("point_clouds", dict(seed=12)), "icp", {}),
    "points_102": (("point_clouds", dict(seed=12)), "icp", dict(ep=0.0, maxIterTimes=102, decay_rate=1.0)),
    "late_fail": (("point_clouds", dict(seed=28, n_exact=80, n_near=120, n_far=0, n_out=60)), "icp", {}),
    "planar": (("planar_clouds", dict(seed=27)), "p2p", {}),
    "planar_late_stop": (("planar_clouds", dict(seed=8, n_exact=100, n_near=0, n_far=300, far=0.47, n_out=20, per_plane=20, moved_per_plane=20)),
                         "p2p", {}),
    "planar_103": (("planar_clouds", dict(seed=27)), "p2p", dict(ep=0.0, maxIterTimes=103, decay_rate0=1.0, decay_rate1=1.0)),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def motion():
    """The known motion of frame 1 onto frame 0 -> (R [3,3], T [3]) float64 (Rodrigues)."""
    k = np.array(MOTION_AXIS, np.float64)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(MOTION_DEG)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K), np.array(MOTION_T, np.float64)


def unmove(P):
    """Frame-0 coordinates -> frame-1 coordinates: R^T (P - T), evaluated in float64, stored as float32."""
    R, T = motion()
    return np.ascontiguousarray(((np.asarray(P, np.float64) - T) @ R).astype(np.float32))


def lattice(rng, n, side=11, pitch=1.5, jitter=0.2):
    """n points: a random subset of a side^3 lattice centred on the origin, each jittered by +-jitter; float32."""
    g = np.arange(side) - (side - 1) / 2.0
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * pitch
    pick = rng.permutation(len(nodes))[:n]
    return np.ascontiguousarray((nodes[pick] + rng.uniform(-jitter, jitter, (n, 3))).astype(np.float32))


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def point_clouds(seed, n0=1300, n_exact=300, n_near=120, n_far=120, n_out=60, near=0.21, far=0.34):
    """-> (pc0 [n0,3], pc1 [n_exact + n_near + n_far + n_out, 3]) float32.  pc1, before the inverse motion and a shuffle:
    n_exact points of pc0 copied, n_near displaced by `near` m and n_far by `far` m in random directions, and n_out
    outliers in the corners of the +-15 m box, more than 10 m from the lattice."""
    rng = np.random.RandomState(seed)
    pc0 = lattice(rng, n0)
    pick = rng.permutation(n0)[:n_exact + n_near + n_far]
    src = pc0[pick].astype(np.float64)
    src[n_exact:n_exact + n_near] += near * _directions(rng, n_near)
    src[n_exact + n_near:] += far * _directions(rng, n_far)
    out = rng.uniform(13.5, 15.0, (n_out, 3)) * rng.choice([-1.0, 1.0], (n_out, 3))
    pc1 = unmove(np.r_[src, out])
    return pc0, np.ascontiguousarray(pc1[rng.permutation(len(pc1))])


def planar_clouds(seed, per_plane=150, moved_per_plane=130, lift=0.06, tilt=0.15, **points):
    """-> (pc0, pc1, planar0 [3 per_plane, 6], planar1 [3 moved_per_plane, 6]) float32, rows xyz | unit normal.  Frame 0:
    three planes at -8 m with axis normals, points on a jittered 13 x 13 grid of 1.2 m pitch.  Frame 1: moved_per_plane of
    each plane's points lifted by `lift` m along the normal, with unit normals tilted by up to `tilt` per component, then
    the inverse motion (normals turned with it) and a shuffle.  The lift makes the planar pairs disagree with the point
    pairs about the motion."""
    pc0, pc1 = point_clouds(seed, **points)
    rng = np.random.RandomState(seed + 1000)
    R, _ = motion()
    g = (np.arange(13) - 6.0) * 1.2
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    p0, p1 = [], []
    for axis in range(3):
        uv = grid[rng.permutation(len(grid))[:per_plane]] + rng.uniform(-0.15, 0.15, (per_plane, 2))
        xyz = np.insert(uv, axis, -8.0, axis=1)
        normal = np.zeros(3); normal[axis] = 1.0
        p0.append(np.c_[xyz, np.tile(normal, (per_plane, 1))])
        keep = rng.permutation(per_plane)[:moved_per_plane]
        n1 = normal + rng.uniform(-tilt, tilt, (moved_per_plane, 3))
        n1 /= np.linalg.norm(n1, axis=1, keepdims=True)
        p1.append(np.c_[unmove(xyz[keep] + lift * normal), (n1 @ R).astype(np.float32)])
    planar0 = np.ascontiguousarray(np.concatenate(p0).astype(np.float32))
    planar1 = np.concatenate(p1).astype(np.float32)
    return pc0, pc1, planar0, np.ascontiguousarray(planar1[rng.permutation(len(planar1))])


def clouds(name):
    """The arrays of a case, freshly built (callers may move them in place)."""
    (builder, kw), _, _ = CASES[name]
    return globals()[builder](**kw)


def loop_kw(name):
    """Keyword arguments of the reference's loop for a case."""
    _, loop, over = CASES[name]
    return dict(ICP_KW if loop == "icp" else P2P_KW, **over)


def run_oracle(orc, name, **over):
    """The oracle's loop on a case -> (R_star, T_star, isSuccess, steps)."""
    steps = []
    kw = dict(loop_kw(name), **over)
    fn = orc.ICP if CASES[name][1] == "icp" else orc.ICP_Pt2PtAndPt2Plane
    R, T, ok = fn(*clouds(name), steps=steps, **kw)
    return R, T, ok, steps


def device_kw(name, **over):
    """The same parameters as Engine.icp takes them (caelo_icp_params)."""
    kw = dict(loop_kw(name), **over)
    if CASES[name][1] == "icp":
        return dict(threshold0=kw["inlierThreshold"], decay0=kw["decay_rate"], small_shift=kw["smallShiftThreshold"], ep=kw["ep"],
                    max_iter=kw["maxIterTimes"], min_iter=kw["minIterTimes"], min_pairs=100, fail_only_first=0)
    return dict(threshold0=kw["inlierThreshold0"], threshold1=kw["inlierThreshold1"], decay0=kw["decay_rate0"], decay1=kw["decay_rate1"],
                small_shift=kw["smallShiftThreshold"], ep=kw["ep"], max_iter=kw["maxIterTimes"], min_iter=kw["minIterTimes"],
                min_pairs=200, fail_only_first=1)


# ---- gates: pairs exactly on a threshold and one float32 step inside it -----------------------------------------------
def _below(x):
    """The float32 next to x towards zero."""
    return np.nextafter(np.float32(x), np.float32(0.0))


def gate_clouds():
    """The `planar` clouds with extra points far from everything else, for one iteration with threshold0 = 0.5 and
    threshold1 = 5.0 -> (pc0, pc1, planar0, planar1, extra): `extra` = (point pairs, planar pairs) that the extras add.
    Every gate is a strict <, so of each twin the pair exactly on the threshold is out and the one a float32 step
    inside it is in.  All coordinates are exact in float32 and so are the distances in float64 (0.5; a 3-4-5 offset)."""
    pc0, pc1, planar0, planar1 = planar_clouds(**CASES["planar"][0][1])
    z = [0.0, 0.0, 1.0]
    pc0 = np.r_[pc0, np.array([[12.0, 2.0, 0.0], [12.0, -2.0, 0.0]], np.float32)]
    pc1 = np.r_[pc1, np.array([[12.0, 2.5, 0.0],                 # exactly 0.5 from its neighbour: out
                               [12.0, -_below(2.5), 0.0]], np.float32)]   # one step inside: in
    planar0 = np.r_[planar0, np.array([[12.0, 12.0, 12.0] + z, [12.0, -12.0, 12.0] + z, [-12.0, 12.0, 12.0] + z, [-12.0, -12.0, 12.0] + z], np.float32)]
    planar1 = np.r_[planar1, np.array([[15.0, 16.0, 12.0] + z,             # neighbour exactly 5.0 away: out at threshold1
                                       [15.0, -_below(16.0), 12.0] + z,    # one step inside, in its neighbour's plane (pedal distance 0): in
                                       [-12.0, 12.0, 12.5] + z,            # pedal distance exactly 0.5: out at threshold0
                                       [-12.0, -12.0, _below(12.5)] + z], np.float32)]   # one step inside: in
    return tuple(np.ascontiguousarray(a, np.float32) for a in (pc0, pc1, planar0, planar1)) + ((1, 2),)


# ---- shapes: n0 around the 1024-point tile of the neighbour search, n1 around its 256-thread block --------------------
SHAPE_N0 = (1023, 1024, 1025, 2049)
SHAPE_N1 = (4, 255, 256, 257)


def shape_clouds(n0, n1, seed=11):
    """-> (pc0 [n0,3], pc1 [n1,3], src [n1]): pc1[j] is pc0[src[j]] displaced by 0.05 m and moved by the inverse motion
    scaled down to a fifth (so that every pair is inside a 0.5 m gate at once).  src holds the last point of the first
    tile (1023), the first of the second (1024) where they exist, and n0 - 1."""
    rng = np.random.RandomState(seed + n0 * 7 + n1)
    pc0 = lattice(rng, n0, side=13)
    forced = [i for i in (n0 - 1, 1023, 1024, 0) if i < n0]
    forced = list(dict.fromkeys(forced))[:n1]
    rest = [i for i in rng.permutation(n0) if i not in forced][:n1 - len(forced)]
    src = np.array(forced + rest, np.int64)[rng.permutation(n1)]
    R, T = motion()
    R5 = np.eye(3) + (R - np.eye(3)) / 5.0          # not a rotation to the last bit: only the clouds matter here
    P = pc0[src].astype(np.float64) + 0.05 * _directions(rng, n1)
    return pc0, np.ascontiguousarray(((P - T / 5.0) @ R5).astype(np.float32)), src
