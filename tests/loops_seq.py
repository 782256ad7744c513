"""The 16-frame synthetic revisit sequence of the loop-closure tests (tests/test_detect_loops_gpu.py, tests/test_loops_host.py's
evaluation test): frames 0..7 drive 6 m apart along x at yaw 0; frames 8..15 come back one world period (54 m) later, 0.5 m ahead and
1 m to the side, at headings 0.3, 1.0, ..., 5.2 rad.  The world repeats every 54 m, so frame 8 + k revisits frame k; the ground truth
puts the revisiting frames at x - 54."""
import functools
import math

import numpy as np

N_FRAMES, N_LOOPS, PERIOD = 16, 8, 54.0
TR = np.array([[0.0, -1.0, 0.0, 0.02], [0.0, 0.0, -1.0, -0.07], [1.0, 0.0, 0.0, -0.3]])   # LiDAR -> camera, KITTI-like


def sensor_poses():
    """-> [(translation, yaw)] what synth.make_scan(pose=...) takes"""
    return [((6.0 * k, 0.0, 0.0), 0.0) for k in range(8)] + [((PERIOD + 6.0 * k + 0.5, 1.0, 0.0), 0.7 * k + 0.3) for k in range(8)]


def yaw_of(frame):
    return sensor_poses()[frame][1]


def lidar_world_poses():
    """-> [16, 4, 4] the LiDAR's pose in the world of frame 0, the revisiting frames at x - 54"""
    out = np.tile(np.eye(4), (N_FRAMES, 1, 1))
    for f, ((x, y, z), yaw) in enumerate(sensor_poses()):
        c, s = math.cos(yaw), math.sin(yaw)
        out[f, 0:3, 0:3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        out[f, 0:3, 3] = (x - (PERIOD if f >= 8 else 0.0), y, z)
    return out


def write_ground_truth(folder):
    """-> (poses path, calib path): KITTI camera-frame poses [16, 12] = Tr L Tr^-1 and a label-free calib_.txt whose row 4 is Tr"""
    tr = np.vstack([TR, [0, 0, 0, 1]])
    poses = np.array([(tr @ L @ np.linalg.inv(tr))[0:3].reshape(12) for L in lidar_world_poses()])
    calib = np.tile(np.eye(3, 4).reshape(12), (5, 1))
    calib[4] = TR.reshape(12)
    np.savetxt(str(folder / "gt.txt"), poses, fmt="%.17g")
    np.savetxt(str(folder / "calib_.txt"), calib, fmt="%.17g")
    return str(folder / "gt.txt"), str(folder / "calib_.txt")


def true_motion(i, j):
    """-> (R, T) with p_j = R p_i + T"""
    L = lidar_world_poses()
    m = np.linalg.inv(L[j]) @ L[i]
    return m[0:3, 0:3], m[0:3, 3]


@functools.lru_cache(maxsize=None)
def scans(scene_kind="boxes"):
    from caelo import synth
    return [synth.make_scan(frame=f, pose=p, quantum=1e-3, scene_kind=scene_kind, trajectory="circuit") for f, p in enumerate(sensor_poses())]
