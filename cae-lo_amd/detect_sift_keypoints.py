#!/usr/bin/env python
"""detect_sift_keypoints.py -- SIFT3D key points for every scan of a directory, the row 'sift' of the reference's key point comparison
(PclKeyPts.py:55-58, :63, :114-122; PCLKeypoint.keypointSift, a PCL binding the reference does not ship), on the GPU
(caelo_sift_octave).

    python detect_sift_keypoints.py --scans <seq>/velodyne --out sift_keypts/00
    python run_sequence.py --scans <seq>/velodyne --python-loader --keypts-source 3dfeatnet --keypts-dir sift_keypts/00 --out poses_/00.txt
    python evaluate.py keypoints --keypts-dir sift_keypts/00 --source 3dfeatnet --gt poses/00.txt --calib calib_.txt --out acc.mat

detect_keypoints.py's main() with sift among its methods: the same thinning, subsampling, ensure_keypoint_number, file layouts and
options, --method {iss,harris,sift} with sift as the default, and --min-scale, --n-octaves, --n-scales-per-octave, --min-contrast;
each detector's options are refused under the others.  The key points written are the detector's xyz rows -- centroids of its voxel
pyramid in the order octave, point, scale, a point once per scale it is a key at -- not rows of the thinned cloud.  It is a script of
its own because detect_keypoints.py's command line, where sift is an invalid choice, is kept as it was.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detect_keypoints  # noqa: E402


def main(argv=None):
    detect_keypoints.main(argv, with_sift=True)


if __name__ == "__main__":
    main()
