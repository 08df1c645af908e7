#!/usr/bin/env python3
"""Run ONCE on any machine that has OpenCV: writes tests/golden/frame_stats_opencv_<version>.npz -- seeded frames and what the
reference's frame-statistics ops compute on them with REAL OpenCV: the Y plane of cv2.cvtColor(COLOR_RGB2YUV), the sums of
cv2.Laplacian(frame, CV_64F), SharpnessCPP's meanStdDev + pow + /3 (old/cpp_ops/imgproc.cpp:157-165), BrightnessCPP's
cv2.mean (:70-72) and the Python ops Brightness / Contrast / Sharpness (old/imgproc.py:11-36).  Commit the file:
tests/test_frame_stats.py::test_definitions_against_opencv_golden then pins tests/ref_frame_stats_np.py against it on every
machine.  Until such a file exists the SharpnessCPP row of the contract is not pinned against OpenCV.

    python tests/golden/make_frame_stats_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ (util.py)

SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (37, 53), (120, 160)]


def main():
    import cv2
    from util import random_frames, texture_stream
    out = {"cv2_version": np.array(cv2.__version__)}
    for i, (h, w) in enumerate(SHAPES):
        f = random_frames(40 + i, 1, h, w)[0] if min(h, w) < 16 else texture_stream(40 + i, 1, h, w, margin=2)[0][0]
        yuv = cv2.cvtColor(f, cv2.COLOR_RGB2YUV)
        lap = cv2.Laplacian(f, cv2.CV_64F)
        _, sd = cv2.meanStdDev(lap)
        sd = np.power(sd.ravel(), 2)
        inten = yuv.reshape(-1)[::3]
        avg = np.mean(inten)
        out["frame_%d" % i] = f
        out["y_%d" % i] = yuv[..., 0]
        out["lap_sum_%d" % i] = lap.reshape(-1, 3).sum(0)
        out["lap_sq_%d" % i] = (lap.reshape(-1, 3) ** 2).sum(0)
        out["brightness_cpp_%d" % i] = np.float32(cv2.mean(yuv)[0])
        out["sharpness_cpp_%d" % i] = np.float32((sd[0] + sd[1] + sd[2]) / np.float32(3.0))
        out["brightness_%d" % i] = np.float64(np.mean(yuv, axis=(0, 1))[0])
        out["contrast_%d" % i] = np.float64(np.sqrt(np.mean((inten - avg) ** 2)))
        out["sharpness_%d" % i] = np.float64(lap.var())
    path = os.path.join(HERE, "frame_stats_opencv_%s.npz" % cv2.__version__)
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
