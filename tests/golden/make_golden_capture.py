#!/usr/bin/env python3
"""Generate tests/golden/g24_capture_corners.npz FROM THE REFERENCE ITSELF: where its look-at camera sees the four corners
of the material patch (what svbrdf_estimation_amd.capture.camera_corners restates).

Run in the build container only (needs the reference checkout, never on the GPU box):

    python tests/golden/make_golden_capture.py

The reference is imported read-only exactly as make_golden.py imports it, with its empty `cv2` / `pyredner` placeholders.
Stored: `OrthoToPerspectiveMapping(Camera(pos), sensor_size).target_points` (renderers.py:106-156, float64 [4,3], numpy only)
for eight camera positions -- one straight overhead, where the reference takes its special case for the x axis -- and three
sensor sizes.  NOT covered: `get_homography` and `apply` (renderers.py:158-173) call cv2.findHomography / cv2.warpPerspective,
and cv2 is not installed where this runs; the resampling itself is held against torch's grid_sample instead
(tests/test_capture_cpu.py).  The manifest entry goes to tests/golden/MANIFEST_g24_capture.json.

DATA ONLY: camera positions, sensor sizes and the projected corner positions.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401
from make_golden import ref_env, ref_renderers, synth  # noqa: E402

NAME = "g24_capture_corners.npz"
MANIFEST_NAME = "MANIFEST_g24_capture.json"
CAMERAS = np.array([[0.0, 0.0, 2.0], [0.3, -0.4, 1.5], [-1.2, 0.8, 2.5], [1.0, 1.0, 1.0], [0.0, -1.5, 0.9], [-0.2, 0.1, 3.0],
                    [2.0, 0.0, 0.5], [-0.7, -0.6, 1.2]], np.float64)
SENSOR_SIZES = np.array([[640, 480], [512, 512], [1600, 1200]], np.int64)


def main():
    points = np.empty((len(CAMERAS), len(SENSOR_SIZES), 4, 3), np.float64)
    for a, pos in enumerate(CAMERAS):
        for b, sensor in enumerate(SENSOR_SIZES):
            mapping = ref_renderers.OrthoToPerspectiveMapping(ref_env.Camera(pos.tolist()), tuple(int(s) for s in sensor))
            points[a, b] = mapping.target_points
    assert points.dtype == np.float64 and np.isfinite(points).all()
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, cameras=CAMERAS, sensor_sizes=SENSOR_SIZES, target_points=points)
    print("wrote %s %.1f KiB" % (NAME, os.path.getsize(path) / 1024.0))
    entry = {
        "generator": "tests/golden/make_golden_capture.py", "numpy": np.__version__,
        "sha256": synth.checksum(np.fromfile(path, np.uint8)),
        "not_covered": "OrthoToPerspectiveMapping.get_homography / apply need cv2 (findHomography, warpPerspective), which is not "
                       "installed where the fixtures are generated: only the constructor's target_points are recorded",
    }
    with open(os.path.join(HERE, MANIFEST_NAME), "w") as f:
        json.dump({"fixtures": {NAME: entry}}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
