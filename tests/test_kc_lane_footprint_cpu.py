"""tools/kc_lane_footprint.py: the CPU simulation behind profiles/kc_lanes_footprint.txt (distinct cache lines that one gather instruction of
k_integrate touches, by the sub-box of the block a wave's lanes cover).  A small sample of its views: the counts are consistent with one another,
one voxel plane seen head-on is what geometry says, and the ordering the record states holds -- compact sub-boxes touch fewer lines than the
8 x 8 x 1 z-slice."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kc_lane_footprint as FP  # noqa: E402


def test_counts_are_consistent_and_compact_boxes_touch_fewer_lines():
    R, centre = FP.views(600, 7)
    mean = {}
    for cover in FP.COVERS:
        lines, sectors, pixels = FP.footprint(cover, R, centre)
        assert len(lines) > 500                                                 # few views lose every lane off the image
        assert np.all(lines >= 1) and np.all(lines <= sectors) and np.all(sectors <= pixels) and np.all(pixels <= 64)
        assert np.all(sectors <= 2 * lines)                                     # a 128-byte line holds two 64-byte sectors
        mean[cover] = lines.mean()
    flat = mean[(8, 8, 1)]
    assert 12 < flat < 20                                                       # the record: 15.9
    for cover in ((8, 4, 2), (8, 2, 4), (4, 4, 4)):
        assert mean[cover] < 0.8 * flat, (cover, mean)                          # the record: 11.1, 9.8, 9.8


def test_a_z_slice_seen_head_on_at_one_metre_touches_one_or_two_lines_per_voxel_row():
    """Identity rotation, block centre on the optical axis at 1 m: the 8 x 8 lattice of 5 mm voxels spans 8 * 0.005 * 515 = 20.6 pixels a side, its
    eight rows of voxels fall on eight different image rows 2-3 pixels apart, each row's 18-pixel extent (144 bytes) in one or two 128-byte lines."""
    R = np.eye(3)[None]
    centre = np.array([[0.0, 0.0, 1.0]])
    lines, sectors, pixels = FP.footprint((8, 8, 1), R, centre)
    assert pixels[0] == 64 and 8 <= lines[0] <= 16
