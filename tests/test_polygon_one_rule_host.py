"""The even-odd rule of the polygon kernels is ONE rule (csrc/geom_dev.hpp, edge_crossing): "the face centre lies in some row"
(gr_face_polygon_index) and "the point lies in the region, D = 0" (gr_points_in_region) are the same question.  Here the two
stand-ins answer it on the lattice scene; tests/test_polygon_one_rule_gpu.py asks the device."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import region_standin as rs  # noqa: E402
import vector_standin as vs  # noqa: E402
from geograypher_amd.utils.geometric import polygon_cell_table  # noqa: E402


def test_the_two_stand_ins_agree_on_every_lattice_point():
    points_q, faces, table = vs.lattice_scene()
    assert points_q.shape == (3102, 2) and faces.shape == (3102, 3)
    row, _ = vs.StandInBackend().face_polygon_index(points_q, faces, *table, polygon_cell_table(table[4]))
    mask, stats = rs.StandInBackend().points_in_region(points_q, *table, 0)
    assert np.array_equal(row >= 0, mask)
    assert int(mask.sum()) == 843 == int(stats[0]) and int(stats[1]) == 0 and int(stats[2]) == 0
    assert set(np.unique(row).tolist()) == {-1, 0, 1, 2, 3}   # the hole, both parts of row 2 and the diamond are met
