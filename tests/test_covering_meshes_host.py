"""Host layer of the covering meshes (utils.geometric.covering_meshes, TexturedPhotogrammetryMesh.export_covering_meshes, the
multiview_detections entry point) with the numpy stand-in of tests/covering_standin.py in place of the two device calls, and
the stand-in itself against a case worked by hand.  No GPU."""
import logging
import re
from pathlib import Path

import numpy as np
import pytest
from scipy.spatial import ConvexHull

from geograypher_amd import _hip, build
from geograypher_amd.entrypoints import multiview_detections as entry
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh
from geograypher_amd.utils import geometric, synthetic
from tests.covering_standin import CoverStandIn, bound_tables, cover_grid_np, points_bounds_np
from tests.ray_standin import StandInBackend

ROOT = Path(__file__).resolve().parents[1]
BACKEND = CoverStandIn()


def _lattice(n):
    x, y = (v.ravel().astype(np.float64) for v in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    return x, y


def test_hand_worked_grid():
    """x, y in {0..8}^2, z = 10 x + y, N = 5: grid points 0 2 4 6 8, half-width 1, so cell bounds [-1, 1] [1, 3] [3, 5] [5, 7]
    [7, 9] -- all exact.  A point at an odd coordinate sits on a shared bound and belongs to both neighbours: the columns hold
    x in {0 1} {1 2 3} {3 4 5} {5 6 7} {7 8}."""
    x, y = _lattice(9)
    pts = np.column_stack([x, y, 10 * x + y])
    bounds, bad = points_bounds_np(pts)
    assert bounds.tolist() == [0, 8, 0, 8, 0, 88] and bad == 0
    x_lo, x_hi, y_lo, y_hi = bound_tables(bounds, 5)
    assert x_lo.tolist() == y_lo.tolist() == [-1, 1, 3, 5, 7] and x_hi.tolist() == y_hi.tolist() == [1, 3, 5, 7, 9]
    z_max, z_min, count = cover_grid_np(pts, x_lo, x_hi, y_lo, y_hi)
    per_axis = np.array([2, 3, 3, 3, 2])
    assert np.array_equal(count, np.outer(per_axis, per_axis)) and count.sum() == 169
    # (xi, yi): count, max, min, written out: the largest member is (largest x, largest y) of the cell
    for (xi, yi), (n, hi, lo) in {(0, 0): (4, 11, 0), (1, 1): (9, 33, 11), (2, 3): (9, 57, 35), (4, 0): (4, 81, 70),
                                  (0, 2): (6, 15, 3), (4, 4): (4, 88, 77)}.items():
        assert (count[xi, yi], z_max[xi, yi], z_min[xi, yi]) == (n, hi, lo)
    # the point (1, 1) alone: four cells
    z_max, _, count = cover_grid_np(np.array([[1.0, 1.0, 5.0]]), x_lo, x_hi, y_lo, y_hi)
    assert count.sum() == 4 and np.all(count[:2, :2] == 1) and np.all(z_max[:2, :2] == 5.0) and np.isnan(z_max[2, 2])
    # through covering_meshes: vertices in the order xi * N + yi, buffers added
    (up, up_f), (low, low_f) = geometric.covering_meshes(pts, 5, z_buffer=(0.5, -0.25), backend=BACKEND)
    assert up.shape == low.shape == (25, 3) and np.array_equal(up[:, :2], low[:, :2])
    assert up[1].tolist() == [0, 2, 13 + 0.5] and low[1].tolist() == [0, 2, 1 - 0.25]        # cell (0, 1): x {0 1}, y {1 2 3}
    assert up[5 * 2 + 3].tolist() == [4, 6, 57.5] and low[5 * 2 + 3].tolist() == [4, 6, 34.75]
    assert up_f.dtype == np.int32 and np.array_equal(up_f, low_f)
    # every second point ([::2] of 81 rows in x-major order: even flat indices)
    z_max2, _, count2 = cover_grid_np(pts, x_lo, x_hi, y_lo, y_hi, stride=2)
    assert np.array_equal(count2, cover_grid_np(pts[::2], x_lo, x_hi, y_lo, y_hi)[2]) and count2.sum() < 169


def test_zero_extent_axis_puts_a_point_in_every_column():
    pts = np.array([[3.0, 0.0, 1.0], [3.0, 4.0, 2.0], [3.0, 2.0, 7.0]])
    bounds, _ = points_bounds_np(pts)
    tabs = bound_tables(bounds, 3)
    assert np.all(tabs[0] == 3.0) and np.all(tabs[1] == 3.0)
    z_max, z_min, count = cover_grid_np(pts, *tabs)
    assert np.array_equal(count, np.ones((3, 3), dtype=np.int64))     # y bounds [-1, 1] [1, 3] [3, 5]: one point per row
    assert np.array_equal(z_max, np.tile([1.0, 7.0, 2.0], (3, 1))) and np.array_equal(z_min, np.tile([1.0, 7.0, 2.0], (3, 1)))


@pytest.fixture(scope="module")
def unit_grid():
    x, y = _lattice(10)
    return np.column_stack([x, y, np.random.default_rng(0).uniform(-5.0, 5.0, 100)])


def test_reference_properties_on_a_unit_grid(unit_grid):
    pts = unit_grid
    (up, up_f), (low, low_f) = geometric.covering_meshes(pts, 3, backend=BACKEND)
    assert up.shape == low.shape == (9, 3)
    assert np.all(up[:, 2] >= low[:, 2])
    for surf in (up, low):
        assert (surf[:, 0].min(), surf[:, 0].max(), surf[:, 1].min(), surf[:, 1].max()) == (0.0, 9.0, 0.0, 9.0)
    assert up[:, 2].max() == pts[:, 2].max() and low[:, 2].min() == pts[:, 2].min()
    (up_b, _), (low_b, _) = geometric.covering_meshes(pts, 3, z_buffer=(2.0, -1.5), backend=BACKEND)
    assert np.array_equal(up_b[:, 2], up[:, 2] + 2.0) and np.array_equal(low_b[:, 2], low[:, 2] + (-1.5))
    assert np.array_equal(up_b[:, :2], up[:, :2])
    full = len(geometric.covering_meshes(pts, 10, backend=BACKEND)[0][0])
    assert full == 100
    for subsample in (3, 5, 9):
        (s_up, _), (s_low, _) = geometric.covering_meshes(pts, 10, subsample=subsample, backend=BACKEND)
        assert 0 < len(s_up) == len(s_low) < full
    # the mesh method is the same call over the mesh's points
    mesh = TexturedPhotogrammetryMesh((pts, np.zeros((0, 3), dtype=np.int64)), backend=BACKEND, log_level="ERROR")
    (m_up, m_f), (m_low, _) = mesh.export_covering_meshes(N=3, z_buffer=(2.0, -1.5))
    assert np.array_equal(m_up, up_b) and np.array_equal(m_low, low_b) and np.array_equal(m_f, up_f)
    assert "2399-2482" in TexturedPhotogrammetryMesh.export_covering_meshes.__doc__


def test_empty_points_and_argument_errors(unit_grid, caplog):
    class Never:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was used for an empty point set")

    (up, up_f), (low, low_f) = geometric.covering_meshes(np.zeros((0, 3)), 4, backend=Never())
    assert up.shape == low.shape == (0, 3) and up_f.shape == low_f.shape == (0, 3)
    empty_mesh = TexturedPhotogrammetryMesh((np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)), backend=Never(), log_level="ERROR")
    assert empty_mesh.export_covering_meshes(N=4)[0][0].shape == (0, 3)
    with pytest.raises(ValueError, match="2 buffers"):
        geometric.covering_meshes(unit_grid, 3, z_buffer=(0, 0, 0), backend=BACKEND)
    with pytest.raises(ValueError, match="2 buffers"):
        geometric.covering_meshes(np.zeros((0, 3)), 3, z_buffer=(0,), backend=BACKEND)
    for bad_n in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2"):
            geometric.covering_meshes(unit_grid, bad_n, backend=BACKEND)
    with pytest.raises(ValueError, match="subsample"):
        geometric.covering_meshes(unit_grid, 3, subsample=0, backend=BACKEND)
    for value in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            bad = unit_grid.copy()
            bad[4, axis] = value
            with pytest.raises(ValueError, match="1 of the visited points"):
                geometric.covering_meshes(bad, 3, backend=BACKEND)
    bad = unit_grid.copy()
    bad[5, 2] = np.nan                     # row 5 is not visited by [::2]
    assert len(geometric.covering_meshes(bad, 3, subsample=2, backend=BACKEND)[0][0]) == 9
    with caplog.at_level(logging.WARNING, logger="geograypher_amd.utils.geometric"):
        geometric.covering_meshes(unit_grid, 181, backend=BACKEND)
        assert not caplog.records
        geometric.covering_meshes(unit_grid, 182, backend=BACKEND)
    assert len(caplog.records) == 1 and "65536" in caplog.records[0].getMessage()


def _tri_areas(xy, faces):
    a, b, c = xy[faces[:, 0]], xy[faces[:, 1]], xy[faces[:, 2]]
    return 0.5 * np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))


@pytest.mark.parametrize("N,subsample", [(3, None), (10, None), (10, 3), (7, 5)])
def test_faces_triangulate_the_hull_of_the_survivors(unit_grid, N, subsample):
    (up, faces), (low, low_faces) = geometric.covering_meshes(unit_grid, N, subsample=subsample, backend=BACKEND)
    assert faces.ndim == 2 and faces.shape[1] == 3 and len(faces) > 0 and np.array_equal(faces, low_faces)
    assert faces.min() >= 0 and faces.max() < len(up)
    areas = _tri_areas(up[:, :2], faces)
    assert areas.min() > 0
    # a sum of at most 2 (N - 1)^2 areas of order 1..20 each: a few ulps of the total
    assert abs(areas.sum() - ConvexHull(up[:, :2]).volume) <= 1e-12 * areas.sum()
    assert len(np.unique(faces)) == len(up)    # every surviving grid point is a vertex of the surface


def test_collinear_or_too_few_survivors_have_no_faces():
    t = np.arange(4.0)
    diag = np.column_stack([t, t, t])                    # points AT the grid points of N = 4: cells (i, i) only
    (up, faces), (low, low_faces) = geometric.covering_meshes(diag, 4, backend=BACKEND)
    assert up.shape == (4, 3) and np.array_equal(up[:, 0], up[:, 1])
    assert faces.shape == low_faces.shape == (0, 3) and faces.dtype == np.int32
    one = geometric.covering_meshes(np.array([[1.0, 2.0, 3.0]]), 2, backend=BACKEND)   # every cell, all at one (x, y)
    assert one[0][0].shape == (4, 3) and one[0][1].shape == (0, 3)
    line = np.column_stack([np.full(5, 2.0), np.arange(5.0), np.arange(5.0)])            # x constant: a vertical line
    (up, faces), _ = geometric.covering_meshes(line, 3, backend=BACKEND)
    assert up.shape == (9, 3) and faces.shape == (0, 3)
    two = np.array([[0.0, 0.0, 1.0], [4.0, 4.0, 2.0]])
    (up, faces), _ = geometric.covering_meshes(two, 5, backend=BACKEND)
    assert up.shape == (2, 3) and faces.shape == (0, 3)


def test_header_binding_and_build_list_name_the_new_calls():
    header = (ROOT / "include" / "geograster.h").read_text()
    for name, n_args in (("gr_points_bounds", 7), ("gr_cover_grid", 13)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == n_args == len(_hip._SIGNATURES[name])
    assert "#define GR_VERSION 126" in header and "meshes/meshes.py:2399-2482" in header
    assert any(p.name == "cover.hip" for p in build.SOURCES)
    assert "cover.hip" in (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    assert callable(_hip.HipRaster.points_bounds) and callable(_hip.HipRaster.cover_grid)


class _Both(StandInBackend, CoverStandIn):
    pass


def test_entry_point_runs_end_to_end(tmp_path):
    """The synthetic survey of tests/test_triangulation_host.py over a two-sheet mesh (ground about z = -2, canopy about z = 25)
    that covers it: the entry point writes the two boundaries and the points."""
    s = synthetic.detection_survey(n_objects=12, n_cameras=20, seed=2)
    cams, det = synthetic.detection_survey_cameras(s)
    ground, g_faces = synthetic.heightfield_mesh(161, 400.0, lambda x, y: -2.0 + 0.5 * np.sin(x / 40.0) * np.cos(y / 50.0))
    canopy, c_faces = synthetic.heightfield_mesh(161, 400.0, lambda x, y: 25.0 + np.cos(x / 30.0))
    points = np.concatenate([ground, canopy]) + np.array([100.0, 100.0, 0.0])
    np.savez(tmp_path / "mesh.npz", points=points, faces=np.concatenate([g_faces, c_faces + len(ground)]))
    out = tmp_path / "out"
    got = entry.multiview_detections(None, None, None, tmp_path / "mesh.npz", out, similarity_threshold_meters=0.5,
                                     louvain_resolution=2.0, seed=1, camera_set=cams, detector=det, backend=_Both())
    for name in ("boundary_ceiling.npz", "boundary_floor.npz", "tree_locations.npy", "line_segments.npz", "communities.npz"):
        assert (out / name).is_file(), name
    assert got.ndim == 2 and got.shape[1] == 3 and len(got) >= 1 and np.array_equal(np.load(out / "tree_locations.npy"), got)
    want = geometric.covering_meshes(points, 50, z_buffer=(0, 1.0), subsample=2, backend=BACKEND)   # local scale 1: identity transform
    # ... and the points are those of the reference's call with these boundaries
    assert np.array_equal(got, cams.triangulate_detections(det, boundaries=want, limit_ray_length_meters=160,
                                                           limit_angle_from_vert=np.deg2rad(50), seed=1, backend=_Both(),
                                                           similarity_threshold_meters=0.5, louvain_resolution=2.0))
    for name, (w_pts, w_faces) in zip(("boundary_ceiling.npz", "boundary_floor.npz"), want):
        with np.load(out / name) as d:
            assert np.array_equal(d["points"], w_pts) and np.array_equal(d["faces"], w_faces) and len(w_faces) > 0
    with np.load(out / "line_segments.npz") as d:
        # rays start on the ceiling (canopy sheet, 24..26) and end on the floor (ground sheet + 1: -1.5..-0.5)
        assert len(d["ray_starts"]) > 50
        assert np.all((d["ray_starts"][:, 2] > 23.9) & (d["ray_starts"][:, 2] < 26.1))
        assert np.all((d["ray_ends"][:, 2] > -1.6) & (d["ray_ends"][:, 2] < -0.4))
    args = entry.parse_args(["--images-dir", str(tmp_path), "--detections-dir", str(tmp_path), "--camera-file",
                             str(tmp_path / "mesh.npz"), "--mesh-file", str(tmp_path / "mesh.npz"), "--output-dir", str(out)])
    assert args.similarity_threshold_meters == 4.0 and args.nonlinearity is None and args.louvain_resolution == 2.0
