"""gr_face_polygon_index / vector textures on the device against the stand-in of tests/vector_standin.py (brute force over all rows,
Python integers, the ray along +y): every comparison is exact equality of the int32 arrays on EVERY face.

The kernel stages nothing in chunks (each lane reads its cell's list and the ring vertices straight from memory), so there is no
chunk size to straddle; the sizes that matter are the 64 lanes of a wave and the 256 threads of a workgroup."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import vector_standin as vs  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons, polygon_cell_table  # noqa: E402

pytestmark = pytest.mark.gpu


def one_cell(boxes):
    """The 1 x 1 grid over everything: one list of all rows with a ring, descending."""
    side = 3 * (1 << 42)
    return polygon_cell_table(boxes, grid=[-side, -side, 2 * side + 1, 2 * side + 1, 1, 1])


def device_index(hip, vq, faces, table, cell_table=None, **kw):
    cell_table = polygon_cell_table(table[4]) if cell_table is None else cell_table
    out, stats = hip.face_polygon_index(vq, faces, *table, cell_table, **kw)
    return out.cpu().numpy(), stats.cpu().numpy()


@pytest.fixture(scope="module")
def scene():
    """The random scene, snapped, with the stand-in's answer: computed once, shared, not modified."""
    verts, faces, polygons = vs.random_scene()
    vq, table = vs.snapped_scene(verts, polygons)
    want, info = vs.face_polygon_index_np(vq, faces, table)
    want.setflags(write=False)
    return vq, faces, table, want, info


def test_hand_worked_scene(hip):
    polygons, cases = vs.hand_scene()
    verts, faces = vs.centred_faces([c for c, _, _ in cases])
    vq, table = vs.snapped_scene(verts, polygons)
    got, stats = device_index(hip, vq, faces, table)
    want = np.array([row for _, row, _ in cases], dtype=np.int32)
    for (centre, row, what), g in zip(cases, got):
        assert g == row, (centre, what, int(g))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(vs.face_polygon_index_np(vq, faces, table)[0], want)
    assert stats[1] == np.sum(want >= 0) and stats[3] == 0


def test_random_scene_has_the_hard_cases_and_matches_on_every_face(hip, scene):
    vq, faces, table, want, info = scene
    counts = {k: int(info[k].sum()) for k in ("on_boundary", "multi", "in_hole")}
    print(f"[vector_texture] random scene: {len(faces)} faces, {len(table[4])} rows, {counts}, labelled {int((want >= 0).sum())}")
    assert len(faces) == 4000 and len(table[4]) == 300
    assert counts["on_boundary"] >= 50 and counts["multi"] >= 50 and counts["in_hole"] >= 50
    got, stats = device_index(hip, vq, faces, table)
    assert np.array_equal(got, want)
    assert stats[1] == np.sum(want >= 0) and stats[0] <= info["tested"] and stats[2] >= 1 and stats[3] == 0


def test_result_does_not_depend_on_the_grid(hip, scene):
    vq, faces, table, want, _ = scene
    chosen = polygon_cell_table(table[4])
    assert chosen[0][4] * chosen[0][5] > 1
    got_chosen, stats_chosen = device_index(hip, vq, faces, table, chosen)
    got_one, stats_one = device_index(hip, vq, faces, table, one_cell(table[4]))
    assert np.array_equal(got_chosen, got_one) and np.array_equal(got_one, want)
    assert stats_one[2] == len(np.unique(table[2]))            # the one list holds every row with a ring
    assert stats_chosen[2] < stats_one[2]
    fine = polygon_cell_table(table[4], grid=[int(3 * table[4][:, 0].min()), int(3 * table[4][:, 1].min()), 700_001, 1_300_003,
                                              180, 100])
    assert np.array_equal(device_index(hip, vq, faces, table, fine)[0], want)


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 257])
def test_face_counts_around_a_wave_and_a_workgroup(hip, scene, n_faces):
    vq, faces, table, want, _ = scene
    got, _ = device_index(hip, vq, faces[:n_faces], table)
    assert got.shape == (n_faces,) and np.array_equal(got, want[:n_faces])


def test_no_polygons_and_rings_the_snap_dropped(hip, scene):
    vq, faces, _, _, _ = scene
    empty = PlanarPolygons([], [], []).snapped()
    got, stats = device_index(hip, vq, faces[:300], empty)
    assert np.array_equal(got, np.full(300, -1, dtype=np.int32)) and stats[0] == 0 and stats[1] == 0
    # rings narrower than the grid: the snap collapses both to zero area, the rows stay and hold nothing
    sliver = PlanarPolygons([np.array([[0, 0], [40, 0], [20, 2e-7]]), np.array([[0, 0], [2e-7, 40], [0, 20]])], [0, 2], [False, False])
    table = sliver.snapped()
    assert len(table[2]) == 0 and len(table[4]) == 3
    got, stats = device_index(hip, vq, faces[:300], table)
    assert np.array_equal(got, np.full(300, -1, dtype=np.int32)) and stats[1] == 0


def test_three_vertex_ring_and_a_centre_outside_the_grid(hip):
    polygons = PlanarPolygons([np.array([[0.0, 0.0], [6.0, 0.0], [0.0, 6.0]])], [0], [False])
    centres = [(1.0, 1.0), (3.0, 3.0), (3.5, 3.0), (0.0, 6.0), (6.0, 0.0), (-0.5, 1.0), (1.0, -0.5), (6.5, 0.0), (0.0, 6.5), (50.0, 1.0),
               (1.0, 50.0), (-50.0, -50.0)]
    verts, faces = vs.centred_faces(centres)
    vq, table = vs.snapped_scene(verts, polygons)
    got, stats = device_index(hip, vq, faces, table)
    assert np.array_equal(got, np.array([0, 0, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1], dtype=np.int32))
    assert np.array_equal(got, vs.face_polygon_index_np(vq, faces, table)[0])
    assert stats[0] == 5   # only the centres inside the box started a ring walk


def test_face_referencing_the_last_vertex(hip):
    polygons = PlanarPolygons([vs.square(0, 0, 10, 10)], [0], [False])
    verts = np.array([[20.0, 20.0], [21.0, 20.0], [20.0, 21.0], [1.0, 1.0], [2.0, 1.0], [1.5, 2.5]])
    faces = np.array([[0, 1, 2], [3, 4, 5], [5, 4, 3], [5, 5, 5]], dtype=np.int32)
    vq, table = vs.snapped_scene(verts, polygons)
    got, _ = device_index(hip, vq, faces, table)
    assert np.array_equal(got, np.array([-1, 0, 0, 0], dtype=np.int32))


def test_determinants_need_128_bits(hip):
    """One triangle with corners (-2^40, -2^40), (2^40, -2^40), (0, 2^40) in grid units; centres on its edge of slope -2, one grid
    step inside and one outside.  Expected values from the stand-in; with its determinants truncated to 64 bits the device's own
    predicate decides at least one of them differently (the step off the edge is small, the determinant against the FAR edge is
    not: it settles the parity)."""
    L = 1 << 40
    table = (np.array([[-L, -L], [L, -L], [0, L]], dtype=np.int64), np.array([0, 3], dtype=np.int64), np.array([0], dtype=np.int32),
             np.array([0], dtype=np.int32), np.array([[-L, -L, L, L]], dtype=np.int64))
    k = (1 << 39) + 12345
    p = np.array([L - k, -L + 2 * k], dtype=np.int64)
    d = np.array([7, 3], dtype=np.int64)
    centres = [p, p + [-1, 0], p + [1, 0]]
    vq = np.concatenate([[c - d, c, c + d] for c in centres]).astype(np.int64)
    faces = np.arange(9, dtype=np.int32).reshape(3, 3)
    want = vs.face_polygon_index_np(vq, faces, table)[0]
    assert want.tolist() == [0, 0, -1]
    # the determinants the device forms (its ray, its edges), wrapped to 64 bits: the far edge's is about 2^84
    rings = vs._rings_of_rows(table)[0]
    c3 = vq[faces].sum(axis=1)
    exact = [vs.device_rule_contains(rings, int(x), int(y)) for x, y in c3]
    truncated = [vs.device_rule_contains(rings, int(x), int(y), orient=vs.wrapped_int64_orient) for x, y in c3]
    assert exact == [True, True, False] and truncated != exact
    got, _ = device_index(hip, vq, faces, table)
    assert np.array_equal(got, want)


def test_value_errors_of_the_binding(hip, scene):
    vq, faces, table, want, _ = scene
    grid, offsets, rows = polygon_cell_table(table[4])
    # grids the LIBRARY refuses (GR_EINVAL): no cells, a negative count, a cell of no width, more cells than GR_FPI_MAX_CELLS
    one_list = np.array([0, len(rows)], dtype=np.int64)
    for bad in ([0, 0, 1, 1, 0, 1], [0, 0, 1, 1, 1, -3], [0, 0, 0, 5, 1, 1], [0, 0, 1, 1, 1 << 13, 1 << 13]):
        with pytest.raises(ValueError, match="gr_face_polygon_index: bad cell grid"):
            hip.face_polygon_index(vq, faces[:10], *table, (np.array(bad), one_list, rows))
    with pytest.raises(ValueError, match="cell offsets"):
        hip.face_polygon_index(vq, faces[:10], *table, (grid, offsets[:-1], rows))
    # a face that names a vertex which does not exist: counted on the device, nothing read, no fault; its neighbours are answered
    broken = np.array(faces[:130])
    broken[5, 1] = len(vq)
    broken[77, 2] = -1
    broken[129, 0] = 2 ** 31 - 1
    with pytest.raises(ValueError, match="gr_face_polygon_index: 3 faces"):
        hip.face_polygon_index(vq, broken, *table, (grid, offsets, rows))
    got, stats = device_index(hip, vq, broken, table, check=False)
    ok = np.ones(130, dtype=bool)
    ok[[5, 77, 129]] = False
    assert stats[3] == 3 and np.all(got[~ok] == -1) and np.array_equal(got[ok], want[:130][ok])


class _StandInIndex:
    """A device backend whose face_polygon_index is the stand-in's."""

    face_polygon_index = vs.StandInBackend.face_polygon_index

    def __init__(self, hip):
        self._hip = hip

    def __getattr__(self, name):
        return getattr(self._hip, name)


def test_vector_texture_renders_like_the_stand_in_index(hip):
    """face_polygon_index -> get_values_for_faces_from_vector -> load_texture -> render_flat on the C1 scene, device index against
    stand-in index (render_flat itself is pinned elsewhere)."""
    (points, faces), cams = synthetic.config1_scene()
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    size = hi - lo
    rings = [[vs.square(*(lo + size * [0.1, 0.1]), *(lo + size * [0.7, 0.6])), vs.square(*(lo + size * [0.3, 0.25]), *(lo + size * [0.5, 0.45]))],
             vs.square(*(lo + size * [0.55, 0.4]), *(lo + size * [0.95, 0.9])),
             np.array([lo + size * [0.05, 0.7], lo + size * [0.45, 0.75], lo + size * [0.2, 0.98]])]
    polygons = PlanarPolygons.from_sequence(rings)
    column = {"cls": np.array([3, 7, 5], dtype=np.int64)}
    renders, indices = [], []
    for backend in (hip, _StandInIndex(hip)):
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=backend)
        labeled, all_values = mesh.get_values_for_faces_from_vector((polygons, column), "cls", points_in_polygon_CRS=points)
        assert labeled.dtype == np.int64 and np.array_equal(all_values, column["cls"])
        mesh.load_texture(labeled)
        assert mesh.IDs_to_labels == {0: 0, 1: 3, 2: 5, 3: 7}
        indices.append(labeled)
        renders.append(np.stack(list(mesh.render_flat(cams[0:2], apply_distortion=False))))
    assert np.array_equal(indices[0], indices[1]) and set(np.unique(indices[0])) == {0, 3, 5, 7}
    assert np.array_equal(renders[0], renders[1], equal_nan=True)
    assert np.isfinite(renders[0]).any()
