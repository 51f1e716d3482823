"""gr_simplify_rings on the device against the exact stand-in of tests/simplify_standin.py: `keep`,
`kept_index`, `out_offsets` and every word of the statistics are EQUAL in every case -- the hand scenes, chains that end inside a
wave, span a workgroup or cross five of them, many small rings in one call, ties and exact-tolerance hits by the hundred, one
vertex a pass, the widest products, fixed vertices, fenced outputs, a poisoned stage arena, and the two workflows end to end."""
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import outline_standin as osn  # noqa: E402
import simplify_standin as ss  # noqa: E402

from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402
from tests.fenced_backend import POISON, FencedHipRaster, fenced  # noqa: E402

pytestmark = pytest.mark.gpu

METHOD = "douglas-peucker"


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same(backend, rings, T, fixed=None):
    """The device's answer for the table of `rings` at T grid steps, held against the stand-in's: -> (device arrays, tally)."""
    rv, off = rings if isinstance(rings, tuple) else ss.table(rings)
    want_keep, want_index, want_off, want_stats, tally = ss.simplify_np(rv, off, T, fixed)
    keep, kept_index, out_offsets, stats = backend.ring_simplifier().simplify(rv, off, T * 1e-6, fixed)
    assert keep.dtype == torch.uint8 and kept_index.dtype == torch.int32 and out_offsets.dtype == torch.int64 and keep.is_cuda
    got = [_np(x) for x in (keep, kept_index, out_offsets, stats)]
    assert np.array_equal(got[2], want_off), (got[2][-5:], want_off[-5:])
    assert np.array_equal(got[1], want_index)
    assert np.array_equal(got[0], want_keep)
    assert got[3].tolist() == want_stats.tolist(), (got[3].tolist(), want_stats.tolist())
    return got, tally


def polygon_ring(n, seed):
    """A star-shaped ring of n distinct vertices with rough edges."""
    rng = np.random.default_rng(seed)
    angle = np.sort(rng.uniform(0, 2 * np.pi, n)) + np.arange(n) * 1e-9
    radius = 40_000 + rng.integers(-6_000, 6_000, n)
    return np.column_stack([np.rint(radius * np.cos(angle)), np.rint(radius * np.sin(angle))]).astype(np.int64)


# ---- the hand scenes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ss.hand_scenes()))
def test_hand_scenes(hip, name):
    ring, fixed, T, want = ss.hand_scenes()[name]
    got, _ = same(hip, [ring], T, fixed)
    assert got[1].tolist() == want


def test_all_hand_scenes_in_one_call(hip):
    scenes = [s for s in ss.hand_scenes().values() if s[2] == 5]
    assert len(scenes) >= 2
    same(hip, [s[0] for s in scenes], 5)


# ---- sizes: a wave, a workgroup, a chain across five workgroups -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 255, 256, 257, 1025])
def test_one_ring_of_n_vertices(hip, n):
    ring = polygon_ring(n, seed=n)
    for T in (0, 900, 5_000):
        got, _ = same(hip, [ring], T)
    same(hip, [ring[::-1]], 900)
    same(hip, [np.roll(ring, n // 2, axis=0)], 900)


@pytest.mark.parametrize("count", [64, 257])
def test_many_small_rings_in_one_call(hip, count):
    rng = np.random.default_rng(count)
    rings = [rng.integers(-30, 30, (int(n), 2)) for n in rng.integers(3, 8, count)]
    rings[5] = rings[5][:2]                      # a short ring among them, and one without vertices
    rings[9] = rings[9][:0]
    for T in (0, 7, 25):
        got, tally = same(hip, rings, T)
    assert got[3][ss.SHORT] == 2 and got[3][ss.COLLAPSED] > 0


def test_empty_tables(hip):
    empty = np.zeros((0, 2), dtype=np.int64)
    got, _ = same(hip, (empty, np.zeros(1, dtype=np.int64)), 5)            # N = 0, R = 0
    assert got[2].tolist() == [0] and got[3].tolist() == [0] * 8
    got, _ = same(hip, (empty, np.zeros(4, dtype=np.int64)), 5)            # N = 0, three rings without vertices
    assert got[2].tolist() == [0, 0, 0, 0] and got[3][ss.SHORT] == 3


# ---- ties, the tolerance itself, chord ends ---------------------------------------------------------------------------------------------
def test_random_scene_full_of_ties(hip):
    rings = ss.random_scene(seed=4)
    rv, off = ss.table(rings)
    tally = ss.simplify_np(rv, off, ss.RANDOM_T)[4]
    assert 35 <= len(rings) <= 45 and 3500 <= len(rv) <= 4500
    assert tally["ties"] >= 50 and tally["at_tolerance"] >= 50 and tally["endpoint"] >= 50 and tally["collapsed"] >= 1
    same(hip, (rv, off), ss.RANDOM_T)
    same(hip, (rv, off), 0)
    fixed = ss.shared_border_fixed_np(rv, off)                              # repeated positions: many fixed vertices, many chains a ring
    assert 100 < fixed.sum() < len(rv)
    same(hip, (rv, off), ss.RANDOM_T, fixed)


def test_sawtooth_takes_a_pass_per_interior_vertex(hip):
    ring = ss.sawtooth(300)
    got, _ = same(hip, [ring], 3)
    assert got[3][ss.PASSES] == 299 and got[3][ss.KEPT] == 300


def test_corners_at_the_snap_limit(hip):
    L = 2 ** 40
    ring = [(-L, -L), (0, -L + 1), (L, -L), (L - 1, 0), (L, L), (1, L), (-L, L), (-L + 3, 5)]
    for T in (0, 1, 2, 2 ** 40 - 1):
        got, _ = same(hip, [ring], T)
    assert got[1].tolist() == [0, 2, 4, 6]             # the corners are 2^40 sqrt 2 off the diagonals, everything else goes
    got, _ = same(hip, [ring, [(L, L), (-L, L), (-L, -L)]], 1)
    assert got[3][ss.WIDE] > 0 and got[1].tolist()[-3:] == [8, 9, 10]


# ---- fixed vertices --------------------------------------------------------------------------------------------------------------------
def test_shared_borders_scene_with_fixed_vertices(hip):
    rings, names, wiggle = ss.s9_scene()
    rv, off = ss.table(rings)
    fixed = geometric.shared_border_fixed(rv, off)
    assert np.array_equal(fixed, ss.shared_border_fixed_np(rv, off)) and fixed.sum() == 9
    for T in (0, 3, 6, 40, 400):
        got, _ = same(hip, (rv, off), T, fixed)
        kept = [{tuple(v) for v in rv[got[1][got[2][r]:got[2][r + 1]]].tolist()} for r in range(5)]
        assert kept[0] & set(wiggle) == kept[2] & set(wiggle) and kept[1] == kept[3]
    same(hip, (rv, off), 6, np.ones(len(rv), dtype=np.uint8))               # every vertex fixed: no chain has an interior, no pass
    same(hip, (rv, off), 6, fixed.astype(bool))


# ---- fenced outputs, poisoned scratch ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    backend = FencedHipRaster(0)
    yield backend
    backend.close()


@pytest.mark.parametrize("n", [1, 65, 257])
def test_outputs_between_fences(ctx, n):
    """Every output byte is written -- none keeps the 0x7F it was handed with --, none beside the outputs, and the inputs handed
    over on the device come back bit for bit."""
    rings = [polygon_ring(n, seed=n)] if n >= 3 else [np.array([[4, 4]])]
    rings = rings + [np.array([[0, 0], [50, 1], [100, 0], [50, -1]])]       # ... and a ring that collapses: entries of -1 behind M
    rv, off = ss.table(rings)
    fixed = np.zeros(len(rv), dtype=np.uint8)
    fixed[::7] = 1
    want = ss.simplify_np(rv, off, 900, fixed)
    with fenced(ctx):
        inputs = [torch.as_tensor(a).to(ctx.device) for a in (rv, off, fixed)]
        clones = [t.clone() for t in inputs]
        keep, kept_index, out_offsets, stats = ctx.ring_simplifier().simplify(inputs[0], inputs[1], 900e-6, inputs[2])
        for got, wanted in zip((keep, kept_index, out_offsets, stats), want[:4]):
            assert np.array_equal(_np(got), wanted)
        for t, clone in zip(inputs, clones):
            assert torch.equal(t.reshape(-1).view(torch.uint8), clone.reshape(-1).view(torch.uint8)), "a device input was written"
        whole = [p for p in ctx.fences.payloads(torch.int32) if p.shape == (len(rv),)]
        assert len(whole) == 1 and _np(whole[0]).tolist() == want[1].tolist() + [-1] * (len(rv) - len(want[1]))
        flags = ctx.fences.payloads(torch.uint8)
        assert len(flags) == 1 and int(flags[0].max()) <= 1 and POISON > 1
        assert len(want[1]) < len(rv)


@contextmanager
def poison(backend, bits):
    backend.set_option(_hip.GR_OPT_DEBUG, bits)
    try:
        yield
    finally:
        backend.set_option(_hip.GR_OPT_DEBUG, 0)


def test_poisoned_stage_arena(ctx):
    """The call writes every scratch word before it reads it: the same answers over an arena of 0xFF, of 0x7F and as it was left."""
    rings = ss.random_scene(seed=2, rings=12, total=900) + [ss.sawtooth(40)]
    rv, off = ss.table(rings)
    fixed = ss.shared_border_fixed_np(rv, off)
    same(ctx, (rv, off), ss.RANDOM_T)                                        # grows the arena first
    results = []
    for bits in (0, _hip.GR_DBG_POISON_STAGE, _hip.GR_DBG_POISON_STAGE_7F, _hip.GR_DBG_POISON_STAGE, 0):
        with poison(ctx, bits):
            results.append([same(ctx, (rv, off), ss.RANDOM_T)[0], same(ctx, (rv, off), 0, fixed)[0], same(ctx, [rings[0][:3]], 1)[0]])
            if bits:
                tail, _ = ctx.debug_stage(0, -64, 64)
                assert bool((tail == (0xFF if bits == _hip.GR_DBG_POISON_STAGE else 0x7F)).all())
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
class Host(ss.StandInBackend, osn.StandInBackend):
    pass


def test_export_equals_the_host_path(hip, tmp_path):
    verts_q, faces, quad = osn.grid_mesh(15, 15)
    assert verts_q.shape == (256, 2) and faces.shape == (450, 3)
    points = np.column_stack([verts_q / 1e6, np.zeros(len(verts_q))])
    labels = np.asarray(osn.quad_classes(quad, [(i // 4 + 2 * (j // 4)) % 3 for j in range(15) for i in range(15)]), dtype=np.float64)
    step = 1.0   # metres between the grid's vertices
    results = {}
    for name, backend in (("device", hip), ("host", Host())):
        mesh = TexturedPhotogrammetryMesh((points, faces.astype(np.int64)), log_level="ERROR", backend=backend)
        for tol in (0.0, 0.3 * step, 3 * step):
            polygons, columns = mesh.export_face_labels_vector(labels, tmp_path / f"{name}_{tol:.3f}.geojson", label_names=["a", "b", "c"],
                                                               points_in_export_CRS=points, simplify_tol=tol, simplify_method=METHOD)
            results[name, tol] = (polygons, columns, mesh.last_outline_stats)
    for (name, tol), dev in results.items():
        if name != "device":
            continue
        host = results["host", tol]
        assert dev[2] == host[2] and dev[2]["simplify_passes"] >= 1 and dev[0].n_polygons == host[0].n_polygons
        assert len(dev[0].rings) == len(host[0].rings) and all(np.array_equal(a, b) for a, b in zip(dev[0].rings, host[0].rings))
        assert np.array_equal(dev[0].ring_polygon, host[0].ring_polygon) and np.array_equal(dev[0].ring_is_hole, host[0].ring_is_hole)
        assert (tmp_path / f"device_{tol:.3f}.geojson").read_text() == (tmp_path / f"host_{tol:.3f}.geojson").read_text()
    plain = TexturedPhotogrammetryMesh((points, faces.astype(np.int64)), log_level="ERROR", backend=hip).export_face_labels_vector(
        labels, points_in_export_CRS=points)[0]
    assert sum(len(r) for r in results["device", 0.0][0].rings) < sum(len(r) for r in plain.rings)   # T = 0 drops the collinear ones


def test_region_superset_on_the_device(hip):
    rng = np.random.default_rng(12)
    angle = np.sort(rng.uniform(0, 2 * np.pi, 400))
    radius = 5.0 + rng.uniform(-0.4, 0.4, 400)
    hole = np.column_stack([1.0 * np.cos(angle[::8]), 1.0 * np.sin(angle[::8])])[::-1] + rng.uniform(-0.1, 0.1, (50, 2))
    roi = PlanarPolygons([np.column_stack([radius * np.cos(angle), radius * np.sin(angle)]), hole], [0, 0], [False, True])
    points = rng.uniform(-7.5, 7.5, (20_000, 2))
    for b, s in ((0.0, 0.3), (0.25, 0.5), (0.5, 2.0)):
        simple = roi.simplified(s, hip)
        assert 3 <= sum(len(r) for r in simple.rings) < 200 and simple.last_simplify_stats["passes"] >= 2
        inside = _np(geometric.points_in_region(hip, roi, points, b)[0]).astype(bool)
        wider = _np(geometric.points_in_region(hip, simple, points, b + s)[0]).astype(bool)
        assert inside.sum() > 1000 and (~wider).sum() > 1000 and not np.any(inside & ~wider), (b, s)
