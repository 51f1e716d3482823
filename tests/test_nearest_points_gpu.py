"""gr_nearest_points on the device against the brute-force stand-in of tests/nearest_points_standin.py: every
scene of tests/nearest_points_scenes.py, index and dist2 byte for byte, through fenced outputs over a poisoned stage arena; the
sweep of cell and max_rings (K3: identical bytes); every GR_EINVAL case; the statistics; and `values_from_mesh` and
`aggregate_images` on the C1 scene.

One case differs from the issue that asked for these tests.  It expected that, with face values carried from C1 decimated to 0.25
back onto C1, "every kept face gets its own value".  A kept face of the vertex clustering has the cell representatives for corners,
not its own, so its centre moves: by the brute-force stand-in itself 12.2 % of the 2426 kept faces are nearer to the centre of
another decimated face.  The case is held where it is true -- per vertex, a kept vertex IS an input vertex -- and every face is
compared with the stand-in's gather, which is the stronger statement."""
import ctypes
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import nearest_points_scenes as sc  # noqa: E402
import nearest_points_standin as nn  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402
from tests.fenced_backend import FencedHipRaster, fenced  # noqa: E402
from tests.test_mesh_vis_host import aggregate_scene  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = sc.all_scenes()


@pytest.fixture(scope="module")
def ctx():
    backend = FencedHipRaster(0)
    yield backend
    backend.close()


_wanted = {}


def standin(s):
    """The stand-in's answer for a scene: computed once, shared, not modified."""
    if s["name"] not in _wanted:
        index, dist2, gap, counts = nn.nearest(s["ref"], s["query"], s["max_distance"])
        for a in (index, dist2):
            a.setflags(write=False)
        _wanted[s["name"]] = (index, dist2, counts)
    return _wanted[s["name"]]


def device(backend, s, **kw):
    arguments = dict(max_distance=s["max_distance"], cell=s["cell"], max_rings=s["max_rings"])
    arguments.update(kw)
    index, dist2, stats = geometric.nearest_points(backend, s["ref"], s["query"], return_dist2=True, **arguments)
    return index, dist2, stats


def assert_same(got, want, name):
    for g, w, what in zip(got[:2], want[:2], ("index", "dist2")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, what, g[:16].tolist(), w[:16].tolist())
    stats = got[2]
    assert (stats["ref_nonfinite"], stats["query_nonfinite"], stats["no_answer"]) == want[2], (name, stats)


@contextmanager
def poison(backend, bits):
    backend.set_option(_hip.GR_OPT_DEBUG, bits)
    try:
        yield
    finally:
        backend.set_option(_hip.GR_OPT_DEBUG, 0)


@pytest.mark.parametrize("s", SCENES, ids=lambda s: s["name"])
def test_scene_equals_the_standin_over_a_poisoned_arena(ctx, s):
    """K3, K6: the same bytes over an arena of 0xFF, of 0x7F and as it was left, between intact fences."""
    for bits in (_hip.GR_DBG_POISON_STAGE, _hip.GR_DBG_POISON_STAGE_7F, 0):
        with poison(ctx, bits):
            with fenced(ctx):
                got = device(ctx, s)
        assert_same(got, standin(s), (s["name"], bits))


@pytest.mark.parametrize("s", sc.main_scenes() + [sc.nonfinite_scene(), sc.one_point_scene(), sc.collinear_scene(), sc.corner_scene()],
                         ids=lambda s: s["name"])
def test_cell_and_rings_do_not_reach_the_answer(ctx, s):
    """K3: cell in {0, 1e-3 e1, e1 / 3, 10 e1} x max_rings in {1, 2, 5}: identical bytes."""
    levels = set()
    for cell, rings in sc.sweep_arguments(s):
        with fenced(ctx):
            got = device(ctx, s, cell=cell, max_rings=rings)
        assert_same(got, standin(s), (s["name"], cell, rings))
        levels.add(got[2]["levels"])
        if cell > 0:
            assert got[2]["cell"] == cell, "a cell above e1 / 2^21 is used as it is given"
    assert min(levels) >= 1


def test_same_call_twice_and_fresh_context(ctx):
    fresh = _hip.HipRaster(0)
    try:
        for s in (sc.lattice_scene(), sc.two_clusters_scene()):
            first, again, other = device(ctx, s), device(ctx, s), device(fresh, s)
            for got in (first, again, other):
                assert_same(got, standin(s), s["name"])
            assert first[2] == again[2] == other[2], "the statistics too are the same on every run"
    finally:
        fresh.close()


def test_statistics(ctx):
    s = sc.two_clusters_scene()
    _, _, stats = device(ctx, s)
    assert stats["levels"] > 1 and stats["carried"] >= stats["levels"] - 1 and stats["ring_cap"] == 1
    assert stats["cell"] == 0.01 and stats["cells_probed"] > 0 and stats["candidates"] >= len(s["query"])
    _, _, easy = device(ctx, sc.terrain_scene())
    assert easy["levels"] >= 1 and easy["levels"] <= 12
    assert easy["candidates"] >= 14400 and easy["cell"] > 0 and easy["no_answer"] == 0
    s = sc.nonfinite_scene()
    _, _, stats = device(ctx, s)
    assert (stats["ref_nonfinite"], stats["query_nonfinite"], stats["no_answer"]) == (5, 4, 4)
    _, _, stats = device(ctx, sc.no_finite_ref_scene())
    assert (stats["ref_nonfinite"], stats["query_nonfinite"], stats["no_answer"], stats["levels"], stats["cell_bits"]) == (5, 1, 3, 0, 0)
    _, _, stats = device(ctx, sc.sizes_scene(65, 0))
    assert stats["levels"] == 0 and stats["candidates"] == 0
    kept, dropped = (device(ctx, s) for s in sc.threshold_scenes())
    assert kept[0].tolist() == [0, 0] and kept[1].tolist() == [25.0, 0.0] and dropped[0].tolist() == [-1, 0] and np.isnan(dropped[1][0])


def test_without_dist2(ctx):
    s = sc.duplicates_scene()
    with fenced(ctx):
        index, stats = ctx.nearest_points(s["ref"], s["query"])
        index = index.cpu().numpy()
    assert index.tobytes() == standin(s)[0].tobytes() and stats.shape == (_hip.GR_NN_STAT_WORDS,)


def test_every_einval_case(ctx):
    R, Q = 6, 4
    ref = torch.arange(3 * R, dtype=torch.float64, device=ctx.device).reshape(R, 3)
    query = torch.ones((Q, 3), dtype=torch.float64, device=ctx.device)
    index = torch.full((Q,), 77, dtype=torch.int32, device=ctx.device)
    dist2 = torch.full((Q,), 77.0, dtype=torch.float64, device=ctx.device)
    stats = torch.empty(_hip.GR_NN_STAT_WORDS, dtype=torch.int64, device=ctx.device)
    both = torch.empty(4 * Q, dtype=torch.int32, device=ctx.device)
    good = dict(ref=ref.data_ptr(), query=query.data_ptr(), index_out=index.data_ptr(), dist2_out=dist2.data_ptr(), stats=stats.data_ptr(),
                stream=ctx._stream().value, R=R, Q=Q, cell=0.0, max_distance=float("inf"), max_rings=2, reserved=0)

    def call(**changed):
        args = _hip.NearestArgs(**{**good, **changed})
        return ctx._rc("gr_nearest_points", ctypes.byref(args))

    assert call() == _hip.GR_OK and call(dist2_out=None) == _hip.GR_OK and call(max_distance=0.0) == _hip.GR_OK
    assert call(ref=None, R=0) == _hip.GR_OK and call(query=None, index_out=None, dist2_out=None, Q=0) == _hip.GR_OK
    torch.cuda.synchronize(ctx.device)
    sentinel = torch.full_like(stats, 77)
    index.fill_(77)
    dist2.fill_(77.0)
    bad = [dict(ref=None), dict(query=None), dict(index_out=None), dict(stats=None),
           dict(R=-1), dict(Q=-1), dict(R=2 ** 31 - 1), dict(Q=2 ** 31 - 1), dict(cell=-1.0), dict(cell=float("inf")), dict(cell=float("nan")),
           dict(max_distance=-1.0), dict(max_distance=float("nan")), dict(max_rings=0), dict(max_rings=-2),
           dict(index_out=ref.data_ptr()), dict(index_out=query.data_ptr() + 8), dict(dist2_out=ref.data_ptr() + 16),
           dict(dist2_out=query.data_ptr()), dict(stats=ref.data_ptr()), dict(stats=query.data_ptr() + 24),
           dict(dist2_out=index.data_ptr()), dict(stats=dist2.data_ptr()), dict(index_out=both.data_ptr() + 8, dist2_out=both.data_ptr()),
           dict(index_out=stats.data_ptr())]
    for changed in bad:
        stats.copy_(sentinel)
        assert call(**changed) == _hip.GR_EINVAL, changed
        message = ctx.lib.gr_last_error(ctx._ctx).decode()
        assert message.startswith("gr_nearest_points: "), (changed, message)
        torch.cuda.synchronize(ctx.device)
        if "stats" not in changed and changed.get("index_out") != stats.data_ptr():
            assert torch.equal(stats, sentinel), f"{changed}: device work before the refusal"
        assert bool((index == 77).all()) and bool((dist2 == 77.0).all()), f"{changed}: an output was written before the refusal"
    assert ctx._rc("gr_nearest_points", None) == _hip.GR_EINVAL
    with pytest.raises(ValueError, match="max_rings"):
        ctx.nearest_points(ref, query, max_rings=0)
    with pytest.raises(ValueError, match=r"query must be \(Q, 3\)"):
        ctx.nearest_points(ref, query[:, :2])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def centres(points, faces):
    p, f = np.asarray(points, dtype=np.float64), np.asarray(faces)
    return ((p[f[:, 0]] + p[f[:, 1]]) + p[f[:, 2]]) / 3.0


@pytest.fixture(scope="module")
def c1(ctx):
    (points, faces), _ = synthetic.config1_scene()
    full = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=ctx)
    (small_points, small_faces), point_IDs, face_IDs = full.decimate(0.25, return_original_IDs=True)
    return full, small_points, small_faces, point_IDs, face_IDs


def test_values_from_mesh_decimated_onto_full(ctx, c1):
    full, small_points, small_faces, point_IDs, face_IDs = c1
    assert 0 < len(small_faces) < len(full.faces) and 0 < len(small_points) < len(full.points)
    # face values: every face of the full mesh equals the stand-in's gather
    face_values = np.stack([np.arange(len(small_faces), dtype=np.float64), np.cos(np.arange(len(small_faces)))], axis=1)
    want_index, _, _, _ = nn.nearest(centres(small_points, small_faces), centres(full.points, full.faces))
    with fenced(ctx):
        got, index = full.values_from_mesh((small_points, small_faces), face_values, return_index=True)
    assert index.tobytes() == want_index.tobytes() and got.tobytes() == nn.gather(face_values, want_index, np.nan).tobytes()
    assert full.last_transfer_stats["on"] == "faces" and full.last_transfer_stats["no_answer"] == 0
    # vertex values: a kept vertex IS an input vertex, at distance 0 from itself -- it gets its own value
    vertex_values = np.arange(len(small_points), dtype=np.int32) * 3
    got, index = full.values_from_mesh((small_points, small_faces), vertex_values, fill=-1, return_index=True)
    want_index, want_d2, _, _ = nn.nearest(small_points, full.points)
    assert index.tobytes() == want_index.tobytes() and got.dtype == np.int32 and got.tobytes() == vertex_values[want_index].tobytes()
    assert (want_d2[point_IDs] == 0).all()
    own = np.asarray(small_points)[index[point_IDs]] == np.asarray(small_points)
    assert own.all(), "every kept vertex gets the value of a vertex at its own position"
    unique_rows = np.unique(np.asarray(small_points), axis=0).shape[0] == len(small_points)
    if unique_rows:
        assert got[point_IDs].tolist() == vertex_values.tolist(), "every kept vertex gets its own value"
    # a source mesh object with a texture, and tensors on the device
    source = TexturedPhotogrammetryMesh((small_points, small_faces), log_level="ERROR", backend=ctx)
    source.set_texture(face_values[:, :1], is_vertex_texture=False)
    assert full.values_from_mesh(source).tobytes() == nn.gather(face_values[:, :1], nn.nearest(centres(small_points, small_faces), centres(full.points, full.faces))[0], np.nan).tobytes()


def test_values_from_mesh_tight_max_distance(ctx, c1):
    full, small_points, small_faces, _, _ = c1
    face_values = np.arange(len(small_faces), dtype=np.float64)
    _, d2, _, _ = nn.nearest(centres(small_points, small_faces), centres(full.points, full.faces))
    limit = float(np.sqrt(np.median(d2)))
    want_index, _, _, counts = nn.nearest(centres(small_points, small_faces), centres(full.points, full.faces), limit)
    assert 0.2 < (want_index < 0).mean() < 0.8
    with fenced(ctx):
        got = full.values_from_mesh((small_points, small_faces), face_values, max_distance=limit, fill=-5.0)
    assert got.tobytes() == nn.gather(face_values, want_index, -5.0).tobytes()
    assert np.array_equal(got == -5.0, want_index < 0) and full.last_transfer_stats["no_answer"] == counts[2]


def test_aggregate_images_full_mesh_savefile(ctx, tmp_path):
    from geograypher_amd.entrypoints.aggregate_images import aggregate_images

    args, kw, _ = aggregate_scene(tmp_path)
    (points, faces), _ = synthetic.config1_scene()
    written = {}
    for name, extra in (("plain", {}), ("full", dict(full_mesh_face_classes_savefile=tmp_path / "full" / "full.npy"))):
        folder = tmp_path / name
        mesh, _, classes = aggregate_images(*args, backend=ctx, mesh_downsample=0.25, mesh_downsample_method="cluster",
                                            aggregated_face_values_savefile=folder / "values.npy",
                                            predicted_face_classes_savefile=folder / "classes.npy", **extra, **kw)
        written[name] = {p.name: p.read_bytes() for p in sorted(folder.iterdir())}
    assert set(written["plain"]) == {"values.npy", "classes.npy"}
    assert {k: v for k, v in written["full"].items() if k != "full.npy"} == written["plain"], "the other outputs are what they were"
    full = np.load(tmp_path / "full" / "full.npy")
    assert full.shape == (len(faces), 1) and full.dtype == np.float64 and len(mesh.faces) < len(faces)
    index, _, _, _ = nn.nearest(centres(mesh.points, mesh.faces), centres(points, faces))
    assert full.tobytes() == nn.gather(classes, index, np.nan).tobytes()
    assert np.isfinite(full).any() and mesh.last_transfer_stats["on"] == "faces"
