"""Nearest points without a GPU (include/geograster_nearest.h): the numpy stand-in against scipy's KD-tree --
the reference's arithmetic -- on every scene wherever the nearest ref is unique, the C ABI (header <-> `_NEAREST_SIGNATURES` <->
`NearestArgs` <-> exported symbol), the argument errors of the Python layers, and `values_from_mesh`, `transfer_texture` and the
new arguments of `aggregate_images` over a stand-in backend."""
import ctypes
import logging
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import nearest_points_scenes as sc  # noqa: E402
import nearest_points_standin as nn  # noqa: E402
from decimate_standin import StandInBackend as DecimateBackend  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric  # noqa: E402
from tests.test_mesh_vis_host import OraclePictureBackend, aggregate_scene  # noqa: E402
from tests.test_raster_warp_host import C_TYPES  # noqa: E402


# -- the stand-in is the reference's arithmetic -----------------------------------------------------------------------------------------
def kdtree_rows(s):
    from scipy.spatial import cKDTree

    ref, query = nn.as_points(s["ref"]), nn.as_points(s["query"])
    part = np.nonzero(np.isfinite(ref).all(axis=1))[0]
    finite_q = np.isfinite(query).all(axis=1)
    rows = np.full(len(query), -1, dtype=np.int64)
    if len(part) and finite_q.any():
        with np.errstate(over="ignore", invalid="ignore"):
            _, found = cKDTree(ref[part]).query(query[finite_q])
        none = found >= len(part)      # the tree finds nothing where every distance overflows: the stand-in has a tie there
        rows[finite_q] = np.where(none, -1, part[np.where(none, 0, found)])
    return rows


@pytest.mark.parametrize("s", sc.all_scenes(), ids=lambda s: s["name"])
def test_standin_equals_the_kdtree_where_the_nearest_is_unique(s):
    index, dist2, gap, counts = nn.nearest(s["ref"], s["query"])
    rows = kdtree_rows(s)
    unique = gap > 0
    assert np.array_equal(index[unique], rows[unique]), s["name"]
    tied = float((~unique).mean()) if len(unique) else 0.0
    if s["name"] == "terrain":
        assert tied == 0.0, "no two refs of the terrain are equally near a query"
    if s["name"] == "lattice":
        assert 0.0 < tied <= 0.10, tied
    # among equally near refs the stand-in names the lowest row
    ref, query = nn.as_points(s["ref"]), nn.as_points(s["query"])
    for q in np.nonzero(~unique & (index >= 0))[0][:50]:
        d = query[q] - ref
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert index[q] == np.nonzero(d2 == dist2[q])[0][0]


def test_the_scenes_hold_what_they_are_meant_to():
    by_name = {s["name"]: s for s in sc.all_scenes()}
    assert len(by_name) == len(sc.all_scenes()) == 4 + 8 + 30
    index, dist2, gap, counts = nn.nearest(by_name["duplicates"]["ref"], by_name["duplicates"]["query"])
    assert (gap == 0).all() and (dist2[-40:] == 0).all()
    ref = by_name["duplicates"]["ref"]
    for q in range(len(index)):
        assert index[q] == np.nonzero((ref == ref[index[q]]).all(axis=1))[0][0], "the lowest of the three equal rows"
    kept, dropped = (nn.nearest(s["ref"], s["query"], s["max_distance"]) for s in sc.threshold_scenes())
    assert kept[0].tolist() == [0, 0] and kept[1].tolist() == [25.0, 0.0] and kept[3] == (0, 0, 0)
    assert dropped[0].tolist() == [-1, 0] and np.isnan(dropped[1][0]) and dropped[3] == (0, 0, 1)
    assert nn.nearest(by_name["nonfinite"]["ref"], by_name["nonfinite"]["query"])[3][:2] == (5, 4)
    index, dist2, _, counts = nn.nearest(by_name["no_finite_ref"]["ref"], by_name["no_finite_ref"]["query"])
    assert index.tolist() == [-1, -1, -1] and np.isnan(dist2).all() and counts == (5, 1, 3)
    s = by_name["corner"]
    assert np.floor((64.0 - 0.0) / s["cell"]) == 2 ** 21, "one past the last of 2^21 cells"
    assert by_name["planar"]["ref"].shape[1] == 2 and by_name["sizes_R0_Q257"]["ref"].shape == (0, 3)
    assert len(sc.sweep_arguments(by_name["terrain"])) == 12


# -- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def header_struct(name):
    """[(field, ctypes type)] of `typedef struct <name> { ... } <name>;` in include/geograster_nearest.h, read as
    tests/test_face_sieve_host.py reads its header: a field with a `*` is a pointer, every other one of the four scalar types."""
    text = (ROOT / "include" / "geograster_nearest.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for statement in filter(None, (s.strip() for s in body.split(";"))):
        pointer = re.fullmatch(r"(?:const\s+)?\w+\s*\*\s*(\w+)", statement)
        scalar = re.fullmatch(r"(int64_t|int32_t|float|double)\s+(\w+)", statement)
        assert pointer or scalar, statement
        fields.append((pointer.group(1), ctypes.c_void_p) if pointer else (scalar.group(2), C_TYPES[scalar.group(1)]))
    return fields


def test_descriptor_mirror_equals_the_header_field_by_field():
    want = header_struct("gr_nearest_args")
    assert len(want) == 12
    assert [(n, t) for n, t in _hip.NearestArgs._fields_] == want
    assert ctypes.sizeof(_hip.NearestArgs) == 88
    assert ("stream", ctypes.c_void_p) in want and ("cell", ctypes.c_double) in want


def test_header_binding_and_source_name_the_call():
    main = (ROOT / "include" / "geograster.h").read_text()
    header = (ROOT / "include" / "geograster_nearest.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "nearest.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\bint (gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", stripped))
    assert declared == {"gr_nearest_points": "gr_ctx *ctx, const gr_nearest_args *args_h"}
    assert _hip.NEAREST_SYMBOLS == tuple(declared)
    assert _hip._NEAREST_SIGNATURES == {"gr_nearest_points": [ctypes.c_void_p, ctypes.POINTER(_hip.NearestArgs)]}
    assert not re.search(r"gr_nearest_points\s*\(", main) and main.count('#include "geograster_nearest.h"') == 1
    assert main.index('#include "geograster_nearest.h"') > main.index('#include "geograster_components.h"')
    assert main.index('#include "geograster_nearest.h"') < main.rindex("#ifdef __cplusplus"), "inside the extern \"C\" block"
    flat = " ".join(header.replace(" * ", " ").split())
    assert "#define GR_VERSION 126" in main and "without a GR_VERSION bump" in flat
    assert "never touches another stream" in flat and "once per level" in flat and "tests/test_stream_contract_nearest_gpu.py" in flat
    assert "R and Q < 2^31 - 1" in flat
    text = Path(build.__file__).read_text()
    assert any(p.name == "nearest.hip" for p in build.SOURCES) and "geograster_nearest.h" in text
    kernels = set(re.findall(r"void (k_\w+)\(", source))
    assert {"k_nn_bounds", "k_nn_keys", "k_nn_gather", "k_nn_query", "k_nn_none", "k_nn_stats"} <= kernels
    assert "nearest.hip" in internal and all(k in internal for k in ("k_nn_keys", "k_nn_query"))
    # cub_steps.hpp remains the only file that calls hipcub
    assert "hipcub" not in source and '#include "cub_steps.hpp"' in source and "stage_acquire" in source
    names = [n for n in vars(_hip) if n.startswith("GR_NN_STAT_") and n != "GR_NN_STAT_WORDS"]
    assert len(names) == _hip.GR_NN_STAT_WORDS == len(_hip.NEAREST_STAT_NAMES) == len(geometric.NEAREST_STAT_NAMES) == nn.STAT_WORDS
    assert _hip.NEAREST_STAT_NAMES == geometric.NEAREST_STAT_NAMES
    assert [getattr(_hip, "GR_NN_STAT_" + n.upper()) for n in _hip.NEAREST_STAT_NAMES] == list(range(9))
    enum = dict(re.findall(r"(GR_NN_STAT_\w+) = (\d+)", main))
    assert {k: int(v) for k, v in enum.items()} == {n: getattr(_hip, n) for n in names + ["GR_NN_STAT_WORDS"]}
    assert (nn.REF_NONFINITE, nn.QUERY_NONFINITE, nn.NO_ANSWER, nn.LEVELS, nn.CARRIED, nn.CELLS_PROBED, nn.CANDIDATES, nn.CELL_BITS,
            nn.RING_CAP) == tuple(range(9))


def test_the_library_exports_the_call_and_refuses_without_a_device():
    lib = ctypes.CDLL(str(_hip.library_path()))
    fn = lib.gr_nearest_points
    fn.restype, fn.argtypes = ctypes.c_int, _hip._NEAREST_SIGNATURES["gr_nearest_points"]
    assert fn(None, None) == _hip.GR_EINVAL
    assert fn(None, ctypes.byref(_hip.NearestArgs())) == _hip.GR_EINVAL


# -- the argument errors ------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_on_the_host():
    check = _hip.check_nearest_arguments
    assert check(3, 5, None, 0.0, 2) == (float("inf"), 0.0, 2) and check(0, 0, 5, 1, 1) == (5.0, 1.0, 1)
    for bad, message in (((2 ** 31 - 1, 1, None, 0.0, 2), "each in"), ((1, 2 ** 31 - 1, None, 0.0, 2), "each in"),
                         ((1, 1, -1.0, 0.0, 2), "max_distance"), ((1, 1, float("nan"), 0.0, 2), "max_distance"),
                         ((1, 1, None, -1.0, 2), "cell"), ((1, 1, None, float("inf"), 2), "cell"), ((1, 1, None, float("nan"), 2), "cell"),
                         ((1, 1, None, 0.0, 0), "max_rings"), ((1, 1, None, 0.0, 1.5), "max_rings")):
        with pytest.raises(ValueError, match="gr_nearest_points: .*" + message):
            check(*bad)


def test_module_function_shapes_and_results():
    backend = nn.StandinNearestBackend()
    ref = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [10.0, 0.0, 0.0]])
    index, stats = geometric.nearest_points(backend, ref, np.array([[1.0, 1.0, 0.0], [9.0, 0.0, 1.0], [np.nan, 0.0, 0.0]]))
    assert index.dtype == np.int32 and index.tolist() == [0, 1, -1]
    assert list(stats) == list(geometric.NEAREST_STAT_NAMES) + ["cell"] and stats["query_nonfinite"] == 1 and stats["no_answer"] == 1
    index, dist2, stats = geometric.nearest_points(backend, ref[:, :2], np.array([[4.0, 3.0]]), max_distance=5.0, return_dist2=True)
    assert index.tolist() == [0] and dist2.tolist() == [25.0] and backend.nearest_calls[-1]["max_distance"] == 5.0
    index, _ = geometric.nearest_points(backend, ref[:, :2], np.array([[4.0, 3.0, 0.0]]), max_distance=4.9)
    assert index.tolist() == [-1]
    for bad_ref, bad_query, message in ((ref[:, :1], ref, "ref must be"), (ref, ref.reshape(-1), "query must be"),
                                        (np.zeros((2, 4)), ref, "ref must be"), (ref, np.zeros((2, 3, 1)), "query must be")):
        with pytest.raises(ValueError, match=message):
            geometric.nearest_points(backend, bad_ref, bad_query)
    with pytest.raises(ValueError, match="max_rings"):
        geometric.nearest_points(backend, ref, ref, max_rings=0)
    assert geometric.gather_rows(np.array([[1, 2], [3, 4]]), np.array([1, -1, 0]), -7).tolist() == [[3, 4], [-7, -7], [1, 2]]
    assert geometric.gather_rows(np.zeros((0, 2)), np.array([-1, -1]), np.nan).shape == (2, 2)


# -- the mesh methods ----------------------------------------------------------------------------------------------------------------------
def grid_mesh(n, backend, **kw):
    """An n x n vertex grid of unit squares in the plane z = 0, two faces a square: n^2 vertices, 2 (n - 1)^2 faces."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    points = np.stack([i, j, np.zeros_like(i)], axis=-1).reshape(-1, 3).astype(np.float64)
    v = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([v, v + n, v + 1], axis=1), np.stack([v + 1, v + n, v + n + 1], axis=1)])
    return TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=backend, **kw)


def test_values_from_mesh_inference_fill_and_integers():
    backend = nn.StandinNearestBackend()
    coarse, fine = grid_mesh(3, backend), grid_mesh(3, backend)
    fine.points = fine.points * 1.0 + np.array([0.1, 0.2, 0.0])            # the same scene, shifted a little
    n_points, n_faces = len(coarse.points), len(coarse.faces)
    assert (n_points, n_faces) == (9, 8)
    vertex_values = np.arange(n_points, dtype=np.float64) * 10
    got, index = fine.values_from_mesh(coarse, vertex_values, return_index=True)
    assert index.tolist() == list(range(9)) and got.tolist() == vertex_values.tolist() and fine.last_transfer_stats["on"] == "vertices"
    assert backend.nearest_calls[-1]["R"] == 9 and backend.nearest_calls[-1]["Q"] == 9
    face_values = np.arange(n_faces * 2, dtype=np.float32).reshape(n_faces, 2)
    got = fine.values_from_mesh((coarse.points, coarse.faces), face_values)
    assert got.dtype == np.float32 and got.tolist() == face_values.tolist() and fine.last_transfer_stats["on"] == "faces"
    want_index, _, _, _ = nn.nearest(coarse._face_centres(coarse.points, coarse.faces), fine._face_centres(fine.points, fine.faces))
    assert want_index.tolist() == list(range(8))
    # a tight limit: the shift is sqrt(0.05) = 0.2236...
    got = fine.values_from_mesh(coarse, vertex_values, max_distance=0.2)
    assert np.isnan(got).all() and fine.last_transfer_stats["no_answer"] == 9
    got = fine.values_from_mesh(coarse, vertex_values, max_distance=0.25, fill=-1.0)
    assert got.tolist() == vertex_values.tolist()
    # integers need an integer fill
    labels = np.arange(n_faces, dtype=np.int32)
    with pytest.raises(ValueError, match="integer values need an integer fill"):
        fine.values_from_mesh(coarse, labels)
    got = fine.values_from_mesh(coarse, labels, fill=-1, max_distance=0.01)
    assert got.dtype == np.int32 and got.tolist() == [-1] * 8
    assert fine.values_from_mesh(coarse, labels, fill=-1).tolist() == labels.tolist()
    # counts
    with pytest.raises(ValueError, match="7 values fit neither the 9 vertices nor the 8 faces"):
        fine.values_from_mesh(coarse, np.zeros(7))
    with pytest.raises(ValueError, match="8 values for the 9 vertices"):
        fine.values_from_mesh(coarse, np.zeros(8), on="vertices")
    with pytest.raises(ValueError, match="on='edges'"):
        fine.values_from_mesh(coarse, np.zeros(8), on="edges")
    with pytest.raises(ValueError, match="no texture on its faces"):
        fine.values_from_mesh(coarse, on="faces")
    with pytest.raises(ValueError, match="must be a mesh object"):
        fine.values_from_mesh((coarse.points, coarse.faces))
    # a count that fits vertices and faces alike: four vertices, four faces
    points = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    faces = np.array([[0, 1, 2], [1, 3, 2], [0, 2, 1], [1, 2, 3]])
    with pytest.raises(ValueError, match="Cannot infer"):
        fine.values_from_mesh((points, faces), np.zeros(4))
    assert fine.values_from_mesh((points, faces), np.arange(4.0), on="vertices").shape == (9,)
    assert fine.values_from_mesh((points, faces), np.arange(4.0), on="faces").shape == (8,)
    # values=None: the source's texture
    coarse.set_texture(vertex_values, is_vertex_texture=True)
    assert fine.values_from_mesh(coarse).tolist() == vertex_values.reshape(-1, 1).tolist()


def test_transfer_texture_vertex_face_and_untouched_target(caplog):
    backend = nn.StandinNearestBackend()
    full, small = grid_mesh(5, backend), grid_mesh(3, backend)
    small.points = small.points * 2.0                                      # the same square, every second vertex
    texture = np.arange(25, dtype=np.float64)
    full.set_texture(texture, is_vertex_texture=True)
    full.IDs_to_labels = {k: f"class {k}" for k in range(25)}
    assert full.transfer_texture(small) is small
    want = texture.reshape(5, 5)[::2, ::2].reshape(-1, 1)
    assert small.vertex_texture.tolist() == want.tolist() and small.face_texture is None and small.IDs_to_labels == full.IDs_to_labels
    # a face texture is not transferred: the reference's warning, the target as it was
    full.set_texture(np.arange(32, dtype=np.float64), is_vertex_texture=False)
    assert full.vertex_texture is None
    untouched = grid_mesh(3, backend)
    calls = len(backend.nearest_calls)
    with caplog.at_level(logging.WARNING):
        full.logger.setLevel(logging.WARNING)
        assert full.transfer_texture(untouched) is untouched
    assert untouched.vertex_texture is None and untouched.face_texture is None and untouched.IDs_to_labels is None
    assert len(backend.nearest_calls) == calls and "Textures not transferred" in caplog.text
    # ... unless asked for
    small.face_texture = small.vertex_texture = None
    full.transfer_texture(small, face_textures=True, max_distance=10.0)
    centres_full, centres_small = full._face_centres(full.points, full.faces), small._face_centres(small.points, small.faces)
    index, _, gap, _ = nn.nearest(centres_full, centres_small)
    assert small.face_texture.shape == (8, 1) and small.face_texture[:, 0].tolist() == index.astype(np.float64).tolist()
    assert small.vertex_texture is None


# -- aggregate_images ---------------------------------------------------------------------------------------------------------------------
class RecordingBackend(OraclePictureBackend, DecimateBackend, nn.StandinNearestBackend):
    pass


def test_aggregate_images_plumbing(tmp_path):
    from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args

    args, kw, _ = aggregate_scene(tmp_path)
    with pytest.raises(ValueError, match="without mesh_downsample_method"):
        aggregate_images(*args, backend=RecordingBackend(), full_mesh_face_classes_savefile=tmp_path / "full.npy", **kw)
    with pytest.raises(ValueError, match="nothing is transferred"):
        aggregate_images(*args, backend=RecordingBackend(), transfer_max_distance_meters=1.0, **kw)
    with pytest.raises(ValueError, match="not a distance"):
        aggregate_images(*args, backend=RecordingBackend(), transfer_max_distance_meters=-1.0, mesh_downsample=0.25,
                         mesh_downsample_method="cluster", full_mesh_face_classes_savefile=tmp_path / "full.npy", **kw)
    plain_backend = RecordingBackend()
    _, _, plain = aggregate_images(*args, backend=plain_backend, mesh_downsample=0.25, mesh_downsample_method="cluster",
                                   predicted_face_classes_savefile=tmp_path / "plain.npy", **kw)
    assert "nearest_calls" not in vars(plain_backend), "with the defaults nothing is transferred"
    backend = RecordingBackend()
    mesh, _, classes = aggregate_images(*args, backend=backend, mesh_downsample=0.25, mesh_downsample_method="cluster",
                                        predicted_face_classes_savefile=tmp_path / "classes.npy",
                                        full_mesh_face_classes_savefile=tmp_path / "sub" / "full.npy", transfer_max_distance_meters=50.0, **kw)
    assert np.array_equal(classes, plain, equal_nan=True) and np.array_equal(np.load(tmp_path / "classes.npy"), plain, equal_nan=True)
    full = np.load(tmp_path / "sub" / "full.npy")
    data = np.load(args[0])
    assert full.shape == (len(data["faces"]), 1) and full.dtype == np.float64 and len(mesh.faces) < len(data["faces"])
    assert len(backend.nearest_calls) == 1 and backend.nearest_calls[0]["max_distance"] == 50.0
    assert backend.nearest_calls[0] == dict(backend.nearest_calls[0], R=len(mesh.faces), Q=len(data["faces"]))
    # (a kept face has the cell representatives for corners, not its own: its centre moved, and it need not get its own class back)
    centre =lambda p, f: ((p[f[:, 0]] + p[f[:, 1]]) + p[f[:, 2]]) / 3.0   # noqa: E731
    index, _, _, _ = nn.nearest(centre(np.asarray(mesh.points), np.asarray(mesh.faces)), centre(data["points"], data["faces"]), 50.0)
    assert np.array_equal(full, nn.gather(classes, index, np.nan), equal_nan=True)
    assert mesh.last_transfer_stats["on"] == "faces"
    base = ["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--label-folder", "l",
            "--IDs-to-labels", "ids.json"]
    parsed = parse_args(base)
    assert parsed.full_mesh_face_classes_savefile is None and parsed.transfer_max_distance_meters is None
    parsed = parse_args(base + ["--full-mesh-face-classes-savefile", "full.npy", "--transfer-max-distance-meters", "2.5"])
    assert parsed.full_mesh_face_classes_savefile == Path("full.npy") and parsed.transfer_max_distance_meters == 2.5
