"""The face sieve without a GPU (include/geograster_components.h): the numpy stand-in against the answers
written out by hand, the termination property on the random set, `face_area_weights` and `weld_canon`, the C ABI (header <->
`_COMPONENTS_SIGNATURES` <-> `FaceSieveArgs` <-> exported symbol), the argument errors of the Python layers and the plumbing of
`aggregate_images` through a recording backend."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import face_sieve_scenes as sc  # noqa: E402
import face_sieve_standin as fs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric  # noqa: E402
from tests.test_mesh_vis_host import OraclePictureBackend, aggregate_scene  # noqa: E402
from tests.test_raster_warp_host import C_TYPES  # noqa: E402


def standin(s, **kw):
    return fs.sieve(s["faces"], s["classes"], s["weights"], s["min_measure"], s["fill"], s["canon"], n_vertices=s["V"], **kw)


class StandinSieveBackend:
    """`HipRaster.face_sieve` by the stand-in, on the host; it records its calls."""
    vertex_order = "r1"

    def __init__(self):
        self.calls = []

    def face_sieve(self, faces, classes, weights=None, min_measure=0, fill_unlabelled=False, vertex_canon=None, max_rounds=64,
                   n_vertices=None):
        F = len(faces)
        w = None if weights is None else np.asarray(weights)
        V = len(vertex_canon) if vertex_canon is not None else (n_vertices if n_vertices is not None else int(np.max(faces, initial=-1)) + 1)
        min_measure = _hip.check_sieve_arguments(F, V, w, min_measure, max_rounds)
        self.calls.append(dict(F=F, weights=w, min_measure=min_measure, fill=bool(fill_unlabelled), canon=vertex_canon, max_rounds=max_rounds))
        return fs.sieve(faces, classes, w, min_measure, fill_unlabelled, vertex_canon, max_rounds, n_vertices)[:3]


# -- the rules -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sc.HAND, ids=lambda s: s["name"])
def test_standin_gives_the_hand_answers(s):
    class_out, comp, stats, _ = standin(s)
    assert class_out.tolist() == s["want_class"].tolist()
    assert comp.tolist() == s["want_comp"].tolist()
    assert stats.tolist() == s["want_stats"]


def test_the_hand_table_holds_what_it_is_meant_to():
    by_name = {s["name"]: s for s in sc.HAND}
    assert len(by_name) == len(sc.HAND) == 18
    assert by_name["chain_1_2_3"]["want_stats"][fs.ROUNDS] == 1, "a chain of two pointers resolves in one changing round"
    assert by_name["weights_reach_2_61"]["weights"].sum() == (1 << 62) - 1
    assert float((1 << 61) - 1) == float(1 << 61), "the two measures of that scene are one float64"
    assert by_name["fan_of_4"]["want_stats"][fs.FAN_EDGES] == 1 and by_name["degenerate_between"]["want_comp"][1] == -1


def test_round_cap_is_a_stat_word_not_an_error():
    s = next(s for s in sc.HAND if s["name"] == "unlabelled_filled")          # two changing rounds
    class_out, comp, stats, _ = standin(s, max_rounds=1)
    assert stats.tolist() == [1, 3, 2, 1, 1, 0, 0, 1, 0] and class_out.tolist() == [1, 2, 2, 2, 2] and comp.tolist() == [0, 1, 1, 1, 1]
    assert standin(s, max_rounds=2)[2].tolist() == [2, 3, 1, 2, 0, 0, 0, 1, 0], "the cap is reached although the labelling is final"
    assert standin(s, max_rounds=3)[2].tolist() == s["want_stats"]


def test_border_strips_and_the_spiral():
    for n in sc.BORDER_SIZES:
        class_out, comp, stats, _ = standin(sc.border_scene(n))
        # all measures tie: face i points to i - 1, a chain of n - 1 pointers, resolved in one round
        assert stats.tolist() == [1, n, 1, n // 2, 0, 0, 0, 0, 0] and not comp.any() and (class_out == 1).all()
    s = sc.spiral_scene()
    _, comp, stats, _ = standin(s)
    assert len(s["faces"]) == 4050 and stats[fs.BEFORE] == 2 and (s["classes"] == 1).sum() > 2000
    assert sorted(np.unique(comp).tolist()) == [0, int(np.nonzero(s["classes"] == 2)[0][0])]


def test_random_set_terminates_with_no_mergeable_component_left():
    """I9's termination: the cap is not hit and every small component left has no labelled edge-neighbour; at least one scene
    of the set needs two or more changing rounds."""
    rounds = []
    for s in sc.random_scenes():
        class_out, comp, stats, info = standin(s)
        assert stats[fs.ROUND_CAP] == 0 and stats[fs.ROUNDS] < 64
        assert fs.small_left_have_no_labelled_neighbour(class_out, comp, info), s["name"]
        assert stats[fs.SMALL_LEFT] == info["small"].sum() and stats[fs.AFTER] <= stats[fs.BEFORE]
        if not s["fill"]:
            assert np.array_equal(class_out < 0, s["classes"] < 0), "without filling the unlabelled faces are barriers"
        rounds.append(int(stats[fs.ROUNDS]))
    assert len(rounds) == 24 and max(rounds) >= 2 and min(rounds) >= 1


# -- the host helpers -------------------------------------------------------------------------------------------------------------------
def test_face_area_weights_known_answers():
    points = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [1e-3, 0, 0], [0, 1e-3, 0]], dtype=np.float64)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 4, 5], [0, 1, 1]])
    w = geometric.face_area_weights(points, faces)
    assert w.dtype == np.int64 and w.tolist() == [500000, 1000000, 1, 0]      # 0.5 m^2, 1 m^2, 0.5 mm^2 rounds half up, degenerate
    assert geometric.face_area_weights(points, np.zeros((0, 3), np.int32)).shape == (0,)


def test_weld_canon_known_answers():
    points = np.array([[1, 2, 3], [0, 0, 0], [1, 2, 3], [0, 0, -0.0], [1, 2, 3], [0, 0, 0]], dtype=np.float64)
    assert geometric.weld_canon(points).tolist() == [0, 1, 0, 3, 0, 1], "-0.0 differs from 0.0 in a bit"
    canon = geometric.weld_canon(points)
    assert canon.dtype == np.int32 and geometric.weld_canon(np.zeros((0, 3))).shape == (0,)
    s = next(s for s in sc.HAND if s["name"] == "seam_welded")
    seam = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    assert geometric.weld_canon(seam).tolist() == s["canon"].tolist()


# -- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def header_struct(name):
    """[(field, ctypes type)] of `typedef struct <name> { ... } <name>;` in include/geograster_components.h, read as
    tests/test_raster_warp_host.py reads its header: a field with a `*` is a pointer, every other one of the four scalar types."""
    text = (ROOT / "include" / "geograster_components.h").read_text()
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
    want = header_struct("gr_face_sieve_args")
    assert len(want) == 15
    assert [(n, t) for n, t in _hip.FaceSieveArgs._fields_] == want
    assert ctypes.sizeof(_hip.FaceSieveArgs) == 104
    assert ("stream", ctypes.c_void_p) in want


def test_header_binding_and_source_name_the_call():
    main = (ROOT / "include" / "geograster.h").read_text()
    header = (ROOT / "include" / "geograster_components.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "components.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\bint (gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", stripped))
    assert declared == {"gr_face_sieve": "gr_ctx *ctx, const gr_face_sieve_args *args_h"}
    assert _hip.COMPONENTS_SYMBOLS == tuple(declared)
    assert _hip._COMPONENTS_SIGNATURES == {"gr_face_sieve": [ctypes.c_void_p, ctypes.POINTER(_hip.FaceSieveArgs)]}
    assert not re.search(r"gr_face_sieve\b", main) and main.count('#include "geograster_components.h"') == 1
    assert main.index('#include "geograster_components.h"') > main.index('#include "geograster_warp.h"')
    flat = " ".join(header.replace(" * ", " ").split())
    assert "#define GR_VERSION 126" in main and "without a GR_VERSION bump" in flat
    assert "synchronises `stream` once per round" in flat and "never touches another stream" in flat
    assert "returns with the last kernels enqueued" in flat and "tests/test_stream_contract_components_gpu.py" in flat
    assert "F and V < 2^31 - 1, and 3 F <= 2^31 - 1" in flat
    text = Path(build.__file__).read_text()
    assert any(p.name == "components.hip" for p in build.SOURCES) and "geograster_components.h" in text
    kernels = set(re.findall(r"void (k_\w+)\(", source))
    assert {"k_sieve_keys", "k_cc_hook", "k_cc_compress", "k_measure", "k_target", "k_pointers", "k_jump", "k_relabel"} <= kernels
    assert "components.hip" in internal and all(k in internal for k in ("k_cc_hook", "k_target", "k_relabel"))
    # cub_steps.hpp remains the only file that calls hipcub
    assert "hipcub" not in source and '#include "cub_steps.hpp"' in source and "stage_acquire" in source
    names = [n for n in vars(_hip) if n.startswith("GR_SIEVE_STAT_") and n != "GR_SIEVE_STAT_WORDS"]
    assert len(names) == _hip.GR_SIEVE_STAT_WORDS == len(_hip.SIEVE_STAT_NAMES) == len(geometric.SIEVE_STAT_NAMES) == fs.STAT_WORDS
    assert _hip.SIEVE_STAT_NAMES == geometric.SIEVE_STAT_NAMES
    assert [getattr(_hip, "GR_SIEVE_STAT_" + n.upper()) for n in _hip.SIEVE_STAT_NAMES] == list(range(9))
    assert (fs.ROUNDS, fs.BEFORE, fs.AFTER, fs.CHANGED, fs.SMALL_LEFT, fs.DEGENERATE, fs.FAN_EDGES, fs.ROUND_CAP, fs.BAD_FACES) == tuple(range(9))


def test_the_library_exports_the_call_and_refuses_without_a_device():
    lib = ctypes.CDLL(str(_hip.library_path()))
    fn = lib.gr_face_sieve
    fn.restype, fn.argtypes = ctypes.c_int, _hip._COMPONENTS_SIGNATURES["gr_face_sieve"]
    assert fn(None, None) == _hip.GR_EINVAL
    assert fn(None, ctypes.byref(_hip.FaceSieveArgs())) == _hip.GR_EINVAL


# -- the argument errors ------------------------------------------------------------------------------------------------------------------
def test_weights_are_checked_on_the_host():
    check = _hip.check_sieve_arguments
    assert check(3, 5, np.array([1, 2, 3]), 7, 64) == 7 and check(0, 0, None, 0, 1) == 0
    with pytest.raises(ValueError, match="gr_face_sieve: a weight is negative"):
        check(3, 5, np.array([1, -2, 3]), 7, 64)
    with pytest.raises(ValueError, match="not below 2\\^62"):
        check(4, 6, np.array([1 << 60] * 4, dtype=np.int64), 7, 64)             # the sum is 2^62 exactly
    assert check(4, 6, np.array([1 << 60] * 3 + [(1 << 60) - 1], dtype=np.int64), 7, 64) == 7
    with pytest.raises(ValueError, match="not below 2\\^62"):
        check(3, 5, np.array([(1 << 63) - 1] * 3, dtype=np.int64), 7, 64)       # an int64 sum would wrap
    with pytest.raises(ValueError, match="weights must be"):
        check(3, 5, np.array([1.0, 2.0, 3.0]), 7, 64)
    with pytest.raises(ValueError, match="weights must be"):
        check(3, 5, np.array([1, 2]), 7, 64)
    with pytest.raises(ValueError, match="min_measure"):
        check(3, 5, None, -1, 64)
    with pytest.raises(ValueError, match="max_rounds"):
        check(3, 5, None, 1, 0)
    with pytest.raises(ValueError, match="3 F <= 2\\^31 - 1"):
        check((1 << 31) // 3 + 1, 5, None, 1, 1)


def strip_mesh(backend, n=6):
    points = np.stack([np.arange(n + 2) // 2, np.arange(n + 2) % 2, np.zeros(n + 2)], axis=1).astype(np.float64)
    return TexturedPhotogrammetryMesh((points, sc.strip_faces(n)), log_level="ERROR", backend=backend)


def test_mesh_methods_arguments_and_conventions():
    backend = StandinSieveBackend()
    mesh = strip_mesh(backend)
    labels = np.array([1, 2, 2, 3, 3, np.nan])
    for kw in (dict(), dict(min_faces=2, min_area_m2=1.0)):
        with pytest.raises(ValueError, match="exactly one of min_faces and min_area_m2"):
            mesh.sieve_face_labels(labels, **kw)
    with pytest.raises(ValueError, match="5 face labels for a mesh of 6 faces"):
        mesh.sieve_face_labels(labels[:5], min_faces=2)
    with pytest.raises(ValueError, match="whole numbers"):
        mesh.sieve_face_labels(labels + 0.5, min_faces=2)
    with pytest.raises(ValueError, match="min_area_m2"):
        mesh.sieve_face_labels(labels, min_area_m2=-1.0)
    assert not backend.calls
    # (F, 1) in, (F, 1) out, float64, NaN stays unseen; {0} (1 face) joins {1, 2}
    out = mesh.sieve_face_labels(labels.reshape(-1, 1), min_faces=2)
    assert out.shape == (6, 1) and out.dtype == np.float64 and np.array_equal(out[:, 0], [2, 2, 2, 3, 3, np.nan], equal_nan=True)
    assert mesh.last_sieve_stats["rounds"] == 1 and mesh.last_sieve_stats["faces_changed"] == 1 and backend.calls[-1]["weights"] is None
    # every face of the strip is half a square metre: 5e5 mm^2; a threshold of 0.75 m^2 is 750 000
    mesh.sieve_face_labels(labels, min_area_m2=0.75, fill_unseen=True, max_rounds=7)
    call = backend.calls[-1]
    assert call["min_measure"] == 750000 and call["weights"].tolist() == [500000] * 6 and call["fill"] is True and call["max_rounds"] == 7
    assert call["canon"] is None
    mesh.sieve_face_labels(labels, min_area_m2=1e-7 + 0.5)            # ceil(a * 1e6)
    assert backend.calls[-1]["min_measure"] == 500001
    comp, stats = mesh.face_label_components(labels, weld_vertices=True)
    assert comp.tolist() == [0, 1, 1, 3, 3, 5] and stats["components_before"] == 4 and backend.calls[-1]["canon"].tolist() == list(range(8))
    assert mesh.last_sieve_stats is stats
    same = mesh.sieve_face_labels(labels, min_faces=1)
    assert np.array_equal(same, labels, equal_nan=True)


def test_module_functions_and_the_bad_face_error():
    backend = StandinSieveBackend()
    faces = sc.strip_faces(4)
    class_out, comp, stats = geometric.sieve_face_classes(faces, np.array([1, 1, 2, -3]), None, 3, backend=backend)
    assert class_out.dtype == np.int32 and class_out.tolist() == [1, 1, 1, -1] and comp.tolist() == [0, 0, 0, 3]
    assert list(stats) == list(geometric.SIEVE_STAT_NAMES) and stats["rounds"] == 1
    comp, stats = geometric.face_components(faces, np.array([1, 1, 2, -3]), backend)
    assert comp.tolist() == [0, 0, 2, 3] and stats["components_before"] == 3 and stats["rounds"] == 0
    with pytest.raises(ValueError, match="3 face classes for 4 faces"):
        geometric.sieve_face_classes(faces, np.array([1, 1, 2]), backend=backend)
    with pytest.raises(ValueError, match="1 faces name a vertex"):
        geometric.face_components(np.array([[0, 1, 2], [1, 2, 9]]), np.array([1, 1]), backend, n_vertices=4)


# -- aggregate_images ---------------------------------------------------------------------------------------------------------------------
class RecordingBackend(OraclePictureBackend, StandinSieveBackend):
    def __init__(self):
        OraclePictureBackend.__init__(self)
        StandinSieveBackend.__init__(self)


def test_aggregate_images_plumbing(tmp_path):
    from geograypher_amd.entrypoints.aggregate_images import aggregate_images, parse_args

    args, kw, _ = aggregate_scene(tmp_path)
    for bad, message in ((dict(sieve_min_faces=3, sieve_min_area_m2=1.0), "one threshold"), (dict(sieve_fill_unseen=True), "needs a threshold")):
        with pytest.raises(ValueError, match=message):
            aggregate_images(*args, backend=RecordingBackend(), **bad, **kw)
    plain_backend = RecordingBackend()
    _, _, plain = aggregate_images(*args, backend=plain_backend, predicted_face_classes_savefile=tmp_path / "plain.npy", **kw)
    assert not plain_backend.calls, "with the defaults the sieve is not called"
    backend = RecordingBackend()
    mesh, _, sieved = aggregate_images(*args, backend=backend, predicted_face_classes_savefile=tmp_path / "sieved.npy", sieve_min_faces=40,
                                       sieve_fill_unseen=True, **kw)
    assert len(backend.calls) == 1 and backend.calls[0]["min_measure"] == 40 and backend.calls[0]["fill"] and backend.calls[0]["weights"] is None
    want = mesh.sieve_face_labels(plain, min_faces=40, fill_unseen=True)
    assert sieved.shape == plain.shape == (len(mesh.faces), 1) and np.array_equal(sieved, want, equal_nan=True)
    assert np.array_equal(np.load(tmp_path / "sieved.npy"), sieved, equal_nan=True) and mesh.last_sieve_stats["faces_changed"] > 0
    assert np.array_equal(np.load(tmp_path / "plain.npy"), plain, equal_nan=True) and not np.array_equal(plain, sieved, equal_nan=True)
    backend = RecordingBackend()
    aggregate_images(*args, backend=backend, sieve_min_area_m2=2.5, **kw)
    assert backend.calls[0]["min_measure"] == 2500000 and backend.calls[0]["weights"].dtype == np.int64 and not backend.calls[0]["fill"]
    base = ["--mesh-file", "m.npz", "--mesh-CRS", "EPSG:4978", "--cameras-file", "c.xml", "--image-folder", "i", "--label-folder", "l",
            "--IDs-to-labels", "ids.json"]
    parsed = parse_args(base)
    assert parsed.sieve_min_area_m2 is None and parsed.sieve_min_faces is None and parsed.sieve_fill_unseen is False
    parsed = parse_args(base + ["--sieve-min-area-m2", "1.5", "--sieve-min-faces", "7", "--sieve-fill-unseen"])
    assert parsed.sieve_min_area_m2 == 1.5 and parsed.sieve_min_faces == 7 and parsed.sieve_fill_unseen is True
