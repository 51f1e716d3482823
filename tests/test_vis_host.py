"""The picture calls without a GPU (include/geograster_vis.h): the colour tables and the numpy stand-in against the
reference's own answers (tests/golden/composites.npz, no tolerance), the two descriptor mirrors against the header field by field,
header <-> `_VIS_SIGNATURES` <-> exported symbols, and the argument rules of `utils.visualization`."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import vis_standin as vs  # noqa: E402
from geograypher_amd import _hip, build  # noqa: E402
from geograypher_amd.utils import colormaps, visualization  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "composites.npz"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def golden_case(golden, name):
    """-> (photo, label, weight, grey, IDs_to_labels, the reference's composite)"""
    ids = golden.get(f"{name}/ids")
    table = None if ids is None else {int(k): f"class {k}" for k in ids}
    return (golden[f"{name}/photo"], golden[f"{name}/label"], float(golden[f"{name}/weight"]), bool(golden[f"{name}/grey"]), table,
            golden[f"{name}/composite"])


def standin_composite(photo, label, weight, grey, table):
    """`create_composite` of the reference's signature through the stand-in alone."""
    options = visualization.get_vis_options_from_IDs_to_labels(table)
    label = np.squeeze(label) if not (label.ndim == 3 and label.shape[2] == 3) and label.ndim > 2 else label
    shift, scale = vs.composite_scalars(label, options["discrete"])
    return vs.composite(photo, label, colormaps.table(options["cmap"]), options["discrete"], shift, scale, weight, grey)


class StandinBackend:
    """The three picture methods of `HipRaster` by the stand-in, on CPU tensors."""
    device = torch.device("cpu")

    def _dev(self, array, dtype):
        if isinstance(array, torch.Tensor):
            return array.to(dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(array)).to(dtype=dtype).contiguous()

    def composite_labels(self, photo, label, table=None, discrete=False, shift=0.0, scale=1.0, weight=0.5, grey_overlay=True):
        if len(label.shape) == 3 and str(label.dtype).endswith("uint8") and discrete:
            raise ValueError("gr_composite_labels: a uint8 colour label with discrete classes is not supported")
        return torch.from_numpy(vs.composite(np.asarray(photo), np.asarray(label), table, discrete, shift, scale, weight, grey_overlay))

    def face_light(self, verts, faces, view_dir, ambient=0.3):
        return torch.from_numpy(vs.face_light(np.asarray(verts), np.asarray(faces), view_dir, ambient))

    def shade_view(self, ids, depth, face_rgb, face_light, supersample=1, radius=None, strength=0.0, background=(255, 255, 255)):
        radius = supersample if radius is None else radius
        return torch.from_numpy(vs.shade_view(np.asarray(ids), np.asarray(depth), np.asarray(face_rgb), np.asarray(face_light),
                                              supersample, radius, strength, background))


# -- the colour tables and the stand-in against the reference ----------------------------------------------------------------------
def test_colour_tables_equal_matplotlibs_bit_for_bit(golden):
    for name, rows in (("tab10", 10), ("tab20", 20), ("viridis", 256)):
        table = colormaps.table(name)
        assert table.shape == (rows, 3) and table.dtype == np.float64
        assert np.array_equal(table.view(np.uint64), golden[f"tables/{name}"].view(np.uint64)), name
    assert colormaps.table("tab10")[0].tolist() == [31 / 255, 119 / 255, 180 / 255]
    with pytest.raises(ValueError, match="no colour table"):
        colormaps.table("jet")
    for module in ("colormaps.py", "visualization.py"):   # matplotlib is needed neither at run nor at test time
        assert not re.search(r"^\s*(import|from) matplotlib", (ROOT / "geograypher_amd" / "utils" / module).read_text(), re.M)


def test_the_golden_file_holds_the_cases_the_rules_need(golden):
    names = [str(n) for n in golden["cases"]]
    assert len(names) >= 12 and all(golden[f"{n}/photo"].shape[0] <= 16 and golden[f"{n}/photo"].shape[1] <= 24 for n in names)
    lab4, lab15 = golden["discrete4_u8/label"], golden["discrete15_u8/label"]
    assert lab4.dtype == np.uint8 and {0, 11, 255} <= set(lab4.ravel().tolist()) and {0, 20, 255} <= set(lab15.ravel().tolist())
    cont = golden["continuous_nan_zero_negative/label"]
    assert np.isnan(cont).any() and (cont == 0).any() and (cont < 0).any() and np.isinf(cont).any()
    assert golden["continuous_u8/label"].dtype == np.uint8 and golden["rgb_float_label/label"].shape[2] == 3
    assert {float(golden[f"{n}/weight"]) for n in names} >= {0.0, 0.5, 1.0}
    assert {bool(golden[f"{n}/grey"]) for n in names} == {True, False}
    assert {golden[f"{n}/photo"].dtype for n in names} == {np.dtype(np.uint8), np.dtype(np.float64)}


def test_the_standin_equals_every_golden_byte(golden):
    for name in (str(n) for n in golden["cases"]):
        photo, label, weight, grey, table, want = golden_case(golden, name)
        got = standin_composite(photo, label, weight, grey, table)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def test_the_rules_the_reference_was_run_for(golden):
    """Label 11 on tab10 takes colour 9, label 0 is black, and the last step truncates."""
    photo, label, weight, grey, table, want = golden_case(golden, "discrete4_u8")
    w = photo.shape[1]
    at = tuple(np.argwhere(label == 11)[0])
    tab10 = colormaps.table("tab10")
    assert want[at[0], at[1]].tolist() == [int(v * 255) for v in tab10[9]]
    zero = tuple(np.argwhere(label == 0)[0])
    assert want[zero[0], zero[1]].tolist() == [0, 0, 0]
    # a byte of the photo survives / 255 x 255 truncated, all 256 of them; a float photo shows that the last step truncates
    assert np.array_equal(want[:, w:2 * w], photo) and photo[0, 2].tolist() == [31, 119, 180]
    photo, _, _, _, _, want = golden_case(golden, "discrete4_float_photo")
    assert np.array_equal(want[:, w:2 * w], (photo * 255).astype(np.uint8))
    assert (want[:, w:2 * w] != np.round(photo * 255).astype(np.uint8)).any()


def test_create_composite_through_a_backend_and_its_refusals(golden):
    backend = StandinBackend()
    for name in ("discrete15_u8", "continuous_nan_zero_negative", "continuous_u8", "rgb_float_label", "continuous_positive_float_photo"):
        photo, label, weight, grey, table, want = golden_case(golden, name)
        got = visualization.create_composite(photo, label, weight, table, grey, backend=backend)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want), name
        as_tensor = visualization.create_composite(torch.from_numpy(photo), label[..., None] if label.ndim == 2 else label, weight, table,
                                                   grey, backend=backend)
        assert isinstance(as_tensor, torch.Tensor) and np.array_equal(as_tensor.numpy(), want), name
    photo = golden["rgb_u8_label/photo"]
    with pytest.raises(ValueError, match="uint8 colour label with discrete"):
        visualization.create_composite(photo, golden["rgb_u8_label/label"], IDs_to_labels={0: "a", 1: "b"}, backend=backend)
    with pytest.raises(ValueError, match="Invalid RGB"):
        visualization.create_composite(photo[..., 0], photo[..., 0], backend=backend)
    with pytest.raises(ValueError, match="label_image must be"):
        visualization.create_composite(photo, np.zeros((2, 3, 4, 5)), backend=backend)


def test_composite_scalars_with_torch_equal_the_standins():
    rng = np.random.default_rng(3)
    labels = [rng.normal(size=(5, 7)), rng.integers(0, 256, (5, 7), dtype=np.uint8), np.zeros((3, 3)), np.full((2, 2), np.nan),
              np.array([[0.0, -2.0], [np.inf, 5.0]]), np.zeros((2, 2), dtype=np.uint8), np.array([[0.0, -np.inf], [1.0, 2.0]])]
    labels[0][0, :3] = (np.nan, 0.0, np.inf)
    for label in labels:
        want = vs.composite_scalars(label, False)
        got = visualization.composite_scalars(torch.from_numpy(label), False)
        assert np.array_equal(np.array(got).view(np.uint64), np.array(want).view(np.uint64)), (label, got, want)
    assert visualization.composite_scalars(torch.zeros((2, 2)), True) == (0.0, 1.0)


def test_vis_options_mirror_the_reference():
    options = visualization.get_vis_options_from_IDs_to_labels
    assert options(None) == {"cmap": "viridis", "vmin": None, "vmax": None, "discrete": False}
    assert options({0: "a", 9: "b"}) == {"cmap": "tab10", "vmin": -0.5, "vmax": 9.5, "discrete": True}
    assert options({10: "a"}) == {"cmap": "tab20", "vmin": -0.5, "vmax": 19.5, "discrete": True}
    assert options({19: "a"})["cmap"] == "tab20" and options({20: "a"}) == {"cmap": "viridis", "vmin": None, "vmax": None, "discrete": False}


def test_show_segmentation_labels_sorted_seeded_and_without_a_window(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(5)
    labels, images, saved = tmp_path / "labels", tmp_path / "images", tmp_path / "saved"
    (labels / "sub").mkdir(parents=True)
    (images / "sub").mkdir(parents=True)
    photos, renders = {}, {}
    for k, (stem, suffix) in enumerate((("b", ".png"), ("sub/a", ".png"), ("c", ".npy"), ("d", ".tif"))):
        photos[stem] = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
        renders[stem] = rng.integers(0, 4, (6, 9), dtype=np.uint8)
        Image.fromarray(photos[stem]).save(images / f"{stem}.png")
        if suffix == ".npy":
            np.save(labels / f"{stem}.npy", renders[stem])
        else:
            Image.fromarray(renders[stem]).save(labels / f"{stem}{suffix}")
    (labels / "IDs_to_labels.json").write_text('{"0": "a", "1": "b", "2": "c", "3": "d"}')
    backend = StandinBackend()
    with pytest.raises(NotImplementedError, match="no window"):
        visualization.show_segmentation_labels(labels, images, backend=backend)
    written = visualization.show_segmentation_labels(labels, images, saved, image_suffix=".png", backend=backend)
    assert [p.name for p in written] == ["rendered_label_000.png", "rendered_label_001.png"]
    table = {k: "x" for k in range(4)}
    for path, stem in zip(written, ("b", "sub/a")):   # sorted order
        assert np.array_equal(np.asarray(Image.open(path)), standin_composite(photos[stem], renders[stem], 0.5, True, table))
    for suffix, stem in ((".npy", "c"), (".tif", "d")):
        (one,) = visualization.show_segmentation_labels(labels, images, saved / suffix[1:], label_suffix=suffix, image_suffix=".png",
                                                        backend=backend)
        assert np.array_equal(np.asarray(Image.open(one)), standin_composite(photos[stem], renders[stem], 0.5, True, table))
    first = visualization.show_segmentation_labels(labels, images, saved / "s1", num_show=1, image_suffix=".png", seed=1, backend=backend)
    again = visualization.show_segmentation_labels(labels, images, saved / "s2", num_show=1, image_suffix=".png", seed=1, backend=backend)
    assert np.array_equal(np.asarray(Image.open(first[0])), np.asarray(Image.open(again[0])))


# -- the stand-in of the shaded view on hand-worked planes ------------------------------------------------------------------------
def test_face_light_hand_worked():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 3, 4]], dtype=np.float32)
    faces = np.array([[0, 1, 2],     # in the plane z = 0: faces the view (0, 0, -1) head on
                      [0, 2, 1],     # the same from behind: two-sided
                      [0, 1, 3],     # in the plane y = 0: edge-on to (0, 0, -1)
                      [0, 1, 4],     # three points of a line: no area
                      [0, 1, 5],     # normal (0, -4, 3): |n.d| / |n| = 3 / 5
                      [0, 1, 9]])    # a vertex that does not exist
    light = vs.face_light(verts, faces, (0.0, 0.0, -1.0), 0.25)
    assert light.tolist() == [255, 255, 64, 255, int(np.floor((0.25 + 0.75 * 0.6) * 255 + 0.5)), 255]
    assert vs.face_light(verts, faces[:3], (0.0, 0.0, -1.0), 0.0).tolist() == [255, 255, 0]
    assert vs.face_light(verts, faces[:3], (0.0, 0.0, -1.0), 1.0).tolist() == [255, 255, 255]


def test_shade_standin_hand_worked():
    rgb = np.array([[200, 100, 50], [10, 20, 30]], dtype=np.uint8)
    light = np.array([255, 0], dtype=np.uint8)
    ids = np.array([[0, -1], [1, 0]], dtype=np.int32)
    depth = np.array([[2.0, np.inf], [1.0, 2.0]], dtype=np.float32)
    flat = vs.shade_view(ids, depth, rgb, light, 1, 1, 0.0)
    assert flat.tolist() == [[[200, 100, 50], [255, 255, 255]], [[0, 0, 0], [200, 100, 50]]]
    # one closer neighbour at half the depth: sum = (2 - 1) / 2, occl = 1 / (1 + 2 * 0.5) = 0.5; the far corner sees it diagonally too
    dark = vs.shade_view(ids, depth, rgb, light, 1, 1, 2.0)
    assert dark[0, 0].tolist() == [100, 50, 25] and dark[1, 1].tolist() == [100, 50, 25] and dark[0, 1].tolist() == [255, 255, 255]
    # 2 x 2 samples a pixel: the mean of face, background, black face, face -> (200 + 255 + 0 + 200) / 4 + 0.5 floored
    assert vs.shade_view(ids, depth, rgb, light, 2, 2, 0.0).tolist() == [[[164, 114, 89]]]
    # an id beyond the table is background
    assert vs.shade_view(np.array([[2]], dtype=np.int32), np.ones((1, 1), np.float32), rgb, light, 1, 1, 1.0, (1, 2, 3)).tolist() == [[[1, 2, 3]]]


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}


def header_struct(name):
    """[(field, ctypes type)] of `typedef struct <name> { ... } <name>;` in include/geograster_vis.h: a field with a `*` is a
    pointer, every other one of the four scalar types."""
    text = (ROOT / "include" / "geograster_vis.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for statement in filter(None, (s.strip() for s in body.split(";"))):
        pointer = re.fullmatch(r"(?:const\s+)?\w+\s*\*\s*(\w+)", statement)
        scalar = re.fullmatch(r"(int64_t|int32_t|float|double)\s+(\w+)", statement)
        assert pointer or scalar, statement
        fields.append((pointer.group(1), ctypes.c_void_p) if pointer else (scalar.group(2), C_TYPES[scalar.group(1)]))
    return fields


@pytest.mark.parametrize("struct,mirror,n_fields,size", [("gr_shade_args", _hip.ShadeArgs, 22, 144),
                                                         ("gr_composite_args", _hip.CompositeArgs, 16, 96)])
def test_descriptor_mirrors_equal_the_header_field_by_field(struct, mirror, n_fields, size):
    """The library READS these structures through the caller's pointer: a mirror with a field missing, moved or of another width
    hands it other values than the caller set."""
    want = header_struct(struct)
    assert len(want) == n_fields
    assert [(n, t) for n, t in mirror._fields_] == want
    assert ctypes.sizeof(mirror) == size
    assert ("stream", ctypes.c_void_p) in want


def test_header_binding_and_source_name_the_two_calls():
    main = (ROOT / "include" / "geograster.h").read_text()
    header = (ROOT / "include" / "geograster_vis.h").read_text()
    source = (ROOT / "geograypher_amd" / "csrc" / "vis.hip").read_text()
    internal = (ROOT / "geograypher_amd" / "csrc" / "gr_internal.hpp").read_text()
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\bint (gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", stripped))
    assert declared == {"gr_shade_view": "gr_ctx *ctx, const gr_shade_args *args_h",
                        "gr_composite_labels": "gr_ctx *ctx, const gr_composite_args *args_h"}
    assert _hip.VIS_SYMBOLS == tuple(declared)
    assert _hip._VIS_SIGNATURES == {"gr_shade_view": [ctypes.c_void_p, ctypes.POINTER(_hip.ShadeArgs)],
                                    "gr_composite_labels": [ctypes.c_void_p, ctypes.POINTER(_hip.CompositeArgs)]}
    assert not re.search(r"gr_shade|gr_composite", main) and main.count('#include "geograster_vis.h"') == 1
    assert main.index('#include "geograster_vis.h"') > main.index('#include "geograster_nadir.h"')
    assert "#define GR_VERSION 126" in main and "without a GR_VERSION bump" in " ".join(header.replace(" * ", " ").split())
    flat = " ".join(header.replace(" * ", " ").split())
    assert "NOT exempt from the stream contract" in flat and "tests/test_stream_contract_vis_gpu.py" in flat
    assert any(p.name == "vis.hip" for p in build.SOURCES) and "geograster_vis.h" in Path(build.__file__).read_text()
    kernels = set(re.findall(r"void (k_\w+)\(", source))
    assert kernels == {"k_face_light", "k_shade", "k_composite"} and all(k in internal for k in kernels)
    for name, value in (("SHADE_MAX_S", _hip.SHADE_MAX_SUPERSAMPLE), ("SHADE_MAX_R", _hip.SHADE_MAX_RADIUS),
                        ("SHADE_MAX_SIDE", _hip.SHADE_MAX_SIDE)):
        assert re.search(rf"\b{name} = {value}\b", source), name
    assert not re.search(r"\b(exp|log|pow)[a-z0-9]*\(", re.sub(r"//[^\n]*", "", source))   # + - x / and comparisons only


def test_the_library_exports_both_calls_and_refuses_without_a_device():
    lib = ctypes.CDLL(str(_hip.library_path()))
    for name, argtypes in _hip._VIS_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, argtypes
        assert fn(None, None) == _hip.GR_EINVAL
    assert lib.gr_shade_view(None, ctypes.byref(_hip.ShadeArgs())) == _hip.GR_EINVAL
    assert lib.gr_composite_labels(None, ctypes.byref(_hip.CompositeArgs())) == _hip.GR_EINVAL
