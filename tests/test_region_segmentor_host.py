"""`RegionDetectionSegmentor` on the host: the reference's known answers (tests/test_derived_segmentors.py there, restated with
.geojson files written here), the fill rule against masks of the real `skimage.draw.polygon`
(tests/golden/reference_draw_polygon.npz), the ring tables handed to the device, and the key bound of `add_polygons`."""
import json

import numpy as np
import pytest

from geograypher_amd import _hip
from geograypher_amd.cameras import SegmentorPhotogrammetryCameraSet
from geograypher_amd.predictors import RegionDetectionSegmentor
from geograypher_amd.predictors.derived_segmentors import _ring_box, _ring_contains
from geograypher_amd.utils import synthetic

GOLDEN = __import__("pathlib").Path(__file__).resolve().parent / "golden" / "reference_draw_polygon.npz"


def _write_geojson(path, polygons, multi_polygons=None, labels=None, extra=()):
    geoms = [{"type": "Polygon", "coordinates": [[list(p) for p in poly]]} for poly in polygons]
    if multi_polygons is not None:
        geoms.append({"type": "MultiPolygon", "coordinates": [[[list(p) for p in poly]] for poly in multi_polygons]})
    geoms.extend(extra)
    if labels is None:
        labels = [0] * len(geoms)
    feats = [{"type": "Feature", "geometry": g, "properties": {"unique_ID": f"{i:05}", "labels": labels[i], "score": 0.5}}
             for i, g in enumerate(geoms)]
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps({"type": "FeatureCollection", "features": feats}))


SQUARES = [
    [(0, 50), (0, 60), (10, 60), (10, 50), (0, 50)],
    [(20, 20), (20, 30), (30, 30), (30, 20), (20, 20)],
    [(100, 50), (100, 60), (110, 60), (110, 50), (100, 50)],
]
POLYGONS = [
    [(0, 0), (0, 10), (10, 10), (10, 0), (0, 0)],
    [(20, 20), (20, 30), (30, 30), (30, 20), (20, 20)],
    [(25, 20), (25, 30), (35, 30), (35, 20), (25, 20)],  # overlaps the second
]
MULTI = [
    [(0, 20), (0, 30), (10, 30), (10, 20), (0, 20)],
    [(0, 26), (0, 36), (10, 36), (10, 26), (0, 26)],
]
CLASS_MAP = {"FIG": 0, "PEAR": 1, "APPLE": 2}


@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("im_extension", (".jpg", ".JPG", ".png", ".tif"))
def test_detection_centers(tmp_path, flat, im_extension):
    if flat:
        base_folder = lookup_folder = im_nested = geo_nested = tmp_path
    else:
        base_folder, lookup_folder = tmp_path / "images", tmp_path / "geospatial"
        im_nested, geo_nested = base_folder / "mission" / "00", lookup_folder / "mission" / "00"
        geo_nested.mkdir(parents=True)
    im_paths = []
    for i in range(3):
        im_paths.append(im_nested / f"test_{i}{im_extension}")
        _write_geojson(geo_nested / f"test_{i}.geojson", SQUARES)
    seg = RegionDetectionSegmentor(base_folder, lookup_folder, label_key=None, class_map=None, geo_file_extension=".geojson")
    for im_path in im_paths:
        centers = seg.get_detection_centers(im_path)
        assert centers.shape == (3, 2) and centers.dtype == np.float64
        np.testing.assert_allclose(centers, [[55, 5], [25, 25], [55, 105]])  # (centroid.y, centroid.x)


def test_centers_holes_multipolygons_and_other_geometries(tmp_path):
    # a 10 x 10 square with the 4 x 4 hole [0, 4]^2: area 84, centroid ((500 - 32) / 84,) * 2
    holed = {"type": "Polygon", "coordinates": [[[0, 0], [10, 0], [10, 10], [0, 10], [0, 0]],
                                                [[0, 0], [0, 4], [4, 4], [4, 0], [0, 0]]]}
    # areas 4 and 12: centroid x = (4 * 1 + 12 * 13) / 16, y = (4 * 1 + 12 * 1) / 16
    multi = {"type": "MultiPolygon", "coordinates": [[[[0, 0], [2, 0], [2, 2], [0, 2], [0, 0]]],
                                                     [[[10, 0], [16, 0], [16, 2], [10, 2], [10, 0]]]]}
    _write_geojson(tmp_path / "a.geojson", [], extra=[holed, multi])
    seg = RegionDetectionSegmentor(tmp_path, tmp_path, None, None, ".geojson")
    c = (500 - 32) / 84
    np.testing.assert_allclose(seg.get_detection_centers(tmp_path / "a.png"), [[c, c], [1.0, 10.0]])
    _write_geojson(tmp_path / "b.geojson", SQUARES[:1], extra=[{"type": "Point", "coordinates": [1, 2]}])
    with pytest.raises(NotImplementedError):
        seg.get_detection_centers(tmp_path / "b.png")


def test_missing_file_and_unsupported_extension(tmp_path):
    seg = RegionDetectionSegmentor(tmp_path, tmp_path, "labels", CLASS_MAP, geo_file_extension=".gpkg")
    assert seg.get_detection_centers(str(tmp_path / "nonexistent.JPG")).shape == (0, 2)
    assert seg.segment_image(None, tmp_path / "nonexistent.JPG", (7, 9)).shape == (7, 9, 0)  # the reference's answer
    (tmp_path / "there.gpkg").write_bytes(b"not read")
    with pytest.raises(NotImplementedError, match="geopandas"):
        seg.get_detection_centers(tmp_path / "there.JPG")
    with pytest.raises(NotImplementedError, match="geopandas"):
        seg.segment_image(None, tmp_path / "there.JPG", (7, 9))
    with pytest.raises(ValueError, match="not found"):
        RegionDetectionSegmentor(tmp_path, tmp_path / "no_such_folder", "labels", CLASS_MAP)
    # the camera-set convention: one channel count for every view, an empty ring table
    seg = RegionDetectionSegmentor(tmp_path, tmp_path, "labels", CLASS_MAP, ".geojson", image_shape=(7, 9))
    mask = seg.segment_image(None, filename=tmp_path / "nonexistent.JPG", image_scale=1)
    assert mask.shape == (7, 9, 3) and mask.dtype == bool and not mask.any()
    (boxes, vert_offsets, verts), hw = seg.label_regions(tmp_path / "nonexistent.JPG")
    assert boxes.shape == (0, 5) and vert_offsets.tolist() == [0] and verts.shape == (0, 2) and hw == (7, 9)


@pytest.mark.parametrize("imshape", [(40, 40), (60, 40), (100, 120)])
@pytest.mark.parametrize("xy_order", ["reference", "image"])
def test_segment_image_known_answers(tmp_path, imshape, xy_order):
    _write_geojson(tmp_path / "test.geojson", POLYGONS, MULTI, labels=["APPLE", "APPLE", "PEAR", "FIG"])
    seg = RegionDetectionSegmentor(tmp_path, tmp_path, "labels", CLASS_MAP, ".geojson", xy_order=xy_order)
    assert seg.num_classes == 3
    shape = imshape if xy_order == "reference" else imshape[::-1]
    mask = seg.segment_image(image=None, im_path=tmp_path / "test.JPG", image_shape=shape)
    assert mask.shape == shape + (3,) and mask.dtype == bool
    if xy_order == "image":  # row = y, column = x: the reference's mask transposed
        mask = mask.transpose(1, 0, 2)
    assert mask[..., 0].sum() == 187
    assert mask[..., 1].sum() == 121
    assert mask[..., 2].sum() == 121 + 121
    assert np.allclose(np.average(np.where(mask[..., 0]), axis=1), [5, 28])
    assert np.allclose(np.average(np.where(mask[..., 1]), axis=1), [30, 25])
    assert np.allclose(np.average(np.where(mask[..., 2]), axis=1), [15, 15])


@pytest.mark.parametrize(
    "label_key,class_map,expected_str",
    (
        ["nonexistent", None, "not found in GDF columns"],
        ["labels", {"BETA": 0}, "keys in a GDF which were not in the class map"],
        ["labels", {"ALPHA": 1.5}, "not integer indices"],
        ["labels", {"ALPHA": "BETA"}, "not integer indices"],
    ),
)
def test_segment_image_errors(tmp_path, label_key, class_map, expected_str):
    _write_geojson(tmp_path / "test.geojson", POLYGONS[:1], labels=["ALPHA"])
    seg = RegionDetectionSegmentor(tmp_path, tmp_path, label_key, class_map, ".geojson")
    with pytest.raises(ValueError) as ve:
        seg.segment_image(image=None, im_path=tmp_path / "test.JPG", image_shape=(100, 100))
    assert expected_str in str(ve.value)


def _golden_rings():
    with np.load(GOLDEN, allow_pickle=False) as g:
        names, shapes, offsets, verts, masks = (g[k] for k in ("names", "shapes", "offsets", "verts", "masks"))
    pos = 0
    for k, name in enumerate(names):
        h, w = (int(x) for x in shapes[k])
        yield str(name), (h, w), verts[offsets[k]:offsets[k + 1]], masks[pos:pos + h * w].reshape(h, w)
        pos += h * w


def _paint(rows, cols, h, w):
    out = np.zeros((h, w), dtype=bool)
    box = _ring_box(rows, cols, h, w)
    if box is not None:
        out[box[0]:box[2], box[1]:box[3]] = _ring_contains(rows, cols, box)
    return out


def test_fill_rule_equals_skimage_goldens():
    """Every pixel of every golden mask: the whole (h, w) image is compared, so a pixel outside the candidate box counts too."""
    seen = 0
    for name, (h, w), verts, want in _golden_rings():
        got = _paint(verts[:, 0], verts[:, 1], h, w)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        seen += 1
    assert seen >= 40


def test_half_open_rule_is_not_the_rule():
    """The pre-0.19 half-open rule would fill 100 pixels of the reference test's 10 x 10 squares; the rule here fills 121."""
    v = np.array(POLYGONS[1], dtype=np.float64)
    assert _paint(v[:, 0], v[:, 1], 40, 40).sum() == 121


def test_label_regions_repaint_equals_segment_image(tmp_path):
    polys = POLYGONS + [[(3.5, 4.25), (30.75, 8.5), (12.0, 33.3)],          # a fractional triangle
                        [(200, 200), (200, 210), (210, 210), (210, 200)],   # off the image: dropped
                        [(30, 30), (30, 70), (55, 70), (55, 30)]]           # over the image's edge: clipped box
    labels = ["APPLE", "FIG", "PEAR", "FIG", "APPLE", "PEAR"] + ["PEAR"] + ["FIG"]  # polygons, multipolygon, line
    _write_geojson(tmp_path / "v.geojson", polys, MULTI, labels=labels,
                   extra=[{"type": "LineString", "coordinates": [[0, 0], [5, 5]]}])
    for xy_order in ("reference", "image"):
        seg = RegionDetectionSegmentor(tmp_path, tmp_path, "labels", CLASS_MAP, ".geojson", image_shape=(48, 52),
                                       xy_order=xy_order)
        want = seg.segment_image(None, filename=tmp_path / "v.png", image_scale=1)
        assert want.shape == (48, 52, 3) and want.any(axis=(0, 1)).all()
        (boxes, vert_offsets, verts), hw = seg.label_regions(tmp_path / "v.png")
        assert hw == (48, 52)
        assert boxes.dtype == np.int32 and vert_offsets.dtype == np.int32 and verts.dtype == np.float64
        assert boxes.shape == (7, 5)  # 6 polygons + 2 parts - 1 off the image; the line string is skipped
        assert vert_offsets.shape == (8,) and vert_offsets[0] == 0 and vert_offsets[-1] == verts.shape[0]
        assert np.all(np.diff(boxes[:, 4]) >= 0)                          # class-sorted runs
        assert boxes[:, :2].min() >= 0 and boxes[:, 2].max() <= 48 and boxes[:, 3].max() <= 52
        assert np.all(boxes[:, 2] > boxes[:, 0]) and np.all(boxes[:, 3] > boxes[:, 1])
        got = np.zeros_like(want)
        for r, (i0, j0, i1, j1, cls) in enumerate(boxes.tolist()):
            ring = verts[vert_offsets[r]:vert_offsets[r + 1]]
            assert _ring_box(ring[:, 0], ring[:, 1], 48, 52) == (i0, j0, i1, j1)
            got[i0:i1, j0:j1, cls] |= _ring_contains(ring[:, 0], ring[:, 1], (i0, j0, i1, j1))
        assert np.array_equal(got, want)
        assert seg.label_regions(tmp_path / "v.png", image_scale=0.5) is None
        with pytest.raises(NotImplementedError):
            seg.segment_image(None, filename=tmp_path / "v.png", image_scale=0.5)


def test_camera_set_forwards_regions_and_reads_the_header(tmp_path):
    from PIL import Image

    cams = synthetic.make_simple_camera_set()
    for v, cam in enumerate(cams.cameras):
        cam.image_filename = tmp_path / "images" / f"view_{v}.png"
    (tmp_path / "images").mkdir()
    Image.fromarray(np.zeros((40, 60), dtype=np.uint8)).save(cams.cameras[0].image_filename)
    _write_geojson(tmp_path / "geo" / "view_0.geojson", POLYGONS, labels=["APPLE", "APPLE", "PEAR"])
    seg = RegionDetectionSegmentor(tmp_path / "images", tmp_path / "geo", "labels", CLASS_MAP, ".geojson")
    cs = SegmentorPhotogrammetryCameraSet(cams, seg)
    assert cs.n_image_channels() == 3
    (boxes, _, _), hw = cs.get_label_regions(0)
    assert hw == (40, 60) and boxes[:, 4].tolist() == [1, 2, 2]
    assert cs.get_image_by_index(0).shape == (40, 60, 3)
    assert cs.get_label_regions(0, image_scale=0.5) is None


def test_key_bound_arithmetic():
    """min(F * classes of the view, sum over rings of min(F, box area)) per view, on plain numbers."""
    boxes = np.array([[0, 0, 10, 10, 0],      # view 0: areas 100, 100, 4 in two classes
                      [5, 5, 15, 15, 0],
                      [0, 0, 2, 2, 3],
                      [0, 0, 100, 100, 7],    # view 2 (view 1 is empty): one huge ring
                      [0, 0, 3, 1, 1], [0, 0, 3, 1, 2], [0, 0, 3, 1, 4]])  # view 3: three classes, 3 pixels each
    offs = [0, 3, 3, 4, 7]
    assert _hip.polygon_pair_bounds(boxes, offs, 1000).tolist() == [204, 0, 1000, 9]
    assert _hip.polygon_pair_bounds(boxes, offs, 50).tolist() == [100, 0, 50, 9]   # F * 2; min(F, area); areas
    assert _hip.polygon_pair_bounds(boxes, offs, 2).tolist() == [4, 0, 2, 6]
    assert _hip.polygon_pair_bounds(np.zeros((0, 5)), [0, 0], 10).tolist() == [0]
    assert "gr_project_polygon_pairs" in _hip.EXPORTED_SYMBOLS
