"""The detection and image-ID segmentors (reference: geograypher/predictors/derived_segmentors.py:54-306) against golden
label images made by the REAL reference classes (tests/golden/make_golden_tabular.py), and their rectangle tables
(`label_rectangles`, the input of the device lookup of `gr_project_rect_pairs`) against their own per-pixel images."""
from pathlib import Path

import numpy as np
import pytest

from geograypher_amd.predictors import ImageIDSegmentor, TabularRectangleSegmentor
from tests.golden.make_golden_tabular import CASES, DATA, ID_IMAGES, IMAGE_SHAPE, IMAGES, case_input

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_tabular.npz"


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def _names(case):
    return list(IMAGES) if case.startswith("cols") else ["img0", "img1", "img2"]


def _paint(rects, hw):
    img = np.full(hw, np.nan)
    for imin, jmin, imax, jmax, cls in rects.tolist():
        img[imin:imax, jmin:jmax] = cls
    return img


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("case,kw", CASES, ids=[c for c, _ in CASES])
def test_tabular_segment_image_matches_reference(case, kw, gold):
    seg = TabularRectangleSegmentor(case_input(case), IMAGE_SHAPE, **kw)
    assert seg.class_names == gold[f"{case}__class_names"].tolist()
    assert seg.num_classes == len(gold[f"{case}__class_names"])
    for name in _names(case):
        # matched by the file name alone, whatever folder the camera set keeps the image in
        got = seg.segment_image(None, Path("/elsewhere") / name, 1.0)
        _same(got, gold[f"{case}__{name}"])
        np.testing.assert_array_equal(seg.get_detection_centers(name), gold[f"{case}__centers__{name}"])
    assert (np.isnan(gold[f"{case}__{_names(case)[2]}"])).all()  # the image without detections


@pytest.mark.parametrize("case,kw", CASES, ids=[c for c, _ in CASES])
def test_tabular_rectangles_paint_segment_image(case, kw):
    seg = TabularRectangleSegmentor(case_input(case), IMAGE_SHAPE, **kw)
    for name in _names(case):
        rects, hw = seg.label_rectangles(Path("/x") / name, 1)
        assert rects.dtype == np.int32 and rects.shape[1] == 5 and hw == IMAGE_SHAPE
        # normalised: inside the image, non-empty, in paint order
        assert (rects[:, 0] >= 0).all() and (rects[:, 2] <= hw[0]).all() and (rects[:, 0] < rects[:, 2]).all()
        assert (rects[:, 1] >= 0).all() and (rects[:, 3] <= hw[1]).all() and (rects[:, 1] < rects[:, 3]).all()
        _same(_paint(rects, hw), seg.segment_image(None, Path("/x") / name, 1.0))
    assert seg.label_rectangles(Path("/x") / "img2.png", 1)[0].shape == (0, 5)


def test_tabular_scale_is_not_guessed():
    seg = TabularRectangleSegmentor(DATA / "cols", IMAGE_SHAPE, split_bbox=False)
    assert seg.label_rectangles(Path("img0.png"), 0.5) is None
    with pytest.raises(NotImplementedError):
        seg.segment_image(None, Path("img0.png"), 0.5)


@pytest.mark.parametrize("case,kw", CASES, ids=[c for c, _ in CASES])
def test_tabular_saved_table_is_the_reference_bytes(case, kw, gold, tmp_path):
    seg = TabularRectangleSegmentor(case_input(case), IMAGE_SHAPE, **kw)
    out = tmp_path / "new" / "detections.csv"
    seg.save_detection_data(out)
    assert out.read_bytes() == gold[f"{case}__saved"].tobytes()


def test_tabular_saved_table_is_what_pandas_writes(tmp_path):
    pd = pytest.importorskip("pandas")
    src = DATA / "cols"
    df = pd.concat([pd.read_csv(f) for f in sorted(src.glob("*csv"))], ignore_index=True)
    df["instance_ID"] = df.index
    df.to_csv(tmp_path / "pandas.csv")
    TabularRectangleSegmentor(src, IMAGE_SHAPE, split_bbox=False).save_detection_data(tmp_path / "ours.csv")
    assert (tmp_path / "ours.csv").read_bytes() == (tmp_path / "pandas.csv").read_bytes()


def test_tabular_absolute_paths_and_whole_table(tmp_path):
    seg = TabularRectangleSegmentor(DATA / "bbox.csv", IMAGE_SHAPE, use_absolute_filepaths=True, image_folder="/imgs")
    table = seg.get_all_detections()
    assert table.columns == ["image_path", "bbox", "label", "instance_ID"] and len(table) == 6
    assert seg.image_names == ["/imgs/img0.JPG", "/imgs/img1.JPG"]
    assert table["instance_ID"] == [100, 101, 102, 103, 104, 105]


@pytest.mark.parametrize("tag,scale", [("s100", 1.0), ("s25", 0.25)])
def test_image_id_matches_reference(tag, scale, gold):
    paths = [DATA / "images" / name for name, _ in ID_IMAGES]
    seg = ImageIDSegmentor(paths)
    for p in paths:
        want = gold[f"imageid__{p.name}__{tag}"]
        got = seg.segment_image(None, p, scale)
        assert got.dtype == want.dtype and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        rects, hw = seg.label_rectangles(p, scale)
        assert rects.dtype == np.int32 and hw == want.shape
        np.testing.assert_array_equal(_paint(rects, hw), want.astype(np.float64))


def test_image_id_unknown_or_missing_file(tmp_path):
    paths = [DATA / "images" / name for name, _ in ID_IMAGES]
    seg = ImageIDSegmentor(paths[:1])
    with pytest.raises(ValueError):
        seg.segment_image(None, paths[1], 1.0)
    with pytest.raises(FileNotFoundError):
        ImageIDSegmentor([tmp_path / "missing.png"]).segment_image(None, tmp_path / "missing.png", 1.0)
    assert seg.label_rectangles(paths[0], 0.01)[0].shape == (0, 5)  # a 0 x 0 image holds no rectangle


def test_backend_without_rectangles_takes_the_image_path(oracle_backend_cls, tmp_path):
    """A backend whose accumulator has no `add_rects` (the CPU oracle backend) aggregates the per-pixel images; the
    result is the numpy restatement of derived_meshes.py:470-550 on oracle ids."""
    from geograypher_amd.cameras import SegmentorPhotogrammetryCameraSet
    from geograypher_amd.cameras.cameras import vtk_like_near_planes
    from geograypher_amd.meshes import TexturedPhotogrammetryMeshIndexPredictions
    from geograypher_amd.utils import synthetic
    from oracle import oracle_c, oracle_np

    (points, faces), cams = synthetic.config1_scene()
    cams = cams[0:2]
    h, w = cams[0].get_image_size(1.0)
    rows = ["image_path,xmin,ymin,xmax,ymax"]
    for v in range(2):
        name = cams.get_image_filename(v).name
        rows += [f"{name},{100 + 40 * v},50,400,300", f"{name},-100,200,-20,470.5", f"{name},300.5,0,700,250"]
    (tmp_path / "det.csv").write_text("\n".join(rows) + "\n")
    seg = TabularRectangleSegmentor(tmp_path / "det.csv", (h, w), split_bbox=False)
    be = oracle_backend_cls()
    assert not hasattr(be.new_pair_accumulator(seg.num_classes, np.zeros(faces.shape[0], dtype=np.int32)), "add_rects")
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=be)
    avg, info = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(cams, seg), n_classes=seg.num_classes)
    lo, hi = points.min(axis=0), points.max(axis=0)
    nears = vtk_like_near_planes(np.stack([np.asarray(c.cam_to_world_transform, dtype=np.float64) for c in cams.cameras]),
                                 np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]))
    recs = cams.get_raster_records(1.0, near=list(nears))
    projs = [oracle_np.project_image(oracle_c.raster(points, faces, recs[v], h, w).astype(np.int64),
                                     seg.segment_image(None, cams.get_image_filename(v), 1.0).reshape(h, w, 1),
                                     faces.shape[0], check_null_image=True) for v in range(2)]
    _, counts, summed = oracle_np.aggregate_index_sparse(projs, faces.shape[0], seg.num_classes)
    np.testing.assert_array_equal(info["projection_counts"].toarray(), counts)
    np.testing.assert_array_equal(info["summed_projections"].toarray(), summed)
    assert counts.sum() > 0
