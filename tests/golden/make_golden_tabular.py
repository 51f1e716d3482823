"""tests/golden/make_golden_tabular.py -- golden label images of the detection and image-ID segmentors, made by the REAL
reference classes (geograypher/predictors/derived_segmentors.py:54-306) with pandas and PIL; the modules the reference
imports but these two classes never call (geopandas, scikit-image, imageio, pyproj, ...) are stubbed as in SURVEY.md
Appendix B:

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_tabular.py

Inputs (written here, committed beside the output, read by tests/test_detection_segmentors.py):
  tabular/cols/a.csv, b.csv   four-column boxes (xmin, ymin, xmax, ymax): no instance_ID column, integer corners in
                              one file and fractional ones in the other (the concatenated columns become float64), negative corners (they wrap), corners beyond the image (they clamp), boxes that
                              overlap (paint order decides), a string `species` and an integer `label_int` column
  tabular/bbox.csv            "[x, y, w, h]" strings (split_bbox), an explicit instance_ID, image names with an extension
                              that strip_image_extension removes
  tabular/images/*.png        small images for the ImageID segmentor

Output: tests/golden/reference_tabular.npz
  <case>__<image>            segment_image(None, Path(<image>), 1.0) of each tabular case (float64, NaN background)
  <case>__class_names        class_names;  <case>__saved: the bytes save_detection_data writes (uint8)
  imageid__<image>__sXX      ImageIDSegmentor(list of the image paths).segment_image(..., s) for s = 1 and 0.25
  <case>__centers__<image>   get_detection_centers(<image name as in the table>)
"""
import importlib.abc
import importlib.machinery
import sys
import tempfile
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

HERE = Path(__file__).resolve().parent
DATA = HERE / "tabular"
OUT = HERE / "reference_tabular.npz"
IMAGE_SHAPE = (40, 60)
IMAGES = ("img0.png", "img1.png", "img2.png")  # img2 has no detections
ID_IMAGES = (("id_a.png", (23, 37)), ("id_b.png", (48, 64)))  # (h, w)

# (case, constructor keywords besides the detection path and image_shape)
CASES = (
    ("cols_instance", dict(split_bbox=False)),
    ("cols_species", dict(split_bbox=False, label_key="species")),
    ("cols_int", dict(split_bbox=False, label_key="label_int")),
    ("bbox", dict(split_bbox=True, label_key="instance_ID", strip_image_extension=True)),
    ("bbox_label", dict(split_bbox=True, label_key="label", strip_image_extension=True)),
)

A_CSV = """image_path,xmin,ymin,xmax,ymax,species,label_int,score
img0.png,5,4,30,20,pine,3,0.9
img0.png,20,10,45,35,oak,7,0.5
img0.png,-10,-8,-2,-1,fir,3,0.25
img0.png,50,30,90,70,pine,1,1.0
img1.png,0,0,60,40,oak,7,0.75
img1.png,10,5,20,15,"fir, grand",-4,0.125
"""
B_CSV = """image_path,xmin,ymin,xmax,ymax,species,label_int,score
img1.png,15,12,25,30,pine,3,
img0.png,25.7,18,28.2,22.9,fir,1,0.3
img0.png,-2.5,-9.99,61,50,oak,3,0.6
img0.png,12,30,12,35,oak,7,0.6
"""
# the split_bbox form carries fractional corners (float() then int() truncates toward zero)
BBOX_CSV = """image_path,bbox,label,instance_ID
img0.JPG,"[10.5, 3.2, 20, 15.9]",2,100
img0.JPG,"[7.9, 12.7, 30.2, 8]",0,101
img1.JPG,"[55.5, 35.5, 10, 10]",2,102
img0.JPG,"[12, 2, 3.5, 40]",5,103
img1.JPG,"[-5.5, 0.9, 3, 0.5]",0,104
img0.JPG,"[-20, -3.2, 9.5, 2.1]",0,105
"""


def write_inputs():
    from PIL import Image

    (DATA / "cols").mkdir(parents=True, exist_ok=True)
    (DATA / "images").mkdir(parents=True, exist_ok=True)
    (DATA / "cols" / "a.csv").write_text(A_CSV)
    (DATA / "cols" / "b.csv").write_text(B_CSV)
    (DATA / "bbox.csv").write_text(BBOX_CSV)
    for name, (h, w) in ID_IMAGES:
        Image.fromarray(np.full((h, w), 128, dtype=np.uint8)).save(DATA / "images" / name)


def case_input(case):
    return DATA / "bbox.csv" if case.startswith("bbox") else DATA / "cols"


def stub_missing_modules():
    missing = ("fiona", "geopandas", "pyproj", "pyvista", "rasterio", "shapely", "skimage", "ubelt", "imageio", "piexif",
               "trimesh", "rtree", "rasterstats", "setcoverpy", "chardet", "cchardet", "IPython")

    class Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        def find_spec(self, name, path, target=None):
            if name.split(".")[0] in missing:
                return importlib.machinery.ModuleSpec(name, self, is_package=True)

        def create_module(self, spec):
            m = MagicMock()
            m.__path__ = []
            m.__spec__ = spec
            m.__name__ = spec.name
            return m

        def exec_module(self, module):
            pass

    sys.meta_path.insert(0, Finder())


def main():
    write_inputs()
    stub_missing_modules()
    from geograypher.predictors.derived_segmentors import ImageIDSegmentor, TabularRectangleSegmentor

    out = {}
    for case, kw in CASES:
        seg = TabularRectangleSegmentor(case_input(case), IMAGE_SHAPE, **kw)
        names = list(IMAGES) if case.startswith("cols") else ["img0", "img1", "img2"]
        for name in names:
            out[f"{case}__{name}"] = seg.segment_image(None, Path("/data/images") / name, 1.0)
            out[f"{case}__centers__{name}"] = np.asarray(seg.get_detection_centers(name), dtype=np.float64)
        out[f"{case}__class_names"] = np.array(seg.class_names)
        with tempfile.TemporaryDirectory() as tmp:
            seg.save_detection_data(Path(tmp) / "sub" / "saved.csv")
            out[f"{case}__saved"] = np.frombuffer((Path(tmp) / "sub" / "saved.csv").read_bytes(), dtype=np.uint8)
    paths = [DATA / "images" / name for name, _ in ID_IMAGES]
    ids = ImageIDSegmentor(paths)
    for p in paths:
        for tag, s in (("s100", 1.0), ("s25", 0.25)):
            out[f"imageid__{p.name}__{tag}"] = ids.segment_image(None, p, s)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({len(out)} arrays)")


if __name__ == "__main__":
    main()
