#!/usr/bin/env python3
"""Writes tests/golden/composites.npz: what the REFERENCE's `utils.visualization.create_composite` (utils/visualization.py:113-193)
returns on small images, run with the stub recipe of SURVEY.md Appendix B (pyvista, imageio and the geospatial modules are mocks;
matplotlib is real: its colormaps are what the call is about), and matplotlib's tab10, tab20 and viridis tables as float64.
tests/test_vis_host.py holds `geograypher_amd/utils/colormaps.py` and the stand-in tests/vis_standin.py against the file, byte for
byte; tests/test_vis_gpu.py the device.

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_composites.py

Stored: "tables/<name>" (N, 3) float64; "cases": the case names; per case K "K/photo", "K/label", "K/weight", "K/grey", "K/ids"
(the keys of IDs_to_labels; absent for None) and the answer "K/composite" (h, 3 w, 3) uint8.  No image exceeds 16 x 24 pixels.
"""
import importlib.abc
import importlib.machinery
import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

OUT = Path(__file__).resolve().parent / "composites.npz"
MISSING = ("fiona", "geopandas", "pyproj", "pyvista", "rasterio", "shapely", "skimage", "ubelt", "imageio", "piexif", "trimesh",
           "rtree", "rasterstats", "setcoverpy", "chardet", "cchardet", "IPython")


class Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in MISSING:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        m = MagicMock()
        m.__path__, m.__spec__, m.__name__ = [], spec, spec.name
        return m

    def exec_module(self, module):
        pass


def cases():
    """name -> (photo, label, weight, grey, IDs_to_labels)"""
    rng = np.random.default_rng(20240917)
    h, w = 13, 23
    photo_u8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    photo_u8[0, 0], photo_u8[0, 1], photo_u8[0, 2] = (0, 0, 0), (255, 255, 255), (31, 119, 180)
    photo_f = rng.random((h, w, 3))
    photo_f[0, 0], photo_f[0, 1] = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    four = {k: f"class {k}" for k in range(4)}
    fifteen = {k: f"class {k}" for k in range(15)}
    lab4 = rng.integers(0, 4, (h, w), dtype=np.uint8)
    lab4[1, :6] = (0, 9, 10, 11, 200, 255)           # beyond the table: its last row
    lab15 = rng.integers(0, 15, (h, w), dtype=np.uint8)
    lab15[2, :6] = (0, 14, 19, 20, 21, 255)
    cont = rng.normal(size=(h, w)) * 3.0             # negative values, 0.0, NaN, an infinity
    cont[0, :5] = (np.nan, 0.0, -0.0, np.inf, cont.min() - 1.0)
    cont_pos = rng.random((h, w)) * 40.0 + 2.0       # no nulls: the smallest value is shifted to 0 and stays coloured
    cont_u8 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cont_u8[3, :3] = (0, 1, 255)
    rgb_f = rng.random((h, w, 3))
    rgb_u8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    whole = np.round(rng.random((h, w)) * 3.0) / 4.0   # a float label under discrete classes goes through the table as a float
    wide_u8 = rng.integers(0, 4, (16, 24), dtype=np.uint8)
    wide_photo = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    return {
        "discrete4_u8": (photo_u8, lab4, 0.5, True, four),
        "discrete15_u8": (photo_u8, lab15, 0.5, True, fifteen),
        "discrete4_weight0": (photo_u8, lab4, 0.0, True, four),
        "discrete4_weight1_colour": (photo_u8, lab4, 1.0, False, four),
        "discrete4_float_photo": (photo_f, lab4, 0.5, True, four),
        "discrete15_float_photo_colour": (photo_f, lab15, 0.3, False, fifteen),
        "discrete4_float_label": (photo_u8, whole, 0.5, True, four),
        "continuous_nan_zero_negative": (photo_u8, cont, 0.5, True, None),
        "continuous_positive_float_photo": (photo_f, cont_pos, 0.7, False, None),
        "continuous_u8": (photo_u8, cont_u8, 0.5, True, None),
        "continuous_many_classes_u8": (photo_u8, cont_u8, 0.5, True, {k: str(k) for k in range(25)}),
        "rgb_float_label": (photo_u8, rgb_f, 0.5, True, None),
        "rgb_float_label_discrete": (photo_f, rgb_f, 0.25, False, four),
        "rgb_u8_label": (photo_u8, rgb_u8, 0.5, True, None),
        "smallest_2x3": (photo_u8[:2, :3], lab4[1:3, :3], 0.5, True, four),   # (the reference squeezes a side of 1 away and fails)
        "widest_16x24": (wide_photo, wide_u8, 0.5, True, four),
    }


def main():
    sys.meta_path.insert(0, Finder())
    from matplotlib import colormaps

    from geograypher.utils.visualization import create_composite

    out = {}
    for name in ("tab10", "tab20", "viridis"):
        cmap = colormaps[name]
        out[f"tables/{name}"] = np.asarray(cmap(np.arange(cmap.N)), dtype=np.float64)[:, :3].copy()
    table = cases()
    out["cases"] = np.array(list(table))
    for name, (photo, label, weight, grey, ids) in table.items():
        assert photo.shape[0] <= 16 and photo.shape[1] <= 24
        with np.errstate(all="ignore"):
            composite = create_composite(photo.copy(), label.copy(), label_blending_weight=weight, IDs_to_labels=ids,
                                         grayscale_RGB_overlay=grey)
        assert composite.dtype == np.uint8 and composite.shape == (photo.shape[0], 3 * photo.shape[1], 3)
        out[f"{name}/photo"], out[f"{name}/label"], out[f"{name}/composite"] = photo, label, composite
        out[f"{name}/weight"], out[f"{name}/grey"] = np.array(weight), np.array(grey)
        if ids is not None:
            out[f"{name}/ids"] = np.array(list(ids), dtype=np.int64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(table)} cases, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
