#!/usr/bin/env python3
"""Writes tests/golden/reference_vector_texture.npz: what the REFERENCE's `utils.indexing.determine_IDs_to_labels`
(utils/indexing.py:35-84) and `TexturedPhotogrammetryMesh.remap_texture` (meshes/meshes.py:383-474) return on small arrays, run
with the stub recipe of SURVEY.md Appendix B (the geospatial modules the reference imports are replaced by mocks; the two
functions are plain numpy).  tests/test_vector_texture_host.py replays the stored inputs through this package.

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_vector_texture.py

Stored per case K: "K/texture" (strings as unicode arrays), the keyword arguments that are not None ("K/all_values",
"K/background_ID", "K/given_ids" + "K/given_labels"), and the answers: "K/is_none" (determine: the continuous case),
"K/ids" + "K/labels" (the IDs_to_labels the call returned or left on the mesh; empty when it left None), and for remap cases
"K/remapped".
"""
import importlib.abc
import importlib.machinery
import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

OUT = Path(__file__).resolve().parent / "reference_vector_texture.npz"
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


DETERMINE = {   # case -> (texture, all_discrete_texture_values, background_ID)
    "det_int": (np.array([3, 1, 1, 7]), None, None),
    "det_float_whole": (np.array([0.0, 2.0, np.nan, 2.0]), None, None),
    "det_float_continuous": (np.array([0.5, 1.0, 2.0]), None, None),
    "det_str": (np.array(["oak", "fir", "oak", "ash"], dtype=object), None, None),
    "det_all_values": (np.array(["oak", "null", "oak"], dtype=object), np.array(["oak", "fir", "ash"], dtype=object), None),
    "det_background_1": (np.array([5, 6, 7]), None, 1),
    "det_background_0": (np.array([5, 6, 7]), None, 0),
}
REMAP = {       # case -> (texture, IDs_to_labels, all_discrete_texture_values, background_ID)
    "remap_str": (np.array(["oak", "fir", "oak", "ash"], dtype=object), None, None, None),
    "remap_str_all_values": (np.array(["oak", "null", "fir"], dtype=object), None, np.array(["oak", "fir", "ash"], dtype=object), None),
    "remap_given_table": (np.array(["oak", "elm", "fir"], dtype=object), {0: "fir", 4: "oak"}, None, None),
    "remap_int_identity": (np.array([0, 1, 2, 1]), None, None, None),
    "remap_int_sparse": (np.array([10, 30, 10, 20]), None, None, None),
    "remap_int_background": (np.array([10, 30, 10, 20]), None, None, 1),
    "remap_float_whole": (np.array([2.0, 0.0, 1.0, 1.0]), None, None, None),
    "remap_two_columns": (np.array([[1, 2], [3, 4], [5, 6]]), None, None, None),
}


def store(out, case, texture, table, all_values, background_ID):
    out[f"{case}/texture"] = texture.astype(str) if texture.dtype == object else texture
    if all_values is not None:
        out[f"{case}/all_values"] = all_values.astype(str)
    if background_ID is not None:
        out[f"{case}/background_ID"] = np.array(background_ID)
    out[f"{case}/is_none"] = np.array(table is None)
    keys = list(table) if table else []
    values = np.array([table[k] for k in keys])
    out[f"{case}/ids"] = np.array(keys, dtype=np.int64)
    out[f"{case}/labels"] = values.astype(str) if values.dtype.kind in "OU" else values


def main():
    sys.meta_path.insert(0, Finder())
    from geograypher.meshes.meshes import TexturedPhotogrammetryMesh as TPM
    from geograypher.utils.indexing import determine_IDs_to_labels

    out = {}
    for case, (texture, all_values, background_ID) in DETERMINE.items():
        table = determine_IDs_to_labels(texture, all_discrete_texture_values=all_values, background_ID=background_ID)
        store(out, case, texture, table, all_values, background_ID)

    class FakeMesh:
        IDs_to_labels = "untouched"
        standardize_texture = TPM.standardize_texture

    for case, (texture, given, all_values, background_ID) in REMAP.items():
        fake = FakeMesh()
        remapped = TPM.remap_texture(fake, texture, IDs_to_labels=given, all_discrete_texture_values=all_values,
                                     update_IDs_to_labels=True, background_ID=background_ID)
        assert fake.IDs_to_labels != "untouched"
        store(out, case, texture, fake.IDs_to_labels, all_values, background_ID)
        if given is not None:
            out[f"{case}/given_ids"] = np.array(list(given), dtype=np.int64)
            out[f"{case}/given_labels"] = np.array(list(given.values())).astype(str)
        out[f"{case}/remapped"] = np.asarray(remapped, dtype=np.float64)
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
