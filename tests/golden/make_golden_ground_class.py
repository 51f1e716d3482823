#!/usr/bin/env python3
"""Writes tests/golden/reference_ground_class.npz: what the REFERENCE's `TexturedPhotogrammetryMesh.label_ground_class`
(meshes/meshes.py:1540-1629) and `add_label` (meshes.py:733-735) do on small label arrays, for the branches of the ground ID the
reference can execute, run with the stub recipe of SURVEY.md Appendix B (the geospatial modules the reference imports are replaced
by mocks).  `get_height_above_ground` -- rasterio and pyproj in the reference -- is replaced by a FIXED mask per case, so the golden
pins the label logic alone: which labels are rewritten, to which ID, and what the table holds afterwards.
tests/test_height_above_ground_host.py replays the stored inputs through this package with a DTM that produces the same mask.

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_ground_class.py

Stored per case K: "K/labels_in" (N, 1), "K/mask" (N,) bool, "K/given_ids" + "K/given_labels" (empty: no table), "K/ground_ID"
(NaN: not passed; a passed NaN is "K/ground_ID_is_nan"), "K/only_existing", "K/name", "K/labels_none" (the labels came from the
texture), "K/set_texture"; answers: "K/labels_out", "K/ids" + "K/labels" (the table afterwards), "K/table_is_none",
"K/use_vertex_locations" (what the reference asked the heights for), "K/texture_set" (set_texture was called).
Not here, because the reference raises: a table without the name and no ground_ID (`np.max(dict.keys()) + 1`: TypeError), and a
numeric ground_ID on a mesh without a table (`None[ID] = name`: TypeError).
"""
import importlib.abc
import importlib.machinery
import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

OUT = Path(__file__).resolve().parent / "reference_ground_class.npz"
MISSING = ("fiona", "geopandas", "pyproj", "pyvista", "rasterio", "shapely", "skimage", "ubelt", "imageio", "piexif", "trimesh",
           "rtree", "rasterstats", "setcoverpy", "chardet", "cchardet", "IPython")
N_FACES, N_VERTS = 8, 6
NAN = np.nan
FACE_LABELS = np.array([0.0, 1.0, NAN, 2.0, 1.0, NAN, 0.0, 2.0])
FACE_MASK = np.array([True, False, True, True, False, False, True, False])
VERT_LABELS = np.array([1.0, NAN, 0.0, 0.0, 1.0, NAN])
VERT_MASK = np.array([True, True, False, True, False, False])

CASES = {   # case -> dict(labels, mask, table, ground_ID ("absent": not passed), only_existing, name, labels_none, set_texture)
    "continuous": dict(labels=FACE_LABELS, mask=FACE_MASK, table=None, ground_ID="absent"),
    "continuous_all": dict(labels=FACE_LABELS, mask=FACE_MASK, table=None, ground_ID="absent", only_existing=False),
    "name_present": dict(labels=FACE_LABELS, mask=FACE_MASK, table={0: "oak", 1: "ground", 2: "fir"}, ground_ID="absent"),
    "name_present_overrides": dict(labels=FACE_LABELS, mask=FACE_MASK, table={0: "oak", 1: "ground", 2: "fir"}, ground_ID=99),
    "passed_id": dict(labels=FACE_LABELS, mask=FACE_MASK, table={0: "oak", 1: "ash", 2: "fir"}, ground_ID=7),
    "passed_id_all": dict(labels=FACE_LABELS, mask=FACE_MASK, table={0: "oak", 1: "ash", 2: "fir"}, ground_ID=7, only_existing=False),
    "passed_nan_with_table": dict(labels=FACE_LABELS, mask=FACE_MASK, table={0: "oak", 1: "ash", 2: "fir"}, ground_ID=NAN,
                                  name="GROUND"),
    "vertex_labels": dict(labels=VERT_LABELS, mask=VERT_MASK, table={0: "oak", 1: "ash"}, ground_ID=5),
    "from_texture": dict(labels=FACE_LABELS, mask=FACE_MASK, table={0: "oak", 1: "ash", 2: "fir"}, ground_ID=3, labels_none=True,
                         set_texture=True, name="GROUND"),
}


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


def main():
    sys.meta_path.insert(0, Finder())
    from geograypher.meshes.meshes import TexturedPhotogrammetryMesh as TPM

    out = {}
    for case, spec in CASES.items():
        labels_in = spec["labels"].reshape(-1, 1).copy()
        table = None if spec["table"] is None else dict(spec["table"])
        asked = {}

        class Fake:
            IDs_to_labels = table
            faces = np.zeros((N_FACES, 3), dtype=int)
            pyvista_mesh = MagicMock()
            get_IDs_to_labels = TPM.get_IDs_to_labels
            add_label = TPM.add_label

            def get_texture(self, request_vertex_texture):
                assert request_vertex_texture is False
                return texture

            def get_height_above_ground(self, DTM_file, threshold, use_vertex_locations):
                asked["use_vertex_locations"] = use_vertex_locations
                return spec["mask"].copy()

            def set_texture(self, values):
                asked["texture_set"] = np.array(values)

        Fake.pyvista_mesh.points = np.zeros((N_VERTS, 3))
        texture = labels_in.copy()
        kwargs = {} if isinstance(spec["ground_ID"], str) else {"ground_ID": spec["ground_ID"]}
        name = spec.get("name", "ground")
        fake = Fake()
        got = TPM.label_ground_class(fake, "dtm.tif", 2.0, labels=None if spec.get("labels_none") else labels_in,
                                     only_label_existing_labels=spec.get("only_existing", True), ground_class_name=name,
                                     set_mesh_texture=spec.get("set_texture", False), **kwargs)
        assert got is (texture if spec.get("labels_none") else labels_in)   # rewritten in place
        given = spec["table"] or {}
        after = fake.IDs_to_labels
        passed = spec["ground_ID"]
        out[f"{case}/labels_in"] = spec["labels"].reshape(-1, 1)
        out[f"{case}/mask"] = spec["mask"]
        out[f"{case}/given_ids"] = np.array(list(given), dtype=np.int64)
        out[f"{case}/given_labels"] = np.array(list(given.values()), dtype=str)
        out[f"{case}/table_given"] = np.array(spec["table"] is not None)
        out[f"{case}/ground_ID"] = np.array(NAN if isinstance(passed, str) or passed != passed else float(passed))
        out[f"{case}/ground_ID_is_nan"] = np.array(not isinstance(passed, str) and passed != passed)
        out[f"{case}/only_existing"] = np.array(spec.get("only_existing", True))
        out[f"{case}/name"] = np.array(name)
        out[f"{case}/labels_none"] = np.array(bool(spec.get("labels_none")))
        out[f"{case}/set_texture"] = np.array(bool(spec.get("set_texture")))
        out[f"{case}/labels_out"] = np.asarray(got, dtype=np.float64)
        out[f"{case}/table_is_none"] = np.array(after is None)
        out[f"{case}/ids"] = np.array(list(after or {}), dtype=np.int64)
        out[f"{case}/labels"] = np.array(list((after or {}).values()), dtype=str)
        out[f"{case}/use_vertex_locations"] = np.array(asked["use_vertex_locations"])
        out[f"{case}/texture_set"] = np.array("texture_set" in asked)
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
