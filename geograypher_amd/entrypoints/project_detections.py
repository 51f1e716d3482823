"""Project per-image detections to geospatial polygons: boxes in the images -> a sparse face x detection matrix -> one polygon per
detection with its attributes.

Mirror of geograypher/entrypoints/project_detections.py:21-191 in the formats this package reads: the mesh as `.npz` (points, faces;
EPSG:4978), the cameras as a Metashape XML, the detections as DeepForest-style CSV files (`TabularRectangleSegmentor`).  The two
steps are the reference's.  `project_to_mesh` aggregates the detections (`aggregate_projected_images`; every detection is a class of
its own) and writes the sparse (F, n_detections) matrix as `.npz` with the detection table beside it
(`<stem>_detection_info.csv`).  `convert_to_geospatial` takes that matrix -- from the first step or from the two files -- and traces
the footprint of EVERY detection in one device call (`export_face_labels_vector` on the sparse matrix, `gr_member_outlines`:
DESIGN.md section 8l), joins the rows with the detection table (row `class_ID` = table `instance_ID`, inner join) and writes a
`.geojson`.

Divergences from the reference: `--project-to-mesh` and `--convert-to-geospatial` are flags (the reference declares them
`type=Path`, with which they cannot be switched on without naming a path that is then taken as True); `--image-shape` takes two
integers (the reference's `type=tuple` splits a string into characters); the planar coordinates of the export come from
`export_points_file` or `export_CRS` (the reference reprojects with pyproj); the join is done without pandas; the visualisations
are not carried over."""
import argparse
import csv
import logging
import sys
from pathlib import Path

import numpy as np

from geograypher_amd.cameras.derived_cameras import MetashapeCameraSet
from geograypher_amd.constants import CLASS_ID_KEY, INSTANCE_ID_KEY, PATH_TYPE


def detection_info_path(projections_to_mesh_filename: PATH_TYPE) -> Path:
    """The detection table that lies beside the projections: `<stem>_detection_info.csv`."""
    path = Path(projections_to_mesh_filename)
    return Path(path.parent, path.stem + "_detection_info.csv")


def read_detection_info(path: PATH_TYPE) -> dict:
    """The table `save_detection_data` wrote, as {column: list}, columns in file order and typed as pandas.read_csv types them; the
    leading index column without a name is "Unnamed: 0", as in pandas."""
    from geograypher_amd.predictors.derived_segmentors import _column_values

    with open(path, newline="") as file:
        rows = list(csv.reader(file))
    if not rows:
        raise ValueError(f"No columns to parse from file {path}")
    header = [name if name != "" else f"Unnamed: {k}" for k, name in enumerate(rows[0])]
    body = [r for r in rows[1:] if r]
    return {name: _column_values([r[k] if k < len(r) else "" for r in body]) for k, name in enumerate(header)}


def join_detection_info(columns: dict, detection_info: dict) -> (np.ndarray, dict):
    """The reference's merge (project_detections.py:180-188): an inner join of the projected rows' `class_ID` with the table's
    `instance_ID`, the projected rows' order kept (a table with the ID twice gives the row twice, in table order); a table column
    named like a projected one gets the suffix `_right`; `class_ID` and `Unnamed: 0` are dropped.  -> (the projected row of every
    joined row, {column: array})."""
    if INSTANCE_ID_KEY not in detection_info:
        raise KeyError(INSTANCE_ID_KEY)
    rows_of = {}
    for k, instance in enumerate(detection_info[INSTANCE_ID_KEY]):
        if isinstance(instance, (int, float, np.integer, np.floating)):   # a text ID equals no class_ID
            rows_of.setdefault(float(instance), []).append(k)
    left, right = [], []
    for row, class_id in enumerate(np.asarray(columns[CLASS_ID_KEY], dtype=np.float64).tolist()):
        for k in rows_of.get(class_id, []):   # NaN matches nothing
            left.append(row)
            right.append(k)
    joined = {}
    for name, values in columns.items():
        joined[name] = np.asarray(values)[left] if left else np.asarray(values)[:0]
    for name, values in detection_info.items():
        column = np.empty(len(values), dtype=object)
        column[:] = values
        joined[name + "_right" if name in columns else name] = column[right]
    for name in (CLASS_ID_KEY, "Unnamed: 0"):
        joined.pop(name, None)
    return np.array(left, dtype=np.int64), joined


def project_detections(
    mesh_filename: PATH_TYPE,
    mesh_CRS,
    cameras_filename: PATH_TYPE,
    project_to_mesh: bool = False,
    convert_to_geospatial: bool = False,
    image_folder: PATH_TYPE = None,
    detections_folder: PATH_TYPE = None,
    projections_to_mesh_filename: PATH_TYPE = None,
    projections_to_geospatial_savefilename: PATH_TYPE = None,
    default_focal_length: float = None,
    image_shape: tuple = None,
    segmentor_kwargs: dict = {},
    vis_mesh: bool = False,
    vis_geodata: bool = False,
    *,
    export_points_file=None,
    export_CRS=None,
    backend=None,
):
    """Project per-image detections to geospatial coordinates (see the module docstring).  The reference's arguments and defaults.
    Beyond the reference, keyword-only: `export_points_file` (a `.npy` path or an array: the V mesh vertices (V, 2 | 3) in the planar
    CRS of the export) or `export_CRS` (that CRS, e.g. "EPSG:32610": the vertices are reprojected on the device) -- giving both is a
    ValueError, `convert_to_geospatial` without either a NotImplementedError --, and `backend`, which replaces the device.

    Raises ValueError for `convert_to_geospatial` alone without `projections_to_mesh_filename` and FileNotFoundError when that file
    does not exist, as the reference does; NotImplementedError for `vis_mesh` and `vis_geodata`.  Returns the joined table as
    (PlanarPolygons, {column: array}) after `convert_to_geospatial`, the sparse matrix after `project_to_mesh` alone, else None."""
    from scipy.sparse import load_npz, save_npz

    from geograypher_amd.cameras.segmentor import SegmentorPhotogrammetryCameraSet
    from geograypher_amd.meshes.derived_meshes import TexturedPhotogrammetryMeshIndexPredictions
    from geograypher_amd.predictors.derived_segmentors import TabularRectangleSegmentor
    from geograypher_amd.utils.geometric import PlanarPolygons, write_geojson_multipolygons
    from geograypher_amd.utils.geospatial import points_or_CRS

    export_points = points_or_CRS("export_points_file", export_points_file, "export_CRS", export_CRS)
    if vis_mesh:
        raise NotImplementedError("vis_mesh: visualisations need pyvista, which is outside the projection path")
    if vis_geodata:
        raise NotImplementedError("vis_geodata: plotting needs geopandas and matplotlib, which are outside the projection path")
    if convert_to_geospatial and export_points is None:
        raise NotImplementedError("convert_to_geospatial: the vertices in the CRS of the export are needed (export_points_file or "
                                  "export_CRS); reprojecting them needs pyproj, which is outside the projection path")
    if convert_to_geospatial and not project_to_mesh:   # the reference's checks, before the mesh is read
        if projections_to_mesh_filename is None:
            raise ValueError("No projections_to_mesh_savefilename provided")
        if not Path(projections_to_mesh_filename).is_file():
            raise FileNotFoundError(f"projections_to_mesh_filename {projections_to_mesh_filename} not found")

    mesh = TexturedPhotogrammetryMeshIndexPredictions(mesh_filename, input_CRS=mesh_CRS, backend=backend)
    aggregated_projections = detection_info = None

    if project_to_mesh:
        camera_set = MetashapeCameraSet(cameras_filename, image_folder,
                                        default_sensor_params={"f": default_focal_length, "cx": 0, "cy": 0})
        if image_shape is None:   # from the first image of the folder
            from PIL import Image

            image_filenames = sorted(Path(image_folder).glob("*.*"))
            if not image_filenames:
                raise ValueError(f"No image_shape provided and folder of images {image_folder} was empty")
            logging.info(f"loading image shape from {image_filenames[0]}")
            with Image.open(image_filenames[0]) as first_image:
                image_shape = (first_image.height, first_image.width)
        detections_predictor = TabularRectangleSegmentor(detection_file_or_folder=detections_folder, image_folder=image_folder,
                                                         image_shape=tuple(image_shape), **segmentor_kwargs)
        if projections_to_mesh_filename is not None:
            logging.info(f"Saving detection info to {detection_info_path(projections_to_mesh_filename)}")
            detections_predictor.save_detection_data(detection_info_path(projections_to_mesh_filename))
        detections_camera_set = SegmentorPhotogrammetryCameraSet(camera_set, segmentor=detections_predictor)
        _, info = mesh.aggregate_projected_images(cameras=detections_camera_set, n_classes=detections_predictor.num_classes)
        aggregated_projections = info["summed_projections"]   # summed, not averaged
        if projections_to_mesh_filename is not None:
            Path(projections_to_mesh_filename).parent.mkdir(parents=True, exist_ok=True)
            save_npz(projections_to_mesh_filename, aggregated_projections)
        table = detections_predictor.get_all_detections()
        detection_info = {name: list(table[name]) for name in table.columns}

    if not convert_to_geospatial:
        return aggregated_projections

    if not project_to_mesh:
        aggregated_projections = load_npz(projections_to_mesh_filename)
        detection_info = read_detection_info(detection_info_path(projections_to_mesh_filename))
    if projections_to_geospatial_savefilename is not None and Path(projections_to_geospatial_savefilename).suffix != ".geojson":
        raise NotImplementedError(f"projections_to_geospatial_savefilename {projections_to_geospatial_savefilename}: files other "
                                  "than .geojson need geopandas, which is outside the projection path")
    polygons, columns = mesh.export_face_labels_vector(face_labels=aggregated_projections, points_in_export_CRS=export_points)
    rows, joined = join_detection_info(columns, detection_info)
    ring_row = np.asarray(polygons.ring_polygon, dtype=np.int64)
    rings, ring_polygon, ring_is_hole = [], [], []
    for new_row, old_row in enumerate(rows.tolist()):   # the rings of a row are stored together, exterior before its holes
        for r in np.nonzero(ring_row == old_row)[0].tolist():
            rings.append(polygons.rings[r])
            ring_polygon.append(new_row)
            ring_is_hole.append(bool(polygons.ring_is_hole[r]))
    merged = PlanarPolygons(rings, ring_polygon, ring_is_hole, n_polygons=len(rows))
    if projections_to_geospatial_savefilename is not None:
        write_geojson_multipolygons(projections_to_geospatial_savefilename, merged, joined)
    return merged, joined


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Project per-image detections to geospatial polygons, one per detection.",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--mesh-filename", type=Path, required=True, help="Mesh as .npz (points, faces)")
    parser.add_argument("--mesh-CRS", required=True, help="CRS of the mesh vertices (EPSG:4978)")
    parser.add_argument("--cameras-filename", type=Path, required=True, help="Metashape XML with camera calibrations and positions")
    parser.add_argument("--project-to-mesh", action="store_true", help="Run the projection of the detections to the mesh")
    parser.add_argument("--convert-to-geospatial", action="store_true", help="Run the conversion of the projections to polygons")
    parser.add_argument("--image-folder", type=Path, help="Folder of the images the detections were made on")
    parser.add_argument("--detections-folder", type=Path, help="Folder of detection CSV files, or one such file")
    parser.add_argument("--projections-to-mesh-filename", type=Path,
                        help="Where the sparse face x detection matrix is saved and/or loaded (.npz)")
    parser.add_argument("--projections-to-geospatial-savefilename", type=Path, help="Where the polygons are saved (.geojson)")
    parser.add_argument("--default-focal-length", type=float, help="Focal length in pixels for sensors that have none in the XML")
    parser.add_argument("--image-shape", type=int, nargs=2, metavar=("HEIGHT", "WIDTH"),
                        help="Shape of the images; default: that of the first image in --image-folder")
    parser.add_argument("--export-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 2) or (V, 3) in the planar CRS of the export")
    parser.add_argument("--export-CRS", help="Planar CRS of the export instead of --export-points-file")
    parser.add_argument("--vis-mesh", action="store_true", help="Not available here")
    parser.add_argument("--vis-geodata", action="store_true", help="Not available here")
    args = parser.parse_args(argv)
    if args.image_shape is not None:
        args.image_shape = tuple(args.image_shape)
    return args


def main(argv=None):
    project_detections(**vars(parse_args(argv)))


class _CallableModule(type(sys)):
    """The function and its module share a name, and importing the module binds that name in the package to the module: calling
    the module calls the function, so `geograypher_amd.entrypoints.project_detections(...)` works whichever was bound."""

    def __call__(self, *args, **kwargs):
        return project_detections(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule


if __name__ == "__main__":
    main()
