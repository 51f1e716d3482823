"""Aggregate per-image predictions onto the mesh: label images from many viewpoints -> votes per face -> a class per face.

Mirror of geograypher/entrypoints/aggregate_images.py:19-233 in the formats this package reads: the mesh as `.npz` (points, faces;
EPSG:4978), the cameras as a Metashape XML, the predictions as index images under `label_folder` in the layout of `image_folder`
(`LookUpSegmentor`).  The camera set is cut by `subset_images_folder`, `filename_regex`, `take_every_nth_camera` and -- with `ROI`
and `ROI_camera_points_file` -- to the cameras within `ROI_buffer_radius_meters` of the ROI; the mesh is cropped to the ROI grown by
the same distance (`select_mesh_ROI`, on the device), which needs `ROI_points_file`, the vertices in the ROI's CRS.  The aggregated
face values (`aggregate_projected_images`) and the class per face (`argmax_nonzero`, NaN where nothing was seen) are written as
`.npy`; with `DTM_file`, `DTM_points_file` and `height_above_ground_threshold` the faces near the terrain lose their class first
(`label_ground_class`); with `top_down_vector_projection_savefile` and `top_down_points_file` the classes are then written as a
top-down vector map, one multipolygon per class (`export_face_labels_vector`, traced on the device).  With `mesh_downsample` and
`mesh_downsample_method="cluster"` the mesh is decimated by vertex clustering behind the crop (`TexturedPhotogrammetryMesh.decimate`,
on the device).  With `vis_folder` the two pictures the reference shows in a window are written as PNGs, rendered off-screen on the
device (`TexturedPhotogrammetryMesh.vis`).  Not carried over: the reference's quadric decimation and `vis=True` (there is no window)."""
import argparse
import json
import math
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.constants import PATH_TYPE


def aggregate_images(
    mesh_file,
    cameras_file: PATH_TYPE,
    image_folder: PATH_TYPE,
    label_folder: PATH_TYPE,
    mesh_CRS,
    original_image_folder: typing.Union[PATH_TYPE, None] = None,
    subset_images_folder: typing.Union[PATH_TYPE, None] = None,
    filename_regex: typing.Optional[str] = None,
    take_every_nth_camera: typing.Union[int, None] = 100,
    DTM_file: typing.Union[PATH_TYPE, None] = None,
    height_above_ground_threshold: float = 2.0,
    ROI=None,
    ROI_buffer_radius_meters: float = 50,
    IDs_to_labels: typing.Union[dict, str, None] = None,
    mesh_downsample: float = 1.0,
    n_aggregation_clusters: typing.Union[int, None] = None,
    n_cameras_per_aggregation_cluster: typing.Union[int, None] = None,
    aggregate_image_scale: float = 1.0,
    aggregated_face_values_savefile: typing.Union[PATH_TYPE, None] = None,
    predicted_face_classes_savefile: typing.Union[PATH_TYPE, None] = None,
    top_down_vector_projection_savefile: typing.Union[PATH_TYPE, None] = None,
    vis: bool = False,
    ROI_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    ROI_camera_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    DTM_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    top_down_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    camera_set=None,
    backend=None,
    ROI_CRS=None,
    ROI_camera_CRS=None,
    DTM_CRS=None,
    top_down_CRS=None,
    mesh_downsample_method: typing.Union[str, None] = None,
    top_down_simplify_tol: float = 0.0,
    top_down_simplify_method: typing.Union[str, None] = None,
    top_down_raster_projection_savefile: typing.Union[PATH_TYPE, None] = None,
    top_down_raster_resolution: typing.Union[float, None] = None,
    vis_folder: typing.Union[PATH_TYPE, None] = None,
    sieve_min_area_m2: typing.Union[float, None] = None,
    sieve_min_faces: typing.Union[int, None] = None,
    sieve_fill_unseen: bool = False,
    full_mesh_face_classes_savefile: typing.Union[PATH_TYPE, None] = None,
    transfer_max_distance_meters: typing.Union[float, None] = None,
):
    """Aggregate the labels under `label_folder` onto the mesh (see the module docstring).  The reference's arguments and defaults;
    `mesh_downsample != 1` without `mesh_downsample_method`, `vis`, `ROI` without `ROI_points_file`, `DTM_file` without `DTM_points_file` and
    `top_down_vector_projection_savefile` without `top_down_points_file` raise NotImplementedError.  Beyond the reference:
    `ROI_points_file`, `DTM_points_file` and `top_down_points_file` (`.npy` paths or arrays: the V ORIGINAL vertices in the ROI's / the
    DTM's / the export's planar CRS; with the last, the class per face is written as a `.geojson` map, `export_face_labels_vector`), `ROI_camera_points_file` (the positions of the cameras of the full
    set in the ROI's CRS; without it the camera set is not cut to the ROI, with a log line), and `camera_set` and `backend`, which
    replace the objects built from `cameras_file` and the device.  Each `*_points_file` has a sibling `ROI_CRS`, `ROI_camera_CRS`,
    `DTM_CRS`, `top_down_CRS`: the CRS of the ROI / the DTM / the map (e.g. "EPSG:32610") in place of the points, which are then
    reprojected on the device; giving both is a ValueError.  `mesh_downsample_method="cluster"`
    decimates the mesh to about `mesh_downsample` of its vertices behind the ROI crop (`TexturedPhotogrammetryMesh.decimate`: vertex
    clustering, not the reference's quadric decimation); the `*_points_file` arrays stay those of the ORIGINAL mesh and the results
    are per face of the decimated mesh (`mesh.decimated_face_IDs`).  `top_down_simplify_method="douglas-peucker"` simplifies the rings
    of the top-down map at `top_down_simplify_tol` metres on the device (`export_face_labels_vector(simplify_tol=...,
    simplify_method=...)`: exact Douglas-Peucker, shared borders kept consistent); a tolerance without the method raises
    NotImplementedError and another method name ValueError, both before the aggregation.
    `top_down_raster_projection_savefile` (.tif / .tiff) writes the classes as a uint8 GeoTIFF seen from above, cells of
    `top_down_raster_resolution` map units on a north-up grid over the vertices (`export_face_labels_raster`: where surfaces
    overlap in plan view the upper one wins; nodata 255); it uses the same `top_down_points_file` (here (V, 3): z decides) or
    `top_down_CRS` as the vector map and may be given with or without it.  Its arguments are checked before the aggregation.
    `sieve_min_area_m2` or `sieve_min_faces` (one of them at most) removes the speckle of the class per face on the device before the
    ground step, the saved file and the maps: connected regions of one class below that surface area / face count join their
    greatest neighbour region (`TexturedPhotogrammetryMesh.sieve_face_labels`); `sieve_fill_unseen` also
    fills small regions of unseen faces and needs one of the two.  With the three at their defaults every output is what it is
    without them.
    `full_mesh_face_classes_savefile` (.npy; needs `mesh_downsample_method`) also brings the predicted classes, as they are saved,
    from the faces of the decimated mesh onto the faces of the mesh as it is behind the ROI crop and before the decimation -- that mesh
    is built a second time, without the decimation --: every full-resolution face takes the class of the decimated face whose centre
    is nearest its own (`TexturedPhotogrammetryMesh.values_from_mesh`), NaN where none lies within
    `transfer_max_distance_meters` (None: no limit), and the (F_full, 1) array is saved.  Without a decimation it is a ValueError,
    and so is the distance without the file.  Returns (mesh, aggregated face values, predicted face classes (F, 1))."""
    from geograypher_amd.cameras.segmentor import SegmentorPhotogrammetryCameraSet
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh, TexturedPhotogrammetryMeshChunked
    from geograypher_amd.predictors.derived_segmentors import LookUpSegmentor
    from geograypher_amd.utils.geospatial import is_CRS_designator, points_or_CRS

    ROI_points = points_or_CRS("ROI_points_file", ROI_points_file, "ROI_CRS", ROI_CRS)
    camera_points = points_or_CRS("ROI_camera_points_file", ROI_camera_points_file, "ROI_camera_CRS", ROI_camera_CRS)
    DTM_points = points_or_CRS("DTM_points_file", DTM_points_file, "DTM_CRS", DTM_CRS)
    top_down_points = points_or_CRS("top_down_points_file", top_down_points_file, "top_down_CRS", top_down_CRS)
    if top_down_simplify_method is not None:
        from geograypher_amd.utils.geometric import check_simplify_method

        check_simplify_method(top_down_simplify_method, "top_down_simplify_method")
    elif top_down_simplify_tol > 0:
        raise NotImplementedError("top_down_simplify_tol: shapely's simplification is outside the projection path; ask for the "
                                  "exact Douglas-Peucker by name: top_down_simplify_method='douglas-peucker'")

    if top_down_raster_projection_savefile is None and top_down_raster_resolution is not None:
        raise ValueError("top_down_raster_resolution is given but top_down_raster_projection_savefile is not: there is no raster to write")
    if top_down_raster_projection_savefile is not None:
        if Path(top_down_raster_projection_savefile).suffix.lower() not in (".tif", ".tiff"):
            raise NotImplementedError(f"top_down_raster_projection_savefile {top_down_raster_projection_savefile}: rasters are "
                                      "written as .tif / .tiff only")
        if top_down_raster_resolution is None or not np.isfinite(float(top_down_raster_resolution)) or float(top_down_raster_resolution) <= 0:
            raise ValueError(f"top_down_raster_projection_savefile needs top_down_raster_resolution, a positive cell size in map "
                             f"units, got {top_down_raster_resolution!r}")

    if sieve_min_area_m2 is not None and sieve_min_faces is not None:
        raise ValueError("sieve_min_area_m2 and sieve_min_faces are both given: the sieve has one threshold")
    if sieve_fill_unseen and sieve_min_area_m2 is None and sieve_min_faces is None:
        raise ValueError("sieve_fill_unseen needs a threshold: sieve_min_area_m2 or sieve_min_faces")

    if full_mesh_face_classes_savefile is not None and mesh_downsample_method is None:
        raise ValueError("full_mesh_face_classes_savefile is given without mesh_downsample_method: the mesh is not decimated, "
                         "predicted_face_classes_savefile holds the classes of the full mesh")
    if transfer_max_distance_meters is not None:
        if full_mesh_face_classes_savefile is None:
            raise ValueError("transfer_max_distance_meters is given but full_mesh_face_classes_savefile is not: nothing is transferred")
        if not float(transfer_max_distance_meters) >= 0:
            raise ValueError(f"transfer_max_distance_meters={transfer_max_distance_meters!r} is not a distance >= 0")

    for name, value, why in (
        ("DTM_file", DTM_file if DTM_points is None else None,
         "the vertices in the DTM's CRS are needed (DTM_points_file); reprojecting them needs pyproj"),
        ("ROI", ROI if ROI_points is None else None,
         "the vertices in the ROI's CRS are needed (ROI_points_file); reprojecting them needs pyproj"),
        ("top_down_vector_projection_savefile", top_down_vector_projection_savefile if top_down_points is None else None,
         "the vector export needs geopandas"),
        ("top_down_raster_projection_savefile", top_down_raster_projection_savefile if top_down_points is None else None,
         "the vertices in the map's CRS are needed (top_down_points_file or top_down_CRS); reprojecting them needs pyproj"),
    ):
        if value is not None:
            raise NotImplementedError(f"{name}: {why}, which is outside the projection path")
    if vis:
        raise NotImplementedError("vis: visualisations need pyvista, which is outside the projection path")
    if mesh_downsample != 1 and mesh_downsample_method is None:
        raise NotImplementedError("mesh_downsample: mesh decimation is outside the projection path (meshes.py:215-226)")

    if isinstance(IDs_to_labels, (str, Path)):
        with open(IDs_to_labels, "r") as file:
            IDs_to_labels = {int(k): v for k, v in json.load(file).items()}

    # the cameras first: they are cheap and catch bad inputs early (aggregate_images.py:106-136)
    if camera_set is None:
        from geograypher_amd.cameras.derived_cameras import MetashapeCameraSet

        camera_set = MetashapeCameraSet(cameras_file, image_folder, original_image_folder=original_image_folder,
                                        validate_images=True)
    if is_CRS_designator(camera_points):   # computed for the cameras that are left when the set is cut
        camera_CRS, camera_points = camera_points, None
    else:
        camera_CRS = None
    if camera_points is not None:   # follows the cameras through the filters below
        camera_points = np.asarray(camera_points, dtype=np.float64)
        if camera_points.shape[0] != len(camera_set):
            raise ValueError(f"ROI_camera_points_file has {camera_points.shape[0]} rows for {len(camera_set)} cameras")

    def subset(inds):
        nonlocal camera_set, camera_points
        inds = [int(i) for i in inds]
        camera_set = camera_set.get_subset_cameras(inds)
        camera_points = None if camera_points is None else camera_points[inds]

    if subset_images_folder is not None:
        subset(camera_set.inds_in_folder(subset_images_folder))
    if filename_regex is not None:
        subset(camera_set.inds_matching_filename_regex(filename_regex))
    if take_every_nth_camera is not None:
        subset(range(0, len(camera_set), take_every_nth_camera))

    if top_down_points is not None and top_down_vector_projection_savefile is None and top_down_raster_projection_savefile is None:
        raise ValueError(f"{'top_down_CRS' if is_CRS_designator(top_down_points) else 'top_down_points_file'} is given but "
                         "top_down_vector_projection_savefile is not: there is no map to write")

    MeshClass = (TexturedPhotogrammetryMesh if n_aggregation_clusters is None and n_cameras_per_aggregation_cluster is None
                 else TexturedPhotogrammetryMeshChunked)
    roi_kwargs = {}
    if ROI is not None:
        roi_kwargs = {"ROI": ROI, "ROI_buffer_meters": 0 if ROI_buffer_radius_meters is None else ROI_buffer_radius_meters,
                      "points_in_ROI_CRS": ROI_points}
    if mesh_downsample_method is not None:   # behind the crop (aggregate_images.py:140-148)
        roi_kwargs.update(downsample_target=mesh_downsample, downsample_method=mesh_downsample_method)
    mesh = MeshClass(mesh_file, input_CRS=mesh_CRS, IDs_to_labels=IDs_to_labels, backend=backend, **roi_kwargs)
    kept_point_IDs = mesh.original_point_IDs()   # of the ORIGINAL vertices: what the crop and the decimation kept, or None

    if top_down_vector_projection_savefile is not None:   # fail before the aggregation, not behind it
        if Path(top_down_vector_projection_savefile).suffix != ".geojson":
            raise NotImplementedError(f"top_down_vector_projection_savefile {top_down_vector_projection_savefile}: files other than "
                                      ".geojson need geopandas, which is outside the projection path")
    any_top_down_savefile = top_down_vector_projection_savefile is not None or top_down_raster_projection_savefile is not None
    if any_top_down_savefile and not is_CRS_designator(top_down_points):
        top_down_points = np.asarray(top_down_points, dtype=np.float64)
        n_original = top_down_points.shape[0] if kept_point_IDs is None else None
        if top_down_points.ndim != 2 or top_down_points.shape[1] not in (2, 3) or \
                (n_original is not None and n_original != mesh.points.shape[0]) or \
                (kept_point_IDs is not None and len(kept_point_IDs) and top_down_points.shape[0] <= int(np.max(kept_point_IDs))):
            raise ValueError(f"top_down_points_file must hold the (V, 2) or (V, 3) ORIGINAL vertices, got {top_down_points.shape}")
        if top_down_raster_projection_savefile is not None and top_down_points.shape[1] != 3:
            raise ValueError(f"top_down_raster_projection_savefile needs the (V, 3) ORIGINAL vertices in top_down_points_file (z "
                             f"decides which surface is seen from above), got {top_down_points.shape}")

    if ROI is not None and ROI_buffer_radius_meters is not None:
        if camera_points is not None or camera_CRS is not None:
            camera_set = camera_set.get_subset_ROI(ROI=ROI, buffer_radius=ROI_buffer_radius_meters, is_geospatial=True,
                                                   points_in_ROI_CRS=camera_points if camera_CRS is None else camera_CRS,
                                                   backend=mesh.backend)
        else:
            mesh.logger.info("ROI without ROI_camera_points_file: the camera set is not cut to the ROI")
    if n_aggregation_clusters is None and n_cameras_per_aggregation_cluster is not None:
        n_aggregation_clusters = int(math.ceil(len(camera_set) / n_cameras_per_aggregation_cluster))

    if mesh.get_IDs_to_labels() is None:
        raise ValueError("aggregate_images needs IDs_to_labels: the number of classes is its largest ID + 1")
    if vis_folder is not None:   # the picture the reference shows at aggregate_images.py:163: the mesh and the cameras in use
        mesh.vis(camera_set=camera_set, screenshot_filename=Path(vis_folder, "mesh_and_cameras.png"))
    segmentor = LookUpSegmentor(base_folder=image_folder, lookup_folder=label_folder,
                                num_classes=int(np.max(list(mesh.get_IDs_to_labels().keys()))) + 1)
    segmentor_camera_set = SegmentorPhotogrammetryCameraSet(camera_set, segmentor=segmentor)

    n_clusters_kwargs = {} if n_aggregation_clusters is None else {"n_clusters": n_aggregation_clusters}
    aggregated_face_labels, _ = mesh.aggregate_projected_images(segmentor_camera_set, aggregate_img_scale=aggregate_image_scale,
                                                                **n_clusters_kwargs)
    if aggregated_face_values_savefile is not None:
        Path(aggregated_face_values_savefile).parent.mkdir(parents=True, exist_ok=True)
        np.save(aggregated_face_values_savefile, aggregated_face_labels)

    predicted_face_classes = mesh.backend.argmax_nonzero(aggregated_face_labels)
    if hasattr(predicted_face_classes, "detach"):
        predicted_face_classes = predicted_face_classes.cpu().numpy()
    predicted_face_classes = np.array(predicted_face_classes, dtype=np.float64).reshape(-1, 1)

    if sieve_min_area_m2 is not None or sieve_min_faces is not None:   # before the ground step, which the sieve must not undo
        predicted_face_classes = np.asarray(mesh.sieve_face_labels(predicted_face_classes, min_faces=sieve_min_faces,
                                                                   min_area_m2=sieve_min_area_m2, fill_unseen=sieve_fill_unseen),
                                            dtype=np.float64).reshape(-1, 1)

    if DTM_file is not None and height_above_ground_threshold is not None:   # reference: aggregate_images.py:198-206
        points_in_raster_CRS = DTM_points
        if kept_point_IDs is not None and not is_CRS_designator(points_in_raster_CRS):
            points_in_raster_CRS = np.asarray(points_in_raster_CRS)[kept_point_IDs]
        predicted_face_classes = mesh.label_ground_class(labels=predicted_face_classes,
                                                         height_above_ground_threshold=height_above_ground_threshold,
                                                         DTM_file=DTM_file, ground_ID=np.nan, set_mesh_texture=False,
                                                         points_in_raster_CRS=points_in_raster_CRS)

    if predicted_face_classes_savefile is not None:
        Path(predicted_face_classes_savefile).parent.mkdir(parents=True, exist_ok=True)
        np.save(predicted_face_classes_savefile, predicted_face_classes)

    if full_mesh_face_classes_savefile is not None:   # the same classes on the faces of the mesh before the decimation
        full_kwargs = {k: v for k, v in roi_kwargs.items() if k not in ("downsample_target", "downsample_method")}
        full_mesh = MeshClass(mesh_file, input_CRS=mesh_CRS, IDs_to_labels=IDs_to_labels, backend=mesh.backend, **full_kwargs)
        full_classes = full_mesh.values_from_mesh(mesh, predicted_face_classes, on="faces", max_distance=transfer_max_distance_meters)
        mesh.last_transfer_stats = full_mesh.last_transfer_stats
        Path(full_mesh_face_classes_savefile).parent.mkdir(parents=True, exist_ok=True)
        np.save(full_mesh_face_classes_savefile, np.asarray(full_classes, dtype=np.float64).reshape(-1, 1))

    if vis_folder is not None:   # ... and the one at aggregate_images.py:214: the class per face, behind the ground step
        mesh.vis(screenshot_filename=Path(vis_folder, "predicted_classes.png"), vis_scalars=predicted_face_classes)

    if top_down_vector_projection_savefile is not None:   # reference: aggregate_images.py:216-231, behind the ground step
        points_in_export_CRS = top_down_points
        if kept_point_IDs is not None and not is_CRS_designator(points_in_export_CRS):
            points_in_export_CRS = points_in_export_CRS[kept_point_IDs]
        IDs = mesh.get_IDs_to_labels()
        label_names = None if IDs is None else [IDs.get(i, None) for i in range(max(list(IDs.keys())) + 1)]
        mesh.export_face_labels_vector(face_labels=np.squeeze(predicted_face_classes, axis=1),
                                       export_file=top_down_vector_projection_savefile, label_names=label_names,
                                       points_in_export_CRS=points_in_export_CRS, simplify_tol=top_down_simplify_tol,
                                       simplify_method=top_down_simplify_method)
    if top_down_raster_projection_savefile is not None:   # beside the vector map: the same classes, the upper surface wins
        points_in_raster_CRS = top_down_points
        if kept_point_IDs is not None and not is_CRS_designator(points_in_raster_CRS):
            points_in_raster_CRS = points_in_raster_CRS[kept_point_IDs]
        Path(top_down_raster_projection_savefile).parent.mkdir(parents=True, exist_ok=True)
        mesh.export_face_labels_raster(face_labels=np.squeeze(predicted_face_classes, axis=1),
                                       export_file=top_down_raster_projection_savefile,
                                       resolution=float(top_down_raster_resolution), points_in_raster_CRS=points_in_raster_CRS)
    return mesh, aggregated_face_labels, predicted_face_classes


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Aggregate predictions from individual images onto the mesh.",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--mesh-file", type=Path, required=True, help="Mesh as .npz (points, faces)")
    parser.add_argument("--cameras-file", type=Path, required=True, help="Metashape XML with camera calibrations and positions")
    parser.add_argument("--image-folder", type=Path, required=True, help="Folder of the images the mesh was made from")
    parser.add_argument("--label-folder", type=Path, required=True, help="Folder of index images, laid out like --image-folder")
    parser.add_argument("--mesh-CRS", required=True, help="CRS of the mesh vertices (EPSG:4978)")
    parser.add_argument("--original-image-folder", type=Path,
                        help="Removed from the beginning of the absolute image paths stored in --cameras-file")
    parser.add_argument("--subset-images-folder", type=Path, help="Use only the images under this folder")
    parser.add_argument("--filename-regex", help="Use only the images whose path matches this expression")
    parser.add_argument("--take-every-nth-camera", type=int, help="Use only every nth camera")
    parser.add_argument("--DTM-file", type=Path, help="Single-band GeoTIFF of the terrain: faces near it lose their class")
    parser.add_argument("--DTM-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 3) in the CRS of --DTM-file (required with it)")
    parser.add_argument("--DTM-CRS", help="CRS of --DTM-file (e.g. EPSG:32610) instead of --DTM-points-file: the vertices are "
                        "reprojected on the device")
    parser.add_argument("--height-above-ground-threshold", type=float, default=2.0, help="Only applies with --DTM-file")
    parser.add_argument("--ROI", help=".geojson of the region of interest; needs --ROI-points-file")
    parser.add_argument("--ROI-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 2) or (V, 3) in the CRS of --ROI (required with it)")
    parser.add_argument("--ROI-camera-points-file", type=Path,
                        help=".npy with the camera positions in the CRS of --ROI; without it the camera set is not cut")
    parser.add_argument("--ROI-CRS", help="CRS of --ROI instead of --ROI-points-file")
    parser.add_argument("--ROI-camera-CRS", help="CRS of --ROI instead of --ROI-camera-points-file: the camera set is cut to the ROI")
    parser.add_argument("--ROI-buffer-radius-meters", default=50, type=float, help="Only applies with --ROI")
    parser.add_argument("--IDs-to-labels", type=Path, required=True, help="JSON file {ID: label}")
    parser.add_argument("--mesh-downsample", type=float, default=1.0,
                        help="Fraction of the mesh vertices to keep, in (0, 1]; anything but 1 needs --mesh-downsample-method")
    parser.add_argument("--mesh-downsample-method", choices=["cluster"],
                        help="How --mesh-downsample decimates: cluster = vertex clustering on a uniform grid, on the device (not "
                        "the quadric decimation of the reference, which is not available here)")
    parser.add_argument("--aggregate-image-scale", type=float, default=0.25, help="Aggregate at this fraction of the image size")
    parser.add_argument("--n-aggregation-clusters", type=int, help="Selects the chunked mesh class, as in the reference")
    parser.add_argument("--aggregated-face-values-savefile", type=Path, help="Where the (F, classes) values are saved (.npy)")
    parser.add_argument("--predicted-face-classes-savefile", type=Path, help="Where the (F, 1) classes are saved (.npy)")
    parser.add_argument("--top-down-vector-projection-savefile",
                        help="Where the top-down map of the classes is saved (.geojson); needs --top-down-points-file")
    parser.add_argument("--top-down-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 2) or (V, 3) in the planar CRS of the map (required with it)")
    parser.add_argument("--top-down-CRS", help="Planar CRS of the map instead of --top-down-points-file")
    parser.add_argument("--top-down-simplify-tol", type=float, default=0.0,
                        help="Simplify the rings of the top-down map at this tolerance in metres; needs --top-down-simplify-method")
    parser.add_argument("--top-down-simplify-method", choices=["douglas-peucker"],
                        help="How --top-down-simplify-tol simplifies: douglas-peucker = the exact Douglas-Peucker on the 1e-6 m "
                        "grid, on the device, with the borders two classes share kept identical")
    parser.add_argument("--top-down-raster-projection-savefile", type=Path,
                        help="Where the top-down class raster is saved (.tif): per cell the class of the surface seen from above; "
                        "needs --top-down-raster-resolution and --top-down-points-file (V, 3) or --top-down-CRS")
    parser.add_argument("--top-down-raster-resolution", type=float,
                        help="Cell size of --top-down-raster-projection-savefile in map units")
    parser.add_argument("--sieve-min-area-m2", type=float,
                        help="Sieve the class per face: connected regions of one class below this surface area join their greatest "
                        "neighbour region, on the device")
    parser.add_argument("--sieve-min-faces", type=int, help="... below this number of faces instead (one of the two at most)")
    parser.add_argument("--sieve-fill-unseen", action="store_true",
                        help="The sieve also fills small regions of unseen faces; needs one of the two thresholds")
    parser.add_argument("--full-mesh-face-classes-savefile", type=Path,
                        help="With --mesh-downsample-method: where the (F, 1) classes on the faces of the mesh before the decimation are "
                        "saved (.npy), each face taking the class of the decimated face with the nearest centre, on the device")
    parser.add_argument("--transfer-max-distance-meters", type=float,
                        help="Faces of the full mesh with no decimated face centre within this distance stay unlabelled (NaN)")
    parser.add_argument("--vis", action="store_true", help="Not available here")
    parser.add_argument("--vis-folder", type=Path,
                        help="Write mesh_and_cameras.png and predicted_classes.png (each with its .legend.json) here: the two pictures "
                             "the reference shows in a window, rendered off-screen on the device")
    args = parser.parse_args(argv)
    args.IDs_to_labels = str(args.IDs_to_labels)
    return args


def main(argv=None):
    args = parse_args(argv)
    aggregate_images(**vars(args))


if __name__ == "__main__":
    main()
