"""Render image-based labels from geospatial ground truth: polygons (species, crown ids) -> a label per mesh face -> a label image
per camera.

Mirror of geograypher/entrypoints/render_labels.py:21-204 in the formats this package reads: the mesh as `.npz` (points, faces;
EPSG:4978), the cameras as a Metashape XML, the texture as an array, a `.npy` file or a `.geojson` of Polygon / MultiPolygon
features in a planar CRS.  A vector texture also needs `texture_points_file`: a `.npy` with the mesh vertices (V, 3) in the
polygons' CRS (the reference reprojects them with pyproj).  Every face takes the value of the highest feature that holds its centre
(`TexturedPhotogrammetryMesh.get_values_for_faces_from_vector`, on the device); `save_renders` writes one label image per camera under
`render_savefolder`, at the cameras' paths relative to `image_folder`, and `IDs_to_labels.json` beside them.  With `DTM_file` (a
single-band GeoTIFF or a `PlanarRaster`) and `ground_height_threshold`, labelled faces lower than the threshold above the DTM are
relabelled before rendering (`label_ground_class`, on the device): to a new class "GROUND" with `render_ground_class`, else to NaN;
this needs `DTM_points_file`, the vertices in the DTM's CRS.  With `ROI` (a `.geojson`, a `PlanarPolygons` or ring arrays) and
`ROI_points_file`, the vertices in the ROI's CRS, the mesh is cropped to the ROI grown by `mesh_ROI_buffer_radius_meters` before
anything else (`select_mesh_ROI`, on the device); the camera set is cut to `cameras_ROI_buffer_radius_meters` when
`ROI_camera_points_file` gives the camera positions in the same CRS.  With `mesh_downsample` and `mesh_downsample_method="cluster"`
the mesh is then decimated by vertex clustering (`TexturedPhotogrammetryMesh.decimate`, on the device).  Not carried over: the
reference's quadric decimation, saving the image subset or the textured mesh, and the visualisations (geopandas, pyvista, matplotlib)."""
import argparse
import json
import typing
from math import ceil
from pathlib import Path

import numpy as np

from geograypher_amd.constants import PATH_TYPE


def render_labels(
    mesh_file,
    cameras_file: PATH_TYPE,
    image_folder: PATH_TYPE,
    texture: typing.Union[PATH_TYPE, np.ndarray, None],
    render_savefolder: PATH_TYPE,
    mesh_CRS,
    original_image_folder: typing.Union[PATH_TYPE, None] = None,
    subset_images_savefolder: typing.Union[PATH_TYPE, None] = None,
    texture_column_name: typing.Union[str, None] = None,
    DTM_file: typing.Union[PATH_TYPE, None] = None,
    ground_height_threshold: typing.Union[float, None] = None,
    render_ground_class: bool = False,
    textured_mesh_savefile: typing.Union[PATH_TYPE, None] = None,
    ROI=None,
    mesh_ROI_buffer_radius_meters: float = 50,
    cameras_ROI_buffer_radius_meters: float = 150,
    IDs_to_labels: typing.Union[dict, None] = None,
    render_image_scale: float = 1,
    mesh_downsample: float = 1,
    n_cameras_per_chunk: typing.Union[int, None] = None,
    cast_to_uint8: bool = True,
    save_as_npy: bool = False,
    vis: bool = False,
    mesh_vis_file: typing.Union[PATH_TYPE, None] = None,
    labels_vis_folder: typing.Union[PATH_TYPE, None] = None,
    texture_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    apply_distortion: bool = True,
    camera_set=None,
    backend=None,
    DTM_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    ROI_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    ROI_camera_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    texture_CRS=None,
    DTM_CRS=None,
    ROI_CRS=None,
    ROI_camera_CRS=None,
    mesh_downsample_method: typing.Union[str, None] = None,
):
    """Render the labels of `texture` into every camera's view (see the module docstring for inputs and files).  The reference's
    arguments and defaults; `DTM_file` without `DTM_points_file`, `ROI` without `ROI_points_file`, `mesh_downsample != 1` without `mesh_downsample_method`, `subset_images_savefolder`, `textured_mesh_savefile`, `vis`,
    `mesh_vis_file` and `labels_vis_folder` raise NotImplementedError.  `n_cameras_per_chunk` selects
    `TexturedPhotogrammetryMeshChunked` with ceil(cameras / n_cameras_per_chunk) clusters, as in the reference (the GPU path
    renders the whole mesh either way).  Beyond the reference: `texture_points_file` (a `.npy` path or the array itself, required
    for a vector texture), `DTM_points_file` (likewise, the vertices in the DTM's CRS, required with `DTM_file`), `apply_distortion` (False for a camera set without a lens model), and `camera_set` and `backend`,
    which replace the objects built from `cameras_file` and the device; `ROI_points_file` (the V original vertices in the ROI's CRS,
    required with `ROI`) and `ROI_camera_points_file` (the camera positions in that CRS; without it the camera set is not cut, with a
    log line).  `texture_points_file` and `DTM_points_file` are given for the ORIGINAL mesh and indexed by the kept vertices.  Each
    `*_points_file` has a sibling `texture_CRS`, `DTM_CRS`, `ROI_CRS`, `ROI_camera_CRS`: the CRS of the texture / DTM / ROI (e.g.
    "EPSG:32610") in place of the points, which are then reprojected on the device; giving both is a ValueError.
    `mesh_downsample_method="cluster"` decimates the mesh to about `mesh_downsample` of its vertices behind the ROI crop
    (`TexturedPhotogrammetryMesh.decimate`: vertex clustering, not the reference's quadric decimation); the `*_points_file` arrays
    and a texture array stay those of the ORIGINAL mesh.  Returns the textured mesh."""
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh, TexturedPhotogrammetryMeshChunked
    from geograypher_amd.utils.geospatial import is_CRS_designator, points_or_CRS

    texture_points = points_or_CRS("texture_points_file", texture_points_file, "texture_CRS", texture_CRS)
    DTM_points = points_or_CRS("DTM_points_file", DTM_points_file, "DTM_CRS", DTM_CRS)
    ROI_points = points_or_CRS("ROI_points_file", ROI_points_file, "ROI_CRS", ROI_CRS)
    ROI_camera_points = points_or_CRS("ROI_camera_points_file", ROI_camera_points_file, "ROI_camera_CRS", ROI_camera_CRS)

    for name, value, why in (
        ("DTM_file", DTM_file if DTM_points is None else None,
         "the vertices in the DTM's CRS are needed (DTM_points_file); reprojecting them needs pyproj"),
        ("ROI", ROI if ROI_points is None else None,
         "the vertices in the ROI's CRS are needed (ROI_points_file); reprojecting them needs pyproj"),
        ("subset_images_savefolder", subset_images_savefolder, "copying the image subset is not part of this package"),
        ("textured_mesh_savefile", textured_mesh_savefile, "mesh writers (pyvista) are not part of this package"),
        ("mesh_vis_file", mesh_vis_file, "visualisations need pyvista"),
        ("labels_vis_folder", labels_vis_folder, "visualisations need matplotlib"),
    ):
        if value is not None:
            raise NotImplementedError(f"{name}: {why}, which is outside the projection path")
    if vis:
        raise NotImplementedError("vis: visualisations need pyvista, which is outside the projection path")
    if mesh_downsample != 1 and mesh_downsample_method is None:
        raise NotImplementedError("mesh_downsample: mesh decimation is outside the projection path (meshes.py:215-226)")

    if camera_set is None:
        from geograypher_amd.cameras.derived_cameras import MetashapeCameraSet

        camera_set = MetashapeCameraSet(cameras_file, image_folder, original_image_folder=original_image_folder)

    MeshClass = TexturedPhotogrammetryMesh if n_cameras_per_chunk is None else TexturedPhotogrammetryMeshChunked

    roi_kwargs = {}
    if ROI is not None:   # reference: render_labels.py:120-131 (cameras), 141-149 (mesh)
        roi_kwargs = {"ROI": ROI, "ROI_buffer_meters": mesh_ROI_buffer_radius_meters, "points_in_ROI_CRS": ROI_points}
    if mesh_downsample_method is not None:   # behind the crop, before the texture (render_labels.py:141-149)
        roi_kwargs.update(downsample_target=mesh_downsample, downsample_method=mesh_downsample_method)
    mesh = MeshClass(mesh_file, input_CRS=mesh_CRS, IDs_to_labels=IDs_to_labels, backend=backend, **roi_kwargs)
    if ROI is not None:
        if ROI_camera_points is not None:
            camera_set = camera_set.get_subset_ROI(ROI=ROI, buffer_radius=cameras_ROI_buffer_radius_meters, is_geospatial=True,
                                                   points_in_ROI_CRS=ROI_camera_points, backend=mesh.backend)
        else:
            mesh.logger.info("ROI without ROI_camera_points_file: the camera set is not cut to the ROI")
    n_render_chunks = None if n_cameras_per_chunk is None else int(ceil(len(camera_set) / n_cameras_per_chunk))

    def kept(points):   # the rows of the vertices the ROI and the decimation kept (a CRS names the points of the current mesh already)
        if points is None or mesh.original_point_IDs() is None or is_CRS_designator(points):
            return points
        return np.asarray(points)[mesh.original_point_IDs()]

    points_in_polygon_CRS = kept(texture_points)
    if isinstance(texture, np.ndarray):   # an array for the original mesh is cut like the mesh
        texture = mesh.to_current_mesh(texture)
    mesh.load_texture(texture, texture_column_name=texture_column_name, IDs_to_labels=mesh.IDs_to_labels,
                      points_in_polygon_CRS=points_in_polygon_CRS)

    if DTM_file is not None and ground_height_threshold is not None:   # reference: render_labels.py:161-171
        points_in_raster_CRS = kept(DTM_points)
        mesh.label_ground_class(DTM_file=DTM_file, height_above_ground_threshold=ground_height_threshold,
                                only_label_existing_labels=True, ground_class_name="GROUND",
                                ground_ID=None if render_ground_class else np.nan, set_mesh_texture=True,
                                points_in_raster_CRS=points_in_raster_CRS)

    render_kwargs = {} if n_render_chunks is None else {"n_clusters": n_render_chunks}
    if not apply_distortion:
        render_kwargs["apply_distortion"] = False
    mesh.save_renders(camera_set=camera_set, render_image_scale=render_image_scale, save_native_resolution=True,
                      output_folder=render_savefolder, make_composites=False, cast_to_uint8=cast_to_uint8,
                      save_as_npy=save_as_npy, **render_kwargs)
    return mesh


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Render labels onto individual images using geospatial textures.",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--mesh-file", type=Path, required=True, help="Mesh as .npz (points, faces)")
    parser.add_argument("--mesh-CRS", required=True, help="CRS of the mesh vertices (EPSG:4978)")
    parser.add_argument("--cameras-file", type=Path, required=True, help="Metashape XML with camera calibrations and positions")
    parser.add_argument("--image-folder", type=Path, required=True, help="Folder of the images the mesh was made from")
    parser.add_argument("--texture", type=Path, required=True, help="Texture: a .npy array or a .geojson of polygons")
    parser.add_argument("--render-savefolder", type=Path, required=True, help="Where the rendered labels are written")
    parser.add_argument("--texture-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 3) in the CRS of a .geojson --texture (required for one)")
    parser.add_argument("--texture-CRS", help="CRS of a .geojson --texture (e.g. EPSG:32610) instead of --texture-points-file: the "
                        "vertices are reprojected on the device")
    parser.add_argument("--original-image-folder", type=Path,
                        help="Removed from the beginning of the absolute image paths stored in --cameras-file")
    parser.add_argument("--subset-images-savefolder", type=Path, help="Not available here")
    parser.add_argument("--texture-column-name", help="Property of the .geojson features to use as the label")
    parser.add_argument("--DTM-file", type=Path, help="Single-band GeoTIFF of the terrain: labelled faces near it are relabelled")
    parser.add_argument("--DTM-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 3) in the CRS of --DTM-file (required with it)")
    parser.add_argument("--DTM-CRS", help="CRS of --DTM-file instead of --DTM-points-file")
    parser.add_argument("--ground-height-threshold", type=float, default=2.0,
                        help="Faces lower than this above the DTM are ground; only applies with --DTM-file")
    parser.add_argument("--render-ground-class", action="store_true",
                        help="Render ground as a class GROUND of its own instead of unlabelled; only applies with --DTM-file")
    parser.add_argument("--textured-mesh-savefile", help="Not available here")
    parser.add_argument("--ROI", help=".geojson of the region of interest; needs --ROI-points-file")
    parser.add_argument("--ROI-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 2) or (V, 3) in the CRS of --ROI (required with it)")
    parser.add_argument("--ROI-camera-points-file", type=Path,
                        help=".npy with the camera positions in the CRS of --ROI; without it the camera set is not cut")
    parser.add_argument("--ROI-CRS", help="CRS of --ROI instead of --ROI-points-file")
    parser.add_argument("--ROI-camera-CRS", help="CRS of --ROI instead of --ROI-camera-points-file: the camera set is cut to the ROI")
    parser.add_argument("--mesh-ROI-buffer-radius-meters", default=50, type=float, help="Only applies with --ROI")
    parser.add_argument("--cameras-ROI-buffer-radius-meters", default=100, type=float, help="Only applies with --ROI")
    parser.add_argument("--render-image-scale", type=float, default=1, help="Render at this fraction of the image size")
    parser.add_argument("--mesh-downsample", type=float, default=1,
                        help="Fraction of the mesh vertices to keep, in (0, 1]; anything but 1 needs --mesh-downsample-method")
    parser.add_argument("--mesh-downsample-method", choices=["cluster"],
                        help="How --mesh-downsample decimates: cluster = vertex clustering on a uniform grid, on the device (not "
                        "the quadric decimation of the reference, which is not available here)")
    parser.add_argument("--IDs-to-labels", type=Path, help="JSON file {ID: label}")
    parser.add_argument("--n-cameras-per-chunk", type=int, help="Selects the chunked mesh class, as in the reference")
    parser.add_argument("--cast-to-uint8", action="store_true", help="Write uint8 labels (else uint16 / uint32)")
    parser.add_argument("--save-as-npy", action="store_true", help="Write float64 .npy files instead of .tif")
    parser.add_argument("--vis", action="store_true", help="Not available here")
    parser.add_argument("--mesh-vis-file", type=Path, help="Not available here")
    parser.add_argument("--labels-vis-folder", type=Path, help="Not available here")
    args = parser.parse_args(argv)
    if args.IDs_to_labels is not None:
        with open(args.IDs_to_labels, "r") as file:
            args.IDs_to_labels = {int(k): v for k, v in json.load(file).items()}
    return args


def main(argv=None):
    args = parse_args(argv)
    render_labels(**vars(args))


if __name__ == "__main__":
    main()
