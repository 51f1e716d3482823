"""Choose a small set of images that together see the whole mesh: the images a person should annotate.

Mirror of geograypher/entrypoints/annotation_image_selection.py:17-240 in the formats this package reads: the mesh as `.npz`
(points, faces; EPSG:4978), the cameras as a Metashape XML.  Three stages that can be run together or one at a time, handing
over through files as in the reference:

* `compute_projection`: every view is labelled with its own index (`ImageIDSegmentor`) and aggregated onto the mesh
  (`TexturedPhotogrammetryMeshIndexPredictions.aggregate_projected_images`); the (faces, views) visibility matrix is written with
  scipy's `save_npz`.  With `ROI` the mesh is cropped to the ROI grown by `ROI_buffer_meters` (`select_mesh_ROI`, on the device),
  which needs `ROI_points_file`, the vertices in the ROI's CRS, and the camera set is cut to it where `ROI_camera_points_file`
  gives the camera positions in that CRS.
* `compute_minimal_set`: the set cover over that matrix, on the device (`select_covering_views`; the reference runs SetCoverPy on
  the dense matrix).  The rule-set is DESIGN.md section 8j: greedy by the number of newly seen faces, ties to the lowest view,
  then redundant views pruned; deterministic.  The (views,) bool mask is written with `np.save`.
* `save_selected_images`: the images of the mask are linked into `selected_images_save_folder` (`save_images`).

With `downsample_target` and `downsample_method="cluster"` the mesh of `compute_projection` is decimated by vertex clustering behind
the crop (`TexturedPhotogrammetryMesh.decimate`, on the device).  Not carried over: the reference's quadric decimation and the
visualisations."""
import argparse
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.constants import PATH_TYPE


def determine_minimum_overlapping_images(
    mesh_file,
    cameras_file: PATH_TYPE,
    mesh_CRS,
    image_folder: PATH_TYPE = "",
    ROI=None,
    ROI_buffer_meters: float = 0.0,
    compute_projection: bool = False,
    compute_minimal_set: bool = False,
    save_selected_images: bool = False,
    projections_filename: typing.Union[PATH_TYPE, None] = None,
    selected_images_mask_filename: typing.Union[PATH_TYPE, None] = None,
    selected_images_save_folder: typing.Union[PATH_TYPE, None] = None,
    downsample_target: float = 1,
    min_observations_to_be_included: float = 1,
    vis: bool = False,
    ROI_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    ROI_camera_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    camera_set=None,
    backend=None,
    ROI_CRS=None,
    ROI_camera_CRS=None,
    downsample_method: typing.Union[str, None] = None,
):
    """Determine a subset of images that together observe the entire scene (see the module docstring).  The reference's arguments
    and defaults; `downsample_target != 1` without `downsample_method`, `vis` and `ROI` without `ROI_points_file` raise NotImplementedError.  Beyond the
    reference: `ROI_points_file` (a `.npy` path or array: the V ORIGINAL vertices in the ROI's CRS), `ROI_camera_points_file` (the
    positions of the cameras in that CRS; without it the camera set is not cut to the ROI, with a log line), and `camera_set`
    and `backend`, which replace the objects built from `cameras_file` and the device; `ROI_CRS` and `ROI_camera_CRS`: the CRS of
    the ROI (e.g. "EPSG:32610") in place of the two points files -- the vertices and camera positions are then reprojected on the
    device --, giving a file and its CRS sibling is a ValueError.  `downsample_method="cluster"` decimates the
    mesh of `compute_projection` to about `downsample_target` of its vertices behind the ROI crop (`TexturedPhotogrammetryMesh.decimate`:
    vertex clustering, not the reference's quadric decimation).  `min_observations_to_be_included`: a
    selected set need only see the faces that at least this many cameras see.  Returns a dict with what the stages that ran
    produced: "summed_projections", "selected_images" (the mask), "selection" (the record of `select_covering_views`),
    "subset_camera_set"."""
    from geograypher_amd.utils.geospatial import points_or_CRS

    ROI_points = points_or_CRS("ROI_points_file", ROI_points_file, "ROI_CRS", ROI_CRS)
    ROI_camera_points = points_or_CRS("ROI_camera_points_file", ROI_camera_points_file, "ROI_camera_CRS", ROI_camera_CRS)
    if ROI is not None and ROI_points is None:
        raise NotImplementedError("ROI: the vertices in the ROI's CRS are needed (ROI_points_file); reprojecting them needs pyproj, "
                                  "which is outside the projection path")
    if vis:
        raise NotImplementedError("vis: visualisations need pyvista, which is outside the projection path")
    if downsample_target != 1 and downsample_method is None:
        raise NotImplementedError("downsample_target: mesh decimation is outside the projection path (meshes.py:215-226)")
    if isinstance(mesh_CRS, int) or (isinstance(mesh_CRS, str) and mesh_CRS.isdigit()):
        mesh_CRS = f"EPSG:{int(mesh_CRS)}"   # the reference's --mesh-CRS is an EPSG code

    def load_cameras(roi_backend):
        """The camera set, cut to the ROI (annotation_image_selection.py:89-94, 178-183)."""
        cameras = camera_set
        if cameras is None:
            from geograypher_amd.cameras.derived_cameras import MetashapeCameraSet

            cameras = MetashapeCameraSet(cameras_file, image_folder)
        if ROI is not None:
            if ROI_camera_points is not None:
                cameras = cameras.get_subset_ROI(ROI=ROI, buffer_radius=ROI_buffer_meters, is_geospatial=True,
                                                 points_in_ROI_CRS=ROI_camera_points, backend=roi_backend)
            else:
                import logging

                logging.getLogger(__name__).info("ROI without ROI_camera_points_file: the camera set is not cut to the ROI")
        return cameras

    result = {}
    if compute_projection:
        from scipy.sparse import csr_matrix, save_npz

        from geograypher_amd.cameras.segmentor import SegmentorPhotogrammetryCameraSet
        from geograypher_amd.meshes import TexturedPhotogrammetryMeshIndexPredictions
        from geograypher_amd.predictors.derived_segmentors import ImageIDSegmentor

        roi_kwargs = {}
        if ROI is not None:
            roi_kwargs = {"ROI": ROI, "ROI_buffer_meters": ROI_buffer_meters, "points_in_ROI_CRS": ROI_points}
        if downsample_method is not None:   # behind the crop (annotation_image_selection.py:96-104)
            roi_kwargs.update(downsample_target=downsample_target, downsample_method=downsample_method)
        mesh = TexturedPhotogrammetryMeshIndexPredictions(mesh_file, input_CRS=mesh_CRS, backend=backend, **roi_kwargs)
        cameras = load_cameras(mesh.backend)
        segmentor = ImageIDSegmentor(image_filenames=cameras.get_image_filename(index=None, absolute=True))
        segmentor_camera_set = SegmentorPhotogrammetryCameraSet(base_camera_set=cameras, segmentor=segmentor)
        _, additional_info = mesh.aggregate_projected_images(cameras=segmentor_camera_set, n_classes=len(cameras))
        summed_projections = additional_info["summed_projections"]
        Path(projections_filename).parent.mkdir(parents=True, exist_ok=True)
        save_npz(projections_filename, csr_matrix(summed_projections))
        result["summed_projections"] = summed_projections
        backend = mesh.backend

    if compute_minimal_set:
        from scipy.sparse import load_npz

        from geograypher_amd.utils.numeric import select_covering_views

        projection_matrix = load_npz(projections_filename)
        record = select_covering_views(projection_matrix, min_observations_to_be_included=min_observations_to_be_included,
                                       backend=backend)
        print(f"{int(record['selected'].sum())} of {projection_matrix.shape[1]} images see the {record['n_required']} faces that at "
              f"least {min_observations_to_be_included} image(s) see")
        Path(selected_images_mask_filename).parent.mkdir(parents=True, exist_ok=True)
        np.save(selected_images_mask_filename, record["selected"])
        result["selected_images"] = record["selected"]
        result["selection"] = record

    if save_selected_images:
        cameras = load_cameras(backend)
        cameras_mask = np.load(selected_images_mask_filename)
        subset_cameras_set = cameras.get_subset_cameras([int(i) for i in np.where(cameras_mask)[0]])
        subset_cameras_set.save_images(output_folder=selected_images_save_folder)
        result["subset_camera_set"] = subset_cameras_set
    return result


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Determine a minimum set of images that fully observe the mesh.",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--mesh-file", required=True, help="Mesh as .npz (points, faces)")
    parser.add_argument("--cameras-file", required=True, help="Metashape XML with camera calibrations and positions")
    parser.add_argument("--mesh-CRS", required=True, help="CRS of the mesh vertices: EPSG:4978, or the code alone")
    parser.add_argument("--image-folder", required=True, help="Folder of the images the mesh was made from")
    parser.add_argument("--ROI", help=".geojson of the region of interest; needs --ROI-points-file")
    parser.add_argument("--ROI-points-file", type=Path,
                        help=".npy with the mesh vertices (V, 2) or (V, 3) in the CRS of --ROI (required with it)")
    parser.add_argument("--ROI-camera-points-file", type=Path,
                        help=".npy with the camera positions in the CRS of --ROI; without it the camera set is not cut")
    parser.add_argument("--ROI-CRS", help="CRS of --ROI (e.g. EPSG:32610) instead of --ROI-points-file: the vertices are reprojected "
                        "on the device")
    parser.add_argument("--ROI-camera-CRS", help="CRS of --ROI instead of --ROI-camera-points-file: the camera set is cut to the ROI")
    parser.add_argument("--ROI-buffer-meters", type=float, default=0.0, help="Only applies with --ROI")
    parser.add_argument("--compute-projection", action="store_true", help="Compute which images see which faces")
    parser.add_argument("--compute-minimal-set", action="store_true", help="Choose the images from --projections-filename")
    parser.add_argument("--save-selected-images", action="store_true",
                        help="Link the images of --selected-images-mask-filename into --selected-images-save-folder")
    parser.add_argument("--projections-filename", help="The (faces, views) visibility matrix (.npz, scipy sparse)")
    parser.add_argument("--selected-images-mask-filename", help="The (views,) bool mask of the chosen images (.npy)")
    parser.add_argument("--selected-images-save-folder", help="Where the chosen images are linked")
    parser.add_argument("--downsample-target", default=1.0, type=float,
                        help="Fraction of the mesh vertices to keep, in (0, 1]; anything but 1 needs --downsample-method")
    parser.add_argument("--downsample-method", choices=["cluster"],
                        help="How --downsample-target decimates: cluster = vertex clustering on a uniform grid, on the device (not "
                        "the quadric decimation of the reference, which is not available here)")
    parser.add_argument("--min-observations-to-be-included", default=1, type=float,
                        help="Only faces that at least this many images see must be seen by the chosen images")
    parser.add_argument("--vis", action="store_true", help="Not available here")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    determine_minimum_overlapping_images(**vars(args))


if __name__ == "__main__":
    main()
