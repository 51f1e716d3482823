"""Render height masks made from a mesh and a digital terrain model (DTM), one per camera.  Two modes:

- threshold: a discrete mask, 0 = no height (the DTM has no data there or does not reach), 1 = at most `threshold_cutoff` above the
  DTM, 2 = higher; uint8 `.tif` files.
- raw: the height of the visible face above the DTM in every pixel; float64 `.npy` files, NaN where no face is visible.

Mirror of geograypher/entrypoints/render_height_masks.py in the formats this package reads: the mesh as `.npz` (points, faces;
EPSG:4978), the cameras as a Metashape XML, the DTM as a single-band GeoTIFF or a `PlanarRaster`.  The height of every face centre
is taken on the device (`TexturedPhotogrammetryMesh.get_height_above_ground`), which needs `points_file`: a `.npy` with the mesh
vertices (V, 3) in the DTM's CRS (the reference reprojects them with pyproj).  Not carried over: the visualisations (pyvista,
matplotlib)."""
import argparse
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.constants import PATH_TYPE


def render_height_masks(
    image_folder: PATH_TYPE,
    camera_file: PATH_TYPE,
    mesh_file,
    dtm_file,
    mesh_CRS,
    original_image_folder: typing.Optional[PATH_TYPE],
    output_folder: PATH_TYPE,
    output_mode: str,
    threshold_cutoff: float,
    vis_folder: typing.Optional[PATH_TYPE] = None,
    vis_n_images: int = 10,
    points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    apply_distortion: bool = True,
    camera_set=None,
    backend=None,
    points_CRS=None,
):
    """Render the height of the mesh above `dtm_file` into every camera's view (see the module docstring).  The reference's
    arguments; `vis_folder` raises NotImplementedError, an unknown `output_mode` ValueError.  Beyond the reference: `points_file`
    (a `.npy` path or the array itself) or `points_CRS` (the CRS of `dtm_file`, e.g. "EPSG:32610": the vertices are reprojected on
    the device), one of them required and both a ValueError, `apply_distortion` (False for a camera set without a lens model), and
    `camera_set` and `backend`, which replace the objects built from `camera_file` and the device.  Returns the mesh textured with
    what was rendered."""
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils.geospatial import points_or_CRS

    if vis_folder is not None:
        raise NotImplementedError("vis_folder: visualisations need pyvista and matplotlib, which are outside the projection path")
    if output_mode not in ("threshold", "raw"):
        raise ValueError(f"Unknown mode: {output_mode}")

    points_in_raster_CRS = points_or_CRS("points_file", points_file, "points_CRS", points_CRS)
    mesh = TexturedPhotogrammetryMesh(mesh_file, input_CRS=mesh_CRS, backend=backend)
    # faces outside the DTM, or over its nodata cells, have a height of NaN
    height = mesh.get_height_above_ground(DTM_file=dtm_file, points_in_raster_CRS=points_in_raster_CRS)

    if output_mode == "threshold":
        texture = np.zeros(len(height), dtype=float)
        texture[(~np.isnan(height)) & (height <= threshold_cutoff)] = 1
        texture[(~np.isnan(height)) & (height > threshold_cutoff)] = 2
        cast_to_uint8, save_as_npy = True, False
    else:
        texture = height
        cast_to_uint8, save_as_npy = False, True
    mesh.set_texture(texture.reshape(-1, 1), is_vertex_texture=False)

    if camera_set is None:
        from geograypher_amd.cameras.derived_cameras import MetashapeCameraSet

        camera_set = MetashapeCameraSet(camera_file, image_folder, original_image_folder=original_image_folder)

    render_kwargs = {} if apply_distortion else {"apply_distortion": False}
    mesh.save_renders(camera_set, output_folder=output_folder, save_native_resolution=True, cast_to_uint8=cast_to_uint8,
                      save_as_npy=save_as_npy, **render_kwargs)
    return mesh


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--image-folder", type=Path, required=True, help="Folder of the images the cameras were made from")
    parser.add_argument("--camera-file", type=Path, required=True, help="Metashape XML with camera calibrations and positions")
    parser.add_argument("--mesh-file", type=Path, required=True, help="Mesh as .npz (points, faces)")
    parser.add_argument("--dtm-file", type=Path, required=True, help="Digital terrain model: a single-band GeoTIFF")
    parser.add_argument("--points-file", type=Path, help=".npy with the mesh vertices (V, 3) in the CRS of --dtm-file")
    parser.add_argument("--points-CRS", help="CRS of --dtm-file (e.g. EPSG:32610) instead of --points-file: the vertices are "
                        "reprojected on the device")
    parser.add_argument("--mesh-crs", required=True, help="CRS of the mesh vertices (EPSG:4978)")
    parser.add_argument("--original-image-folder", type=Path,
                        help="Removed from the beginning of the absolute image paths stored in --camera-file")
    parser.add_argument("--output-folder", type=Path, required=True, help="Where the rendered masks are written")
    parser.add_argument("--output-mode", choices=["threshold", "raw"], default="raw",
                        help="'threshold': 0 = invalid, 1 = below the cutoff, 2 = above it; 'raw': the height values")
    parser.add_argument("--threshold-cutoff", type=float, default=1.0, help="Height (m) that separates ground from above ground")
    parser.add_argument("--vis-folder", type=Path, help="Not available here")
    parser.add_argument("--vis-n-images", type=int, default=10, help="Only applies with --vis-folder")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    render_height_masks(image_folder=args.image_folder, camera_file=args.camera_file, mesh_file=args.mesh_file,
                        dtm_file=args.dtm_file, mesh_CRS=args.mesh_crs, original_image_folder=args.original_image_folder,
                        output_folder=args.output_folder, output_mode=args.output_mode, threshold_cutoff=args.threshold_cutoff,
                        vis_folder=args.vis_folder, vis_n_images=args.vis_n_images, points_file=args.points_file, points_CRS=args.points_CRS)


if __name__ == "__main__":
    main()
