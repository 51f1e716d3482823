"""A picture of a mesh and its camera set, written to a file.

Mirror of geograypher/entrypoints/visualize.py in the formats this package reads: the mesh as `.npz` (points, faces), the cameras as
a Metashape XML, the texture as `.npy`.  The reference opens a window on a graphical desktop; here the picture is rendered
off-screen on the device (`TexturedPhotogrammetryMesh.vis`) and `screenshot_filename` is required.  The legend goes beside the
picture as `<name>.legend.json`."""
import argparse
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.constants import PATH_TYPE


def visualize(
    mesh_file: PATH_TYPE,
    mesh_CRS,
    camera_file: typing.Optional[PATH_TYPE],
    screenshot_filename: PATH_TYPE,
    texture: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    texture_column_name: typing.Optional[str] = None,
    IDs_to_labels: typing.Union[PATH_TYPE, dict, None] = None,
    downsample_target: float = 1.0,
    ROI: typing.Optional[PATH_TYPE] = None,
    ROI_buffer_meters: float = 0.0,
    convert_texture_to_max_class: bool = False,
    window_size=(1024, 768),
    supersample: int = 2,
    azimuth_deg: typing.Optional[float] = None,
    elevation_deg: typing.Optional[float] = None,
    frustum_scale: float = 2,
    enable_ssao: bool = True,
    ROI_points_file: typing.Union[PATH_TYPE, np.ndarray, None] = None,
    ROI_CRS=None,
    camera_set=None,
    backend=None,
):
    """The reference's arguments (entrypoints/visualize.py:13-24) and a required `screenshot_filename`; `window_size`, `supersample`,
    `azimuth_deg`, `elevation_deg`, `frustum_scale` and `enable_ssao` are `TexturedPhotogrammetryMesh.vis`'s.  `ROI` needs the
    vertices in its CRS (`ROI_points_file`, a `.npy` path or an array) or the name of that CRS (`ROI_CRS`), as the mesh class does;
    the camera set is not cut to the ROI.  `convert_texture_to_max_class`: the `.npy` texture is an (F, classes) matrix of weights
    and the most common non-zero class per face is shown.  `camera_set` and `backend` replace the objects built from `camera_file`
    and the device.  -> the mesh."""
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh

    if isinstance(texture, (str, Path)) and (convert_texture_to_max_class or Path(texture).suffix == ".npy"):
        texture = np.load(texture)
    if camera_set is None and camera_file is not None:
        from geograypher_amd.cameras.derived_cameras import MetashapeCameraSet

        camera_set = MetashapeCameraSet(camera_file, "")
    roi_kwargs = {}
    if ROI is not None:
        if ROI_points_file is not None and ROI_CRS is not None:
            raise ValueError("ROI_points_file and ROI_CRS are both given")
        points = ROI_CRS if ROI_CRS is not None else ROI_points_file
        roi_kwargs = {"ROI": ROI, "ROI_buffer_meters": ROI_buffer_meters,
                      "points_in_ROI_CRS": np.load(points) if isinstance(points, (str, Path)) and ROI_CRS is None else points}
    mesh = TexturedPhotogrammetryMesh(mesh_file, input_CRS=mesh_CRS, IDs_to_labels=IDs_to_labels, backend=backend,
                                      downsample_target=downsample_target, **roi_kwargs)
    if convert_texture_to_max_class:
        classes = mesh.backend.argmax_nonzero(np.asarray(texture, dtype=np.float64))
        texture = np.asarray(classes.cpu() if hasattr(classes, "cpu") else classes, dtype=np.float64).reshape(-1, 1)
    if texture is not None:
        if texture_column_name is not None:
            raise NotImplementedError("texture_column_name: vector textures are loaded by load_texture(..., points_in_polygon_CRS=...)")
        mesh.set_texture(mesh.to_current_mesh(np.asarray(texture)))
    view = {k: v for k, v in (("azimuth_deg", azimuth_deg), ("elevation_deg", elevation_deg)) if v is not None}
    mesh.vis(camera_set=camera_set, screenshot_filename=screenshot_filename, frustum_scale=frustum_scale, enable_ssao=enable_ssao,
             view=view or None, window_size=window_size, supersample=supersample)
    return mesh


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--mesh-file", type=Path, required=True, help="Mesh as .npz (points, faces)")
    parser.add_argument("--mesh-CRS", required=True, help="CRS of the mesh vertices (EPSG:4978 or another WGS84 system)")
    parser.add_argument("--camera-file", type=Path, help="Metashape XML with camera calibrations and positions")
    parser.add_argument("--screenshot-filename", type=Path, required=True, help="Where the picture is written (.png)")
    parser.add_argument("--texture", type=Path, help="Per-face or per-vertex values as .npy")
    parser.add_argument("--texture-column-name", help="Not available here (vector textures)")
    parser.add_argument("--IDs-to-labels", type=Path, help="JSON file {ID: label}")
    parser.add_argument("--downsample-target", type=float, default=1.0, help="Not available here unless 1")
    parser.add_argument("--ROI", help=".geojson of the region of interest; needs --ROI-points-file or --ROI-CRS")
    parser.add_argument("--ROI-points-file", type=Path, help=".npy of the (V, 2) mesh vertices in the CRS of --ROI")
    parser.add_argument("--ROI-CRS", help="CRS of --ROI (e.g. EPSG:32610) instead of --ROI-points-file")
    parser.add_argument("--ROI-buffer-meters", type=float, default=0.0)
    parser.add_argument("--convert-texture-to-max-class", action="store_true",
                        help="--texture is an (F, classes) matrix: show the most common non-zero class per face")
    parser.add_argument("--window-size", type=int, nargs=2, default=(1024, 768), metavar=("WIDTH", "HEIGHT"))
    parser.add_argument("--supersample", type=int, default=2, choices=[1, 2, 3, 4], help="Samples a pixel side")
    parser.add_argument("--azimuth-deg", type=float, help="Where the view is from, clockwise from north (default 225: the south-west)")
    parser.add_argument("--elevation-deg", type=float, help="Elevation of the view (default 35.264)")
    parser.add_argument("--frustum-scale", type=float, default=2, help="Size of the drawn cameras in world units")
    parser.add_argument("--no-ssao", dest="enable_ssao", action="store_false", help="Switch the screen-space occlusion off")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    visualize(**vars(args))


if __name__ == "__main__":
    main()
