"""Synthetic pinhole rigs for 360-degree photos: mirror of geograypher/cameras/rig_cameras.py:9-105.

The Metashape cameras of the equirectangular photos become one pinhole camera per (photo, rig orientation); the perspective
images themselves come from geograypher_amd.entrypoints.equirectangular_to_cube_mapped.  The resulting set goes through
`pix2face` / `aggregate_projected_images` like any other camera set."""
from pathlib import Path
from typing import Dict, List

from geograypher_amd.cameras.cameras import PhotogrammetryCameraSet
from geograypher_amd.cameras.derived_cameras import MetashapeCameraSet
from geograypher_amd.constants import PATH_TYPE
from geograypher_amd.utils.image import rotate_by_roll_pitch_yaw


def create_rig_cameras_from_equirectangular(
    camera_file: PATH_TYPE,
    original_images: PATH_TYPE,
    perspective_images: PATH_TYPE,
    rig_camera: Dict[str, float],
    rig_orientations: List[Dict[str, float]],
    perspective_filename_format_str: str,
) -> PhotogrammetryCameraSet:
    """A camera set for a rig of perspective cameras derived from equirectangular cameras.

    camera_file: Metashape export of the real equirectangular photos.  original_images: the folder their labels are relative
    to.  perspective_images: the folder of the resampled views.  rig_camera: "f", "cx", "cy", "image_width", "image_height" of
    the synthetic camera.  rig_orientations: dicts with "roll_deg", "pitch_deg", "yaw_deg", one per camera of the rig.
    perspective_filename_format_str: format string of those three names; its result, appended to the stem of the
    equirectangular photo's name, plus ".png" is the perspective image's name.

    Cameras are ordered photo-major: every orientation of the first photo, then of the second, ..."""
    # Only a parser here: a spherical sensor has no f, cx, cy, so they are defaulted (rig_cameras.py:48-56)
    initial_camera_set = MetashapeCameraSet(
        camera_file=camera_file,
        image_folder=perspective_images,
        original_image_folder=original_images,
        default_sensor_params={"f": 1.0, "cx": 0.0, "cy": 0.0},
    )
    cam_to_world_transforms = [c.cam_to_world_transform for c in initial_camera_set.cameras]
    image_filenames = [Path(c.image_filename) for c in initial_camera_set.cameras]
    rig_transforms = [rotate_by_roll_pitch_yaw(**orientation, return_4x4=True) for orientation in rig_orientations]
    image_extensions = [perspective_filename_format_str.format(**orientation) for orientation in rig_orientations]
    new_transforms = [
        cam_to_world @ rig_transform for cam_to_world in cam_to_world_transforms for rig_transform in rig_transforms
    ]
    new_image_filenames = [
        Path(image_filename.parent, image_filename.stem + image_extension + ".png")
        for image_filename in image_filenames
        for image_extension in image_extensions
    ]
    return PhotogrammetryCameraSet(
        cam_to_world_transforms=new_transforms,
        intrinsic_params_per_sensor_type={0: rig_camera},
        image_filenames=new_image_filenames,
        sensor_IDs=[0] * len(new_image_filenames),
        local_to_epsg_4978_transform=initial_camera_set.get_local_to_epsg_4978_transform(),
    )
