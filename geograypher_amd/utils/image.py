"""360-degree (equirectangular) photos: perspective views resampled on the device.

Mirror of geograypher/utils/image.py:29-69 and 129-267.  The host prepares what is a few kilobytes -- the ray coordinates of the
oversampled view's columns and rows and the rotation matrix, with numpy and scipy exactly as the reference does --; the 354 M
samples of a photo at the entrypoint's default sizes are formed, interpolated, round-tripped and averaged by
`gr_equirect_view` (csrc/equirect.hip; arithmetic order in DESIGN.md "Equirectangular resampling").  There is no CPU path: the
`backend` argument takes a `HipRaster` (default: the calling thread's shared one) or an object with its two equirect methods.
"""
from typing import Iterable, Optional, Tuple

import numpy as np


def rotate_by_roll_pitch_yaw(roll_deg: float, pitch_deg: float, yaw_deg: float, return_4x4: bool = False) -> np.ndarray:
    """utils/image.py:29-69: roll about the camera's Z (forward) axis, pitch about X, yaw about Y."""
    from scipy.spatial.transform import Rotation

    yaw = np.deg2rad(yaw_deg)
    pitch = np.deg2rad(pitch_deg)
    roll = np.deg2rad(roll_deg)
    # the camera frame expressed in the roll-pitch-yaw frame: new Z is old -Y, new Y is old X, new X is old Z
    permutation_matrix = np.array([[0, 0, 1], [1, 0, 0], [0, -1, 0]])
    rotation_matrix = Rotation.from_euler("ZYX", [yaw, pitch, roll]).as_matrix()
    rotation_matrix_in_cam_frame = permutation_matrix.T @ rotation_matrix @ permutation_matrix
    if return_4x4:
        out = np.eye(4)
        out[:3, :3] = rotation_matrix_in_cam_frame
        return out
    return rotation_matrix_in_cam_frame


def _view_axes(fov_deg: float, output_size: Tuple[int, int], oversample_factor):
    """utils/image.py:174-196: x and y of the oversampled view's rays (z = 1), pixel centres."""
    out_h, out_w = output_size
    out_w = int(out_w * oversample_factor)
    out_h = int(out_h * oversample_factor)
    fov = np.deg2rad(fov_deg)
    aspect_ratio = out_h / out_w
    x_dist = np.tan(fov / 2)
    y_dist = x_dist * aspect_ratio
    pixel_width = (2 * x_dist) / out_w
    x = np.arange(-x_dist + pixel_width / 2, x_dist, pixel_width)
    y = np.arange(-y_dist + pixel_width / 2, y_dist, pixel_width)
    if len(x) != out_w or len(y) != out_h:
        raise ValueError(f"the ray grid came out as {len(y)} x {len(x)} for an oversampled view of {out_h} x {out_w}")
    return x, y


def _backend(backend):
    if backend is not None:
        return backend
    from geograypher_amd._hip import default_backend

    return default_backend()


def perspectives_from_equirectangular(equi_img: np.ndarray, views: Iterable[tuple], output_size: Tuple[int, int] = (1440, 1440),
                                      warp_order: int = 1, oversample_factor: int = 1, return_mask: bool = False,
                                      backend=None):
    """Yield one perspective view of `equi_img` per entry (fov_deg, yaw_deg, pitch_deg[, roll_deg]) of `views`, each what
    `perspective_from_equirectangular` returns.  The photo is uploaded once and stays on the device across its views."""
    if warp_order not in (0, 1):
        raise NotImplementedError(f"warp_order {warp_order} is not implemented on the device (0 or 1)")
    views = [tuple(v) for v in views]
    for v in views:
        if len(v) not in (3, 4):
            raise ValueError(f"a view is (fov_deg, yaw_deg, pitch_deg[, roll_deg]), got {v}")
    backend = _backend(backend)
    source = backend.equirect_upload(equi_img)

    def generate():
        for v in views:
            fov, yaw, pitch = v[:3]
            roll = v[3] if len(v) == 4 else 0
            x, y = _view_axes(fov, output_size, oversample_factor)
            rot = rotate_by_roll_pitch_yaw(roll, pitch, yaw)
            yield backend.equirect_view(source, x, y, rot, output_size, oversample_factor=oversample_factor, order=warp_order,
                                        return_mask=return_mask)

    return generate()


def perspective_from_equirectangular(
    equi_img: np.ndarray,
    fov_deg: float,
    output_size: Tuple[int, int] = (1440, 1440),
    yaw_deg: float = 0,
    pitch_deg: float = 0,
    roll_deg: float = 0,
    warp_order: int = 1,
    oversample_factor: int = 1,
    return_mask: bool = False,
    backend=None,
) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """Sample a perspective image from an equirectangular (H, W, C) image: utils/image.py:129-267 on the device.

    With roll, pitch and yaw zero the camera looks at the centre of the equirectangular image.  Returns the view --
    float64 when `oversample_factor` > 1 or the source is float, the source dtype at factor 1 -- and, with `return_mask`, the
    (H, W) bool mask of the source pixels that were sampled."""
    (res,) = perspectives_from_equirectangular(
        equi_img, [(fov_deg, yaw_deg, pitch_deg, roll_deg)], output_size=output_size, warp_order=warp_order,
        oversample_factor=oversample_factor, return_mask=return_mask, backend=backend)
    return res
