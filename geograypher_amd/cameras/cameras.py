"""Camera records of the projection path: `PhotogrammetryCamera` and `PhotogrammetryCameraSet`.

Host-side mirror of geograypher/cameras/cameras.py (same names, arguments and error behaviour) restricted to what
`pix2face` / `render_flat` / `project_images` / `aggregate_projected_images` touch.  No pyvista: where the reference
builds a `pv.Camera` (cameras.py:446-477) this module exposes the same view parameters as plain numbers and packs
them into the 16-float record the HIP rasterizer consumes (`include/geograster.h`).
"""
from __future__ import annotations

import hashlib
import json
import os
from copy import deepcopy
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from geograypher_amd.constants import EXAMPLE_INTRINSICS, PATH_TYPE


def _imread(filename) -> np.ndarray:
    """Image file -> numpy array (the reference uses skimage.io.imread, cameras.py:157)."""
    from PIL import Image

    with Image.open(filename) as im:
        return np.array(im)  # a writable copy (PIL hands out a read-only view)


def vtk_like_clipping_range(cam_to_world: np.ndarray, bounds: np.ndarray, tolerance: float = 0.001):
    """(near, far) clipping distances the reference's renderer would pick for this camera and mesh bounds.

    The pyvista path never sets a clipping range (cameras.py:446-477), so VTK derives one from the actor bounds
    (`vtkRenderer::ResetCameraClippingRange`): the range of the 8 bounding-box corners along the view direction,
    widened by 1 % plus half its extent, with the near plane kept at >= `tolerance` x far (0.001 for depth buffers
    deeper than 16 bit).  Restated from the published VTK algorithm; VTK is not runnable here (parity unpinned).  The far
    plane lies beyond every corner of the bounds by construction, so only the near plane can ever cut the mesh.
    bounds: (xmin, xmax, ymin, ymax, zmin, zmax) in the cameras' local frame.
    """
    forward = cam_to_world[:3, 2]
    position = cam_to_world[:3, 3]
    xs, ys, zs = bounds[0:2], bounds[2:4], bounds[4:6]
    dists = [float(np.dot(forward, np.array([x, y, z]) - position)) for x in xs for y in ys for z in zs]
    near, far = min(dists), max(max(dists), 1e-18)
    near = max(near, 0.0)
    expansion = 0.5
    near = 0.99 * near - (far - near) * expansion
    far = 1.01 * far + (far - near) * expansion
    if near >= far:
        near = 0.01 * far
    if near < tolerance * far:
        near = tolerance * far
    return float(near), float(far)


def vtk_like_near_plane(cam_to_world: np.ndarray, bounds: np.ndarray, tolerance: float = 0.001) -> float:
    """The near distance of `vtk_like_clipping_range` (the only one of the two planes that can cut the mesh)."""
    return vtk_like_clipping_range(cam_to_world, bounds, tolerance)[0]


def vtk_like_near_planes(cam_to_worlds: np.ndarray, bounds: np.ndarray, tolerance: float = 0.001) -> np.ndarray:
    """`vtk_like_near_plane` for N cameras at once: cam_to_worlds (N,4,4) -> (N,) near distances."""
    T = np.asarray(cam_to_worlds, dtype=np.float64)
    corners = np.array([[x, y, z] for x in bounds[0:2] for y in bounds[2:4] for z in bounds[4:6]], dtype=np.float64)
    d = np.einsum("nk,nck->nc", T[:, :3, 2], corners[None, :, :] - T[:, None, :3, 3])
    near = np.maximum(d.min(axis=1), 0.0)
    far = np.maximum(d.max(axis=1), 1e-18)
    near = 0.99 * near - (far - near) * 0.5
    far = 1.01 * far + (far - near) * 0.5
    near = np.where(near >= far, 0.01 * far, near)
    return np.where(near < tolerance * far, tolerance * far, near)


def _locations_in_CRS(local_points: np.ndarray, local_to_epsg_4978_transform, as_CRS, backend=None,
                      force_easting_northing: bool = False) -> np.ndarray:
    """(n, 3) points of the chunk-local frame in `as_CRS`: local_to_epsg_4978 as the pre-transform of the device's reprojection
    from EPSG:4978 (DESIGN.md "CRS reprojection", G1)."""
    from geograypher_amd.constants import EARTH_CENTERED_EARTH_FIXED_CRS
    from geograypher_amd.utils.geospatial import reproject_points

    if local_to_epsg_4978_transform is None:
        raise ValueError("camera positions in a CRS need the local_to_epsg_4978_transform")
    if backend is None:
        from geograypher_amd._hip import HipRaster

        backend = HipRaster(None)
    out, _ = reproject_points(backend, np.ascontiguousarray(local_points, dtype=np.float64), EARTH_CENTERED_EARTH_FIXED_CRS, as_CRS,
                              pre_transform=np.asarray(local_to_epsg_4978_transform, dtype=np.float64),
                              force_easting_northing=force_easting_northing)
    return np.array(out, dtype=np.float64)


class PhotogrammetryCamera:
    def __init__(
        self,
        image_filename: PATH_TYPE,
        cam_to_world_transform: np.ndarray,
        f: float,
        cx: float,
        cy: float,
        image_width: int,
        image_height: int,
        distortion_params: Dict[str, float] = {},
        lon_lat: Union[None, Tuple[float, float]] = None,
        local_to_epsg_4978_transform: Union[np.ndarray, None] = None,
    ):
        """One camera pose + intrinsics as determined by photogrammetry (reference: cameras.py:55-102).

        Args:
            image_filename: the image used for reconstruction (may be None for synthetic cameras)
            cam_to_world_transform: 4x4 camera-to-world (chunk-local) transform; camera frame +X right, +Y down,
                +Z forward
            f: focal length in pixels
            cx, cy: principal point in pixels from the image centre
            image_width, image_height: sensor size in pixels
            distortion_params: lens distortion coefficients (Metashape names)
            lon_lat: optional (lon, lat)
            local_to_epsg_4978_transform: 4x4 chunk-local -> EPSG:4978
        """
        self.image_filename = image_filename
        self.cam_to_world_transform = cam_to_world_transform
        self.world_to_cam_transform = np.linalg.inv(cam_to_world_transform)
        self.f = f
        self.cx = cx
        self.cy = cy
        self.image_width = image_width
        self.image_height = image_height
        self.distortion_params = distortion_params
        self._local_to_epsg_4978_transform = local_to_epsg_4978_transform
        self.lon_lat = (None, None) if lon_lat is None else lon_lat
        self.image_size = (image_height, image_width)
        self.image = None
        self.cache_image = False

    # -- identity ------------------------------------------------------------------------------------------------
    def get_camera_hash(self, include_image_hash: bool = False):
        """sha256 of the camera geometry (reference: cameras.py:104-134; same JSON layout, same digest)."""
        camera_settings = {
            "transform": np.asarray(self.cam_to_world_transform).tolist(),
            "f": self.f,
            "cx": self.cx,
            "cy": self.cy,
            "image_width": self.image_width,
            "image_height": self.image_height,
            "distortion_params": self.distortion_params,
            "lon_lat": self.lon_lat,
        }
        if include_image_hash:
            camera_settings["image_filename"] = str(self.image_filename)
        data = json.dumps(camera_settings, sort_keys=True)
        return hashlib.sha256(data.encode("utf-8")).hexdigest()

    def get_camera_properties(self):
        """reference: cameras.py:136-152"""
        return {
            "focal_length": self.f,
            "principal_point_x": self.cx,
            "principal_point_y": self.cy,
            "image_height": self.image_height,
            "image_width": self.image_width,
            "distortion_params": self.distortion_params,
            "world_to_cam_transform": self.world_to_cam_transform,
        }

    # -- image access --------------------------------------------------------------------------------------------
    def get_image_native(self) -> np.ndarray:
        """The image as its file holds it (`imread`, cameras.py:157; cached like the reference's float image when
        `cache_image` is set).  The device paths take this: a uint8 photo crosses the link as uint8 and is divided by 255 and
        down-scaled there (`HipRaster.resize_image`)."""
        native = getattr(self, "_image_native", None)
        if native is None:
            from geograypher_amd.utils.decoded_cache import cached_decode

            # decoded_cache (set by the camera set / aggregate_projected_images(decoded_cache=...)): the decoded photo as an
            # uncompressed .npy keyed by (path, mtime, size), memory-mapped by later passes; None: decode every time
            native = cached_decode(self.image_filename, getattr(self, "decoded_cache", None),
                                   lambda: _imread(self.image_filename), "photo-native")
            if self.cache_image:
                self._image_native = native
        return native

    def get_image(self, image_scale: float = 1.0, backend=None) -> np.ndarray:
        """reference: cameras.py:154-174 -- uint8 images are returned as float in [0, 1]; `image_scale != 1` resizes with
        scikit-image's `resize` defaults (anti-aliasing Gaussian + order 1).  The resize runs on the device
        (`gr_resize_image_f64`, pinned to the real scikit-image's output in tests/test_photo_resize.py); there is no CPU
        resizer in the product: without a GPU a scaled image raises RuntimeError.  The scaled image is float64 whatever the
        file's dtype (scikit-image >= 0.19, the reference's pinned 0.21, returns float32 for a float32 FILE; photos are uint8
        and come back float64 there too): documented, values within float32 rounding of that."""
        if self.image is None:
            native = self.get_image_native()
            image = native / 255.0 if native.dtype == np.uint8 else native
            # `cache_image` keeps ONE copy per photo: the file's own array (a uint8 photo: an eighth of its float image, and
            # what the device paths upload; `/ 255.0` is redone per call) -- the reference caches the float image
            if self.cache_image and native.dtype != np.uint8:
                self.image = image             # the file's array itself
                self._image_native = None
        else:
            native = None
            image = self.image
        if image_scale != 1.0:
            if backend is None:
                from geograypher_amd._hip import default_backend

                backend = default_backend()
            out_hw = (int(image.shape[0] * image_scale), int(image.shape[1] * image_scale))
            src = native if native is not None else image  # the file dtype when it is at hand (uint8: an eighth of the bytes)
            resized = backend.resize_image(src, out_hw, divide_by_255=src.dtype == np.uint8)
            image = resized.cpu().numpy() if hasattr(resized, "cpu") else np.asarray(resized)
        return image

    def get_image_filename(self):
        return self.image_filename

    def get_image_size(self, image_scale=1.0):
        """(h, w) in pixels, truncated like the reference (cameras.py:179-200)."""
        if self.image_size is not None:
            pass
        elif self.image is not None:
            self.image_size = self.image.shape[:2]
        else:
            self.image_size = self.get_image().shape[:2]
        return (int(self.image_size[0] * image_scale), int(self.image_size[1] * image_scale))

    def get_local_to_epsg_4978_transform(self) -> np.ndarray:
        """reference: cameras.py:311-326"""
        return self._local_to_epsg_4978_transform

    def get_camera_location(self, get_z_coordinate: bool = False, as_CRS=None, backend=None):
        """The camera centre (reference: cameras.py:212-242): the translation of cam_to_world_transform in the chunk-local frame,
        or with `as_CRS` (what `geograypher_amd.utils.geospatial.WGS84CRS.parse` takes) in that CRS and its axis order, through
        local_to_epsg_4978 and the device's reprojection.  (x, y) or with `get_z_coordinate` (x, y, z).  backend: an object with
        `HipRaster.reproject_points` (default: a `HipRaster` on the current device)."""
        point = np.asarray(self.cam_to_world_transform, dtype=np.float64)[0:3, 3]
        if as_CRS is not None:
            point = _locations_in_CRS(point.reshape(1, 3), self._local_to_epsg_4978_transform, as_CRS, backend)[0]
        return tuple(float(v) for v in (point if get_z_coordinate else point[:2]))

    def cast_rays(self, pixel_coords_ij: np.ndarray, line_length: float = 10):
        """Rays from the camera centre through pixels (reference: cameras.py:574-628): pixel_coords_ij (n, 2) (i, j) pixel
        coordinates -> (2 n, 3) points in the local frame, alternating start (the camera centre) and end rows, every segment
        `line_length` long in camera units; None when there are no pixels.  The principal point is
        (image_width / 2 + cx, image_height / 2 + cy); a homogeneous scale in the transform's [3, 3] is divided out."""
        pixel_coords_xy = np.flip(np.asarray(pixel_coords_ij), axis=1)
        principal_point = np.array([[self.image_width / 2.0 + self.cx, self.image_height / 2.0 + self.cy]])
        scaled = (pixel_coords_xy - principal_point) / self.f
        n_points = len(scaled)
        if n_points == 0:
            return None
        homogeneous = np.concatenate([scaled, np.ones((n_points, 1))], axis=1)
        ends = homogeneous / np.linalg.norm(homogeneous, axis=1, keepdims=True) * line_length
        line_verts = np.zeros((2 * n_points, 4))
        line_verts[:, 3] = 1
        line_verts[1::2, :3] = ends
        transform = np.asarray(self.cam_to_world_transform, dtype=np.float64)
        projected = transform @ line_verts.T
        if transform[3, 3] != 1.0:
            projected = projected / transform[3, 3]
        return projected[:3, :].T

    # -- view ----------------------------------------------------------------------------------------------------
    def get_view_parameters(self, focal_dist: float = 10) -> dict:
        """The numbers the reference loads into a pyvista camera (cameras.py:446-477): position, focal point,
        view-up and the VERTICAL field of view in degrees.  The principal point is not part of this view."""
        T = np.asarray(self.cam_to_world_transform, dtype=np.float64)
        position = T[:3, 3]
        focal_point = position + T[:3, :3] @ np.array((0, 0, focal_dist), dtype=np.float64)
        up = T[:3, :3] @ np.array((0, -1, 0), dtype=np.float64)
        view_angle = np.rad2deg(2 * np.arctan((self.image_height / 2) / self.f))
        return {"position": position, "focal_point": focal_point, "up": up, "view_angle": view_angle}

    def get_vis_mesh(self, frustum_scale: float = 0.1):
        """This camera as a frustum (reference: cameras.py:479-553): -> (points (5, 3) float64 in the chunk-local frame: the
        centre and the four corners of the image plane at distance `frustum_scale`; faces (6, 3) int64: four sides and the two
        triangles of the end cap; face_rgb (6, 3) uint8: blue, the side at the image's top (-Y) red) in place of the
        reference's pv.PolyData."""
        halfwidth, halfheight = self.image_width / (self.f * 2), self.image_height / (self.f * 2)
        scaled_cx, scaled_cy = self.cx / self.f, self.cy / self.f
        right, left = scaled_cx + halfwidth, scaled_cx - halfwidth
        top, bottom = scaled_cy + halfheight, scaled_cy - halfheight
        vertices = np.array([[0, 0, 0], [right, top, 1], [right, bottom, 1], [left, bottom, 1], [left, top, 1]],
                            dtype=np.float64).T * frustum_scale
        transform = np.asarray(self.cam_to_world_transform, dtype=np.float64)
        projected = transform @ np.vstack((vertices, np.ones((1, 5))))
        if transform[3, 3] != 1.0:
            projected = projected / transform[3, 3]
        faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [1, 2, 3], [3, 4, 1]], dtype=np.int64)
        face_rgb = np.array([[0, 0, 255], [255, 0, 0], [0, 0, 255], [0, 0, 255], [0, 0, 255], [0, 0, 255]], dtype=np.uint8)
        return np.ascontiguousarray(projected[:3].T), faces, face_rgb

    def get_raster_record(
        self, image_scale: float = 1.0, near: float = 1e-3, principal_point: str = "center", origin=None,
        focal_scaling: str = "scaled",
    ) -> np.ndarray:
        """Pack this view into the 16-float record of include/geograster.h.

        The pinhole that a pyvista camera with the parameters above realises in an (h, w) window is
        u = w/2 + f_eff X/Z, v = h/2 + f_eff Y/Z with f_eff = (h/2)/tan(view_angle/2) = f*h/image_height
        (cameras.py:469-475, meshes.py:1801, 1820-1822).  principal_point="center" reproduces that (cx, cy ignored
        exactly as the reference's pyvista path does); "intrinsics" places it at (w/2 + cx*s, h/2 + cy*s), the
        convention of the reference's PyTorch3D plugin (derived_meshes.py:772-780) scaled to the window.

        origin: float64 point subtracted from the camera position before the fp32 cast (the mesh class subtracts the
            same point from the vertices: ECEF-magnitude coordinates keep their metres, VTK does the same with its
            automatic VBO shift).
        focal_scaling: "scaled" = f * h / image_height (what the pyvista camera's vertical view angle gives in an
            (h, w) window); "unscaled" reproduces the PyTorch3D plugin, which hands the FULL-resolution focal length and
            principal point to a down-scaled image (derived_meshes.py:686-692, 772-780: `focal_length=camera.f`,
            `image_size` scaled) -- a bug-compatibility switch, only meaningful with principal_point="intrinsics".
        """
        h, w = self.get_image_size(image_scale)
        T = np.asarray(self.cam_to_world_transform, dtype=np.float64)
        if focal_scaling == "scaled":
            f_eff = float(self.f) * h / float(self.image_height)
        elif focal_scaling == "unscaled":
            f_eff = float(self.f)
        else:
            raise ValueError(f"focal_scaling must be 'scaled' or 'unscaled', not {focal_scaling!r}")
        if principal_point == "center":
            cxp, cyp = w / 2.0, h / 2.0
        elif principal_point == "intrinsics":
            k = 1.0 if focal_scaling == "unscaled" else h / float(self.image_height)
            cxp = w / 2.0 + float(self.cx) * k
            cyp = h / 2.0 + float(self.cy) * k
        else:
            raise ValueError(f"principal_point must be 'center' or 'intrinsics', not {principal_point!r}")
        rec = np.empty(16, dtype=np.float32)
        rec[0:9] = T[:3, :3].reshape(9)
        rec[9:12] = T[:3, 3] if origin is None else T[:3, 3] - np.asarray(origin, dtype=np.float64)
        rec[12] = f_eff
        rec[13] = cxp
        rec[14] = cyp
        rec[15] = near
        return rec


class PhotogrammetryCameraSet:
    def __init__(
        self,
        cameras: Union[None, PhotogrammetryCamera, List[PhotogrammetryCamera]] = None,
        cam_to_world_transforms: Optional[List[np.ndarray]] = None,
        intrinsic_params_per_sensor_type: Dict[int, Dict[str, float]] = {0: EXAMPLE_INTRINSICS},
        image_filenames: Optional[List[PATH_TYPE]] = None,
        lon_lats: Optional[List[Union[None, Tuple[float, float]]]] = None,
        image_folder: Optional[PATH_TYPE] = None,
        sensor_IDs: Optional[List[int]] = None,
        validate_images: bool = False,
        local_to_epsg_4978_transform: np.ndarray = np.eye(4),
    ):
        """A set of cameras in one chunk-local frame (reference: cameras.py:661-781, same arguments).

        Raises:
            ValueError: if the number of sensor IDs differs from the number of transforms.
        """
        self._local_to_epsg_4978_transform = local_to_epsg_4978_transform
        self._maps_ideal_to_warped = {}
        self._maps_warped_to_ideal = {}

        if cameras is not None:
            if isinstance(cameras, PhotogrammetryCamera):
                self.image_folder = None if cameras.image_filename is None else Path(cameras.image_filename).parent
                cameras = [cameras]
            else:
                names = [str(cam.image_filename) for cam in cameras if cam.image_filename is not None]
                self.image_folder = Path(os.path.commonpath(names)) if len(names) == len(cameras) and names else None
            self.cameras = cameras
            return

        n_transforms = len(cam_to_world_transforms)
        if image_filenames is None:
            image_filenames = [None] * n_transforms
        if sensor_IDs is None and len(intrinsic_params_per_sensor_type) == 1:
            sensor_IDs = [list(intrinsic_params_per_sensor_type.keys())[0]] * n_transforms
        elif len(sensor_IDs) != n_transforms:
            raise ValueError(
                f"Number of sensor_IDs ({len(sensor_IDs)}) is different than the number of transforms ({n_transforms})"
            )
        if lon_lats is None:
            lon_lats = [None] * n_transforms

        self.cam_to_world_transforms = cam_to_world_transforms
        self.intrinsic_params_per_sensor_type = intrinsic_params_per_sensor_type
        self.image_filenames = image_filenames
        self.lon_lats = lon_lats
        self.sensor_IDs = sensor_IDs
        self.image_folder = image_folder

        if validate_images:
            missing_images, invalid_mask = self.find_missing_images()
            if len(missing_images) > 0:
                print(f"Deleting {len(missing_images)} missing images")
                keep = [i for i, bad in enumerate(invalid_mask) if not bad]
                self.image_filenames = [self.image_filenames[i] for i in keep]
                self.cam_to_world_transforms = [self.cam_to_world_transforms[i] for i in keep]
                self.sensor_IDs = [self.sensor_IDs[i] for i in keep]
                self.lon_lats = [self.lon_lats[i] for i in keep]

        self.cameras = []
        for image_filename, cam_to_world_transform, sensor_ID, lon_lat in zip(
            self.image_filenames, self.cam_to_world_transforms, self.sensor_IDs, self.lon_lats
        ):
            sensor_params = self.intrinsic_params_per_sensor_type[sensor_ID]
            if sensor_params is None:  # sensor without a full calibration
                continue
            self.cameras.append(
                PhotogrammetryCamera(
                    image_filename,
                    cam_to_world_transform,
                    lon_lat=lon_lat,
                    local_to_epsg_4978_transform=local_to_epsg_4978_transform,
                    **sensor_params,
                )
            )

    # -- container -----------------------------------------------------------------------------------------------
    def __deepcopy__(self, memo):
        """`get_subset_cameras` deep-copies the set (cameras.py:861-864); device-resident sampling maps and the GPU
        context they belong to are shared, never duplicated."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = v if k == "_maps_device" else deepcopy(v, memo)
        return new

    def __len__(self):
        return self.n_cameras()

    def __getitem__(self, slice):
        subset_cameras = self.cameras[slice]
        if isinstance(subset_cameras, PhotogrammetryCamera):
            return subset_cameras
        return PhotogrammetryCameraSet(
            subset_cameras, local_to_epsg_4978_transform=self._local_to_epsg_4978_transform
        )

    def get_image_folder(self):
        return self.image_folder

    def find_missing_images(self):
        invalid_mask = [not Path(image_file).is_file() for image_file in self.image_filenames]
        invalid_images = [f for f, bad in zip(self.image_filenames, invalid_mask) if bad]
        return invalid_images, invalid_mask

    def n_cameras(self) -> int:
        return len(self.cameras)

    def n_image_channels(self) -> int:
        return 3

    def get_subset_cameras(self, inds: List[int]):
        """reference: cameras.py:861-864 (a copy of the set holding only `inds`; IndexError when out of range)."""
        subset_camera_set = deepcopy(self)
        subset_camera_set.cameras = [subset_camera_set[i] for i in inds]
        return subset_camera_set

    def inds_in_folder(self, folder: PATH_TYPE) -> List[int]:
        """The cameras whose image lies under `folder`."""
        folder = Path(folder)
        return [i for i, cam in enumerate(self.cameras)
                if cam.image_filename is not None and Path(cam.image_filename).is_relative_to(folder)]

    def inds_matching_filename_regex(self, filename_regex: str) -> List[int]:
        """The cameras whose image path `re.search` finds the expression in."""
        import re

        return [i for i, cam in enumerate(self.cameras) if re.search(filename_regex, str(cam.image_filename))]

    def get_cameras_in_folder(self, folder: PATH_TYPE):
        """reference: cameras.py:819-836"""
        return self.get_subset_cameras(self.inds_in_folder(folder))

    def get_cameras_matching_filename_regex(self, filename_regex: str):
        """reference: cameras.py:838-859"""
        return self.get_subset_cameras(self.inds_matching_filename_regex(filename_regex))

    def get_camera_locations(self, as_CRS=None, backend=None, force_easting_northing: bool = False) -> np.ndarray:
        """(n, 3) float64: the translation of every camera's cam_to_world_transform, in the chunk-local frame (reference:
        cameras.py:955-966); with `as_CRS` (what `geograypher_amd.utils.geospatial.WGS84CRS.parse` takes) in that CRS, in its
        axis order unless `force_easting_northing`, one device call for the set."""
        local = np.array([np.asarray(cam.cam_to_world_transform, dtype=np.float64)[:3, 3] for cam in self.cameras],
                         dtype=np.float64).reshape(-1, 3)
        if as_CRS is None:
            return local
        return _locations_in_CRS(local, self._local_to_epsg_4978_transform, as_CRS, backend, force_easting_northing)

    def get_lon_lat_coords(self, backend=None):
        """[(lon, lat)] of every camera, computed from its position on every call (the reference reads the cameras' stored
        `lon_lat`, cameras.py:951-953): `lon_lats` is not filled, it enters `get_camera_hash`."""
        from geograypher_amd.constants import LAT_LON_CRS

        lon_lat = self.get_camera_locations(as_CRS=LAT_LON_CRS, backend=backend, force_easting_northing=True)
        return [(float(lon), float(lat)) for lon, lat, _ in lon_lat]

    def get_subset_ROI(self, ROI, buffer_radius: float = 0, is_geospatial: Optional[bool] = None, *, points_in_ROI_CRS=None,
                       backend=None):
        """The cameras within `buffer_radius` of a region (reference: cameras.py:1207-1273; DESIGN.md "Region of interest").

        ROI: a `PlanarPolygons`, a sequence its `from_sequence` takes, or a `.geojson` path.  is_geospatial: None takes a
        `.geojson` for geospatial and ring arrays for local.  A local ROI is compared with `get_camera_locations()` (x, y of the
        chunk-local frame); a geospatial one needs the camera positions in ITS planar CRS as points_in_ROI_CRS (n, 2) or (n, 3),
        or the name of that CRS (`WGS84CRS.parse`: the positions are then computed on the device, `get_camera_locations(as_CRS=)`)
        -- the reference reprojects lon / lat with pyproj -- else NotImplementedError.  A camera ON the buffered region's
        boundary is kept (`within` drops it).  backend: an object with `HipRaster.points_in_region` (default: a `HipRaster` on
        the current device)."""
        from geograypher_amd.utils.geometric import points_in_region

        if is_geospatial is None:
            is_geospatial = isinstance(ROI, (str, os.PathLike))
        if points_in_ROI_CRS is not None:
            from geograypher_amd.utils.geospatial import is_CRS_designator

            if is_CRS_designator(points_in_ROI_CRS):   # the positions in that CRS, easting first, computed on the device
                points_in_ROI_CRS = self.get_camera_locations(as_CRS=points_in_ROI_CRS, backend=backend,
                                                              force_easting_northing=True)
            locations = np.asarray(points_in_ROI_CRS, dtype=np.float64)
            if locations.ndim != 2 or locations.shape[0] != len(self.cameras) or locations.shape[1] not in (2, 3):
                raise ValueError(f"points_in_ROI_CRS must be ({len(self.cameras)}, 2) or ({len(self.cameras)}, 3), got "
                                 f"{locations.shape}")
        elif is_geospatial:
            raise NotImplementedError(
                "a geospatial ROI needs points_in_ROI_CRS: the camera positions in the ROI's planar CRS (CRS reprojection needs "
                "pyproj and is outside the projection path)")
        else:
            locations = self.get_camera_locations()
        if backend is None:
            from geograypher_amd._hip import HipRaster

            backend = HipRaster(None)
        mask, _ = points_in_region(backend, ROI, locations, buffer_radius)
        mask = np.asarray(mask.cpu() if hasattr(mask, "detach") else mask, dtype=bool)
        return self.get_subset_cameras(np.nonzero(mask)[0].tolist())

    def get_image_by_index(self, index: int, image_scale: float = 1.0) -> np.ndarray:
        return self[index].get_image(image_scale=image_scale)

    # May `get_image_by_index` of this set run on the mesh class's loader thread while the caller's thread rasterizes?  False
    # by default: a subclass (a segmentor set around a stateful or GPU segmentor, a user's own look-up) must say so itself.
    # The plain file-backed set needs no flag: the mesh class recognises it by its un-overridden methods and decodes ahead.
    thread_safe_lookup = False

    def set_decoded_cache(self, spec) -> None:
        """Opt in to (or, with None, out of) the decoded-input cache for this set's photos (utils/decoded_cache.py): True --
        `CACHE_FOLDER/decoded`, the reference's cache root (constants.py:18) --, or a folder.  Passes after the first
        memory-map the decoded photos instead of decoding them again."""
        for cam in self.cameras:
            cam.decoded_cache = spec

    def get_native_image_by_index(self, index: int) -> np.ndarray:
        """The image of camera `index` in its file dtype, for the device input pipeline of project_images /
        aggregate_projected_images: `get_image_by_index(i, s)` == resize(native / 255 if uint8 else native, s), with the
        division and the resize done on the device."""
        return self[index].get_image_native()

    def get_image_filename(self, index: Union[int, None], absolute=True):
        """reference: cameras.py:883-909"""
        if index is None:
            return [self.get_image_filename(i, absolute=absolute) for i in range(len(self.cameras))]
        filename = self.cameras[index].get_image_filename()
        if absolute:
            return Path(filename)
        return Path(filename).relative_to(self.get_image_folder())

    def get_local_to_epsg_4978_transform(self):
        """reference: cameras.py:911-926"""
        return self._local_to_epsg_4978_transform

    def save_images(self, output_folder: PATH_TYPE, copy: bool = False, remove_folder: bool = True):
        """Link (default) or copy the set's images into `output_folder`, keeping their paths relative to the image folder
        (reference: cameras.py:928-949).  An existing `output_folder` is removed first when `remove_folder`; with `copy` a source
        that does not exist is logged and skipped."""
        import logging
        import shutil

        if remove_folder and os.path.isdir(output_folder):
            logging.info(f"about to remove {output_folder}")
            shutil.rmtree(output_folder)
        for i in range(len(self.cameras)):
            output_file = Path(output_folder, self.get_image_filename(i, absolute=False))
            output_file.parent.mkdir(parents=True, exist_ok=True)
            src_file = self.get_image_filename(i, absolute=True)
            if copy:
                try:
                    shutil.copy(src_file, output_file)
                except FileNotFoundError:
                    logging.warning(f"Could not find {src_file}")
            else:
                os.symlink(src_file, output_file)

    def get_vis_mesh(self, frustum_scale: Optional[float] = 2, correct_for_scale: bool = True):
        """The frusta of all cameras as one mesh in the chunk-local frame: (points (5 N, 3), faces (6 N, 3) int64, face_rgb
        (6 N, 3) uint8), `PhotogrammetryCamera.get_vis_mesh` per camera.  `correct_for_scale`: `frustum_scale` is in world units
        and divided by the cube root of the determinant of local_to_epsg_4978's upper-left 3 x 3, as the reference's mesh.vis
        does (meshes.py:2212-2220).  frustum_scale None: the camera's own default, 0.1 local units."""
        transform = self.get_local_to_epsg_4978_transform()
        if frustum_scale is None:
            frustum_scale = 0.1
        elif correct_for_scale and transform is not None:
            frustum_scale = frustum_scale / np.cbrt(np.linalg.det(np.asarray(transform, dtype=np.float64)[:3, :3]))
        parts = [camera.get_vis_mesh(frustum_scale) for camera in self.cameras]
        if not parts:
            return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3), dtype=np.uint8)
        points = np.concatenate([p for p, _, _ in parts])
        faces = np.concatenate([f + 5 * k for k, (_, f, _) in enumerate(parts)])
        return points, faces, np.concatenate([c for _, _, c in parts])

    def get_raster_records(
        self, image_scale: float = 1.0, near: Union[float, List[float]] = 1e-3, principal_point: str = "center",
        origin=None, focal_scaling: str = "scaled",
    ) -> np.ndarray:
        """(N,16) float32 records for the HIP rasterizer; all cameras must share one image size."""
        nears = [near] * len(self.cameras) if np.isscalar(near) else list(near)
        sizes = {cam.get_image_size(image_scale) for cam in self.cameras}
        if len(sizes) > 1:
            raise ValueError("Not all cameras have the same image size")
        return np.stack(
            [cam.get_raster_record(image_scale, nr, principal_point, origin, focal_scaling)
             for cam, nr in zip(self.cameras, nears)], axis=0
        )

    # -- multiview detections (reference: cameras.py:1275-1398, 1483-1608) -------------------------------------------
    def calc_line_segments(self, detector, boundaries=None, ray_length_local: float = 1e3, out_dir: Optional[PATH_TYPE] = None,
                           limit_ray_length_local: Optional[float] = None, limit_angle_from_vert: Optional[float] = None,
                           backend=None):
        """One ray per detection centre of every image (cameras.py:1483-1608): `detector.get_detection_centers(filename)` ->
        `cast_rays` -> optional filter by the angle from the vertical (radians) -> optional clip between two boundary surfaces
        ((points, faces) pairs; `clip_line_segments`, on the device).  Returns {"ray_starts", "ray_ends", "ray_IDs"} or, with
        `out_dir`, the path of the `line_segments.npz` saved there."""
        from geograypher_amd.utils.geometric import clip_line_segments

        all_line_segments, all_image_IDs = [], []
        for camera_ind in range(len(self.cameras)):
            centers = detector.get_detection_centers(str(self.get_image_filename(camera_ind)))
            if len(centers) > 0:
                line_segments = self.cameras[camera_ind].cast_rays(pixel_coords_ij=centers, line_length=ray_length_local)
                all_line_segments.append(line_segments)
                all_image_IDs.append(np.full(int(line_segments.shape[0] / 2), fill_value=camera_ind))
        if len(all_line_segments) > 0:
            all_line_segments = np.concatenate(all_line_segments, axis=0)
            all_image_IDs = np.concatenate(all_image_IDs, axis=0)
            ray_starts, ray_ends = all_line_segments[0::2], all_line_segments[1::2]
            ray_directions = ray_ends - ray_starts
            ray_directions = ray_directions / np.linalg.norm(ray_directions, axis=1, keepdims=True)
            if limit_angle_from_vert is not None:
                keep_mask = np.arccos(np.abs(ray_directions[:, 2])) <= limit_angle_from_vert
                ray_starts, ray_ends = ray_starts[keep_mask], ray_ends[keep_mask]
                ray_directions, all_image_IDs = ray_directions[keep_mask], all_image_IDs[keep_mask]
            if boundaries is not None:
                ray_starts, ray_ends, ray_directions, all_image_IDs = clip_line_segments(
                    boundaries=boundaries, origins=ray_starts, directions=ray_directions, image_indices=all_image_IDs,
                    ray_limit=limit_ray_length_local, backend=backend)
        else:
            ray_starts, ray_ends = np.empty((0, 3)), np.empty((0, 3))
            all_image_IDs = np.empty((0,), dtype=int)
        data = {"ray_starts": ray_starts, "ray_ends": ray_ends, "ray_IDs": all_image_IDs}
        if out_dir is None:
            return data
        path = Path(out_dir) / "line_segments.npz"
        np.savez(path, **data)
        return path

    def triangulate_detections(self, detector, ray_length_meters: float = 1e3, boundaries=None,
                               limit_ray_length_meters: Optional[float] = None, limit_angle_from_vert: Optional[float] = None,
                               similarity_threshold_meters: float = 0.1, transform=None, louvain_resolution: float = 1.0,
                               out_dir: Optional[PATH_TYPE] = None, seed=None, backend=None,
                               community_method: str = "networkx") -> np.ndarray:
        """Per-image detections -> 3D locations (cameras.py:1275-1398): rays through the detection centres
        (`calc_line_segments`), the graph of rays from different images that pass within `similarity_threshold_meters` of each
        other (`calc_graph_weights`: the ray-pair kernel on the device), Louvain communities and one point per community
        (`calc_communities`).  Lengths in metres are scaled to local units by the local -> EPSG:4978 transform.  With `out_dir`
        each stage saves its file there (`line_segments.npz`, `edge_weights.json`, `communities.npz`) and a stage whose file
        exists is not computed again.  Returns (M, 3): lat / lon / alt when a transform and pyproj are at hand, local
        coordinates otherwise.  Beyond the reference's keywords: `seed` (Louvain), `backend` (the device backend) and
        `community_method`: "networkx" as in the reference, or "device" for the deterministic Louvain and the community points of
        DESIGN.md section 8p, which ignore `seed`; without `out_dir` the edge arrays then go straight from the ray-pair kernel to
        the community kernel: no tuple list, no JSON."""
        from geograypher_amd.utils.geometric import get_scale_from_transform
        from geograypher_amd.utils.numeric import calc_communities, calc_graph_weights, ray_pair_edges

        if community_method not in ("networkx", "device"):
            raise ValueError(f"community_method must be 'networkx' or 'device', got {community_method!r}")

        if out_dir is not None:
            out_dir = Path(out_dir)

        def check_exists(file):
            if out_dir is None:
                return False
            if isinstance(file, str):
                return (out_dir / file).is_file()
            return isinstance(file, Path) and file.is_file()

        transform_to_epsg_4978 = self.get_local_to_epsg_4978_transform()
        meters_to_local_scale = 1 / get_scale_from_transform(transform_to_epsg_4978)
        ray_length_local = ray_length_meters * meters_to_local_scale
        similarity_threshold_local = similarity_threshold_meters * meters_to_local_scale
        limit_ray_length_local = None if limit_ray_length_meters is None else limit_ray_length_meters * meters_to_local_scale

        if check_exists("line_segments.npz"):
            line_results = out_dir / "line_segments.npz"
        else:
            line_results = self.calc_line_segments(
                detector=detector, boundaries=boundaries, ray_length_local=ray_length_local, out_dir=out_dir,
                limit_ray_length_local=limit_ray_length_local, limit_angle_from_vert=limit_angle_from_vert, backend=backend)
        if check_exists(line_results):
            with np.load(line_results) as d:
                line_results = {k: d[k] for k in d.files}

        if check_exists("edge_weights.json"):
            weight_results = out_dir / "edge_weights.json"
        elif community_method == "device" and out_dir is None:
            weight_results = ray_pair_edges(
                line_results["ray_starts"], line_results["ray_ends"], line_results["ray_IDs"], similarity_threshold_local,
                step=5000, transform=transform, backend=backend)
        else:
            weight_results = calc_graph_weights(
                starts=line_results["ray_starts"], ends=line_results["ray_ends"], ray_IDs=line_results["ray_IDs"],
                similarity_threshold=similarity_threshold_local, out_dir=out_dir, step=5000, transform=transform,
                backend=backend)
        if check_exists(weight_results):
            with weight_results.open("r") as file:
                weight_results = json.load(file)

        if check_exists("communities.npz"):
            community_results = out_dir / "communities.npz"
        else:
            community_results = calc_communities(
                starts=line_results["ray_starts"], ends=line_results["ray_ends"], edge_weights=weight_results,
                louvain_resolution=louvain_resolution, out_dir=out_dir, transform_to_epsg_4978=transform_to_epsg_4978,
                seed=seed, **({"method": "device", "backend": backend} if community_method == "device" else {}))
        if check_exists(community_results):
            with np.load(community_results) as d:
                community_results = {k: d[k] for k in d.files}
        return community_results.get("community_points_latlon", community_results["community_points"])

    # -- distortion (the warp stage itself is the "next" row f1 of SURVEY.md section 8) -------------------------------
    def distortion_key(self, parameters: Dict[str, float], image_scale: float = 1.0) -> str:
        """reference: cameras.py:968-993 (8-decimal repeatable key)"""
        keys = sorted(parameters.keys())
        strings = [f"{key}:{parameters[key]:.8f}" for key in keys] + [f"image_scale:{image_scale:.8f}"]
        return "|".join(strings)

    def make_distortion_map(self, camera: PhotogrammetryCamera, inversion_downsample: int = 8, image_scale: float = 1.0,
                            backend=None, reference_inverse: bool = False) -> None:
        """Build and cache the two sampling maps of a distortion key (reference: cameras.py:995-1062).

        `_maps_ideal_to_warped[key]` (2, H, W): for every pixel of the IDEAL image, where it lands in the warped image
        (`ideal_to_warped` evaluated on the pixel grid; for a down-scaled image the model is evaluated at the original
        pixel positions of the scaled pixel centres and the result is scaled) -- bit-equal to the reference's.
        `_maps_warped_to_ideal[key]`: its inverse.  The reference inverts by scattered-data interpolation
        (scipy griddata) on every `inversion_downsample`-th pixel, minutes of host time at full resolution; here every
        pixel solves the lens model with Newton's method on the device (`gr_invert_distortion_f64`, float64, residual
        below 1e-9 px): the DENSE inverse, from which the reference's down-sampled one differs by its own interpolation
        error (0.022 px at downsample 8, 0.003 px at 2 on the reference's test lens; tests/test_warp.py) -- enough to move
        about 0.01 % of the nearest-neighbour samples of an id image.  One-time work per key.

        reference_inverse=True inverts the way the reference does instead -- `utils.indexing.inverse_map_interpolation` over
        every `inversion_downsample`-th pixel, on the host, bit-equal to the reference's map -- for parity runs.  The same
        host inversion is what a machine without a GPU gets (and only then is `inversion_downsample` used by default):
        building the maps and `warp_dewarp_pixels` need no device; the image warps themselves do.
        """
        im_h, im_w = camera.image_size
        if np.isclose(image_scale, 1.0):
            h_range = np.arange(im_h)
            w_range = np.arange(im_w)
        else:
            start, step = 1 / (2 * image_scale), 1 / image_scale
            h_range = np.arange(start, im_h, step)[: int(im_h * image_scale)]
            w_range = np.arange(start, im_w, step)[: int(im_w * image_scale)]
        rows, cols = np.meshgrid(h_range, w_range, indexing="ij")
        warp_cols, warp_rows = self.ideal_to_warped(camera, cols, rows)
        if not np.isclose(image_scale, 1.0):
            warp_cols = warp_cols * image_scale
            warp_rows = warp_rows * image_scale
        dkey = self.distortion_key(camera.distortion_params, image_scale)
        self._maps_ideal_to_warped[dkey] = np.stack([warp_rows, warp_cols], axis=0)
        maps_device = self.__dict__.setdefault("_maps_device", {})
        for mkey in [mkey for mkey in maps_device if mkey[0] == dkey]:  # the key's uploads, on every backend
            del maps_device[mkey]
        if backend is None and not reference_inverse:
            import torch

            if torch.cuda.is_available():
                from geograypher_amd._hip import default_backend

                backend = default_backend()
        if reference_inverse or backend is None:
            from geograypher_amd.utils.indexing import inverse_map_interpolation

            self._maps_warped_to_ideal[dkey] = inverse_map_interpolation(self._maps_ideal_to_warped[dkey], inversion_downsample)
            return
        inv = backend.invert_distortion(self.distortion_model(camera), len(h_range), len(w_range), image_scale)
        maps_device[(dkey, False, id(backend))] = (backend, inv)  # already where the warp kernels want it
        self._maps_warped_to_ideal[dkey] = inv.cpu().numpy()

    def distortion_model(self, camera: PhotogrammetryCamera) -> Dict[str, float]:
        """Parameters of the camera's lens model in the layout `gr_invert_distortion_f64` takes -- only derived sets
        know a distortion model (as for `ideal_to_warped`, cameras.py:1064-1090)."""
        raise NotImplementedError(f"distortion_model not implemented for {self.__class__}.")

    def ideal_to_warped(self, camera: PhotogrammetryCamera, xpix: np.ndarray, ypix: np.ndarray):
        """reference: cameras.py:1064-1090 -- only derived sets know a distortion model."""
        raise NotImplementedError(f"ideal_to_warped not implemented for {self.__class__}.")

    def warp_dewarp_image(
        self,
        camera: PhotogrammetryCamera,
        input_image,
        fill_value: float = 0.0,
        inversion_downsample: int = 8,
        interpolation_order: int = 1,
        warped_to_ideal: bool = True,
        image_scale: float = 1.0,
        backend=None,
        reference_float_roundtrip: bool = False,
    ):
        """Apply (ideal->warped) or undo (warped->ideal) a camera's lens distortion on an image
        (reference: cameras.py:1092-1156 + utils/image.py:72-126).

        The cached (2, H, W) map gives, for every output pixel, the position to sample in the input; the resampling
        itself (nearest neighbour for `interpolation_order=0`, bilinear for 1; `fill_value` outside the input) is a
        HIP gather kernel (`gr_warp_nearest_i32` / `gr_warp_f64`).  Input may be a numpy array (numpy is returned,
        same dtype) or a device tensor (a tensor is returned).

        reference_float_roundtrip: the reference pushes every image -- integer face-id images included -- through a
            float rescale to [0,1] and back before truncating to the input dtype (utils/image.py:102, 123), which
            returns ids that are off by one for a few percent of the pixels.  False (default) gathers integers exactly;
            True reproduces the reference's arithmetic bit for bit for `interpolation_order=0` on an integer image within
            the int32 range with an integer `fill_value`, and raises NotImplementedError for every other combination.
        """
        dkey = self.ensure_distortion_map(camera, inversion_downsample, image_scale, backend=backend)
        if backend is None:
            from geograypher_amd._hip import default_backend

            backend = default_backend()
        # one upload per (key, direction, backend); the entry holds the backend, so its id() is not reused while the entry
        # lives.  Threads that drive different backends write different entries, and each reads only what it looked up here
        mkey = (dkey, bool(warped_to_ideal), id(backend))
        held = self.__dict__.setdefault("_maps_device", {}).get(mkey)
        if held is None:
            inverse_map = self._maps_ideal_to_warped[dkey] if warped_to_ideal else self._maps_warped_to_ideal[dkey]
            held = self._maps_device[mkey] = (backend, backend.upload_map(inverse_map))
        return backend.warp_image(
            input_image, held[1], order=interpolation_order, fill_value=fill_value,
            reference_float_roundtrip=reference_float_roundtrip,
        )

    def ensure_distortion_map(self, camera: PhotogrammetryCamera, inversion_downsample: int = 8, image_scale: float = 1.0,
                              backend=None) -> str:
        """The camera's distortion key, its two host maps built (`make_distortion_map`) unless they are there already.  The
        device-list driver calls this for all its cameras before its device threads start: they then only read the maps."""
        dkey = self.distortion_key(camera.distortion_params, image_scale)
        if dkey not in self._maps_ideal_to_warped:  # a set without a lens model raises NotImplementedError here
            self.make_distortion_map(camera, inversion_downsample, image_scale, backend=backend)
        return dkey

    def warp_dewarp_pixels(self, camera: PhotogrammetryCamera, pixels: np.ndarray, inversion_downsample: int = 8,
                           warped_to_ideal: bool = True, backend=None):
        """(N,2) integer (i,j) pixels -> their float positions in the other image (reference: cameras.py:1158-1205)."""
        dkey = self.ensure_distortion_map(camera, inversion_downsample, backend=backend)
        rowmap, colmap = self._maps_warped_to_ideal[dkey] if warped_to_ideal else self._maps_ideal_to_warped[dkey]
        rows = rowmap[pixels[:, 0], pixels[:, 1]]
        cols = colmap[pixels[:, 0], pixels[:, 1]]
        return np.stack([rows, cols], axis=0).T
