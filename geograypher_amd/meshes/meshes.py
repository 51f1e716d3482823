"""`TexturedPhotogrammetryMesh`: the image<->mesh projection path of geograypher on MI355X.

Host-side mirror of the hot-path slice of geograypher/meshes/meshes.py (1631-2084): same method names, arguments,
return types and error behaviour, so `render_labels` / `aggregate_images`-style callers run unchanged.  All per-pixel
and per-face work happens in hand-written HIP kernels behind the C ABI of include/geograster.h:

    pix2face                     -> gr_raster_face_ids           (replaces the VTK render of meshes.py:1776-1836)
    render_flat                  -> + gr_gather_texture_f64      (meshes.py:1921-1937)
    project_images               -> + gr_project_view_f64        (meshes.py:1987-2002)
    aggregate_projected_images   -> + gr_project_labels_u8 / gr_project_values_f64 + gr_finalize_*  (2044-2084)

There is no CPU implementation in this package: without the HIP extension or a GPU the constructor of the backend
raises.  (`backend=` exists so tests can drive this host logic against the CPU oracle; the product never does.)
"""
from __future__ import annotations

import hashlib
import logging
import math
import sys
import contextlib
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.cameras.cameras import (
    PhotogrammetryCamera,
    PhotogrammetryCameraSet,
    vtk_like_near_planes,
)
from geograypher_amd.constants import (
    CACHE_FOLDER,
    CLASS_ID_KEY,
    CLASS_NAMES_KEY,
    EARTH_CENTERED_EARTH_FIXED_CRS,
    NULL_TEXTURE_INT_VALUE,
    PATH_TYPE,
    VIS_FOLDER,
)

try:  # tqdm is optional: the reference wraps its view loops in it (meshes.py:2049-2053)
    from tqdm import tqdm
except Exception:  # pragma: no cover

    def tqdm(it, **_):
        return it


class LocalMesh:
    """A mesh expressed in the cameras' chunk-local frame: what `get_mesh_in_cameras_coords` returns in place of
    the reference's transformed `pv.PolyData` (meshes.py:1641-1676)."""

    def __init__(self, points: np.ndarray, faces: np.ndarray, key: typing.Optional[str] = None):
        self.points = points
        self.faces = faces
        self.key = key

    @property
    def n_faces(self):
        return int(self.faces.shape[0])

    def bounds(self) -> np.ndarray:
        if getattr(self, "_bounds", None) is None:
            lo, hi = self.points.min(axis=0), self.points.max(axis=0)
            self._bounds = np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], dtype=np.float64)
        return self._bounds

    def origin(self) -> np.ndarray:
        """float64 point the rasterizer's fp32 frame is centred on.  The kernels compute p - t in fp32, so coordinates
        of ECEF magnitude (6.4e6 m: fp32 ulp 0.5 m) must be re-centred before the cast -- VTK does the same with its
        automatic VBO shift/scale.  Meshes whose coordinates are already small (|x| < 4096: ulp <= 0.5 mm) keep the
        frame they have; otherwise the origin is the bounding-box centre rounded to whole metres."""
        if getattr(self, "_origin", None) is None:
            b = self.bounds()
            finite = np.all(np.isfinite(b))
            if finite and np.max(np.abs(b)) >= 4096.0:
                self._origin = np.round(np.array([(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2]))
            else:
                self._origin = np.zeros(3)
        return self._origin


def _parse_mesh(mesh) -> typing.Tuple[np.ndarray, np.ndarray]:
    """Accept (points, faces), a pyvista-like object (.points/.faces), or a .npz file with those two arrays."""
    if isinstance(mesh, (str, Path)):
        path = Path(mesh)
        if path.suffix != ".npz":
            raise NotImplementedError(
                f"Mesh file loading is limited to .npz (points, faces) here; {path.suffix} readers (pyvista) are "
                "outside the projection path (SURVEY.md section 8)"
            )
        with np.load(path) as data:
            return _parse_mesh((data["points"], data["faces"]))
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        points, faces = mesh
    elif hasattr(mesh, "points") and hasattr(mesh, "faces"):
        points, faces = mesh.points, mesh.faces
    else:
        raise TypeError("mesh must be (points, faces), an object with .points/.faces, or a .npz path")
    points = np.asarray(points)
    faces = np.asarray(faces)
    if faces.ndim == 1:  # pyvista's padded layout [3, a, b, c, 3, ...]
        faces = faces.reshape(-1, 4)
        if not np.all(faces[:, 0] == 3):
            raise ValueError("only triangular faces are supported")
        faces = faces[:, 1:4]
    if points.ndim != 2 or points.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"expected (V,3) points and (F,3) faces, got {points.shape} and {faces.shape}")
    return points, faces.astype(np.int64, copy=True)


def _reproject_stats(stats) -> dict:
    """The statistics words of `reproject_points` as a dict."""
    stats = np.asarray(stats.cpu() if hasattr(stats, "detach") else stats)
    return {"nonfinite": int(stats[0]), "beyond_central_meridian": int(stats[1]), "bad_faces": int(stats[2])}


class TexturedPhotogrammetryMesh:
    def __init__(
        self,
        mesh,
        input_CRS=EARTH_CENTERED_EARTH_FIXED_CRS,
        downsample_target: float = 1.0,
        texture: typing.Union[PATH_TYPE, np.ndarray, None] = None,
        texture_column_name: typing.Union[PATH_TYPE, None] = None,
        IDs_to_labels: typing.Union[PATH_TYPE, dict, None] = None,
        shift: typing.Union[np.ndarray, None] = None,
        ROI=None,
        ROI_buffer_meters: float = 0,
        log_level: str = "INFO",
        device: typing.Optional[int] = None,
        backend=None,
        neg1_is_last_face: bool = True,
        devices: typing.Optional[typing.Sequence[int]] = None,
        vertex_order: str = "r1",
        points_in_ROI_CRS: typing.Optional[np.ndarray] = None,
        downsample_method: typing.Optional[str] = None,
        ROI_simplify_tol_meters: float = 0,
        ROI_simplify_method: typing.Optional[str] = None,
    ):
        """A textured mesh that renders to / aggregates from camera views on an MI355X.

        Same leading arguments as the reference constructor (meshes.py:55-156).  `mesh` is `(points (V,3), faces
        (F,3))`, any object with `.points`/`.faces` (pyvista layout accepted) or a `.npz` path.  The coordinates are
        interpreted in `input_CRS`: EPSG:4978 (the frame the reference reprojects every mesh into, meshes.py:1659) or
        another WGS84 system `geograypher_amd.utils.geospatial.WGS84CRS.parse` takes (EPSG:4326 / 4979 in the authority's
        axis order lat, lon, h; the UTM zones), whose vertices are brought to EPSG:4978 on the device here; any other CRS
        needs pyproj and raises NotImplementedError.  The reference's quadric decimation (`downsample_target != 1` without
        `downsample_method`) and
        vector/raster texture files are likewise outside it and raise NotImplementedError (a `.geojson` texture is
        loaded afterwards, by `load_texture(..., points_in_polygon_CRS=...)`).  `ROI` with `ROI_buffer_meters` crops
        the mesh before the texture is loaded (`select_mesh_ROI`; needs `points_in_ROI_CRS`) and leaves the kept
        original indices in `self.ROI_point_IDs` and `self.ROI_face_IDs`; a texture array of the ORIGINAL face or vertex
        count is indexed by them, one of the cropped count is taken as it is.

        Extra keyword arguments (defaults keep reference behaviour):
            ROI_simplify_tol_meters, ROI_simplify_method: `select_mesh_ROI`'s simplify_tol_meters and simplify_method: the ROI is
                simplified by the exact Douglas-Peucker of DESIGN.md section 8q when the method "douglas-peucker" is named
                (the reference's load_mesh simplifies every ROI at 2 m with shapely, meshes.py:695).
            device: GPU index for the HIP backend (default: current torch device).
            devices: several GPU indices, e.g. `[0, 1, 2, 3, 4, 5, 6, 7]`: `aggregate_projected_images` deals its views round-robin to
                one libgeograster context + host thread per entry (the mesh is uploaded to each), adds the per-device partial
                votes (or float sums + counts) on the first device and finalises there -- the unchanged single-process caller
                (entrypoints/aggregate_images.py:146-184) uses the whole node.  Everything else runs on `devices[0]`.  The same
                index may appear more than once (contexts are independent).  Default None: one device, `device`.
            backend: test hook -- an object with the `HipRaster` interface (or a list of them: one per entry of `devices`).
            vertex_order: "r1" (default) -- the rule-set's own vertex stage --, or "gl": perspective divide,
                viewport transform and sub-pixel snap in the order of operations of an OpenGL pipeline, op for op what Mesa's
                llvmpipe (the software GL of the reference's Dockerfile) executes behind the camera transform
                (`GR_OPT_VERTEX_ORDER`).  The two put a few per cent of a view's vertices on neighbouring 1/256 px steps, which
                decides 0.004 % of its pixels; with "gl" a C2 view differs from a real llvmpipe render on 14 of 12 000 000 pixels
                (`profiles/r06_gl_residue.txt`).  Needs the pyvista camera's principal point (`principal_point="center"`).
            neg1_is_last_face: reproduce meshes.py:1998-2001, where background pixels (-1) index the LAST face
                during projection.  True matches the reference's aggregated textures on every face.
            points_in_ROI_CRS: the mesh vertices (V, 2) or (V, 3) in the ROI's planar CRS, or the name of that CRS ("EPSG:32610",
                32610, a `WGS84CRS`: the vertices are then reprojected on the device), required with `ROI` (the reference
                reprojects them with pyproj); without it `ROI` raises NotImplementedError.
            downsample_method: None (default) -- `downsample_target != 1` raises NotImplementedError: the reference's quadric
                decimation (VTK) is not built --, or "cluster": the mesh is decimated to about `downsample_target` of its vertices,
                0 < downsample_target <= 1, by vertex clustering on a uniform grid (`decimate`; DESIGN.md section 8n: NOT the
                reference's algorithm), on the device, after the reprojection and the ROI crop and before the texture.  The kept
                indices, into the mesh after the crop, are left in `self.decimated_point_IDs` and `self.decimated_face_IDs`; a
                texture array of an earlier vertex or face count is indexed by them (`to_current_mesh`).
        """
        if downsample_method is None:
            if downsample_target != 1.0:
                raise NotImplementedError("mesh decimation is outside the projection path (meshes.py:215-226)")
        elif downsample_method != "cluster":
            raise ValueError(f"downsample_method must be None or 'cluster', got {downsample_method!r}")
        elif not 0 < downsample_target <= 1:
            raise ValueError(f"downsample_target must lie in (0, 1], got {downsample_target!r}")
        if ROI is not None and points_in_ROI_CRS is None:
            raise NotImplementedError("ROI cropping is outside the projection path (meshes.py:646-731) unless the vertices "
                                      "in the ROI's CRS are given: points_in_ROI_CRS")
        source_CRS = None   # a WGS84 system other than EPSG:4978: the vertices are brought there on the device below
        if input_CRS is not None and str(input_CRS).upper().replace(" ", "") not in ("EPSG:4978",):
            from geograypher_amd.utils.geospatial import KIND_ECEF, WGS84CRS

            try:
                source_CRS = WGS84CRS.parse(input_CRS)
            except NotImplementedError:
                raise NotImplementedError(
                    f"input_CRS={input_CRS!r}: only meshes in EPSG:4978 or another WGS84 system (EPSG:4326, EPSG:4979, the UTM "
                    "zones EPSG:326xx / 327xx) are accepted (any other CRS needs pyproj and is outside the projection path)"
                ) from None
            if source_CRS.kind == KIND_ECEF:
                source_CRS = None
        self.downsample_target = downsample_target
        self.CRS = input_CRS if source_CRS is None else EARTH_CENTERED_EARTH_FIXED_CRS
        self.texture = None
        self.vertex_texture = None
        self.face_texture = None
        self.IDs_to_labels = None
        self.neg1_is_last_face = neg1_is_last_face

        self.logger = logging.getLogger(f"mesh_{id(self)}")
        self.logger.setLevel(log_level)
        if not self.logger.hasHandlers():
            self.logger.addHandler(logging.StreamHandler(stream=sys.stdout))

        self.logger.info("Loading mesh")
        points, faces = _parse_mesh(mesh)
        if shift is not None:
            points = points + np.asarray(shift).reshape(1, 3)
        self.points = points
        self.faces = faces

        if devices is not None:
            devices = [int(d) for d in devices]
            if len(devices) == 0:
                raise ValueError("devices must name at least one GPU")
            if device is not None and int(device) != devices[0]:
                raise ValueError(f"device={device} contradicts devices[0]={devices[0]}")
            device = devices[0]
        backends = None
        if isinstance(backend, (list, tuple)):
            backends = list(backend)
            if devices is not None and len(backends) != len(devices):
                raise ValueError(f"{len(backends)} backends for {len(devices)} devices")
            backend = backends[0]
        self._device_index = device
        self._devices = devices
        self._backend = backend
        self._backends = backends
        self._uploaded = {}   # id(backend) -> (points, faces) it holds
        if vertex_order not in ("r1", "gl"):
            raise ValueError(f"vertex_order must be 'r1' or 'gl', got {vertex_order!r}")
        self.vertex_order = vertex_order

        if source_CRS is not None:   # the projection path needs EPSG:4978 (reference: meshes.py:1659)
            from geograypher_amd.utils.geospatial import reproject_points

            self.points, stats = reproject_points(self.backend, np.ascontiguousarray(self.points, dtype=np.float64), source_CRS,
                                                  EARTH_CENTERED_EARTH_FIXED_CRS)
            self.points = np.array(self.points, dtype=np.float64)
            self.last_reproject_stats = _reproject_stats(stats)

        self.ROI_point_IDs = None
        self.ROI_face_IDs = None
        self._n_original = (self.points.shape[0], self.faces.shape[0])   # vertices, faces before the crop
        if ROI is not None:   # before the texture, as the reference does (meshes.py:200-213)
            (self.points, self.faces), self.ROI_point_IDs, self.ROI_face_IDs = self.select_mesh_ROI(
                ROI, buffer_meters=ROI_buffer_meters, simplify_tol_meters=ROI_simplify_tol_meters, return_original_IDs=True,
                points_in_ROI_CRS=points_in_ROI_CRS, simplify_method=ROI_simplify_method)

        self.downsample_method = downsample_method
        self.decimated_point_IDs = None
        self.decimated_face_IDs = None
        self._n_before_decimation = (self.points.shape[0], self.faces.shape[0])   # vertices, faces behind the crop
        if downsample_method == "cluster":   # in EPSG:4978, behind the crop: where the reference decimates (meshes.py:215-226)
            (self.points, self.faces), self.decimated_point_IDs, self.decimated_face_IDs = self.decimate(
                downsample_target, return_original_IDs=True)

        self.logger.info("Loading texture")
        if isinstance(IDs_to_labels, (str, Path)):
            import json

            with open(IDs_to_labels, "r") as file:
                IDs_to_labels = {int(k): v for k, v in json.load(file).items()}
        self.IDs_to_labels = IDs_to_labels
        if isinstance(texture, (str, Path)):
            if Path(texture).suffix != ".npy":
                raise NotImplementedError("only .npy texture files are read here; a .geojson texture needs the vertices in "
                                          "its CRS: load_texture(..., points_in_polygon_CRS=...)")
            texture = np.load(texture)
        if texture is not None:
            self.set_texture(self.to_current_mesh(np.asarray(texture)))

    # -- region of interest (DESIGN.md "Region of interest"; reference: meshes.py:646-731) -------------------------
    def crop_to_ROI(self, values: np.ndarray):
        """A per-vertex or per-face array of the ORIGINAL mesh -> the rows of the vertices or faces the constructor's `ROI`
        kept.  An array with a cropped count (or any other) is returned as it is, and so is everything on a mesh without ROI."""
        if self.ROI_point_IDs is None or values.ndim == 0:
            return values
        n_points, n_faces = self._n_original
        n = values.shape[0]
        if n in (self.points.shape[0], self.faces.shape[0]):
            return values
        if n == n_points == n_faces:
            raise ValueError("Cannot infer whether the array belongs to vertices or faces because the number is the same")
        if n == n_points:
            return values[self.ROI_point_IDs]
        if n == n_faces:
            return values[self.ROI_face_IDs]
        return values

    def select_mesh_ROI(self, region_of_interest, buffer_meters: float = 0, simplify_tol_meters: float = 0, default_CRS=None,
                        return_original_IDs: bool = False, *, points_in_ROI_CRS=None, simplify_method: typing.Optional[str] = None):
        """The part of the mesh in a region of interest (reference: meshes.py:646-731; rules Q1-Q6).

        region_of_interest: a `PlanarPolygons`, a sequence its `from_sequence` takes or a `.geojson` path; all rows together
        are the region.  None returns the mesh unchanged.  buffer_meters: a vertex within this distance of the region is in
        it too.  simplify_tol_meters: 0, or any tolerance s together with simplify_method="douglas-peucker" (another name:
        ValueError; a tolerance without the method: NotImplementedError): the ROI's rings are simplified at s by the exact
        Douglas-Peucker of DESIGN.md section 8q (`PlanarPolygons.simplified`) and the region test runs with the buffer
        buffer_meters + s.  The reference buffers first and simplifies the buffered polygon (meshes.py:695); here the order is
        the other way round, with a guarantee in its place: every point within buffer_meters of the original region is within
        buffer_meters + s of the simplified one, so the selection is a superset of the unsimplified one.  default_CRS:
        accepted and unused (coordinates are taken as they stand).  points_in_ROI_CRS (required, keyword): the mesh vertices
        (V, 2) or (V, 3) in the ROI's planar CRS, or a CRS designator (`WGS84CRS.parse`: the vertices are then reprojected on the device).

        A face is kept iff one of its vertices is in the region (`extract_points(adjacent_cells=True)`), a vertex iff a kept
        face uses it; both keep their order.  Returns (points, faces) -- faces index the kept points --, or with
        `return_original_IDs` ((points, faces), point_IDs, face_IDs): the ascending int64 indices into the original mesh.
        The point query and the compaction run on the device; the call's figures are left in `self.last_ROI_stats`."""
        from geograypher_amd.utils.geometric import check_simplify_method, points_in_region, region_polygons

        if region_of_interest is None:
            return self.points, self.faces
        if simplify_method is not None:
            check_simplify_method(simplify_method)
        elif simplify_tol_meters != 0:
            raise NotImplementedError("simplify_tol_meters: shapely's simplification is outside the projection path; ask for the "
                                      "exact Douglas-Peucker by name: simplify_method='douglas-peucker'")
        if points_in_ROI_CRS is None:
            raise NotImplementedError(
                "select_mesh_ROI needs points_in_ROI_CRS: the mesh vertices in the ROI's planar CRS (CRS reprojection needs "
                "pyproj and is outside the projection path)")
        verts = np.asarray(self._points_in_CRS(points_in_ROI_CRS), dtype=np.float64)
        if verts.ndim != 2 or verts.shape[0] != self.points.shape[0] or verts.shape[1] not in (2, 3):
            raise ValueError(f"points_in_ROI_CRS must be ({self.points.shape[0]}, 2) or ({self.points.shape[0]}, 3), got "
                             f"{verts.shape}")
        backend = self.backend
        if simplify_method is not None:
            region_of_interest = region_polygons(region_of_interest).simplified(simplify_tol_meters, backend)
            buffer_meters = buffer_meters + simplify_tol_meters
        mask, stats = points_in_region(backend, region_of_interest, verts, buffer_meters)
        face_IDs, point_IDs, new_faces, counts = backend.submesh_extract(mask, self.faces.astype(np.int32))
        face_IDs, point_IDs, new_faces, stats = (np.asarray(_to_host(a) if hasattr(a, "detach") else a)
                                                 for a in (face_IDs, point_IDs, new_faces, stats))
        face_IDs = np.array(face_IDs, dtype=np.int64).reshape(-1)
        point_IDs = np.array(point_IDs, dtype=np.int64).reshape(-1)
        self.last_ROI_stats = {"points_inside": int(stats[0]), "points_inside_by_buffer_only": int(stats[1]),
                               "wide_comparisons": int(stats[2]), "faces_kept": len(face_IDs), "points_kept": len(point_IDs)}
        subset = (self.points[point_IDs], np.array(new_faces, dtype=np.int64).reshape(-1, 3))
        if return_original_IDs:
            return subset, point_IDs, face_IDs
        return subset

    # -- decimation (stands where the reference decimates: meshes.py:215-226, 288-323) ---------
    def to_current_mesh(self, values: np.ndarray):
        """A per-vertex or per-face array of the mesh as it was passed in, or as the ROI crop left it -> the rows of the vertices
        or faces of the mesh as it is now: `crop_to_ROI`, then the rows `decimated_point_IDs` / `decimated_face_IDs` (rule D9: a
        kept vertex IS an input vertex, so the reference's nearest-neighbour transfer is this gather; face arrays are carried
        over too).  The count-matching rules of `crop_to_ROI`: an array with a current count (or any other) is returned as it is;
        one that fits vertices and faces alike is a ValueError.  Without a decimation this is `crop_to_ROI`."""
        values = self.crop_to_ROI(values)
        if self.decimated_point_IDs is None or values.ndim == 0:
            return values
        n_points, n_faces = self._n_before_decimation
        n = values.shape[0]
        if n in (self.points.shape[0], self.faces.shape[0]):
            return values
        if n == n_points == n_faces:
            raise ValueError("Cannot infer whether the array belongs to vertices or faces because the number is the same")
        if n == n_points:
            return values[self.decimated_point_IDs]
        if n == n_faces:
            return values[self.decimated_face_IDs]
        return values

    def original_point_IDs(self):
        """The indices of the current vertices in the mesh as it was passed in: `ROI_point_IDs`, `decimated_point_IDs`, or the
        one through the other; None when the mesh was neither cropped nor decimated."""
        ids = self.ROI_point_IDs
        if getattr(self, "decimated_point_IDs", None) is not None:
            ids = self.decimated_point_IDs if ids is None else np.asarray(ids)[self.decimated_point_IDs]
        return ids

    def decimate(self, downsample_target: typing.Optional[float] = None, *, cell_size_meters: typing.Optional[float] = None,
                 return_original_IDs: bool = False):
        """The mesh decimated by vertex clustering on a uniform grid (rules D1-D9 of DESIGN.md section 8n), on the device.

        The vertices are snapped to the 1e-6 m grid; every occupied cell of side s keeps ONE of its vertices, the one nearest
        the cell's centre (ties: the lowest index); a face with two corners in one cell is dropped, and so is every face behind an
        earlier one with the same three cells.  Exactly one of: downsample_target, 0 < target <= 1 -- s is searched so that at
        most floor(target V) cells are occupied (`utils.geometric.cluster_cell_size`: one device probe per step) --, or
        cell_size_meters, the cell side itself (ValueError outside the range the mesh's extent allows).  Everything is integer
        arithmetic: the result is exact and the same on every run and device.

        Returns (points, faces) -- the points are rows of `self.points`, faces index them --, or with `return_original_IDs`
        ((points, faces), point_IDs, face_IDs): the ascending int64 indices into the mesh as it is.  The mesh itself is not
        changed.  A result without faces is a ValueError.  The call's figures are left in `self.last_decimation_stats`.

        Out of scope: quadric-error vertex placement (float accumulation in a fixed order, vertices off the input set), parity
        with VTK's decimation, topology repair, and `face_to_vert_texture`."""
        from geograypher_amd._hip import (GR_DECIM_STAT_BAD_FACES, GR_DECIM_STAT_CELLS, GR_DECIM_STAT_COLLAPSED,
                                          GR_DECIM_STAT_DUPLICATES, GR_DECIM_STAT_OUTSIDE)
        from geograypher_amd.utils.geometric import SNAP_GRID_METERS, cluster_cell_range, cluster_cell_size, snap_points_3d

        if (downsample_target is None) == (cell_size_meters is None):
            raise ValueError("decimate takes exactly one of downsample_target and cell_size_meters")
        if downsample_target is not None and not 0 < downsample_target <= 1:
            raise ValueError(f"downsample_target must lie in (0, 1], got {downsample_target!r}")
        verts_q = snap_points_3d(self.points)
        s_min, s_max = cluster_cell_range(verts_q)
        backend = self.backend
        held = backend.to_device(verts_q, "int64") if hasattr(backend, "to_device") else verts_q
        if cell_size_meters is not None:
            s, probes = int(np.rint(float(cell_size_meters) / SNAP_GRID_METERS)), 0
            if not s_min <= s <= s_max:
                raise ValueError(f"cell_size_meters={cell_size_meters} is outside [{s_min * SNAP_GRID_METERS:g}, "
                                 f"{s_max * SNAP_GRID_METERS:g}] m, the cell sides this mesh allows")
        else:
            s, _, probes = cluster_cell_size(backend, verts_q, downsample_target, held=held)
        _, face_IDs, point_IDs, new_faces, stats = backend.cluster_decimate(held, self.faces.astype(np.int32), s)
        face_IDs, point_IDs, new_faces, stats = (np.asarray(_to_host(a) if hasattr(a, "detach") else a)
                                                 for a in (face_IDs, point_IDs, new_faces, stats))
        face_IDs = np.array(face_IDs, dtype=np.int64).reshape(-1)
        point_IDs = np.array(point_IDs, dtype=np.int64).reshape(-1)
        n_points, n_faces = self.points.shape[0], self.faces.shape[0]
        self.last_decimation_stats = {
            "requested_vertex_fraction": None if downsample_target is None else float(downsample_target),
            "achieved_vertex_fraction": len(point_IDs) / max(n_points, 1), "achieved_face_fraction": len(face_IDs) / max(n_faces, 1),
            "cell_size_meters": s * SNAP_GRID_METERS, "cell_size_steps": s, "probes": probes,
            "cells": int(stats[GR_DECIM_STAT_CELLS]), "points_kept": len(point_IDs), "faces_kept": len(face_IDs),
            "faces_collapsed": int(stats[GR_DECIM_STAT_COLLAPSED]), "faces_duplicate": int(stats[GR_DECIM_STAT_DUPLICATES]),
            "bad_faces": int(stats[GR_DECIM_STAT_BAD_FACES]), "points_outside": int(stats[GR_DECIM_STAT_OUTSIDE])}
        if len(face_IDs) == 0:
            raise ValueError(f"the decimation left no face: every face has two corners in one cell of {s * SNAP_GRID_METERS:g} m "
                             "(a larger downsample_target or a smaller cell_size_meters keeps some)")
        subset = (self.points[point_IDs], np.array(new_faces, dtype=np.int64).reshape(-1, 3))
        if return_original_IDs:
            return subset, point_IDs, face_IDs
        return subset

    # -- CRS reprojection (DESIGN.md "CRS reprojection"; reference: meshes.py:231-286, 752-783) ----------------------
    def get_mesh_points_in_CRS(self, output_CRS, use_vertices: bool = False, force_easting_northing: bool = True,
                               return_tensor: bool = False):
        """The face centres, or with `use_vertices` the vertices, in `output_CRS`: (n_faces | n_points, 3) float64, computed
        on the device.  output_CRS: what `geograypher_amd.utils.geospatial.WGS84CRS.parse` takes.  A face centre is the mean
        of the face's REPROJECTED vertices (`cell_centers()` of the reprojected mesh).  force_easting_northing: EPSG:4326 /
        4979 come out as (lon, lat, h) instead of the authority's (lat, lon, h).  A mesh whose CRS is None is returned
        untransformed, as the reference does.  `return_tensor=True` leaves the result on the device.  The counters of the call
        are left in `self.last_reproject_stats` (nonfinite, beyond_central_meridian, bad_faces)."""
        from geograypher_amd.utils.geospatial import reproject_points

        if self.CRS is None:
            self.logger.warning("mesh CRS is None, get_mesh_points_in_CRS is doing nothing")
            if use_vertices:
                return np.array(self.points, dtype=np.float64)
            corners = np.asarray(self.points, dtype=np.float64)[self.faces]
            return ((corners[:, 0] + corners[:, 1]) + corners[:, 2]) / 3.0
        faces = None if use_vertices else np.ascontiguousarray(self.faces, dtype=np.int32)
        out, stats = reproject_points(self.backend, np.ascontiguousarray(self.points, dtype=np.float64), self.CRS, output_CRS,
                                      faces=faces, force_easting_northing=force_easting_northing, return_tensor=return_tensor)
        self.last_reproject_stats = _reproject_stats(stats)
        return out

    def reproject_CRS(self, target_CRS, inplace: bool = False):
        """The mesh vertices (n_points, 3) in `target_CRS`, in the CRS's own axis order.  The reference updates the mesh with
        `inplace=True` (its default); here the projection path needs the mesh in EPSG:4978, so that raises NotImplementedError
        and the default is False."""
        if inplace:
            raise NotImplementedError("reproject_CRS(inplace=True): the projection path needs the mesh in EPSG:4978; use the "
                                      "returned points")
        return self.get_mesh_points_in_CRS(target_CRS, use_vertices=True, force_easting_northing=False)

    def _points_in_CRS(self, points_or_CRS):
        """What every `points_in_*_CRS` keyword takes: an array is returned as it is; a CRS designator (a string, an EPSG
        integer, a WGS84CRS) becomes the (V, 3) vertices in that CRS, easting first, computed on the device."""
        from geograypher_amd.utils.geospatial import is_CRS_designator

        if is_CRS_designator(points_or_CRS):
            return self.get_mesh_points_in_CRS(points_or_CRS, use_vertices=True, force_easting_northing=True)
        return points_or_CRS

    # -- backend -------------------------------------------------------------------------------------------------
    @property
    def backend(self):
        if self._backend is None:
            from geograypher_amd._hip import HipRaster

            self._backend = HipRaster(self._device_index)  # raises when the extension or the GPU is missing
        self._apply_vertex_order(self._backend)
        return self._backend

    def _apply_vertex_order(self, backend):
        if getattr(backend, "vertex_order", "r1") != self.vertex_order:
            if not hasattr(backend, "set_vertex_order"):
                raise NotImplementedError(f"backend {type(backend).__name__} has no vertex_order switch")
            backend.set_vertex_order(self.vertex_order)

    @property
    def backends(self):
        """One backend per entry of `devices` (the first is `self.backend`); a single-device mesh has one."""
        if self._backends is None:
            if not self._devices or len(self._devices) == 1:
                self._backends = [self.backend]
            else:
                from geograypher_amd._hip import HipRaster

                self._backends = [self.backend] + [HipRaster(d) for d in self._devices[1:]]
        for b in self._backends:
            self._apply_vertex_order(b)
        return self._backends

    # -- texture (reference: meshes.py:325-531) ------------------------------------------------------------------
    def standardize_texture(self, texture_array: np.ndarray):
        if texture_array.ndim == 1:
            texture_array = np.expand_dims(texture_array, axis=1)
        elif texture_array.ndim != 2:
            raise ValueError(f"Input texture should have 1 or 2 dimensions but instead has {texture_array.ndim}")
        return texture_array

    def is_discrete_texture(self):
        return self.IDs_to_labels is not None

    def get_IDs_to_labels(self):
        return self.IDs_to_labels

    def set_texture(self, texture_array, is_vertex_texture: typing.Union[bool, None] = None, delete_existing=True):
        """reference: meshes.py:476-531 (same inference rules and errors)."""
        texture_array = self.standardize_texture(np.asarray(texture_array))
        if is_vertex_texture is None:
            n_values = texture_array.shape[0]
            n_faces = self.faces.shape[0]
            n_verts = self.points.shape[0]
            if n_verts == n_faces:
                raise ValueError(
                    "Cannot infer whether texture should be applied to vertices of faces because the number is the same"
                )
            elif n_values == n_verts:
                is_vertex_texture = True
            elif n_values == n_faces:
                is_vertex_texture = False
            else:
                raise ValueError(
                    f"The number of elements in the texture ({n_values}) did not match the number of faces "
                    f"({n_faces}) or vertices ({n_verts})"
                )
        if is_vertex_texture:
            self.vertex_texture = texture_array
            if delete_existing:
                self.face_texture = None
        else:
            self.face_texture = texture_array
            if delete_existing:
                self.vertex_texture = None

    def vert_to_face_texture(self, vert_IDs, discrete=True):
        """reference: meshes.py:947-987.  Continuous textures: mean of the three vertex rows.  The discrete branch
        of the reference votes with an UNSEEDED random tie-break (utils/numeric.py:622-659); here ties go to the
        smallest value so results are reproducible."""
        if vert_IDs is None:
            raise ValueError("None")
        vert_IDs = np.squeeze(vert_IDs)
        if vert_IDs.ndim != 1 and discrete:
            raise ValueError(
                f"Can only perform discrete conversion with one dimensional array but instead had {vert_IDs.ndim}"
            )
        values_per_face = vert_IDs[self.faces]
        if not discrete:
            return np.mean(values_per_face, axis=1)
        a, b, c = values_per_face[:, 0], values_per_face[:, 1], values_per_face[:, 2]
        out = np.where((b == c) & np.isfinite(b), b, np.fmin(np.fmin(a, b), c))
        out = np.where(((a == b) | (a == c)) & np.isfinite(a), a, out)
        return out

    def get_texture(self, request_vertex_texture: typing.Union[bool, None] = None, try_verts_faces_conversion=True):
        """reference: meshes.py:337-378"""
        if self.vertex_texture is None and self.face_texture is None:
            return
        if request_vertex_texture is None:
            if self.vertex_texture is not None and self.face_texture is not None:
                raise ValueError("Ambigious which texture is requested, set request_vertex_texture appropriately")
            request_vertex_texture = self.vertex_texture is not None
        if request_vertex_texture:
            if self.vertex_texture is not None:
                return self.standardize_texture(self.vertex_texture)
            raise NotImplementedError("face -> vertex texture conversion is outside the projection path")
        if self.face_texture is not None:
            return self.standardize_texture(self.face_texture)
        elif try_verts_faces_conversion:
            face_texture = self.vert_to_face_texture(self.vertex_texture, discrete=self.is_discrete_texture())
            self.set_texture(face_texture, is_vertex_texture=False)
            return self.face_texture
        raise ValueError("Face texture not present and conversion was not requested")

    def remap_texture(self, texture_array: np.ndarray, IDs_to_labels: typing.Union[None, dict] = None,
                      all_discrete_texture_values=None, update_IDs_to_labels: bool = True, background_ID: int = None):
        """Texture values -> floats, or IDs of a discrete texture (reference: meshes.py:383-474).  Several columns: cast to
        float, `self.IDs_to_labels` cleared.  One column: `IDs_to_labels` (default: `determine_IDs_to_labels` of the values,
        or of `all_discrete_texture_values`) maps labels back to IDs unless its keys equal its values; a value without an ID
        becomes NaN.  ValueError for a table that is not one-to-one or whose IDs are not ints.  A continuous float column has no
        table: the reference fails on it with AttributeError (`None.keys()`), and so does this."""
        from geograypher_amd.utils.indexing import determine_IDs_to_labels

        texture_array = self.standardize_texture(np.asarray(texture_array))
        if texture_array.shape[1] != 1:
            self.IDs_to_labels = None
            return texture_array.astype(float)
        if IDs_to_labels is None:
            IDs_to_labels = determine_IDs_to_labels(texture_array, all_discrete_texture_values, background_ID)
        if list(IDs_to_labels.keys()) != list(IDs_to_labels.values()):
            labels_to_IDs = {label: ID for ID, label in IDs_to_labels.items()}
            if len(labels_to_IDs) != len(IDs_to_labels):
                raise ValueError("IDs_to_labels is not a one-to-one mapping")
            if not all(isinstance(ID, int) for ID in labels_to_IDs.values()):
                raise ValueError("The labels to IDs mapping does not produce only ints")
            texture_array = np.expand_dims(np.array([labels_to_IDs.get(label, np.nan) for label in texture_array.squeeze(axis=1)]),
                                           axis=1)
        if update_IDs_to_labels:
            self.IDs_to_labels = IDs_to_labels
        return texture_array

    def load_texture(self, texture, texture_column_name=None, IDs_to_labels=None, background_ID=None, *,
                     points_in_polygon_CRS=None):
        """Set the face or vertex texture from an array, a `.npy` file or a `.geojson` of polygons (reference: meshes.py:533-644;
        tried in that order).  texture=None only sets `IDs_to_labels` (there is no texture in the mesh file here).  A vector
        file goes through `get_values_for_faces_from_vector(texture, texture_column_name, points_in_polygon_CRS=...)`; any
        other file is taken for a raster, which needs rasterio: NotImplementedError.  The values then pass `remap_texture` (which
        sets `IDs_to_labels`) and `set_texture`."""
        if texture is None:
            self.logger.warning("No texture provided")
            if IDs_to_labels is not None:
                self.IDs_to_labels = IDs_to_labels
            return
        all_values = None
        if isinstance(texture, np.ndarray):
            texture_array = texture
        elif not isinstance(texture, (str, Path)):
            raise ValueError(f"Could not load texture for {texture}")
        elif Path(texture).suffix == ".npy":
            texture_array = np.load(texture, allow_pickle=True)
        elif Path(texture).suffix == ".geojson":
            texture_array, all_values = self.get_values_for_faces_from_vector(texture, texture_column_name,
                                                                              points_in_polygon_CRS=points_in_polygon_CRS)
        else:
            raise NotImplementedError(f"texture file {texture}: raster textures need rasterio, which is outside the projection "
                                      "path: pass an array, a .npy or a .geojson")
        self.set_texture(self.remap_texture(texture_array, IDs_to_labels=IDs_to_labels, all_discrete_texture_values=all_values,
                                            update_IDs_to_labels=True, background_ID=background_ID))

    # -- geometry ------------------------------------------------------------------------------------------------
    def get_mesh_hash(self):
        """sha256 over the vertex bytes and pyvista's padded int64 face layout (reference: meshes.py:1631-1639)."""
        hasher = hashlib.sha256()
        hasher.update(np.ascontiguousarray(self.points).tobytes())
        padded = np.concatenate([np.full((self.faces.shape[0], 1), 3, dtype=np.int64), self.faces], axis=1)
        hasher.update(np.ascontiguousarray(padded).tobytes())
        return hasher.hexdigest()

    def get_mesh_in_cameras_coords(self, cameras, inplace: bool = False) -> typing.Optional[LocalMesh]:
        """Mesh in the chunk-local frame of `cameras` (reference: meshes.py:1641-1676): x_local = inv(T) x_ecef in
        float64, with T = cameras.get_local_to_epsg_4978_transform()."""
        T = cameras.get_local_to_epsg_4978_transform()
        T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
        key = hashlib.sha1(T.tobytes()).hexdigest()
        cache = self.__dict__.setdefault("_local_mesh_cache", {})
        if not inplace and key in cache and cache[key][0] is self.points and cache[key][1].faces is self.faces:
            return cache[key][1]  # the reference transforms the whole mesh again for every call (meshes.py:1659-1666)
        epsg_4978_to_camera = np.linalg.inv(T)
        pts = np.asarray(self.points, dtype=np.float64)
        local = pts @ epsg_4978_to_camera[:3, :3].T + epsg_4978_to_camera[:3, 3]
        mesh = LocalMesh(local, self.faces, key=key)
        if not inplace:
            cache.clear()
            cache[key] = (self.points, mesh)
        if inplace:
            self.points = local
            self.CRS = None
            return None
        return mesh

    def export_covering_meshes(self, N: int, z_buffer: tuple = (0, 0), subsample: typing.Union[int, None] = None):
        """Upper and lower covering surface of `self.points` (reference: meshes.py:2399-2482): an (N, N) grid over the mesh's
        (x, y) extent, every grid point at the highest (+ z_buffer[0]) and the lowest (+ z_buffer[1]) vertex of its cell,
        `subsample` visiting points[::subsample].  Returns ((upper_points, upper_faces), (lower_points, lower_faces)) in
        place of the reference's two pv.PolyData: the pairs `triangulate_detections(boundaries=...)` takes.  The device does
        the work; rule, errors and the one divergence (Delaunay diagonals) are those of
        `geograypher_amd.utils.geometric.covering_meshes`."""
        from geograypher_amd.utils.geometric import covering_meshes

        # (an empty mesh and arguments that raise need no device: the backend is not created for them)
        backend = self.backend if len(self.points) and len(z_buffer) == 2 and int(N) >= 2 else None
        return covering_meshes(self.points, N, z_buffer, subsample, backend=backend)

    def _ensure_uploaded(self, mesh: LocalMesh, backend=None):
        """Upload `mesh` to `backend` (default: the first) unless that device already holds exactly these arrays.  The cache
        holds strong references and compares identity (`is`) of the point and face arrays: a different array -- also one
        that happens to reuse the id() of a freed temporary -- is always uploaded again."""
        backend = self.backend if backend is None else backend
        held = self._uploaded.get(id(backend))
        if held is None or held[0] is not mesh.points or held[1] is not mesh.faces:
            origin = mesh.origin()
            pts = np.asarray(mesh.points, dtype=np.float64)
            if np.any(origin != 0.0):
                pts = pts - origin
            backend.upload_mesh(pts.astype(np.float32), mesh.faces.astype(np.int32))
            self._uploaded[id(backend)] = (mesh.points, mesh.faces)

    # -- pix2face ------------------------------------------------------------------------------------------------
    def _raster_records(self, cameras, mesh, render_img_scale, near=None, principal_point="center", focal_scaling="scaled",
                        backend=None):
        """Upload the local mesh if needed and pack the (N,16) camera records; returns (records, (h, w))."""
        cameras = _as_camera_set(cameras)
        if mesh is None:
            mesh = self.get_mesh_in_cameras_coords(cameras)
        elif not isinstance(mesh, LocalMesh):
            pts, fcs = _parse_mesh(mesh)
            mesh = LocalMesh(np.asarray(pts, dtype=np.float64), fcs)
        if self.vertex_order == "gl" and principal_point != "center":
            raise ValueError('vertex_order="gl" restates an OpenGL viewport: it needs principal_point="center" (the pyvista camera)')
        self._ensure_uploaded(mesh, backend)
        if near is None:
            near = vtk_like_near_planes(
                np.stack([np.asarray(c.cam_to_world_transform, dtype=np.float64) for c in cameras.cameras]), mesh.bounds()
            )
        records = cameras.get_raster_records(render_img_scale, near=near, principal_point=principal_point,
                                             origin=mesh.origin(), focal_scaling=focal_scaling)
        return records, cameras.cameras[0].get_image_size(render_img_scale)

    def _view_ids(self, backend, cameras, mesh, scale, *, near=None, principal_point="center", focal_scaling="scaled",
                  distortion_set=None, apply_distortion=True):
        """(N, h, w) int32 face ids of a camera or camera set, rasterized -- and, with a `distortion_set` and
        `apply_distortion`, warped -- by `backend`, on `backend.device`.  Everything here that touches a device names
        `backend`: the thread that drives it is the only one that does."""
        records, (h, w) = self._raster_records(cameras, mesh, scale, near=near, principal_point=principal_point,
                                               focal_scaling=focal_scaling, backend=backend)
        ids = backend.raster_face_ids(records, h, w)
        if distortion_set is None or not apply_distortion:
            return ids
        # reference: meshes.py:1842-1854.  A base camera set raises NotImplementedError here, as the reference does
        torch = _torch()
        warped = []
        for i, cam in enumerate(_as_camera_set(cameras).cameras):
            # the id image stays on the device: tensor in, tensor out (gr_warp_nearest_i32)
            out_i = distortion_set.warp_dewarp_image(camera=cam, input_image=ids[i], warped_to_ideal=False, fill_value=-1,
                                                     interpolation_order=0, image_scale=scale, backend=backend)
            warped.append(out_i if isinstance(out_i, torch.Tensor) else torch.as_tensor(np.asarray(out_i)))
        return torch.stack([w.to(torch.int32) for w in warped], dim=0)

    def _driver_ids(self, backend, cameras, mesh, scale, pix2face_kwargs):
        """`_view_ids` for the drivers (render_flat, the view loop, the label path, the table paths), which hold pix2face's
        keywords as their caller gave them; `mesh` is the driver's local mesh, which an explicit `mesh=` keyword replaces.
        A subclass that overrides `pix2face` decides what its views see, so the drivers still ask it -- that route goes
        through `self.backend` whatever `backend` is, and only moves the ids over."""
        _check_pix2face_kwargs(pix2face_kwargs)
        kwargs = {"mesh": mesh, **pix2face_kwargs}
        if type(self).pix2face is not TexturedPhotogrammetryMesh.pix2face:
            ids = self.pix2face(cameras=cameras, render_img_scale=scale, return_tensor=True, **kwargs)
            return backend._dev(ids, _torch().int32)
        return self._view_ids(backend, cameras, kwargs["mesh"], scale, distortion_set=kwargs.get("distortion_set"),
                              apply_distortion=kwargs.get("apply_distortion", True), **_raster_kwargs(kwargs))

    def pix2face(
        self,
        cameras: typing.Union[PhotogrammetryCamera, PhotogrammetryCameraSet],
        mesh=None,
        render_img_scale: float = 1,
        save_to_cache: bool = False,
        cache_folder: typing.Union[None, PATH_TYPE] = CACHE_FOLDER,
        distortion_set: typing.Optional[PhotogrammetryCameraSet] = None,
        apply_distortion: bool = True,
        return_tensor: bool = False,
        near: typing.Union[None, float, typing.List[float]] = None,
        principal_point: str = "center",
        focal_scaling: str = "scaled",
    ):
        """Face hit by the ray through each pixel, per camera (reference: meshes.py:1678-1856).

        Returns an int64 numpy array of shape (h, w) for a single camera or (n_cameras, h, w) for a camera set, with
        -1 where no face is visible and (h, w) = (int(H*scale), int(W*scale)).  With `return_tensor=True` the int32
        device tensor is returned instead (no host copy).  `save_to_cache` / `cache_folder` are accepted for API
        compatibility and unused, as in the reference's own GPU plugin (derived_meshes.py:665-668): rasterizing on
        the GPU is faster than reading a cached array from disk.

        `principal_point="intrinsics"` + `focal_scaling="unscaled"` reproduces the reference's PyTorch3D plugin
        (derived_meshes.py:686-692, 772-780), including its use of the full-resolution focal length on a down-scaled
        image; the defaults reproduce the pyvista path (cameras.py:446-477).
        """
        if distortion_set is None and apply_distortion:
            self.logger.warning("Distortion requested but no distortion parameters provided. Skipping")
            apply_distortion = False
        single = isinstance(cameras, PhotogrammetryCamera)
        if not single and not isinstance(cameras, PhotogrammetryCameraSet):
            raise TypeError()
        ids = self._view_ids(self.backend, cameras, mesh, render_img_scale, near=near, principal_point=principal_point,
                             focal_scaling=focal_scaling, distortion_set=distortion_set, apply_distortion=apply_distortion)
        if not return_tensor:
            ids = _ids_to_host_int64(ids)  # int64 like the reference (meshes.py:1804)
        return ids[0] if single else ids

    # -- render_flat ---------------------------------------------------------------------------------------------
    def render_flat(
        self,
        cameras: typing.Union[PhotogrammetryCamera, PhotogrammetryCameraSet],
        batch_size: int = 1,
        render_img_scale: float = 1,
        return_camera: bool = False,
        return_tensor: bool = False,
        **pix2face_kwargs,
    ):
        """Generator: the face texture seen from each camera, (h, w, C) float64 with NaN where no face is visible
        (reference: meshes.py:1858-1942, including its batch arithmetic).  `return_tensor=True` yields the renders as
        device tensors instead (no 96 MB host copy per 4000 x 3000 channel: the numpy path is bound by the link)."""
        mesh = self.get_mesh_in_cameras_coords(cameras)
        cameras = _as_camera_set(cameras)
        if not isinstance(cameras, PhotogrammetryCameraSet):
            raise TypeError()
        face_texture = self.get_texture(request_vertex_texture=False, try_verts_faces_conversion=True)
        face_texture = np.asarray(face_texture, dtype=np.float64)
        backend, tex_dev = self.backend, None

        for batch_start in range(0, _batched_views(len(cameras), batch_size)[0], batch_size):
            batch_cameras = cameras[batch_start : batch_start + batch_size]
            batch_pix2face = self._driver_ids(backend, batch_cameras, mesh, render_img_scale, pix2face_kwargs)
            if tex_dev is None:
                tex_dev = backend._dev(face_texture, _torch().float64)
            rendered = backend.gather_texture(batch_pix2face, tex_dev)
            if not return_tensor:
                rendered = _to_host(rendered)
            for i in range(rendered.shape[0]):
                if return_camera:
                    yield (rendered[i], batch_cameras[i])
                else:
                    yield rendered[i]

    # -- project_images ------------------------------------------------------------------------------------------
    def _iter_view_inputs(self, backend, cameras, batch_size, aggregate_img_scale, check_null_image, pix2face_kwargs,
                          loader_threads=None, lookups=None):
        """Shared view loop of project_images / aggregate_projected_images (reference: meshes.py:1970-1996) on ONE backend,
        driven by the calling thread: yields (view index, ids (h,w) int32 device tensor, image (h,w,C) device tensor or None
        for a null image, n_channels).  Trailing cameras that do not fill a batch are dropped, as in the reference (1976-1977).
        `lookups` is the call's `_lookup_rule` (default: that of `cameras`, one device thread).

        Input pipeline: the reference converts every image to float64 on the host and the first versions here uploaded that
        (a 4000 x 3000 RGB photo: 36 MB of uint8 blown up to 288 MB, copied from pageable memory, synchronously).  Now the
        image crosses the link in ITS OWN dtype (bool one-hot masks and uint8 photos are 8x smaller than float64) through a
        pinned double buffer; a loader thread fetches and stages view i + 1 (`get_image_by_index`, row blocks copied by a
        small pool) while the device works on view i; the consumers widen to float64 on the device, which is exact for every
        dtype numpy widens exactly."""
        mesh = self.get_mesh_in_cameras_coords(cameras)
        torch = _torch()
        from concurrent.futures import ThreadPoolExecutor

        on_gpu = backend.device.type == "cuda"
        batch_stop, order = _batched_views(len(cameras), batch_size)
        slots = [None, None]        # pinned staging tensors
        slot_free = [None, None]    # event after the last copy out of the slot
        # File-backed photos of a plain camera set (cameras.py:154-174 not overridden): the image is staged in its FILE dtype
        # and `get_image`'s own arithmetic -- / 255.0 for uint8, skimage's resize for aggregate_img_scale != 1 -- runs on the
        # device (HipRaster.resize_image): a 4000 x 3000 RGB photo crosses the link as 36 MB of uint8 instead of a float64
        # image, and no CPU resizer exists in the product.
        native_files = _plain_files(cameras) and hasattr(backend, "resize_image")
        # a loader thread stages view i + 1 while the device works on view i -- only where look-ups are known to be
        # independent (`_lookup_rule`): an arbitrary segmentor may run its own GPU work or keep state that must not run
        # beside pix2face on another thread
        threaded, lookup_lock = lookups or _lookup_rule(cameras)
        native = {"uint8": torch.uint8, "int8": torch.int8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64,
                  "float16": torch.float16, "float32": torch.float32, "float64": torch.float64}

        # file-backed photos: the DECODE (PNG / JPEG inflate, one core per image) is what binds, so a window of the next views
        # is decoded ahead by a pool of threads (PIL releases the interpreter lock while it decodes); staging and upload of
        # view i + 1 still overlap the device work on view i
        import os as _os

        n_dec = int(loader_threads or min(16, _os.cpu_count() or 1)) if native_files else 0
        decoded = {}

        def decode_ahead(pool, pos):
            for p in range(pos, min(pos + max(n_dec, 1), len(order))):
                if p not in decoded:
                    decoded[p] = pool.submit(cameras.get_native_image_by_index, order[p])

        def stage(k, pos, copy_pool):
            """-> (host tensor, n_channels, resize target or None)"""
            resize_to = None
            if native_files:
                decode_ahead(dec_pool, pos)
                img = np.asarray(decoded.pop(pos).result())
                out_hw = (int(img.shape[0] * aggregate_img_scale), int(img.shape[1] * aggregate_img_scale))
                if aggregate_img_scale != 1.0 or img.dtype == np.uint8:
                    resize_to = (out_hw, img.dtype == np.uint8)  # target size, `/ 255.0` first (cameras.py:158-159)
            else:
                img = np.asarray(_locked(lookup_lock, cameras.get_image_by_index, order[pos], aggregate_img_scale))
            n_channels = 1 if img.ndim == 2 else img.shape[-1]
            flat = np.reshape(img, (img.shape[0], img.shape[1], -1))
            if flat.dtype == np.bool_:
                flat = flat.view(np.uint8)
            tdtype = native.get(flat.dtype.name)
            if tdtype is None:  # anything else takes the reference's route: float64 on the host
                flat, tdtype = flat.astype(np.float64), torch.float64
            if not flat.flags.writeable:  # a memory-mapped cache entry: torch wants a writable array
                flat = np.array(flat)
            if not on_gpu:
                return torch.from_numpy(np.ascontiguousarray(flat)), n_channels, resize_to
            if slot_free[k] is not None:
                slot_free[k].synchronize()  # the copy that read this slot two views ago is done
            if slots[k] is None or slots[k].shape != flat.shape or slots[k].dtype != tdtype:
                try:
                    slots[k] = torch.empty(flat.shape, dtype=tdtype, pin_memory=True)
                except RuntimeError:  # no pinned memory left: pageable upload
                    return torch.from_numpy(np.ascontiguousarray(flat)), n_channels, resize_to
            dst = slots[k].numpy()
            rows = flat.shape[0]
            if flat.nbytes >= (32 << 20) and rows >= 8:  # numpy releases the interpreter lock inside large copies
                step = (rows + 7) // 8
                list(copy_pool.map(lambda r0: np.copyto(dst[r0:r0 + step], flat[r0:r0 + step]), range(0, rows, step)))
            else:
                np.copyto(dst, flat)
            return slots[k], n_channels, resize_to

        class _Now:  # a finished "future": staging on the caller's thread
            def __init__(self, value):
                self._value = value

            def result(self):
                return self._value

        with ThreadPoolExecutor(max_workers=1) as loader, ThreadPoolExecutor(max_workers=8) as copy_pool, \
                ThreadPoolExecutor(max_workers=max(n_dec, 1)) as dec_pool:
            def submit(k, pos):
                if pos >= len(order):
                    return None
                return loader.submit(stage, k, pos, copy_pool) if threaded else None

            pending = submit(0, 0)
            pos = 0
            for batch_start in range(0, batch_stop, batch_size):
                batch_inds = list(range(batch_start, batch_start + batch_size))
                batch_cameras = cameras.get_subset_cameras(batch_inds)
                batch_pix2face = self._driver_ids(backend, batch_cameras, mesh, aggregate_img_scale, pix2face_kwargs)
                for i in range(batch_pix2face.shape[0]):
                    if pending is None:  # not threaded: the view is fetched when it is consumed, like the reference does
                        pending = _Now(stage(pos & 1, pos, copy_pool))
                    host, n_channels, resize_to = pending.result()
                    k = pos & 1
                    pos += 1
                    pending = submit(pos & 1, pos)
                    if on_gpu:
                        dev_img = host.to(backend.device, non_blocking=True)
                        if host.is_pinned():
                            slot_free[k] = torch.cuda.Event()
                            slot_free[k].record(torch.cuda.current_stream(backend.device))
                    else:
                        dev_img = host
                    if resize_to is not None:  # get_image's own arithmetic, on the device (cameras.py:158-172)
                        dev_img = backend.resize_image(dev_img, resize_to[0], divide_by_255=resize_to[1])
                    if check_null_image and dev_img.is_floating_point() and not bool(torch.isfinite(dev_img).any()):
                        yield batch_start + i, batch_pix2face[i], None, n_channels
                        continue
                    yield batch_start + i, batch_pix2face[i], dev_img, n_channels

    def project_images(
        self,
        cameras: typing.Union[PhotogrammetryCamera, PhotogrammetryCameraSet],
        batch_size: int = 1,
        aggregate_img_scale: float = 1,
        check_null_image: bool = False,
        **pix2face_kwargs,
    ):
        """Generator: per-face projection of each camera's image, (F, C) float64 with NaN for unseen faces
        (reference: meshes.py:1944-2002).  Per view the LAST pixel (row-major) mapped to a face provides its value;
        with `neg1_is_last_face` background pixels address the last face exactly like numpy's index -1 does."""
        n_faces = self.faces.shape[0]
        loader_threads = pix2face_kwargs.pop("loader_threads", None)
        backend = self.backend
        for _, ids, img, n_channels in self._iter_view_inputs(
            backend, cameras, batch_size, aggregate_img_scale, check_null_image, pix2face_kwargs, loader_threads
        ):
            if img is None:
                yield np.full((n_faces, n_channels), fill_value=np.nan)
            else:
                yield _to_host(backend.project_view(ids, img, neg1_is_last_face=self.neg1_is_last_face))

    @staticmethod
    @contextlib.contextmanager
    def _decoded_cache_scope(cameras, spec):
        """`decoded_cache=` of project_images / aggregate_projected_images: for the duration of the call the camera set's photos
        and its segmentor's label files go through the decoded-input cache (utils/decoded_cache.py); None changes nothing."""
        if spec is None:
            yield
            return
        segmentor = getattr(cameras, "segmentor", None)
        base = getattr(cameras, "base_camera_set", cameras)
        before_seg = getattr(segmentor, "decoded_cache", None) if hasattr(segmentor, "decoded_cache") else None
        before_cams = [getattr(cam, "decoded_cache", None) for cam in getattr(base, "cameras", [])]
        try:
            if hasattr(segmentor, "decoded_cache"):
                segmentor.decoded_cache = spec
            for cam in getattr(base, "cameras", []):
                cam.decoded_cache = spec
            yield
        finally:
            if hasattr(segmentor, "decoded_cache"):
                segmentor.decoded_cache = before_seg
            for cam, old in zip(getattr(base, "cameras", []), before_cams):
                cam.decoded_cache = old

    # -- aggregate_projected_images ------------------------------------------------------------------------------
    def aggregate_projected_images(
        self,
        cameras: typing.Union[PhotogrammetryCamera, PhotogrammetryCameraSet],
        batch_size: int = 1,
        aggregate_img_scale: float = 1,
        return_all: bool = False,
        distributed: bool = False,
        decoded_cache=None,
        **kwargs,
    ):
        """`_aggregate_projected_images` (below: the reference's method) with one more opt-in keyword, `decoded_cache`: None
        (default) -- every pass decodes the label PNGs / photos it reads, like the reference --; True or a folder -- decoded
        inputs are kept as uncompressed `.npy` files keyed by (path, mtime, size, scale) under `CACHE_FOLDER/decoded` (the
        reference's cache root, constants.py:18; its own `save_to_cache` precedent: meshes.py:1759-1770, 1838-1840) or the
        folder, and the second and later passes memory-map them: the host side of a pass is bound by PNG / JPEG inflate
        otherwise (bench `io`)."""
        with self._decoded_cache_scope(cameras, decoded_cache):
            return self._aggregate_projected_images(cameras, batch_size=batch_size, aggregate_img_scale=aggregate_img_scale,
                                                    return_all=return_all, distributed=distributed, **kwargs)

    def _aggregate_projected_images(
        self,
        cameras: typing.Union[PhotogrammetryCamera, PhotogrammetryCameraSet],
        batch_size: int = 1,
        aggregate_img_scale: float = 1,
        return_all: bool = False,
        distributed: bool = False,
        **kwargs,
    ):
        """Average the images of many cameras per face (reference: meshes.py:2004-2084).

        Returns `(average (F,C), {"projection_counts": (F,), "summed_projections": (F,C)[, "all_projections"]})`,
        all float64, NaN for faces no view observed.

        Fast path: when `cameras` can supply class-index images (`get_label_index_image`, e.g. a
        `SegmentorPhotogrammetryCameraSet`) and `return_all` is False, face ids and vote histograms stay on the GPU:
        per view one winner pass + one vote pass in uint32 (bit-exact, order independent), one finalize at the end.
        `distributed=True` (inside an initialised torch.distributed job): this rank handles views rank::world and the
        per-face votes (index labels: [F x (C+1)] int32, bit-identical for every world size) or sums + counts (float
        images: [F x (C+1)] float64) are added with ONE all-reduce (RCCL over xGMI) before finalising.
        """
        from geograypher_amd import distributed as dist_utils

        if len(cameras) == 0 or batch_size > len(cameras):
            raise IndexError("list index out of range")  # what the reference's get_subset_cameras raises here
        rank, world = dist_utils.rank_world() if distributed else (0, 1)
        n_faces = self.faces.shape[0]
        check_null_image = bool(kwargs.pop("check_null_image", False))

        _, view_inds = _batched_views(len(cameras), batch_size)

        loader_threads = kwargs.pop("loader_threads", None)
        _check_pix2face_kwargs(kwargs)
        # The fused path rasterizes with the plain pinhole records.  Whatever else pix2face honours -- a distortion set
        # (unless explicitly switched off), an explicit mesh -- takes the ids of each chunk from `_driver_ids(backend, ...)`,
        # then the unfused winner + vote kernels.
        wants_warp = kwargs.get("distortion_set") is not None and kwargs.get("apply_distortion", True)
        fused_ok = not wants_warp and kwargs.get("mesh") is None
        label_fn = getattr(cameras, "get_label_index_image", None) if not return_all else None
        if label_fn is not None and int(cameras.n_image_channels()) > 255:
            label_fn = None  # class indices do not fit the uint8 label images of the fast path
        first_label = label_fn(view_inds[0], aggregate_img_scale) if label_fn is not None else None

        # devices=[...]: a backend is driven by ONE host thread, and everything that touches a device names its backend.  What
        # the device threads share is settled here, on the caller's thread, before `_on_each_device` starts them: the local
        # mesh (cached), the host distortion maps of every lens among the views (built with the first backend, as the first
        # warp would; afterwards each thread only adds the uploads of its own backend) and the call's one look-up rule
        single_view = len(view_inds) == 1
        backends = self.backends if first_label is not None or not (return_all or single_view) else self.backends[:1]
        mesh = self.get_mesh_in_cameras_coords(cameras)
        if wants_warp:
            for i in view_inds:
                kwargs["distortion_set"].ensure_distortion_map(cameras.cameras[i], image_scale=aggregate_img_scale,
                                                               backend=backends[0])
        lookups = _lookup_rule(cameras, n_device_threads=len(backends))

        if first_label is not None:
            # ---- index-label fast path: uint32 votes on device --------------------------------------------------------
            C = int(cameras.n_image_channels())
            labels_known = {view_inds[0]: first_label}

            def run(backend, inds, first):
                return self._aggregate_label_views(backend, cameras, inds, mesh, C, label_fn, labels_known, batch_size,
                                                   aggregate_img_scale, loader_threads, fused_ok, kwargs, lookups, progress=first)

            # integer sums: the result is the single-device one bit for bit, whatever the number of devices
            votes, counts = _add_on_first(_on_each_device(backends, view_inds[rank::world], run))
            if distributed and world > 1:
                dist_utils.all_reduce_votes(votes, counts)
            avg, summed, cnt = backends[0].finalize_votes(votes, counts)
            return _to_host(avg), {
                "projection_counts": _to_host(cnt),
                "summed_projections": _to_host(summed),
            }

        # ---- general path: float images; nansum + finite-row counts accumulate on device (meshes.py:2057-2067) ----------
        shard = distributed and world > 1 and not single_view
        if shard and return_all:
            raise NotImplementedError("return_all keeps every view's projection: not available with distributed=True")
        projections = []   # every view's own projection, for return_all and for the single view: first device only
        mine = view_inds[rank::world] if shard else view_inds   # the per-view arithmetic does not depend on the other views
        whole = len(backends) == 1 and not shard   # the caller's set in the caller's batches; a share of it goes view by view

        def run(backend, inds, first):
            """The per-view recurrence over `inds` on one device.  The float contract of several devices is that of views
            sharded over processes (include/geograster.h, gr_project_values_f64): counts exact, sums of finite inputs within
            1e-12 relative of the serial result."""
            if not inds:
                return None, None, None
            my_cams, per_batch = (cameras, batch_size) if whole else (cameras.get_subset_cameras(inds), 1)
            gen = self._iter_view_inputs(backend, my_cams, per_batch, aggregate_img_scale, check_null_image, kwargs,
                                         loader_threads, lookups)
            if len(backends) == 1:
                gen = tqdm(gen, total=len(my_cams), desc="Aggregating projected viewpoints")

            def views():
                for _, ids, img, nch in gen:
                    if return_all or single_view:
                        if img is None:
                            projections.append(np.full((n_faces, nch), fill_value=np.nan))
                        else:
                            projections.append(_to_host(backend.project_view(ids, img, neg1_is_last_face=self.neg1_is_last_face)))
                    yield ids, img, nch

            return self._nansum_views(backend, views())

        parts = [p for p in _on_each_device(backends, mine, run) if p[0] is not None]   # a device without views: nothing
        sums, counts = _add_on_first([p[:2] for p in parts]) if parts else (None, None)
        n_channels = parts[0][2] if parts else None
        if shard:
            if sums is None:  # a rank without views still takes part in the collective
                n_channels = int(np.asarray(cameras.get_image_by_index(view_inds[0], aggregate_img_scale)).reshape(
                    cameras.cameras[view_inds[0]].get_image_size(aggregate_img_scale) + (-1,)).shape[-1])
                sums, counts = self._zero_sums(backends[0], n_channels)
            dist_utils.all_reduce_sums(sums, counts)
        avg, summed, cnt = backends[0].finalize_sums(sums, counts)
        avg, summed, cnt = _to_host(avg), _to_host(summed), _to_host(cnt)
        if single_view:
            # the reference keeps the first projection as is (meshes.py:2057-2058): a NaN channel of a seen face survives
            summed = projections[0].astype(float)
            summed[cnt == 0] = np.nan
            with np.errstate(divide="ignore", invalid="ignore"):
                avg = np.divide(summed, np.expand_dims(cnt, 1))
        info = {"projection_counts": cnt, "summed_projections": summed}
        if return_all:
            info["all_projections"] = projections
        return avg, info

    def _zero_sums(self, backend, n_channels):
        torch, n_faces = _torch(), self.faces.shape[0]
        return (torch.zeros((n_faces, n_channels), dtype=torch.float64, device=backend.device),
                torch.zeros((n_faces,), dtype=torch.int32, device=backend.device))

    def _nansum_views(self, backend, views):
        """The per-view recurrence of the float path (meshes.py:2057-2067) on ONE backend: `views` yields (ids, image or None
        for a null image, n_channels); returns that device's (sums (F,C) float64, counts (F,) int32, n_channels), all None
        without a view."""
        sums = counts = n_channels = None
        for ids, img, n_channels in views:
            if sums is None:
                sums, counts = self._zero_sums(backend, n_channels)
            if img is not None:
                backend.project_values(ids, img, sums, counts, neg1_is_last_face=self.neg1_is_last_face)
            else:
                # a skipped (null) image still passes through np.nansum([summed, all-NaN projection]) in the reference
                # (meshes.py:2060-2062), which drops a NaN of the running sum (+inf met -inf) like every other view does
                _torch().nan_to_num_(sums, nan=0.0, posinf=float("inf"), neginf=float("-inf"))
        return sums, counts, n_channels

    def _aggregate_label_views(self, backend, cameras, inds, mesh, C, label_fn, labels_known, batch_size, aggregate_img_scale,
                               loader_threads, fused_ok, kwargs, lookups, progress=True):
        """The index-label fast path of aggregate_projected_images for the views `inds` on ONE backend, driven by the calling
        thread (a `run` of `_on_each_device`): returns that device's (votes (F,C), counts (F,)) int32 tensors.  `lookups` is
        the call's `_lookup_rule`."""
        torch = _torch()
        import os
        from concurrent.futures import ThreadPoolExecutor

        on_gpu = backend.device.type == "cuda"
        thread_safe, lookup_lock = lookups
        self._ensure_uploaded(mesh, backend)
        votes, counts = backend.new_vote_buffers(C)
        if len(inds) == 0:
            return votes, counts
        # launch groups of up to 32 views; a short run is still cut into at least four chunks, so that the loader stages
        # chunk i + 1 while chunk i crosses the link (16 views in ONE chunk ran staging, copy and kernels back to back)
        chunk = max(int(batch_size), min(32, max(1, -(-len(inds) // 4))))
        chunks = [inds[c0 : c0 + chunk] for c0 in range(0, len(inds), chunk)]

        # Input pipeline (row f4).  The label images of a chunk are decoded straight into ONE pinned (n,h,w) uint8
        # staging tensor (no stack / pin copies), by `loader_threads` workers when the look-ups are thread safe (file
        # look-ups and in-memory arrays are; an arbitrary model may not be), while the GPU works on the previous chunk.
        n_workers = int(loader_threads if loader_threads is not None else (min(16, os.cpu_count() or 1) if thread_safe else 1))
        # the label images must have the size the camera records are built for (the reference fails with a shape
        # error in `textured_faces[flat_pix2face] = flat_img` otherwise, meshes.py:1998-2001)
        h0, w0 = cameras.cameras[inds[0]].get_image_size(aggregate_img_scale)

        def check_shape(shape, i):
            if tuple(shape[:2]) != (h0, w0):
                raise ValueError(
                    f"label image of view {i} has shape {tuple(shape[:2])}, but the camera renders {(h0, w0)} at "
                    f"aggregate_img_scale={aggregate_img_scale}"
                )

        def one_label(i):
            return labels_known[i] if i in labels_known else _locked(lookup_lock, label_fn, i, aggregate_img_scale)

        probe = next(iter(labels_known.values()))

        def load_chunk(chunk_inds, img_pool):
            if isinstance(probe, torch.Tensor):  # the segmentor already produces tensors
                labs = [one_label(i) for i in chunk_inds]
                for i, lab in zip(chunk_inds, labs):
                    check_shape(lab.shape, i)
                labs = [torch.where((lab < 0) | (lab > 255), torch.full_like(lab, 255), lab)
                        if lab.dtype != torch.uint8 else lab for lab in labs]
                return torch.stack([lab.to(backend.device, torch.uint8) for lab in labs], dim=0)
            stage = torch.empty((len(chunk_inds), h0, w0), dtype=torch.uint8, pin_memory=on_gpu)
            view = stage.numpy()

            def fill(k):
                lab = np.asarray(one_label(chunk_inds[k]))
                check_shape(lab.shape, chunk_inds[k])
                if lab.dtype != np.uint8:  # an index outside [0, 255] is no class: the ignore value, not a wrapped class
                    lab = np.where((lab < 0) | (lab > 255), 255, lab)
                view[k] = lab  # casts to uint8 while copying

            list(img_pool.map(fill, range(len(chunk_inds))))
            return stage

        steps = range(len(chunks))
        if progress:
            steps = tqdm(steps, total=len(chunks), desc="Aggregating projected viewpoints")
        with ThreadPoolExecutor(max_workers=1) as pool, ThreadPoolExecutor(max_workers=max(n_workers, 1)) as img_pool:
            pending = pool.submit(load_chunk, chunks[0], img_pool)
            for ci in steps:
                lab = pending.result()
                pending = pool.submit(load_chunk, chunks[ci + 1], img_pool) if ci + 1 < len(chunks) else None
                # the chunk's cameras only: a subset of the segmentor wrapper would deep-copy the segmentor with it
                # (segmentor.py:49-55) -- every in-memory label image of an ArrayLabelSegmentor, per chunk
                sub = getattr(cameras, "base_camera_set", cameras).get_subset_cameras(chunks[ci])
                if lab.device.type != backend.device.type:
                    lab = lab.to(backend.device, non_blocking=True)
                if fused_ok:
                    # fused: face ids stay in the rasterizer's LDS tiles, only per-face winners reach HBM
                    records, _ = self._raster_records(sub, mesh, aggregate_img_scale, backend=backend, **_raster_kwargs(kwargs))
                    backend.raster_project_labels(records, lab, C, votes, counts, neg1_is_last_face=self.neg1_is_last_face)
                else:
                    ids = self._driver_ids(backend, sub, mesh, aggregate_img_scale, kwargs)
                    if tuple(ids.shape[-2:]) != (h0, w0):
                        raise ValueError(f"pix2face returned {tuple(ids.shape[-2:])} ids for {(h0, w0)} label images")
                    backend.project_labels(ids, lab, C, votes, counts, neg1_is_last_face=self.neg1_is_last_face)
        return votes, counts

    # the north star's name for the same method
    aggregate_viewpoints = aggregate_projected_images

    # -- label_polygons (DESIGN.md "Polygon labels"; reference: meshes.py:1141-1306) ----------------------------------------
    @staticmethod
    def _squeezed_1d(values):
        """np.squeeze + the reference's one-dimensional check (meshes.py:1181-1191), for arrays and device tensors."""
        values = values.squeeze() if hasattr(values, "detach") else np.squeeze(np.asarray(values))
        if values.ndim != 1:
            raise ValueError(f"Faces labels must be one-dimensional, but is {values.ndim}")
        return values

    def _face_classes(self, face_labels):
        """(class per face: int32 array or tensor, -1 = skip; n_classes).  Non-finite labels are skipped; a finite label must
        be a whole number >= 0."""
        n_faces = self.faces.shape[0]
        if face_labels.shape[0] != n_faces:
            raise ValueError(f"{face_labels.shape[0]} face labels for a mesh of {n_faces} faces")
        if hasattr(face_labels, "detach"):
            torch = _torch()
            labels = face_labels.to(torch.float64)
            finite = torch.isfinite(labels)
            kept = labels[finite]
            bad = bool(((kept != torch.floor(kept)) | (kept < 0)).any()) if kept.numel() else False
            top = float(kept.max()) if kept.numel() else -1.0
            classes = torch.where(finite, labels, torch.full_like(labels, -1.0))
            to_int = lambda c: c.to(torch.int32)
        else:
            labels = np.asarray(face_labels, dtype=np.float64)
            finite = np.isfinite(labels)
            kept = labels[finite]
            bad = bool(np.any((kept != np.floor(kept)) | (kept < 0)))
            top = float(kept.max()) if kept.size else -1.0
            classes = np.where(finite, labels, -1.0)
            to_int = lambda c: c.astype(np.int32)
        if bad:
            raise ValueError("finite face labels must be whole numbers >= 0 (class ids)")
        if top >= 2 ** 31 - 1:
            raise ValueError(f"class id {top:.0f} does not fit the int32 class table")
        return to_int(classes), int(top) + 1

    # -- the face sieve --------------------------------------------------------------------------
    def _labels_like(self, classes, face_labels, return_tensor: bool):
        """int32 classes (-1: unseen) back in the convention of `face_labels`: float64, NaN for unseen, its shape."""
        if hasattr(classes, "detach"):
            torch = _torch()
            labels = torch.where(classes < 0, torch.full((), float("nan"), dtype=torch.float64, device=classes.device),
                                 classes.to(torch.float64)).reshape(tuple(face_labels.shape))
            return labels if return_tensor else labels.cpu().numpy()
        labels = np.where(classes < 0, np.nan, classes.astype(np.float64)).reshape(tuple(face_labels.shape))
        return _torch().as_tensor(labels).to(self.backend.device) if return_tensor else labels

    def face_label_components(self, face_labels, weld_vertices: bool = False, return_tensor: bool = False):
        """The connected regions of a per-face class map (rule I4): (comp (F,) int32 -- the smallest face index of the face's
        component of edge-neighbours of equal label, unseen (NaN) faces forming components of their own kind, -1 for a degenerate
        face --, stats: a dict over `utils.geometric.SIEVE_STAT_NAMES`).  face_labels as `_face_classes` takes them.
        weld_vertices: vertices with bit-equal coordinates count as one (`utils.geometric.weld_canon`), which closes split seams."""
        from geograypher_amd.utils.geometric import face_components, weld_canon

        classes, _ = self._face_classes(self._squeezed_1d(face_labels))
        canon = weld_canon(self.points) if weld_vertices else None
        comp, stats = face_components(np.ascontiguousarray(self.faces, dtype=np.int32), classes, self.backend, canon,
                                      n_vertices=int(self.points.shape[0]), return_tensor=return_tensor)
        self.last_sieve_stats = stats
        return comp, stats

    def sieve_face_labels(self, face_labels, *, min_faces=None, min_area_m2=None, fill_unseen: bool = False, weld_vertices: bool = False,
                          max_rounds: int = 64, return_tensor: bool = False):
        """A per-face class map with its speckle removed (rules I1-I10): every connected region of equal label that is smaller
        than the threshold joins its greatest labelled neighbour region, round after round, until none is left that has one.
        Exactly one threshold: min_faces (a region of fewer faces is small) or min_area_m2 (a region of less surface area, counted
        in mm^2 per face by `utils.geometric.face_area_weights`; the threshold is ceil(min_area_m2 * 1e6)).  fill_unseen: small
        regions of unseen (NaN) faces are filled from their neighbours too; without it they stay and separate what they separate.
        Labels go in and come out in the convention of `_face_classes` and `argmax_nonzero`: float, NaN unseen, (F,) or (F, 1),
        array or device tensor (out: float64; a device tensor with `return_tensor`).  The call's figures are kept in
        `last_sieve_stats`."""
        from geograypher_amd.utils.geometric import SIEVE_AREA_UNITS_PER_M2, face_area_weights, sieve_face_classes, weld_canon

        if (min_faces is None) == (min_area_m2 is None):
            raise ValueError("exactly one of min_faces and min_area_m2 must be given")
        classes, _ = self._face_classes(self._squeezed_1d(face_labels))
        faces = np.ascontiguousarray(self.faces, dtype=np.int32)
        if min_faces is not None:
            if int(min_faces) != min_faces or min_faces < 0:
                raise ValueError(f"min_faces={min_faces!r} is not a whole number >= 0")
            weights, min_measure = None, int(min_faces)
        else:
            if not (min_area_m2 >= 0 and math.isfinite(min_area_m2)):
                raise ValueError(f"min_area_m2={min_area_m2!r} is not a finite area >= 0")
            weights, min_measure = face_area_weights(self.points, faces), int(math.ceil(min_area_m2 * SIEVE_AREA_UNITS_PER_M2))
        canon = weld_canon(self.points) if weld_vertices else None
        class_out, _comp, stats = sieve_face_classes(faces, classes, weights, min_measure, fill_unseen, canon, max_rounds, self.backend,
                                                     n_vertices=int(self.points.shape[0]), return_tensor=True)
        self.last_sieve_stats = stats
        return self._labels_like(class_out, face_labels, return_tensor)

    # -- values from another mesh of the same scene ------------------------------------------------
    @staticmethod
    def _face_centres(points, faces):
        corners = np.asarray(points, dtype=np.float64)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
        return ((corners[:, 0] + corners[:, 1]) + corners[:, 2]) / 3.0   # the expression of get_mesh_points_in_CRS

    def values_from_mesh(self, source, values=None, *, on: typing.Optional[str] = None, max_distance: typing.Optional[float] = None,
                         fill=np.nan, return_index: bool = False):
        """Values of another mesh of the same scene, in the same frame, on this mesh: per-vertex values go to this mesh's vertices by
        the nearest source vertex, per-face values to this mesh's faces by the nearest source face centre (((a + b) + c) / 3.0), the
        lowest row among equally near ones (rules K1-K9: exact, found and gathered on the device).  source: a mesh object or a
        (points, faces) pair.  values: (n,) or (n, k), one row per source vertex or per source face -- which one is inferred from
        the count as `to_current_mesh` does, a count that fits both needs on="vertices" | "faces"; None: the source's texture.
        Rows with no source within `max_distance` (None: no limit) get `fill`; integer values need an integer `fill`.  Returns the
        array (dtype and trailing axes of `values`), with `return_index` also the (n,) int32 source rows, -1 beside `fill`.  The
        call's figures are left in `self.last_transfer_stats`."""
        from geograypher_amd.utils.geometric import gather_rows, nearest_points

        if isinstance(source, (tuple, list)):
            if len(source) != 2:
                raise ValueError("source must be a mesh or a (points, faces) pair")
            src_points, src_faces = np.asarray(source[0], dtype=np.float64), np.asarray(source[1]).reshape(-1, 3)
            source_mesh = None
        else:
            src_points, src_faces = np.asarray(source.points, dtype=np.float64), np.asarray(source.faces).reshape(-1, 3)
            source_mesh = source
        if on not in (None, "vertices", "faces"):
            raise ValueError(f"on={on!r}: 'vertices', 'faces' or None")
        if values is None:
            if source_mesh is None:
                raise ValueError("values=None takes the source's texture: the source must be a mesh object")
            vertex_texture, face_texture = source_mesh.vertex_texture, source_mesh.face_texture
            if on is None:
                if vertex_texture is not None and face_texture is not None:
                    raise ValueError("the source has a vertex texture and a face texture: say which with on='vertices' | 'faces'")
                on = "vertices" if vertex_texture is not None else "faces"
            values = vertex_texture if on == "vertices" else face_texture
            if values is None:
                raise ValueError(f"the source has no texture on its {on}")
        values = np.asarray(_to_host(values) if hasattr(values, "detach") else values)
        if values.ndim == 0:
            raise ValueError("values must have one row per source vertex or face")
        n, n_points, n_faces = values.shape[0], src_points.shape[0], src_faces.shape[0]
        if on is None:
            if n == n_points == n_faces:
                raise ValueError("Cannot infer whether the array belongs to vertices or faces because the number is the same")
            if n == n_points:
                on = "vertices"
            elif n == n_faces:
                on = "faces"
            else:
                raise ValueError(f"{n} values fit neither the {n_points} vertices nor the {n_faces} faces of the source")
        elif n != (n_points if on == "vertices" else n_faces):
            raise ValueError(f"{n} values for the {n_points if on == 'vertices' else n_faces} {on} of the source")
        if values.dtype.kind in "iub":
            if isinstance(fill, (float, np.floating)) and not float(fill).is_integer():
                raise ValueError(f"integer values need an integer fill, got {fill!r}")
            fill = values.dtype.type(fill)
        elif values.dtype.kind not in "fc":
            raise ValueError(f"values of dtype {values.dtype} cannot be transferred")
        if on == "vertices":
            ref, query = src_points, np.asarray(self.points, dtype=np.float64)
        else:
            ref, query = self._face_centres(src_points, src_faces), self._face_centres(self.points, self.faces)
        index, stats = nearest_points(self.backend, ref, query, max_distance=max_distance, return_tensor=True)
        self.last_transfer_stats = dict(stats, on=on)
        out = gather_rows(values, index, fill)
        if return_index:
            return out, np.asarray(_to_host(index) if hasattr(index, "detach") else index, dtype=np.int32)
        return out

    def transfer_texture(self, downsampled_mesh, *, face_textures: bool = False, max_distance: typing.Optional[float] = None):
        """The reference's method (meshes.py:288-323): this mesh's vertex texture is carried onto `downsampled_mesh` -- another
        mesh object of the same scene, coarser or finer --, every vertex of it taking the row of the nearest vertex here
        (`values_from_mesh`), set there as its vertex texture, `IDs_to_labels` with it.  A face texture is, as in the reference, not
        transferred and logs the reference's warning; `face_textures=True` carries it by the nearest face centre.  Vertices or faces
        with nothing within `max_distance` get NaN (an integer texture becomes float64 then).  Returns `downsampled_mesh`."""
        target = downsampled_mesh
        if self.vertex_texture is not None:
            on, texture = "vertices", self.vertex_texture
        elif self.face_texture is not None and face_textures:
            on, texture = "faces", self.face_texture
        else:
            self.logger.warning("Textures not transferred, active scalars data is assoicated with cell data not point data")
            return target
        texture = np.asarray(texture)
        if texture.dtype.kind in "iub" and max_distance is not None:
            texture = texture.astype(np.float64)
        fill = 0 if texture.dtype.kind in "iub" else np.nan   # (an integer texture has no limit here: nothing is filled)
        target.set_texture(target.values_from_mesh(self, texture, on=on, max_distance=max_distance, fill=fill),
                           is_vertex_texture=on == "vertices", delete_existing=False)
        target.IDs_to_labels = self.IDs_to_labels
        return target

    @staticmethod
    def _snap_with_polygons(verts, polygons):
        """Rule P3 / V2: (snapped vertices (V, 2) int64, the polygons' snapped ring table), both on the 1e-6 m grid behind ONE
        integer origin, the middle of their joint bounds."""
        from geograypher_amd.utils.geometric import snap_with_polygons

        return snap_with_polygons(verts, polygons)

    def label_polygon_weights(self, face_labels, polygons, face_weighting=None, sjoin_overlay: bool = True,
                              return_class_labels: bool = True, unknown_class_label: str = "unknown",
                              buffer_dist_meters: float = 2.0, *, points_in_polygon_CRS=None) -> np.ndarray:
        """The (n_polygons, n_classes) float64 matrix behind `label_polygons`: entry (p, c) is the weighted area the faces of
        class c contribute to polygon p (same arguments; `return_class_labels`, `unknown_class_label` and `buffer_dist_meters`
        play no part).  n_classes is the largest finite label + 1.  The pair statistics of the call are left in
        `self.last_polygon_stats` (pairs_tested, pairs_contributing, largest_ring)."""
        from geograypher_amd.utils.geometric import PlanarPolygons

        face_labels = self._squeezed_1d(face_labels)
        if face_weighting is not None:
            face_weighting = self._squeezed_1d(face_weighting)
        if points_in_polygon_CRS is None:
            raise NotImplementedError(
                "label_polygons needs points_in_polygon_CRS: the mesh vertices (V, 3) in the polygons' planar CRS (CRS "
                "reprojection needs pyproj and is outside the projection path)")
        if isinstance(polygons, (str, Path)) or hasattr(polygons, "geometry"):
            raise NotImplementedError(
                "polygon files and GeoDataFrames need geopandas, which is outside the projection path: pass a PlanarPolygons "
                "(geograypher_amd.utils.geometric)")
        if not isinstance(polygons, PlanarPolygons):
            polygons = PlanarPolygons.from_sequence(polygons)
        verts = np.asarray(self._points_in_CRS(points_in_polygon_CRS), dtype=np.float64)
        if verts.shape != (self.points.shape[0], 3):
            raise ValueError(f"points_in_polygon_CRS must be ({self.points.shape[0]}, 3), got {verts.shape}")
        if face_weighting is not None and face_weighting.shape[0] != self.faces.shape[0]:
            raise ValueError(f"{face_weighting.shape[0]} face weights for a mesh of {self.faces.shape[0]} faces")
        classes, n_classes = self._face_classes(face_labels)

        # rule 4: area3D / area2D of the unsnapped corners, in the operation order of utils/numeric.py:305-327
        A, B, C = (verts[self.faces[:, k]] for k in range(3))
        u, v = B - A, C - A
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u0v1_min_u1v0 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
            c0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
            c1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
            area = 1 / 2 * np.sqrt(c0 * c0 + c1 * c1 + u0v1_min_u1v0 * u0v1_min_u1v0)
            ratio = area / (np.abs(u0v1_min_u1v0) / 2)
        if face_weighting is None:
            weight = ratio
        elif hasattr(face_weighting, "detach"):
            torch = _torch()
            fw = face_weighting.to(torch.float64)
            weight = torch.as_tensor(ratio).to(fw.device) * fw
        else:
            weight = ratio * np.asarray(face_weighting, dtype=np.float64)

        vq, table = self._snap_with_polygons(verts, polygons)   # rule 3
        tri = vq[self.faces].reshape(-1, 6)

        weights, stats = self.backend.polygon_class_weights(tri, classes, weight, *table, n_classes, within=bool(sjoin_overlay))
        weights = _to_host(weights) if hasattr(weights, "detach") else np.asarray(weights)
        stats = _to_host(stats) if hasattr(stats, "detach") else np.asarray(stats)
        self.last_polygon_stats = {"pairs_tested": int(stats[0]), "pairs_contributing": int(stats[1]),
                                   "largest_ring": int(stats[2])}
        return np.array(weights, dtype=np.float64).reshape(len(polygons), n_classes)

    def label_polygons(self, face_labels, polygons, face_weighting=None, sjoin_overlay: bool = True,
                       return_class_labels: bool = True, unknown_class_label: str = "unknown",
                       buffer_dist_meters: float = 2.0, *, points_in_polygon_CRS=None):
        """Assign a class to polygons from labels per face (reference: meshes.py:1141-1306; rule-set: DESIGN.md "Polygon
        labels").

        face_labels: (n_faces,) class ids, NaN = no label; numpy or a device tensor (e.g. `backend.argmax_nonzero` of the
        aggregated votes).  polygons: a `geograypher_amd.utils.geometric.PlanarPolygons`, or a sequence its `from_sequence`
        takes; a file path or GeoDataFrame raises NotImplementedError (no geopandas here).  face_weighting: (n_faces,) factors
        multiplied with each face's 3D / 2D area ratio.  sjoin_overlay: True counts the faces that lie entirely within a polygon
        (decided exactly on the 1e-6 m grid), False the area of every face's intersection with it.  buffer_dist_meters: accepted
        and unused (the reference's buffered ROI pre-filter is not reproduced).  points_in_polygon_CRS (required, keyword): the
        mesh vertices (V, 3) in the polygons' planar CRS, x, y in metres, z up -- what the reference gets from
        get_vertices_in_CRS --, or a CRS designator (`WGS84CRS.parse`: the vertices are then reprojected on the device).

        Returns the (n_polygons,) list of the reference: the class with the largest weighted area as a float (the lowest class on
        equality), NaN where nothing contributes; with `return_class_labels` and IDs_to_labels, the label strings, and
        `unknown_class_label` for NaN."""
        weights = self.label_polygon_weights(face_labels, polygons, face_weighting=face_weighting, sjoin_overlay=sjoin_overlay,
                                             buffer_dist_meters=buffer_dist_meters, points_in_polygon_CRS=points_in_polygon_CRS)
        predicted_class_IDs = np.full(weights.shape[0], np.nan)
        if weights.shape[1] > 0:
            best = np.argmax(weights, axis=1)   # the first maximum: groupby + idxmax over ascending class ids
            top = weights[np.arange(weights.shape[0]), best]
            has = top != 0
            predicted_class_IDs[has] = best[has].astype(float)
        predicted_class_IDs = predicted_class_IDs.tolist()
        if return_class_labels and ((IDs_to_labels := self.get_IDs_to_labels()) is not None):
            predicted_class_IDs = [(IDs_to_labels[int(pi)] if np.isfinite(pi) else unknown_class_label)
                                   for pi in predicted_class_IDs]
        return predicted_class_IDs

    # -- vector textures (DESIGN.md "Vector textures"; reference: meshes.py:990-1079) -----------------------------------------
    def face_polygon_index(self, polygons, *, points_in_polygon_CRS=None, return_tensor: bool = False):
        """The polygon row every face CENTRE lies in: (n_faces,) int32, -1 for none; the HIGHEST row where rows overlap, a centre
        on a polygon's boundary (its holes' included) is inside.  polygons: a `PlanarPolygons` or a sequence its `from_sequence`
        takes; points_in_polygon_CRS (required, keyword): the mesh vertices (V, 3) in the polygons' planar CRS, or a CRS designator (`WGS84CRS.parse`: the vertices are then reprojected on the device).  Decided exactly on
        the 1e-6 m grid (rules V1-V5).  `return_tensor=True` leaves the result on the device.  The statistics of the call are left
        in `self.last_vector_stats` (pairs_tested, faces_labelled, longest_cell_list, cells)."""
        from geograypher_amd.utils.geometric import PlanarPolygons, polygon_cell_table

        if points_in_polygon_CRS is None:
            raise NotImplementedError(
                "face_polygon_index needs points_in_polygon_CRS: the mesh vertices (V, 3) in the polygons' planar CRS (CRS "
                "reprojection needs pyproj and is outside the projection path)")
        if isinstance(polygons, (str, Path)) or hasattr(polygons, "geometry"):
            raise NotImplementedError(
                "polygon files and GeoDataFrames need geopandas, which is outside the projection path: pass a PlanarPolygons "
                "(geograypher_amd.utils.geometric)")
        if not isinstance(polygons, PlanarPolygons):
            polygons = PlanarPolygons.from_sequence(polygons)
        verts = np.asarray(self._points_in_CRS(points_in_polygon_CRS), dtype=np.float64)
        if verts.shape != (self.points.shape[0], 3):
            raise ValueError(f"points_in_polygon_CRS must be ({self.points.shape[0]}, 3), got {verts.shape}")
        vq, table = self._snap_with_polygons(verts, polygons)
        cell_table = polygon_cell_table(table[4])
        index, stats = self.backend.face_polygon_index(vq, self.faces.astype(np.int32), *table, cell_table)
        stats = _to_host(stats) if hasattr(stats, "detach") else np.asarray(stats)
        self.last_vector_stats = {"pairs_tested": int(stats[0]), "faces_labelled": int(stats[1]),
                                  "longest_cell_list": int(stats[2]), "cells": (int(cell_table[0][4]), int(cell_table[0][5]))}
        if return_tensor:
            return index
        index = _to_host(index) if hasattr(index, "detach") else np.asarray(index)
        return np.array(index, dtype=np.int32)

    def get_values_for_faces_from_vector(self, vector_source, column_names, *, points_in_polygon_CRS=None):
        """The value of a polygon column at every face centre (reference: meshes.py:990-1079; rule V6).  vector_source: a
        `.geojson` path (`PlanarPolygons.from_geojson`) or a `(PlanarPolygons, {column: array})` pair; other files and
        GeoDataFrames raise NotImplementedError.  column_names: a name, a list of names, or None when there is exactly one
        column.  A face in no polygon gets "null" (str / object columns), NULL_TEXTURE_INT_VALUE (integer columns) or NaN; the
        result has the column's dtype (object for strings).  One column returns (labeled_faces, all_values), several return two dicts."""
        from geograypher_amd.utils.geometric import PlanarPolygons

        if isinstance(vector_source, (tuple, list)) and len(vector_source) == 2 and isinstance(vector_source[1], dict):
            polygons, properties = vector_source
        elif isinstance(vector_source, (str, Path)) and Path(vector_source).suffix == ".geojson":
            polygons, properties = PlanarPolygons.from_geojson(vector_source)
        else:
            raise NotImplementedError(
                "vector files other than .geojson and GeoDataFrames need geopandas, which is outside the projection path: pass "
                "a .geojson path or a (PlanarPolygons, {column: values}) pair")
        if column_names is None:
            if len(properties) != 1:
                self.logger.error("No column name provided and ambigious which column to use")
                raise ValueError("No column name provided and ambigious which column to use")
            column_names = list(properties)
        elif isinstance(column_names, str):
            column_names = [column_names]
        index = self.face_polygon_index(polygons, points_in_polygon_CRS=points_in_polygon_CRS)
        inside = index >= 0
        labeled_faces, all_values = {}, {}
        for name in column_names:
            column = np.asarray(properties[name])
            if len(column) != len(polygons):
                raise ValueError(f"column {name!r} has {len(column)} values for {len(polygons)} polygons")
            if column.dtype.kind in "US":   # a fixed-width string column would cut "null" short
                column = column.astype(object)
            if column.dtype.kind == "O":
                null_value = "null"
            elif column.dtype.kind in "iu":
                null_value = NULL_TEXTURE_INT_VALUE
            else:
                null_value = np.nan
            values = np.full(shape=index.shape[0], dtype=column.dtype, fill_value=null_value)
            values[inside] = column[index[inside]]
            labeled_faces[name], all_values[name] = values, column
        if len(column_names) == 1:
            return labeled_faces[column_names[0]], all_values[column_names[0]]
        return labeled_faces, all_values

    # -- class outlines (reference: meshes.py:1308-1445) -------------------------------------------------
    def _outline_call(self, vq, faces, classes, n_classes, points, members=None):
        """One backend call and what the host adds to it: (ring_offsets, class index per ring, ring_vertex_ids, ring_xy,
        ring_is_hole, stats words, twice the exact area per ring as Python integers) as host arrays.  members = (face_ptr,
        face_members): `member_outlines` on that table instead of `class_outlines` on `classes`."""
        from geograypher_amd.utils.geometric import ring_areas2_exact

        if members is not None:
            _, ring_vertices, ring_offsets, ring_class, stats = self.backend.member_outlines(vq, faces, *members, n_classes)
        else:
            _, ring_vertices, ring_offsets, ring_class, stats = self.backend.class_outlines(vq, faces, classes, n_classes)
        ring_vertices = np.array(_host_array(ring_vertices), dtype=np.int32)
        ring_offsets = np.array(_host_array(ring_offsets), dtype=np.int64)
        ring_class = np.array(_host_array(ring_class), dtype=np.int64)
        areas2 = ring_areas2_exact(vq[ring_vertices], ring_offsets)
        is_hole = np.array([a < 0 for a in areas2], dtype=bool)
        return (ring_offsets, ring_class, ring_vertices, points[ring_vertices, :2], is_hole, np.array(_host_array(stats), dtype=np.int64),
                areas2)

    def face_label_outlines(self, face_labels=None, *, points_in_export_CRS, drop_nan: bool = True, return_tensor: bool = False):
        """The outline rings of every class of a per-face labelling, traced on the device (rules X1-X7 of DESIGN.md section 8i): a
        `geograypher_amd.utils.geometric.FaceLabelOutlines`.

        face_labels: (F,) or (F, 1) class ids, float or int, NaN = no label, numpy or a device tensor; None: the mesh's face
        texture; (F, C) with C > 1: many-hot, one call per column with a value > 0, a face takes part where its value is > 0 and
        `ring_class` is the column; a `scipy.sparse` matrix or array (F, C) of any format and any C: many-hot too (duplicates are
        summed, then the entries > 0 count), traced in ONE `member_outlines` call whatever C (at most 2^31 - 2 columns, fewer than
        2^31 / 3 entries; a backend without `member_outlines` gets a call per non-empty column).  points_in_export_CRS (required, keyword): the V vertices (V, 2 | 3) in the planar CRS of the
        export, metres, or a CRS designator (`WGS84CRS.parse`: the vertices are then reprojected on the device); z is not used.  drop_nan=False: the faces without a label form one more class, reported with id NaN.
        A wrong number of labels is a ValueError.  Filled with the non-zero rule, the rings of a class are the union of its faces
        in plan view on the 1e-6 m grid; where a class overlaps itself in plan view its rings overlap too.  `return_tensor=True`
        returns the arrays as tensors on the backend's device.  The counters are also left in `self.last_outline_stats`."""
        from geograypher_amd.utils.geometric import (MEMBER_MAX_CLASSES, OUTLINE_MAX_CLASSES, FaceLabelOutlines, csr_members, is_sparse,
                                                     snap_points)

        if face_labels is None:
            face_labels = self.get_texture(request_vertex_texture=False)
            if face_labels is None:
                raise ValueError("face_label_outlines: no face labels given and the mesh has no face texture")
        n_faces = self.faces.shape[0]
        if face_labels.shape[0] != n_faces:
            raise ValueError(f"{face_labels.shape[0]} face labels for a mesh of {n_faces} faces")
        if points_in_export_CRS is None:
            raise NotImplementedError(
                "face_label_outlines needs points_in_export_CRS: the mesh vertices (V, 2 | 3) in the planar CRS of the export (CRS "
                "reprojection needs pyproj and is outside the projection path)")
        points = np.asarray(self._points_in_CRS(points_in_export_CRS), dtype=np.float64)
        if points.ndim != 2 or points.shape[0] != self.points.shape[0] or points.shape[1] not in (2, 3):
            raise ValueError(f"points_in_export_CRS must be ({self.points.shape[0]}, 2) or ({self.points.shape[0]}, 3), got {points.shape}")
        vq = snap_points(points)   # X1
        faces = np.ascontiguousarray(self.faces, dtype=np.int32)
        on_device = hasattr(face_labels, "detach")
        sparse_labels = is_sparse(face_labels)
        if face_labels.ndim > 2:
            raise ValueError(f"face labels must be (F,), (F, 1) or (F, C), got {tuple(face_labels.shape)}")
        parts = []
        if sparse_labels:   # a sparse many-hot (F, C): the members with a value > 0, traced in one call (section 8l)
            face_ptr, face_members = csr_members(face_labels)
            if hasattr(self.backend, "member_outlines"):
                if face_labels.shape[1] > MEMBER_MAX_CLASSES or 3 * len(face_members) >= 2 ** 31:
                    raise ValueError(f"a sparse ({n_faces}, {face_labels.shape[1]}) labelling with {len(face_members)} entries > 0: "
                                     f"one call takes at most {MEMBER_MAX_CLASSES} columns and fewer than 2^31 / 3 entries")
                out = self._outline_call(vq, faces, None, int(face_labels.shape[1]), points, members=(face_ptr, face_members))
                parts.append((out, out[1].astype(np.float64)))
            else:   # an older backend: a call per non-empty column, as for a dense array
                face_of_member = np.repeat(np.arange(n_faces), np.diff(face_ptr))
                order = np.argsort(face_members, kind="stable")
                columns, starts = np.unique(face_members[order], return_index=True)
                for column, rows in zip(columns.tolist(), np.split(face_of_member[order], starts[1:])):
                    classes = np.full(n_faces, -1, dtype=np.int32)
                    classes[rows] = 0
                    out = self._outline_call(vq, faces, classes, 1, points)
                    parts.append((out, np.full(len(out[1]), float(column))))
        elif face_labels.ndim == 2 and face_labels.shape[1] != 1:   # many-hot
            for column in range(face_labels.shape[1]):
                member = face_labels[:, column] > 0
                if not bool(member.any()):
                    continue
                classes = member.to(_torch().int32) - 1 if on_device else member.astype(np.int32) - 1
                out = self._outline_call(vq, faces, classes, 1, points)
                parts.append((out, np.full(len(out[1]), float(column))))
        else:
            labels = face_labels.reshape(-1)
            if on_device:
                torch = _torch()
                labels = labels.to(torch.float64)
                nan = torch.isnan(labels)
                ids = torch.unique(labels[~nan])
                classes = torch.searchsorted(ids, torch.where(nan, torch.zeros_like(labels), labels)).to(torch.int32)
                classes = torch.where(nan, torch.full_like(classes, -1 if drop_nan else int(ids.numel())), classes)
                ids = ids.cpu().numpy()
                any_nan = bool(nan.any())
            else:
                labels = np.asarray(labels, dtype=np.float64)
                nan = np.isnan(labels)
                ids = np.unique(labels[~nan])
                classes = np.searchsorted(ids, np.where(nan, 0.0, labels)).astype(np.int32)
                classes = np.where(nan, np.int32(-1 if drop_nan else len(ids)), classes).astype(np.int32)
                any_nan = bool(nan.any())
            if ids.size and (not np.all(np.isfinite(ids)) or np.any(ids != np.floor(ids)) or ids.min() < 0):
                raise ValueError("face labels must be whole numbers >= 0 (class ids) or NaN")
            ids = np.concatenate([ids, [np.nan]]) if (any_nan and not drop_nan) else ids
            if len(ids) > OUTLINE_MAX_CLASSES:
                raise ValueError(f"{len(ids)} distinct classes: one call takes at most {OUTLINE_MAX_CLASSES}")
            out = self._outline_call(vq, faces, classes, len(ids), points)
            parts.append((out, ids[out[1]] if len(out[1]) else np.zeros(0)))
        shift, offsets, stats = 0, [np.zeros(1, dtype=np.int64)], np.zeros(8, dtype=np.int64)
        for out, _ in parts:
            offsets.append(out[0][1:] + shift)
            shift += int(out[0][-1])
            stats = stats + out[5]

        def joined(k, dtype, tail=()):
            chosen = [out[k] for out, _ in parts]
            return np.concatenate(chosen).astype(dtype) if chosen else np.zeros((0, *tail), dtype=dtype)

        ring_offsets = np.concatenate(offsets)
        ring_class = np.concatenate([ids_ for _, ids_ in parts]).astype(np.float64) if parts else np.zeros(0)
        stats = {"faces_without_class": int(stats[0]), "zero_area_faces": int(stats[1]), "turned_faces": int(stats[2]),
                 "cancelled_edge_pairs": int(stats[3]), "multi_edges": int(stats[4]), "edges": int(ring_offsets[-1]),
                 "rings": len(ring_offsets) - 1, "calls": len(parts)}
        self.last_outline_stats = stats
        fields = [ring_offsets, ring_class, joined(2, np.int32), joined(3, np.float64, (2,)), joined(4, bool)]
        snapped = (vq[fields[2]], [a for out, _ in parts for a in out[6]])   # what the nesting of X8 works on
        if return_tensor:
            torch = _torch()
            device = getattr(self.backend, "device", None)
            fields = [torch.as_tensor(a).to(device) if device is not None else torch.as_tensor(a) for a in fields]
        return FaceLabelOutlines(*fields, stats, snapped)

    def export_face_labels_vector(self, face_labels=None, export_file: PATH_TYPE = None, export_crs=None, label_names=None,
                                  ensure_non_overlapping: bool = False, simplify_tol: float = 0.0, drop_nan: bool = True,
                                  vis: bool = False, *, points_in_export_CRS, simplify_method: typing.Optional[str] = None):
        """Export the labels per face as one multipolygon per class (reference: meshes.py:1308-1445; rules X1-X8 of DESIGN.md
        section 8i): `(PlanarPolygons, columns)` in the shape `PlanarPolygons.from_geojson` returns -- one row per present class in
        ascending order (the NaN class last), every hole behind the exterior it lies in; a hole no exterior of its class holds
        is a row of its own behind them (`self.last_outline_stats["orphan_holes"]`).  columns: CLASS_ID_KEY (float64, NaN for the
        NaN class) and, with `label_names`, CLASS_NAMES_KEY (`label_names[int(id)]`, "nan" for NaN).  The coordinates are those
        of `points_in_export_CRS`, which also names the CRS: `export_crs` must be None or equal what the caller passes the points
        in.  `export_file` ending in `.geojson` is written as a FeatureCollection of MultiPolygon features (`json`).  Other
        extensions, ensure_non_overlapping, vis and a reprojection raise NotImplementedError.  Where a class
        overlaps itself in plan view (a crown above ground of the same class) its rings overlap: the output is then right under
        the non-zero fill rule only and is not an OGC-valid polygon.

        simplify_method="douglas-peucker" (any other name: ValueError) simplifies the rings at `simplify_tol` metres with the
        exact Douglas-Peucker of DESIGN.md section 8q, on the device, where the reference calls `geometry.simplify`
        (meshes.py:1417): the rings are nested first (X8), then simplified with the junctions of the class map fixed (S9), so
        two classes keep the same vertices along a shared border; a ring that collapses (S6) is left out, the holes of a
        collapsed exterior with it, and a class left without rings loses its row.  `self.last_outline_stats` gains the words
        of the call (simplify_kept_vertices, simplify_collapsed_rings, simplify_passes, ...).  Without simplify_method,
        simplify_tol > 0 raises NotImplementedError: GEOS's topology-preserving simplifier is not built."""
        from geograypher_amd.utils.geometric import (PlanarPolygons, check_simplify_method, nest_outline_rings,
                                                     write_geojson_multipolygons)

        if ensure_non_overlapping:
            raise NotImplementedError("ensure_non_overlapping: resolving classes that overlap in plan view needs a polygon overlay "
                                      "(geopandas), which is outside the projection path; export_face_labels_raster answers it "
                                      "in raster form (the surface seen from above wins)")
        if simplify_method is not None:
            check_simplify_method(simplify_method)
        elif simplify_tol > 0:
            raise NotImplementedError("simplify_tol: shapely's simplification is outside the projection path; ask for the exact "
                                      "Douglas-Peucker by name: simplify_method='douglas-peucker'")
        if vis:
            raise NotImplementedError("vis: plotting needs geopandas and matplotlib, which are outside the projection path")
        if export_crs is not None:
            raise NotImplementedError(f"export_crs={export_crs!r}: reprojection needs pyproj, which is outside the projection path; "
                                      "pass points_in_export_CRS in the CRS of the export and leave export_crs as None")
        if export_file is not None and Path(export_file).suffix != ".geojson":
            raise NotImplementedError(f"export_file {export_file}: files other than .geojson need geopandas, which is outside the "
                                      "projection path")
        outlines = self.face_label_outlines(face_labels, points_in_export_CRS=points_in_export_CRS, drop_nan=drop_nan)
        ids = outlines.ring_class
        order = sorted(set(ids[np.isfinite(ids)].tolist())) + ([np.nan] if np.isnan(ids).any() else [])
        row_of = {(-1.0 if np.isnan(v) else v): k for k, v in enumerate(order)}
        class_row = np.array([row_of[-1.0 if np.isnan(v) else v] for v in ids.tolist()], dtype=np.int64)
        off = outlines.ring_offsets
        areas2, home = nest_outline_rings(outlines.snapped[0], off, class_row, areas2=outlines.snapped[1])   # X8
        holes_of = {}
        for r in np.nonzero(home >= 0)[0]:
            holes_of.setdefault(int(home[r]), []).append(int(r))
        shown = outlines   # the rings that are written: the traced ones, or (S9) their simplification -- same rings, fewer vertices
        if simplify_method is not None:
            shown = outlines.simplified(simplify_tol, self.backend, shared_borders=True)
        s_off = shown.ring_offsets
        rings, rows, holes, row_class = [], [], [], list(order)
        for r in range(len(ids)):   # every exterior, followed by its holes; an orphan hole: a row of its own behind the class rows
            is_orphan = areas2[r] < 0 and home[r] < 0
            if (areas2[r] > 0 or is_orphan) and s_off[r + 1] > s_off[r]:   # (a collapsed exterior takes its holes with it)
                row = int(class_row[r])
                if is_orphan:
                    row = len(row_class)
                    row_class.append(order[int(class_row[r])])
                for k, ring in enumerate([r] + holes_of.get(r, [])):
                    if s_off[ring + 1] > s_off[ring]:
                        rings.append(shown.ring_xy[s_off[ring]:s_off[ring + 1]])
                        rows.append(row)
                        holes.append(k > 0)
        n_orphans = len(row_class) - len(order)   # (an orphan's row is made for a ring that is written)
        if simplify_method is not None:   # a class left without rings loses its row
            used = np.unique(np.asarray(rows, dtype=np.int64))
            rows = np.searchsorted(used, rows).tolist()
            row_class = [row_class[k] for k in used.tolist()]
        polygons = PlanarPolygons(rings, rows, holes, n_polygons=len(row_class))
        class_ids = np.array(row_class, dtype=np.float64)
        columns = {CLASS_ID_KEY: class_ids}
        if label_names is not None:
            names = np.empty(len(row_class), dtype=object)
            names[:] = [(label_names[int(v)] if np.isfinite(v) else "nan") for v in class_ids.tolist()]
            columns[CLASS_NAMES_KEY] = names
        self.last_outline_stats = dict(shown.stats, orphan_holes=n_orphans, rows=len(row_class))
        if export_file is not None:
            write_geojson_multipolygons(export_file, polygons, columns)
        return polygons, columns

    # -- the mesh seen from above on a raster grid (rules N1-N9; the reference has no counterpart) -----
    def _top_down_grid(self, like, resolution, points_in_raster_CRS, what: str):
        """(points (V, 3) float64 in the grid's CRS, (height, width, transform), the EPSG code to write or None) of the three
        top-down raster methods: the grid is `like` or, with `resolution`, `grid_from_bounds` over the vertices -- exactly one of
        the two.  The code is the grid's; without one, that of a CRS designator given for the points."""
        from geograypher_amd.utils.geospatial import WGS84CRS, _grid_like, grid_from_bounds, is_CRS_designator

        if (like is None) == (resolution is None):
            raise ValueError(f"{what} takes the grid (like=) or a cell size (resolution=), exactly one of the two")
        if points_in_raster_CRS is None:
            raise NotImplementedError(
                f"{what} needs points_in_raster_CRS: the mesh vertices (V, 3) in the grid's CRS, or a CRS designator")
        points = np.ascontiguousarray(self._points_in_CRS(points_in_raster_CRS), dtype=np.float64)
        if points.shape != (self.points.shape[0], 3):
            raise ValueError(f"points_in_raster_CRS must be ({self.points.shape[0]}, 3), got {points.shape}")
        if like is None:
            like = grid_from_bounds(points[:, :2], resolution)
        height, width, transform, epsg = _grid_like(like)
        if epsg is None and is_CRS_designator(points_in_raster_CRS):
            epsg = WGS84CRS.parse(points_in_raster_CRS).epsg
        return points, (height, width, tuple(transform)), epsg

    def top_down_face_raster(self, like=None, *, resolution=None, points_in_raster_CRS, return_tensor: bool = False):
        """The mesh seen from above on a raster grid, on the device (`utils.geospatial.top_down_raster`; rules N1-N9 of DESIGN.md
        section 8r): (face_ids (H, W) int32, the face whose surface is highest at the cell's centre, -1 where there is none;
        heights (H, W) float64, that height in the units of the points' z, NaN there; transform (a, b, c, d, e, f) of the grid).
        like: the grid -- a `PlanarRaster`, a GeoTIFF path (header only) or ((H, W), transform) --, or resolution: the cell size of
        a north-up grid over the vertices' bounds (`grid_from_bounds`).  points_in_raster_CRS (required, keyword): the mesh
        vertices (V, 3) in the grid's CRS, or a CRS designator (the vertices are then reprojected on the device).  The statistics
        of the call are left in `self.last_top_down_stats`."""
        from geograypher_amd.utils.geospatial import top_down_raster

        points, (height, width, transform), _epsg = self._top_down_grid(like, resolution, points_in_raster_CRS, "top_down_face_raster")
        face_ids, heights, stats = top_down_raster(points, np.ascontiguousarray(self.faces, dtype=np.int32), ((height, width), transform),
                                                   backend=self.backend, return_tensor=return_tensor)
        self.last_top_down_stats = stats
        return face_ids, heights, transform

    def export_surface_height_raster(self, export_file: PATH_TYPE = None, *, like=None, resolution=None, points_in_raster_CRS,
                                     nodata: float = -9999.0):
        """The digital surface model of the mesh: a float64 `PlanarRaster` of the highest surface at every cell centre (arguments
        as `top_down_face_raster`), `nodata` where no face holds the centre.  `export_file` (.tif / .tiff) is written as a float32
        GeoTIFF with the transform, nodata and, where known, the EPSG code, which `PlanarRaster.from_geotiff` reads back."""
        from geograypher_amd.utils.raster import PlanarRaster
        from geograypher_amd.utils.tiff import write_tiff_deflate

        nodata = float(nodata)
        if not np.isfinite(nodata) or np.float64(np.float32(nodata)) != nodata:
            raise ValueError(f"nodata={nodata!r} is not a finite value a float32 file can hold")
        _check_tiff_suffix(export_file)
        points, (height, width, transform), epsg = self._top_down_grid(like, resolution, points_in_raster_CRS,
                                                                        "export_surface_height_raster")
        from geograypher_amd.utils.geospatial import top_down_raster

        _ids, heights, stats = top_down_raster(points, np.ascontiguousarray(self.faces, dtype=np.int32), ((height, width), transform),
                                               backend=self.backend)
        self.last_top_down_stats = stats
        heights = np.where(np.isnan(heights), nodata, heights)
        if export_file is not None:
            write_tiff_deflate(export_file, heights.astype(np.float32), transform=transform, nodata=nodata, epsg=epsg)
        return PlanarRaster(heights, transform, nodata, epsg)

    def export_canopy_height_raster(self, DTM_file, export_file: PATH_TYPE = None, *, like=None, resolution=None, points_in_raster_CRS,
                                    dtm_CRS=None, return_tensor: bool = False):
        """Canopy height as a DSM - DTM product: the surface heights of `top_down_raster` on the grid (arguments as
        `top_down_face_raster`) minus band 0 of the DTM warped bilinearly onto the same grid (`utils.geospatial.warp_raster`; rules
        W1-W9 of DESIGN.md section 8t) -> a float64 `PlanarRaster` with nodata -9999 where no face holds the centre or the DTM has
        no value (with `return_tensor`: the (H, W) float64 tensor on the backend's device, NaN there, instead).  DTM_file: a
        single-band GeoTIFF path or a `PlanarRaster`; dtm_CRS: the DTM's CRS where the file names none.  The DTM is reprojected where
        its CRS and the grid's are both known and differ; exactly one known is a ValueError.  `export_file` (.tif / .tiff) is
        written as a float32 GeoTIFF with nodata -9999, like `export_surface_height_raster`."""
        from geograypher_amd.utils.geospatial import _as_planar_raster, top_down_raster, warp_raster
        from geograypher_amd.utils.raster import PlanarRaster
        from geograypher_amd.utils.tiff import write_tiff_deflate

        nodata = -9999.0
        _check_tiff_suffix(export_file)
        points, (height, width, transform), epsg = self._top_down_grid(like, resolution, points_in_raster_CRS,
                                                                        "export_canopy_height_raster")
        _ids, surface, stats = top_down_raster(points, np.ascontiguousarray(self.faces, dtype=np.int32), ((height, width), transform),
                                               backend=self.backend, return_tensor=return_tensor)
        self.last_top_down_stats = stats
        dtm = _as_planar_raster(DTM_file)
        first = PlanarRaster(dtm.data[:1], dtm.transform, dtm.nodata, dtm.epsg)
        ground = warp_raster(first, ((height, width), transform), src_crs=dtm_CRS if dtm_CRS is not None else dtm.epsg, dst_crs=epsg,
                             resampling="bilinear", dst_nodata=float("nan"), backend=self.backend, return_tensor=return_tensor)
        self.last_warp_stats = ground.last_warp_stats
        canopy = surface - ground.data[0]     # NaN where either is missing
        if return_tensor and export_file is None:
            return canopy
        filled = np.asarray(canopy.cpu() if hasattr(canopy, "cpu") else canopy, dtype=np.float64)
        filled = np.where(np.isnan(filled), nodata, filled)
        if export_file is not None:
            write_tiff_deflate(export_file, filled.astype(np.float32), transform=transform, nodata=nodata, epsg=epsg)
        return canopy if return_tensor else PlanarRaster(filled, transform, nodata, epsg)

    def export_face_labels_raster(self, face_labels=None, export_file: PATH_TYPE = None, *, like=None, resolution=None,
                                  points_in_raster_CRS, nodata: int = 255, drop_nan: bool = True):
        """The per-face classes as a class raster seen from above: a `PlanarRaster` whose band holds the class of the face whose
        surface is highest at every cell centre (uint8 values), `nodata` where no face holds the centre or -- with `drop_nan` --
        the winning face has no label; drop_nan=False is a ValueError when such a face wins a cell (a uint8 raster has no NaN
        class).  Where classes overlap in plan view the upper surface wins: this is the raster answer to what
        `export_face_labels_vector(ensure_non_overlapping=True)` asks.  face_labels: (F,) or (F, 1) class ids, NaN = no label;
        None: the mesh's face texture.  A class above 254 or equal to `nodata`, a `nodata` outside [0, 255]: ValueError.  Grid
        and points as `top_down_face_raster`.  `export_file` (.tif / .tiff) is written as a uint8 GeoTIFF with the transform,
        nodata and, where known, the EPSG code."""
        from geograypher_amd.utils.geospatial import top_down_raster
        from geograypher_amd.utils.raster import PlanarRaster
        from geograypher_amd.utils.tiff import write_tiff_deflate

        if isinstance(nodata, bool) or nodata != int(nodata) or not 0 <= int(nodata) <= 255:
            raise ValueError(f"nodata={nodata!r} is not an integer in [0, 255]")
        nodata = int(nodata)
        _check_tiff_suffix(export_file)
        if face_labels is None:
            face_labels = self.get_texture(request_vertex_texture=False)
            if face_labels is None:
                raise ValueError("export_face_labels_raster: no face labels given and the mesh has no face texture")
        classes, n_classes = self._face_classes(self._squeezed_1d(face_labels))
        classes = _host_array(classes).astype(np.int64)
        if n_classes - 1 > 254:
            raise ValueError(f"class id {n_classes - 1} does not fit a uint8 class raster (at most 254)")
        if np.any(classes == nodata):
            raise ValueError(f"class id {nodata} is the raster's nodata value; choose another nodata")
        points, (height, width, transform), epsg = self._top_down_grid(like, resolution, points_in_raster_CRS,
                                                                        "export_face_labels_raster")
        face_ids, _heights, stats = top_down_raster(points, np.ascontiguousarray(self.faces, dtype=np.int32), ((height, width), transform),
                                                    backend=self.backend)
        self.last_top_down_stats = stats
        cell_class = np.where(face_ids >= 0, classes[np.maximum(face_ids, 0)] if len(classes) else -1, -2)   # -1: no label, -2: no face
        if not drop_nan and np.any(cell_class == -1):
            raise ValueError(f"{int(np.sum(cell_class == -1))} cells are won by a face without a label, and a uint8 class raster has "
                             "no NaN class: keep drop_nan=True (they become nodata)")
        out = np.where(cell_class >= 0, cell_class, nodata).astype(np.uint8)
        if export_file is not None:
            write_tiff_deflate(export_file, out, transform=transform, nodata=nodata, epsg=epsg)
        return PlanarRaster(out, transform, nodata, epsg)

    # -- raster samples (DESIGN.md "Raster samples"; reference: meshes.py:1449-1629) ---------------------------------------------
    def add_label(self, label_name, label_ID):
        """reference: meshes.py:733-735 -- nothing for a NaN ID; beyond it, a numeric ID on a mesh without a table starts one
        (the reference fails there: None has no items)."""
        if isinstance(label_ID, float) and np.isnan(label_ID):
            return
        if self.IDs_to_labels is None:
            self.IDs_to_labels = {}
        self.IDs_to_labels[label_ID] = label_name

    def _sample_raster(self, raster_file, use_vertex_locations, points_in_raster_CRS, what, nodata_fill_value=np.nan, **kwargs):
        """The backend's sample_raster for this mesh: (values, height, labels, stats as the backend returns them, points (V, 3))."""
        from geograypher_amd.utils.raster import PlanarRaster

        if points_in_raster_CRS is None:
            raise NotImplementedError(
                f"{what} needs points_in_raster_CRS: the mesh vertices (V, 3) in the raster's CRS (CRS reprojection needs pyproj "
                "and is outside the projection path)")
        raster = raster_file if isinstance(raster_file, PlanarRaster) else PlanarRaster.from_geotiff(raster_file)
        points = np.ascontiguousarray(self._points_in_CRS(points_in_raster_CRS), dtype=np.float64)
        if points.shape != (self.points.shape[0], 3):
            raise ValueError(f"points_in_raster_CRS must be ({self.points.shape[0]}, 3), got {points.shape}")
        faces = None if use_vertex_locations else np.ascontiguousarray(self.faces, dtype=np.int32)
        values, height, labels, stats = self.backend.sample_raster(points, faces, raster.data, raster.inverse, raster.nodata,
                                                                   float(nodata_fill_value), **kwargs)
        stats_h = _host_array(stats)
        self.last_raster_stats = {"queries": int(points.shape[0] if faces is None else faces.shape[0]), "inside": int(stats_h[0]),
                                  "nodata": int(stats_h[1]), "ground": int(stats_h[2]), "bad_faces": int(stats_h[3])}
        return values, height, labels, points

    def get_values_from_raster_file(self, raster_file, use_vertex_locations: bool = False, return_mesh_points: bool = False,
                                    nodata_fill_value: float = np.nan, *, points_in_raster_CRS=None):
        """The value of a raster under every face centre, or vertex (reference: meshes.py:1449-1499; rules T1-T5): (N,) float64
        for one band, (N, B) for several.  raster_file: a single-band GeoTIFF path or a `PlanarRaster`
        (geograypher_amd.utils.raster); points_in_raster_CRS (required, keyword): the mesh vertices (V, 3) in the raster's CRS, or a CRS designator (`WGS84CRS.parse`: the vertices are then reprojected on the device) -- e.g. `raster.epsg`.
        The sample is that of the cell the point falls into; outside the raster it is nodata (0.0 without one); a sample equal
        to nodata becomes `nodata_fill_value`.  `return_mesh_points` also returns the (N, 3) query points: the vertices, or the
        face centres ((p0 + p1) + p2) / 3.0, the very operations the device forms them with.  The statistics of the call are left
        in `self.last_raster_stats` (queries, inside, nodata, ground, bad_faces)."""
        values, _, _, points = self._sample_raster(raster_file, use_vertex_locations, points_in_raster_CRS,
                                                   "get_values_from_raster_file", nodata_fill_value, want_values=True,
                                                   want_height=False)
        values = np.array(_host_array(values), dtype=np.float64)
        if values.shape[1] == 1:
            values = values[:, 0]
        if not return_mesh_points:
            return values
        if not use_vertex_locations:
            corners = points[self.faces]
            points = ((corners[:, 0] + corners[:, 1]) + corners[:, 2]) / 3.0   # rule T3
        return values, points

    def get_height_above_ground(self, DTM_file, use_vertex_locations: bool = False, threshold: float = None, *,
                                points_in_raster_CRS=None, return_tensor: bool = False):
        """Height of every face centre (or vertex) above the first band of a DTM (reference: meshes.py:1501-1538; rule T6): (N,)
        float64, NaN where the DTM has no data or does not reach; with `threshold`, the bool array `height < threshold` (NaN:
        False).  Arguments as for `get_values_from_raster_file`.  `return_tensor=True` leaves the result on the device."""
        _, height, _, _ = self._sample_raster(DTM_file, use_vertex_locations, points_in_raster_CRS, "get_height_above_ground",
                                              want_values=False, want_height=True)
        if threshold is not None:
            height = height < threshold
        if return_tensor:
            return height
        return np.array(_host_array(height))

    def label_ground_class(self, DTM_file, height_above_ground_threshold: float, labels=None,
                           only_label_existing_labels: bool = True, ground_class_name: str = "ground", ground_ID=None,
                           set_mesh_texture: bool = False, *, points_in_raster_CRS=None):
        """Give the faces (or vertices) lower than `height_above_ground_threshold` above the DTM the ground class (reference:
        meshes.py:1540-1629; rule T7).  labels: None (the face texture), or V vertex labels, or F face labels -- V is tried
        first --, (N,) or (N, 1), numpy or a float64 device tensor; they are rewritten IN PLACE and returned, a device tensor on
        the device.  The ground ID: NaN when the mesh has no IDs_to_labels and no ground_ID was passed; the existing ID when
        `ground_class_name` is a label already; else `ground_ID`; else the largest ID + 1 (the reference's
        `np.max(dict.keys()) + 1` raises TypeError there).  `add_label` records the name unless the ID is NaN."""
        if labels is None:
            use_vertex_locations = False
            labels = self.get_texture(request_vertex_texture=False)
            if labels is None:
                raise ValueError("label_ground_class: no labels given and the mesh has no texture")
        elif labels.shape[0] == self.points.shape[0]:
            use_vertex_locations = True
        elif labels.shape[0] == self.faces.shape[0]:
            use_vertex_locations = False
        else:
            raise ValueError("Labels were provided but didn't match the shape of vertices or faces")
        if labels.ndim > 2 or (labels.ndim == 2 and labels.shape[1] != 1):
            raise ValueError(f"labels must be (N,) or (N, 1), got {tuple(labels.shape)}")

        IDs_to_labels = self.get_IDs_to_labels()
        if IDs_to_labels is None and ground_ID is None:
            ground_ID = np.nan
        elif IDs_to_labels is not None and ground_class_name in IDs_to_labels.values():
            ground_ID = {v: k for k, v in IDs_to_labels.items()}.get(ground_class_name)
        elif IDs_to_labels is not None and ground_ID is None:
            ground_ID = max(IDs_to_labels.keys()) + 1

        on_device = hasattr(labels, "detach")
        in_place = on_device or labels.dtype == np.float64
        _, height, relabelled, _ = self._sample_raster(
            DTM_file, use_vertex_locations, points_in_raster_CRS, "label_ground_class", want_values=False,
            want_height=not in_place, labels=labels if in_place else None,
            threshold=height_above_ground_threshold if in_place else None, ground_id=ground_ID if in_place else None,
            only_existing=bool(only_label_existing_labels))
        self.add_label(label_name=ground_class_name, label_ID=ground_ID)
        if on_device:
            if relabelled.data_ptr() != labels.data_ptr():   # another device, dtype or layout: the backend worked on a copy
                labels.copy_(relabelled.reshape(labels.shape))
        elif in_place:
            np.copyto(labels, _host_array(relabelled).reshape(labels.shape))
        else:   # labels of another dtype: the assignment converts the ID as numpy does
            ground_mask = _host_array(height) < height_above_ground_threshold
            column = labels if labels.ndim == 1 else labels[:, 0]
            if only_label_existing_labels:
                ground_mask = np.logical_and(np.isfinite(column), ground_mask)
            column[ground_mask] = ground_ID
            self.last_raster_stats["ground"] = int(ground_mask.sum())
        if set_mesh_texture:
            self.set_texture(_host_array(labels) if on_device else labels)
        return labels

    # -- save_renders ----------------------------------------------------------------
    def save_IDs_to_labels(self, savepath: PATH_TYPE):
        """reference: meshes.py:1081-1108"""
        import json

        Path(savepath).parent.mkdir(parents=True, exist_ok=True)
        if self.is_discrete_texture():
            self.logger.info(f"Saving IDs_to_labels to {str(savepath)}")
            try:
                with open(savepath, "w") as outfile_h:
                    json.dump(self.get_IDs_to_labels(), outfile_h, ensure_ascii=False, indent=4, default=str)
            except Exception:
                self.logger.warning("Could not serialize IDs_to_labels due to JSON error")
        else:
            self.logger.warning("non-discrete texture, not saving classes")

    def vis(self, camera_set=None, screenshot_filename: typing.Optional[PATH_TYPE] = None, vis_scalars=None,
            IDs_to_labels: typing.Union[None, dict] = None, frustum_scale: float = 2, enable_ssao: bool = True, *, view=None,
            window_size=(1024, 768), supersample: int = 2, return_image: bool = False, mesh_kwargs=None, **ignored):
        """A picture of the mesh and the cameras (reference: meshes.py:2087-2246) without VTK: the scene is rastered by the
        projection path at window_size x supersample and shaded on the device (`gr_shade_view`) -- flat colours
        under a two-sided headlight, darkened where neighbouring samples are closer (`enable_ssao`), averaged to the window.

        camera_set: drawn as frusta of `frustum_scale` world units, the image's top side red (`get_vis_mesh`).  vis_scalars: per
        face or per vertex (default: the mesh's texture); one column with `IDs_to_labels` (default: the mesh's) whose largest ID
        is below 20 takes tab10 / tab20 by class, any other single column viridis over [nanmin, nanmax], several columns are RGB
        (bytes where the maximum exceeds 1), NaN is (169, 169, 169); the background is white.  No scalar bar is drawn: the
        legend {label: [r, g, b]} is written beside the picture as `<name>.legend.json`.
        view: None -- from the south-west (azimuth 225 degrees, clockwise from north) at 35.264 degrees elevation, 30 degrees
        vertical view angle, the whole scene in the window; a dict with any of azimuth_deg, elevation_deg, view_angle_deg; or a
        `PhotogrammetryCamera`, whose view the picture then is.  The frame is east-north-up at the centre of the mesh's bounds
        (`meshes.vis.picture_frame`).  -> the (H, W, 3) uint8 picture with `return_image`, else None; without a
        `screenshot_filename` and without `return_image` NotImplementedError: there is no window.  `plotter`, `interactive`,
        `interactive_jupyter`, `plotter_kwargs` and `force_xvfb` are accepted and ignored, any other keyword is a TypeError.
        The scene (mesh and frusta) is uploaded as one mesh; the mesh the device held before is uploaded again afterwards."""
        from geograypher_amd.meshes import vis as _vis

        unknown = sorted(set(ignored) - set(_vis.IGNORED))
        if unknown:
            raise TypeError(f"vis() got unexpected keyword arguments {unknown}")
        if ignored:
            self.logger.info(f"vis: {sorted(ignored)} are ignored -- there is no plotter and no window, the picture is rendered "
                             "off-screen on the device")
        return _vis.render(self, camera_set=camera_set, screenshot_filename=screenshot_filename, vis_scalars=vis_scalars,
                           IDs_to_labels=IDs_to_labels, frustum_scale=frustum_scale, enable_ssao=enable_ssao, view=view,
                           window_size=window_size, supersample=supersample, return_image=return_image, mesh_kwargs=mesh_kwargs)

    @staticmethod
    def _resize_map(src_hw, dst_hw):
        """(2, H, W) sampling map of skimage.transform.resize: destination pixel centres mapped into the source grid,
        mirrored at the borders (skimage's default mode "reflect")."""
        (h, w), (H, W) = src_hw, dst_hw
        r = (np.arange(H) + 0.5) * (h / H) - 0.5
        c = (np.arange(W) + 0.5) * (w / W) - 0.5
        r = np.where(r < 0, -r, np.where(r > h - 1, 2 * (h - 1) - r, r))
        c = np.where(c < 0, -c, np.where(c > w - 1, 2 * (w - 1) - c, c))
        rr, cc = np.meshgrid(r, c, indexing="ij")
        return np.stack([rr, cc], axis=0)

    def save_renders(
        self,
        camera_set: PhotogrammetryCameraSet,
        render_image_scale=1.0,
        output_folder: PATH_TYPE = Path(VIS_FOLDER, "renders"),
        make_composites: bool = False,
        save_native_resolution: bool = False,
        cast_to_uint8: bool = True,
        save_as_npy: bool = False,
        uint8_value_for_null_texture: np.uint8 = NULL_TEXTURE_INT_VALUE,
        **render_kwargs,
    ):
        """Render the face texture from every camera and save one file per image (reference: meshes.py:2248-2397).

        Same arguments, same on-disk layout (`<output_folder>/<image path relative to camera_set.image_folder>` as
        deflate-compressed .tif, or .npy with `save_as_npy`; `IDs_to_labels.json` for discrete textures).  The
        post-processing of meshes.py:2312-2349 runs on the device: with `cast_to_uint8` the texture gather, the
        null/out-of-range masking and the uint8 cast are ONE kernel (`gr_gather_texture_u8`), so a 4000x3000 view
        leaves the GPU as 12 MB instead of the reference's 96 MB float64 image; the optional native-resolution
        upsampling (nearest for discrete textures, bilinear otherwise) is the warp kernel with a resize map.
        Like the reference this renders with `distortion_set=camera_set` (a camera set without a distortion model
        needs `apply_distortion=False`).  With `make_composites` every file is the three-panel composite [label colours | photo
        | overlay] of `utils.visualization.create_composite` as a 3-channel image (meshes.py:2336-2344): the photo is
        `camera.get_image` at the render's scale (1.0 with `save_native_resolution`), the label image stays on the device and the
        composite kernel is the only extra device work of a view.

        Extra keywords (not forwarded to pix2face): `writer_threads` (default min(16, cores)) host threads that deflate
        and write while the GPU renders the next views -- results travel through a ring of pinned buffers, one
        asynchronous copy per view; `views_per_group` (default 8) views rasterized per device call.
        """
        from concurrent.futures import ThreadPoolExecutor

        from PIL import Image

        from geograypher_amd.utils.tiff import write_tiff_deflate

        torch = _torch()
        writer_threads = int(render_kwargs.pop("writer_threads", min(16, __import__("os").cpu_count() or 1)))
        views_per_group = int(render_kwargs.pop("views_per_group", 8))
        output_folder = Path(output_folder)
        output_folder.mkdir(parents=True, exist_ok=True)
        self.logger.info(f"Saving renders to {output_folder}")
        self.save_IDs_to_labels(Path(output_folder, "IDs_to_labels.json"))

        face_texture = np.asarray(
            self.get_texture(request_vertex_texture=False, try_verts_faces_conversion=True), dtype=np.float64
        )
        tex_dev = self.backend._dev(face_texture, torch.float64)
        mesh = self.get_mesh_in_cameras_coords(camera_set)
        discrete = self.is_discrete_texture()
        resize_maps = {}
        render_kwargs = dict(render_kwargs)
        render_kwargs.setdefault("distortion_set", camera_set)
        on_gpu = self.backend.device.type == "cuda"

        # Output paths first: a camera outside the image folder fails before any rendering, as in the reference
        output_files = []
        for camera in camera_set.cameras:
            try:
                camera_filename = Path(camera.get_image_filename()).relative_to(camera_set.image_folder)
            except (ValueError, TypeError):
                raise ValueError(
                    "Tried to find the relative path of the camera path"
                    f" ({camera.get_image_filename()}) inside of the camera set image"
                    f" folder ({camera_set.image_folder}), but failed. The tool being called"
                    " may have an 'original_image_folder' argument, which could be used to"
                    " delete the initial, mismatched portion of the camera path."
                )
            output_files.append(Path(output_folder, camera_filename))

        def write_one(host, event, output_filename):
            """Writer thread: wait for the view's copy to land in its pinned slot, finish the reference's post-processing
            (meshes.py:2325-2349) where it was not fused into the gather kernel, compress and write."""
            if event is not None:
                event.synchronize()
            rendered = host.numpy() if hasattr(host, "numpy") else host
            if rendered.dtype != np.uint8 and cast_to_uint8 and not make_composites:
                rendered = rendered.copy()
                mask = np.logical_or.reduce([rendered < 0, rendered > 255, np.logical_not(np.isfinite(rendered))])
                rendered[mask] = uint8_value_for_null_texture
                rendered = rendered.astype(np.uint8)
            rendered = np.squeeze(rendered)
            if rendered.ndim == 3:
                rendered = rendered[..., :3]
            output_filename.parent.mkdir(parents=True, exist_ok=True)
            if save_as_npy is True:
                np.save(str(output_filename.with_suffix(".npy")), rendered)
            else:
                if cast_to_uint8 is False and not make_composites:
                    with np.errstate(invalid="ignore"):
                        if np.nanmax(rendered) <= np.iinfo(np.uint16).max:
                            rendered = rendered.astype(np.uint16)
                        else:
                            rendered = rendered.astype(np.uint32)
                target = output_filename.with_suffix(".tif")
                if rendered.dtype in (np.uint8, np.uint16, np.uint32) and (rendered.ndim == 2 or rendered.shape[2] == 3):
                    write_tiff_deflate(target, rendered)  # zlib releases the interpreter lock: the writers run in parallel
                else:
                    Image.fromarray(rendered).save(str(target), compression="tiff_deflate")

        # Pipeline (row f2): the GPU rasterizes / gathers a group of views and copies each result into a slot of a pinned
        # ring while `writer_threads` host threads deflate and write the views before it.  A slot is reused only after
        # the writer that read it last is done, so at most ring_slots results are in flight.
        ring_slots = max(2 * writer_threads, 2)
        ring_budget = _PINNED_LIMIT_BYTES  # pinned bytes the ring may hold: float64 (h, w, C) frames are 8 C bytes per pixel
        ring = {}
        slot_writer = {}
        futures = []
        n = len(camera_set)
        with ThreadPoolExecutor(max_workers=max(writer_threads, 1)) as pool:
            for g0 in tqdm(range(0, n, views_per_group), total=(n + views_per_group - 1) // views_per_group,
                           desc="Computing and saving renders"):
                group = list(range(g0, min(g0 + views_per_group, n)))
                sub = camera_set.get_subset_cameras(group) if len(group) > 1 else camera_set[g0]
                ids_group = self.pix2face(cameras=sub, mesh=mesh, render_img_scale=render_image_scale, return_tensor=True,
                                          **render_kwargs)
                if isinstance(ids_group, np.ndarray):
                    ids_group = self.backend._dev(ids_group.astype(np.int32), torch.int32)
                if ids_group.ndim == 2:
                    ids_group = ids_group[None]
                for k, i in enumerate(group):
                    camera = camera_set.cameras[i]
                    ids = ids_group[k]
                    native = save_native_resolution and render_image_scale != 1
                    if native:
                        key = (tuple(ids.shape), tuple(camera.get_image_size()))
                        if key not in resize_maps:
                            resize_maps[key] = self.backend.upload_map(self._resize_map(*key))
                    if cast_to_uint8 and (not native or discrete):
                        if native:  # nearest-neighbour upsampling commutes with the per-pixel gather: resize the ids
                            ids = self.backend.warp_image(ids, resize_maps[key], order=0, fill_value=-1)
                        rendered = self.backend.gather_texture_u8(ids, tex_dev, int(uint8_value_for_null_texture))
                    else:
                        rendered = self.backend.gather_texture(ids, tex_dev)  # (h, w, C) float64, NaN without a face
                        if native:
                            rendered = self.backend.warp_image(rendered, resize_maps[key], order=0 if discrete else 1,
                                                               fill_value=float("nan"))
                    if make_composites:
                        from geograypher_amd.utils.visualization import create_composite

                        photo = camera.get_image(image_scale=(1.0 if save_native_resolution else render_image_scale),
                                                 backend=self.backend)
                        photo = photo[..., :3] if photo.ndim == 3 else photo
                        label = rendered if isinstance(rendered, torch.Tensor) else torch.as_tensor(np.asarray(rendered))
                        label = label[..., 0] if label.ndim == 3 and label.shape[-1] == 1 else label
                        rendered = create_composite(photo, label, IDs_to_labels=self.get_IDs_to_labels(), backend=self.backend)
                    frame_bytes = rendered.numel() * rendered.element_size() if hasattr(rendered, "numel") else rendered.nbytes
                    slots_now = max(2, min(ring_slots, ring_budget // max(frame_bytes, 1)))
                    slot = i % slots_now
                    if slot in slot_writer:
                        slot_writer[slot].result()  # the slot's previous view is on disk (a failed writer raises here)
                    if on_gpu and rendered.is_cuda:
                        skey = (slot, tuple(rendered.shape), rendered.dtype)
                        if ring.get(slot, (None,))[0] != skey[1:]:
                            ring.pop(slot, None)
                            try:
                                ring[slot] = (skey[1:], torch.empty(rendered.shape, dtype=rendered.dtype, pin_memory=True))
                            except RuntimeError:  # the host refuses more pinned memory: this view takes a blocking pageable copy
                                ring[slot] = None
                        if ring[slot] is not None:
                            host = ring[slot][1]
                            host.copy_(rendered, non_blocking=True)
                            event = torch.cuda.Event()
                            event.record(torch.cuda.current_stream(rendered.device))
                        else:
                            del ring[slot]
                            host, event = rendered.cpu(), None
                    else:
                        host, event = rendered, None
                    slot_writer[slot] = pool.submit(write_one, host, event, output_files[i])
                    futures.append(slot_writer[slot])
            for f in futures:
                f.result()


_FUSED_KWARGS = ("near", "principal_point", "focal_scaling")
_PIX2FACE_KWARGS = _FUSED_KWARGS + ("mesh", "save_to_cache", "cache_folder", "distortion_set", "apply_distortion")


@contextlib.contextmanager
def _driving(backend, own_stream=False):
    """This host thread drives `backend` inside the block: the backend's device is the thread's current one (a property of the
    host thread) and, with `own_stream`, the work goes to a stream of its own -- contexts that share a device would otherwise
    queue on its one default stream --, which is complete when the block ends: the thread hands a finished partial back."""
    torch = _torch()
    on_gpu = backend.device.type == "cuda"
    if on_gpu:
        torch.cuda.set_device(backend.device)
    with torch.cuda.stream(torch.cuda.Stream(backend.device)) if on_gpu and own_stream else contextlib.nullcontext():
        yield
        if on_gpu and own_stream:
            torch.cuda.current_stream(backend.device).synchronize()


def _on_each_device(backends, inds, run):
    """The `devices=[...]` fan-out: the views `inds` dealt round-robin, `run(backend, inds[k::n], first=k == 0)` for every
    backend on a host thread of its own (the C calls and torch's copies release the interpreter lock) -- the only thread that
    drives that backend during the call.  One backend runs on the caller's thread.  Returns the partials in device order;
    `_add_on_first` is where they meet."""
    n = len(backends)

    def drive(k):
        with _driving(backends[k], own_stream=n > 1):
            return run(backends[k], inds[k::n], first=k == 0)

    if n == 1:
        return [drive(0)]
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=len(backends)) as dev_pool:
        return list(dev_pool.map(drive, range(n)))


def _plain_files(cameras) -> bool:
    """File-backed photos of a plain camera set: neither the set's nor its cameras' image look-up is overridden."""
    return (type(cameras).get_image_by_index is PhotogrammetryCameraSet.get_image_by_index and len(cameras.cameras) > 0
            and all(type(cam).get_image is PhotogrammetryCamera.get_image for cam in cameras.cameras))


def _lookup_rule(cameras, n_device_threads: int = 1):
    """(thread_safe, lock) -- how a call fetches the images / labels of `cameras`.  thread_safe: file reads, or a camera set
    or segmentor that says so (`thread_safe_lookup`); only then are look-ups made ahead on loader threads.  Otherwise one
    caller at a time: with several device threads every look-up goes through the one lock (`_locked`); one thread needs none."""
    thread_safe = _plain_files(cameras) or bool(getattr(cameras, "thread_safe_lookup", False)
                                                or getattr(getattr(cameras, "segmentor", None), "thread_safe_lookup", False))
    if thread_safe or n_device_threads == 1:
        return thread_safe, None
    import threading

    return thread_safe, threading.Lock()


def _locked(lock, fn, *args):
    if lock is None:
        return fn(*args)
    with lock:
        return fn(*args)


def _as_camera_set(cameras):
    """A single camera as the one-element set the raster calls walk; a set as it is."""
    if isinstance(cameras, PhotogrammetryCamera):
        return PhotogrammetryCameraSet([cameras], local_to_epsg_4978_transform=cameras._local_to_epsg_4978_transform)
    return cameras


def _batched_views(n_views: int, batch_size: int):
    """(batch_stop, the views that batches of `batch_size` use, in order): trailing views that do not fill a batch are
    dropped, and a batch larger than the set still names its views, as in the reference (meshes.py:1976-1977)."""
    batch_stop = max(n_views - batch_size + 1, 1)
    return batch_stop, [start + i for start in range(0, batch_stop, batch_size) for i in range(batch_size)]


def _check_pix2face_kwargs(kwargs: dict) -> None:
    unknown = [k for k in kwargs if k not in _PIX2FACE_KWARGS]
    if unknown:
        raise TypeError(f"pix2face() got an unexpected keyword argument {unknown[0]!r}")


def _add_on_first(parts):
    """Per-device partials (tuples of tensors, in device order) added onto the first one, on its device (peer copies)."""
    total = parts[0]
    for part in parts[1:]:
        for t, p in zip(total, part):
            t += p.to(t.device)
    return total


def _raster_kwargs(kwargs: dict) -> dict:
    return {k: kwargs[k] for k in _FUSED_KWARGS if k in kwargs}


# device -> host through pinned memory.  A pageable destination moves at ~10 GB/s on the MI355X host link, a pinned one
# at the link rate; torch's caching host allocator hands the same pinned blocks back once earlier results are dropped.
_PINNED_LIMIT_BYTES = 8 << 30


def _ids_to_host_int64(ids, views_per_step: int = 4, threads: typing.Optional[int] = None) -> np.ndarray:
    """(n, h, w) int32 ids on the device -> int64 numpy, as the reference returns them (meshes.py:1804).  The PCIe link is the
    bottleneck of this call, so the ids cross it as int32 (half the bytes of a device-side widening) into a pinned ring,
    and host threads widen slot k into the result while slot k+1 is on the wire."""
    torch = _torch()
    if not ids.is_cuda or ids.dim() != 3 or ids.numel() < (1 << 21):
        return _to_host(ids.to(torch.int64))
    import os
    from concurrent.futures import ThreadPoolExecutor

    n, h, w = ids.shape
    ids = ids.contiguous()
    if threads is None:
        threads = max(1, min(16, os.cpu_count() or 1))
    step = max(1, min(int(views_per_step), n))
    try:
        ring = [torch.empty((step, h, w), dtype=torch.int32, pin_memory=True) for _ in range(2)]
    except RuntimeError:  # pinned memory exhausted
        return _to_host(ids.to(torch.int64))
    out = np.empty((n, h, w), dtype=np.int64)
    stream = torch.cuda.current_stream(ids.device)
    events = [torch.cuda.Event() for _ in range(2)]
    rows = max(1, (step * h + threads - 1) // threads)

    def widen(dst2d, src2d, r0, r1):
        np.copyto(dst2d[r0:r1], src2d[r0:r1], casting="safe")  # numpy releases the interpreter lock for this loop

    with ThreadPoolExecutor(max_workers=threads) as pool:
        jobs = [[], []]
        starts = list(range(0, n, step))
        for k, v0 in enumerate(starts):
            slot = k & 1
            for j in jobs[slot]:  # the slot's previous contents have been widened
                j.result()
            m = min(step, n - v0)
            ring[slot][:m].copy_(ids[v0 : v0 + m], non_blocking=True)
            events[slot].record(stream)
            if k >= 1:  # widen the previous slot while this one is on the wire
                ps = (k - 1) & 1
                pv0 = starts[k - 1]
                pm = min(step, n - pv0)
                events[ps].synchronize()
                src = ring[ps][:pm].numpy().reshape(pm * h, w)
                dst = out[pv0 : pv0 + pm].reshape(pm * h, w)
                jobs[ps] = [pool.submit(widen, dst, src, r0, min(r0 + rows, pm * h)) for r0 in range(0, pm * h, rows)]
        ls = (len(starts) - 1) & 1
        lv0 = starts[-1]
        lm = min(step, n - lv0)
        events[ls].synchronize()
        src = ring[ls][:lm].numpy().reshape(lm * h, w)
        dst = out[lv0 : lv0 + lm].reshape(lm * h, w)
        jobs[ls] = [pool.submit(widen, dst, src, r0, min(r0 + rows, lm * h)) for r0 in range(0, lm * h, rows)]
        for js in jobs:
            for j in js:
                j.result()
    return out


def _to_host(t) -> np.ndarray:
    """numpy copy of a tensor.  Device tensors are copied into a pinned staging tensor and returned as a numpy view of
    it (kept alive through the array's base); tensors that are already on the host are returned as they are."""
    torch = _torch()
    if not t.is_cuda:
        return t.numpy()
    nbytes = t.numel() * t.element_size()
    if nbytes == 0 or nbytes > _PINNED_LIMIT_BYTES:
        return t.cpu().numpy()
    try:
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    except RuntimeError:  # pinned memory exhausted: pageable copy
        return t.cpu().numpy()
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host.numpy()


def _check_tiff_suffix(export_file):
    """The raster exports write GeoTIFF only: NotImplementedError for another extension."""
    if export_file is not None and Path(export_file).suffix.lower() not in (".tif", ".tiff"):
        raise NotImplementedError(f"export_file {export_file}: rasters are written as .tif / .tiff only")


def _host_array(x) -> np.ndarray:
    """What a backend returned, on the host: a tensor through `_to_host`, anything else as a numpy array."""
    return _to_host(x) if hasattr(x, "detach") else np.asarray(x)


def _torch():
    import torch

    return torch
