"""Geometric helpers: the multiview-detection workflow (reference: geograypher/utils/geometric.py:97-106, 144-254) and the planar
polygons of `label_polygons` and of vector textures (`PlanarPolygons`, the 1e-6 m grid, `polygon_cell_table`).

This package has no pyvista: a boundary surface is a `(points (V, 3) float, faces (F, 3) int)` pair, and the ray / surface
intersection runs on the device (`HipRaster.clip_rays`, gr_rays_clip: brute force over a coarse covering mesh).  The covering
meshes themselves come from `covering_meshes` (`HipRaster.points_bounds`, `HipRaster.cover_grid`).
"""
from __future__ import annotations

import math
import typing
from pathlib import Path

import numpy as np


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def get_scale_from_transform(transform: typing.Union[np.ndarray, None]):
    """Isotropic scale of a 4x4 transform: the cube root of the determinant of its 3x3 block; 1 for None
    (geometric.py:97-106)."""
    if transform is None:
        return 1
    if transform.shape != (4, 4):
        raise ValueError(f"Transform shape was {transform.shape}")
    return np.cbrt(np.linalg.det(transform[:3, :3]))


def clip_line_segments(boundaries, origins: np.ndarray, directions: np.ndarray,
                       image_indices: typing.Union[typing.List[int], np.ndarray],
                       ray_limit: typing.Optional[float] = None, backend=None):
    """Clip rays between two boundary surfaces, keeping the rays that hit both (geometric.py:144-254).

    boundaries: two (points, faces) pairs, e.g. (ceiling, floor).  Returns (starts, ends, directions, image indices) of the
    kept rays: start = the nearest hit on boundaries[0], end = the nearest hit on boundaries[1] (along the infinite ray from
    the origin, t >= 0), direction re-normalised from the two hits.  `ray_limit` drops a ray whose |origin - end| exceeds it.
    The kept rays come in ascending ray index (the reference iterates a Python set of ray indices: its order is whatever the
    set yields).  `backend`: a `HipRaster` (default: the shared one) or an object with its `clip_rays` method."""
    if len(boundaries) != 2:
        raise ValueError(f"2 boundaries required, not {len(boundaries)}")
    if any(not (isinstance(b, (tuple, list)) and len(b) == 2) for b in boundaries):
        raise ValueError(f"(points, faces) pairs required, found {[type(b) for b in boundaries]}")
    origins, directions = np.asarray(origins), np.asarray(directions)
    if origins.shape != directions.shape:
        raise ValueError(f"origins and directions mismatched ({origins.shape} != {directions.shape})")
    if origins.ndim != 2 or origins.shape[1] != 3:
        raise ValueError(f"(N, 3) input arrays required, found {origins.shape}")
    if len(origins) != len(image_indices):
        raise ValueError(f"origins and image indices mismatched ({len(origins)} != {len(image_indices)})")
    if len(origins) == 0:
        return origins.copy(), origins.copy(), directions.copy(), np.array(image_indices)
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    origins = origins.astype(np.float64)
    hits = []
    for points, faces in boundaries:
        hit, _t, pts = (_host(x) for x in backend.clip_rays(origins, directions.astype(np.float64), np.asarray(points),
                                                            np.asarray(faces)))
        hits.append((hit.astype(bool), pts))
    keep = hits[0][0] & hits[1][0]
    pt0, pt1 = hits[0][1], hits[1][1]
    if ray_limit is not None:
        with np.errstate(invalid="ignore"):
            keep &= ~(np.linalg.norm(origins - pt1, axis=1) > ray_limit)
    pt0, pt1 = pt0[keep], pt1[keep]
    with np.errstate(invalid="ignore", divide="ignore"):
        new_directions = (pt1 - pt0) / np.linalg.norm(pt1 - pt0, axis=1, keepdims=True)
    return pt0, pt1, new_directions, np.asarray(image_indices)[keep]


COVER_FACE_WARN_N = 181   # 2 (N - 1)^2 triangles of a full N x N surface stay within gr_rays_clip's 65 536 up to here


def _delaunay_faces(xy: np.ndarray) -> np.ndarray:
    """(F, 3) int32 Delaunay triangles of planar points; (0, 3) for fewer than three points or points on one line."""
    empty = np.zeros((0, 3), dtype=np.int32)
    if len(xy) < 3:
        return empty
    d = xy - xy[0]
    if np.linalg.matrix_rank(d) < 2:   # all on one line (or one point): Qhull would refuse
        return empty
    from scipy.spatial import Delaunay, QhullError

    try:
        return np.ascontiguousarray(Delaunay(xy).simplices, dtype=np.int32)
    except QhullError:   # numerically flat input the rank test let through
        return empty


def covering_meshes(points, N: int, z_buffer=(0, 0), subsample: typing.Optional[int] = None, backend=None):
    """Two coarse surfaces that enclose a point set from above and below: the boundaries `clip_line_segments` and
    `triangulate_detections(boundaries=...)` take (reference: TexturedPhotogrammetryMesh.export_covering_meshes,
    meshes/meshes.py:2399-2482).

    With P = points[::subsample] (all points for None): an N x N grid of (x, y) points, np.linspace over P's x and y extent;
    grid point (xi, yi) owns the points within half a grid step of it on both axes, bounds included (a point on a shared
    bound belongs to both neighbours; an axis of zero extent puts every point in all its columns); the upper surface has the
    grid point at max(z of its points) + z_buffer[0], the lower one at min(z) + z_buffer[1]; grid points without points are
    dropped.  The extent (`gr_points_bounds`) and the per-cell extremes (`gr_cover_grid`) are computed on the device, in
    float64 and exactly: the vertices equal the reference's bit for bit.

    Returns ((upper_points (M, 3) float64, upper_faces (F, 3) int32), (lower_points, lower_faces)), vertices in the order
    xi * N + yi.  The faces are the Delaunay triangulation of the surviving (x, y) (scipy / Qhull); fewer than three
    survivors, or survivors on one line, give faces of shape (0, 3).  One divergence from the reference: the four corners of
    a grid square lie on a circle, where VTK's delaunay_2d and Qhull may choose different diagonals -- the vertices are the
    same, and the two surfaces differ only inside such a square.

    ValueError: len(z_buffer) != 2; N < 2 (the reference divides by zero); a NaN or infinite coordinate among the visited
    points (in the reference it poisons the extent).  N > 181 logs a warning: a full surface then has more than the 65 536
    triangles `gr_rays_clip` takes.  Empty `points` returns two empty pairs without touching the device.  `backend`: a
    `HipRaster` (default: the shared one) or an object with its `points_bounds` and `cover_grid` methods."""
    if len(z_buffer) != 2:
        raise ValueError(f"2 buffers (top, bottom) are required, not {len(z_buffer)}")
    N = int(N)
    if N < 2:
        raise ValueError(f"N must be at least 2, got {N}")
    if subsample is not None and int(subsample) < 1:
        raise ValueError(f"subsample must be a positive step, got {subsample}")
    stride = 1 if subsample is None else int(subsample)
    n_points = int(points.shape[0]) if hasattr(points, "shape") else len(points)
    if n_points == 0:
        empty = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32))
        return empty, (empty[0].copy(), empty[1].copy())
    if N > COVER_FACE_WARN_N:
        import logging

        logging.getLogger(__name__).warning(
            "covering_meshes: N=%d can give a surface of %d triangles, more than the 65536 gr_rays_clip takes", N,
            2 * (N - 1) ** 2)
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    if not hasattr(points, "detach"):
        points = np.asarray(points, dtype=np.float64)
    bounds, nonfinite = (_host(x) for x in backend.points_bounds(points, stride))
    if int(np.asarray(nonfinite).reshape(-1)[0]) != 0:
        raise ValueError(f"{int(np.asarray(nonfinite).reshape(-1)[0])} of the visited points have a NaN or infinite coordinate")
    x_min, x_max, y_min, y_max = (np.float64(v) for v in bounds[:4])
    # the reference's operands, formed as it forms them (meshes.py:2440-2446, 2453-2462)
    x_grid = np.linspace(x_min, x_max, N)
    y_grid = np.linspace(y_min, y_max, N)
    cell_w_half = (x_max - x_min) / (N - 1) / 2
    cell_h_half = (y_max - y_min) / (N - 1) / 2
    z_max, z_min, count = (_host(x) for x in backend.cover_grid(points, x_grid - cell_w_half, x_grid + cell_w_half,
                                                                y_grid - cell_h_half, y_grid + cell_h_half, stride))
    keep = np.asarray(count).reshape(-1) != 0
    xi, yi = np.divmod(np.arange(N * N), N)
    xy = np.column_stack([x_grid[xi], y_grid[yi]])[keep]
    upper = np.column_stack([xy, np.asarray(z_max, dtype=np.float64).reshape(-1)[keep] + z_buffer[0]])
    lower = np.column_stack([xy, np.asarray(z_min, dtype=np.float64).reshape(-1)[keep] + z_buffer[1]])
    faces = _delaunay_faces(xy)
    return (upper, faces), (lower, faces.copy())


# -- label_polygons: planar polygons and the 1e-6 m grid (DESIGN.md "Polygon labels") ---------------------------------------------
SNAP_GRID_METERS = 1e-6       # shapely.set_precision(..., 1e-6) of meshes.py:1222-1227
SNAP_LIMIT = 1 << 40          # largest |snapped coordinate| behind the common origin: the device's 128-bit products stay exact


def snap_to_grid(xy: np.ndarray) -> np.ndarray:
    """Coordinates in metres -> int64 units of SNAP_GRID_METERS: np.rint(x / 1e-6)."""
    q = np.rint(np.asarray(xy, dtype=np.float64) / SNAP_GRID_METERS)
    if q.size and not np.all(np.abs(q) < 2.0 ** 62):
        raise ValueError("coordinates are non-finite or too large to snap to the 1e-6 m grid")
    return q.astype(np.int64)


def _signed_area2_exact(q: np.ndarray) -> int:
    """Twice the signed area of an integer ring, in Python integers (no overflow)."""
    xs, ys = [int(v) for v in q[:, 0]], [int(v) for v in q[:, 1]]
    return sum(xs[i - 1] * ys[i] - xs[i] * ys[i - 1] for i in range(len(xs)))


class PlanarPolygons:
    """Polygons in a planar CRS (x, y in metres), the `polygons` of `TexturedPhotogrammetryMesh.label_polygons` in place of the
    reference's GeoDataFrame.

    rings: list of (n, 2) float arrays, one closed ring each (a repeated closing vertex is dropped); ring_polygon[r]: the output
    row ring r belongs to; ring_is_hole[r]: whether it is cut out of that row.  Several exterior rings on one row make a
    multi-part polygon.  n_polygons: the number of rows (default: the largest row + 1); a row without rings is a polygon no
    face can touch.  A ring with fewer than 3 distinct vertices or a non-finite coordinate is a ValueError.  Orientation does
    not matter: every ring is stored counter-clockwise by its signed area.  A polygon's region is its exterior rings minus its
    holes; rings of one polygon must not cross or overlap (a valid OGC polygon), and a SELF-INTERSECTING ring is undefined
    behaviour: nothing checks for it, the containment test and the clipped area then mean nothing in particular."""

    def __init__(self, rings, ring_polygon, ring_is_hole, n_polygons: typing.Optional[int] = None):
        if isinstance(rings, (str, bytes)) or hasattr(rings, "geometry"):
            raise NotImplementedError("polygon files and GeoDataFrames need geopandas, which is outside the projection path: "
                                      "pass the rings as arrays")
        ring_polygon = np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
        ring_is_hole = np.asarray(ring_is_hole, dtype=bool).reshape(-1)
        if not (len(rings) == ring_polygon.shape[0] == ring_is_hole.shape[0]):
            raise ValueError(f"{len(rings)} rings need as many polygon rows and hole flags, got {ring_polygon.shape[0]} and "
                             f"{ring_is_hole.shape[0]}")
        if ring_polygon.size and ring_polygon.min() < 0:
            raise ValueError("ring_polygon holds a negative row")
        rows = int(ring_polygon.max()) + 1 if ring_polygon.size else 0
        self.n_polygons = rows if n_polygons is None else int(n_polygons)
        self.epsg = None   # read only: the EPSG code `from_geojson` found in the file's `crs` member
        if self.n_polygons < rows:
            raise ValueError(f"ring_polygon names row {rows - 1} but n_polygons is {self.n_polygons}")
        clean = []
        for r, ring in enumerate(rings):
            ring = np.asarray(ring, dtype=np.float64)
            if ring.ndim != 2 or ring.shape[1] != 2:
                raise ValueError(f"ring {r} must be an (n, 2) array, got shape {ring.shape}")
            if not np.all(np.isfinite(ring)):
                raise ValueError(f"ring {r} has a non-finite coordinate")
            if len(ring) > 1 and np.array_equal(ring[0], ring[-1]):
                ring = ring[:-1]
            if len(np.unique(ring, axis=0)) < 3:
                raise ValueError(f"ring {r} has fewer than 3 distinct vertices")
            x, y = ring[:, 0] - ring[0, 0], ring[:, 1] - ring[0, 1]
            if np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y) < 0:
                ring = ring[::-1]
            clean.append(np.ascontiguousarray(ring))
        order = np.argsort(ring_polygon, kind="stable")   # the device walks a polygon's rings consecutively
        self.rings = [clean[i] for i in order]
        self.ring_polygon = ring_polygon[order]
        self.ring_is_hole = ring_is_hole[order]

    def __len__(self):
        return self.n_polygons

    @classmethod
    def from_sequence(cls, seq):
        """One row per item: an (n, 2) array (a polygon without holes) or a list [exterior, hole, ...]."""
        if isinstance(seq, (str, bytes)) or hasattr(seq, "geometry") or hasattr(seq, "__fspath__"):
            raise NotImplementedError("polygon files and GeoDataFrames need geopandas, which is outside the projection path: "
                                      "pass a sequence of ring arrays or a PlanarPolygons")
        rings, rows, holes = [], [], []
        for p, item in enumerate(seq):
            parts = [item] if (isinstance(item, np.ndarray) and item.ndim == 2) else list(item)
            if parts and np.ndim(parts[0]) == 1:   # a plain list of (x, y) pairs
                parts = [np.asarray(item)]
            for k, ring in enumerate(parts):
                rings.append(ring)
                rows.append(p)
                holes.append(k > 0)
        return cls(rings, rows, holes, n_polygons=len(seq))

    def snapped(self, origin=(0, 0)):
        """The ring table the device takes, on the 1e-6 m grid behind the integer `origin`: (ring_vertices (N, 2) int64,
        ring_offsets (R + 1,) int64, ring_polygon (R,) int32, ring_is_hole (R,) int32, polygon_boxes (P, 4) int64 xmin ymin
        xmax ymax).  Rings the snap collapses to zero area are dropped (GEOS makes them empty); one it turns over is turned back.
        A row without rings has the empty box (1, 1, 0, 0)."""
        origin = np.asarray(origin, dtype=np.int64).reshape(2)
        verts, offsets, rows, holes = [], [0], [], []
        boxes = np.tile(np.array([1, 1, 0, 0], dtype=np.int64), (self.n_polygons, 1))
        seen = np.zeros(self.n_polygons, dtype=bool)
        for ring, row, hole in zip(self.rings, self.ring_polygon, self.ring_is_hole):
            q = snap_to_grid(ring) - origin
            if np.abs(q).max() > SNAP_LIMIT:
                raise ValueError(f"a polygon vertex lies more than 2^40 grid steps ({SNAP_LIMIT * SNAP_GRID_METERS:.0f} m) from "
                                 "the common origin")
            a2 = _signed_area2_exact(q)
            if a2 == 0:
                continue
            if a2 < 0:
                q = q[::-1]
            lo, hi = q.min(axis=0), q.max(axis=0)
            if seen[row]:
                boxes[row, :2] = np.minimum(boxes[row, :2], lo)
                boxes[row, 2:] = np.maximum(boxes[row, 2:], hi)
            else:
                boxes[row, :2], boxes[row, 2:], seen[row] = lo, hi, True
            verts.append(q)
            offsets.append(offsets[-1] + len(q))
            rows.append(row)
            holes.append(hole)
        ring_vertices = np.concatenate(verts) if verts else np.zeros((0, 2), dtype=np.int64)
        return (np.ascontiguousarray(ring_vertices, dtype=np.int64), np.asarray(offsets, dtype=np.int64),
                np.asarray(rows, dtype=np.int32), np.asarray(holes, dtype=np.int32), boxes)

    @classmethod
    def from_geojson(cls, path):
        """(polygons, properties) of a GeoJSON FeatureCollection, parsed with `json`: one row per feature in file order, so row
        numbers equal feature numbers.  A Polygon feature is [exterior, hole, ...]; a MultiPolygon is a multi-part row (the
        first ring of every part an exterior); a feature of any other geometry type, or without geometry, keeps its row and
        has no rings.  A third coordinate is dropped.  properties: {name: (n_features,) array} over the union of the features'
        property names, None where a feature lacks one: int64 when every value is an int, float64 when every value is a
        number (bool is neither), otherwise object.  The coordinates are taken as they stand: planar metres, no CRS handling; the
        EPSG code of a `crs` member is recorded as `.epsg` of the polygons (None without one); only the polygon burn
        (`utils.geospatial.burn_polygons`, `write_chips`) consults it."""
        import json

        with open(path, "r") as file:
            data = json.load(file)
        features = data.get("features") if isinstance(data, dict) else None
        if not isinstance(features, list):
            raise ValueError(f"{path} is not a GeoJSON FeatureCollection")
        rings, rows, holes = [], [], []
        for row, feature in enumerate(features):
            geometry = feature.get("geometry") or {}
            kind = geometry.get("type")
            parts = {"Polygon": [geometry.get("coordinates")], "MultiPolygon": geometry.get("coordinates")}.get(kind) or []
            for part in parts:
                for k, ring in enumerate(part or []):
                    rings.append(np.asarray(ring, dtype=np.float64)[:, :2])
                    rows.append(row)
                    holes.append(k > 0)
        names = []
        for feature in features:
            names += [k for k in (feature.get("properties") or {}) if k not in names]
        properties = {}
        for name in names:
            values = [(feature.get("properties") or {}).get(name) for feature in features]
            is_int = [isinstance(v, int) and not isinstance(v, bool) for v in values]
            is_num = [i or isinstance(v, float) for i, v in zip(is_int, values)]
            dtype = np.int64 if all(is_int) else (np.float64 if all(is_num) else object)
            column = np.empty(len(values), dtype=dtype)
            column[:] = values
            properties[name] = column
        polygons = cls(rings, rows, holes, n_polygons=len(features))
        polygons.epsg = _geojson_epsg(data.get("crs"))
        return polygons, properties

    def bounds_snapped(self):
        """(lo (2,), hi (2,)) int64 of all rings on the grid, before any origin; None without rings."""
        if not self.rings:
            return None
        q = [snap_to_grid(r) for r in self.rings]
        return np.min([v.min(axis=0) for v in q], axis=0), np.max([v.max(axis=0) for v in q], axis=0)

    def simplified(self, tol_meters, backend=None, fixed=None) -> "PlanarPolygons":
        """These polygons with every ring simplified by the exact Douglas-Peucker of DESIGN.md section 8q (rules S1-S8) at
        `tol_meters`, on the device: the rings are snapped to the 1e-6 m grid behind the middle of their bounds, `simplify_rings`
        keeps a subset of their vertices, and the kept ones come back in metres.  The rows keep their numbers.  S8: a hole stays
        unless it collapses itself; a row whose exterior rings all collapse loses its holes too and is a row without rings.
        fixed: (N,) flags over the vertices of `self.snapped(origin)` that must stay (S2), or None.  The call's figures are left
        in `.last_simplify_stats` of the result.  Like `shapely.simplify(preserve_topology=False)`, a simplified ring may touch
        or cross itself or a neighbour (S10)."""
        bounds = self.bounds_snapped()
        origin = np.zeros(2, dtype=np.int64) if bounds is None else bounds[0] + (bounds[1] - bounds[0]) // 2
        rv, off, rows, holes, _ = self.snapped(origin)
        keep, kept_index, out_off, stats = simplify_rings(backend, rv, off, tol_meters, fixed)
        alive = np.diff(out_off) > 0
        row_alive = np.zeros(self.n_polygons, dtype=bool)
        row_alive[rows[alive & (holes == 0)]] = True
        rings, ring_rows, ring_holes = [], [], []
        for r in np.nonzero(alive & row_alive[rows])[0]:
            q = rv[kept_index[out_off[r]:out_off[r + 1]]] + origin
            rings.append(q.astype(np.float64) * SNAP_GRID_METERS)
            ring_rows.append(int(rows[r]))
            ring_holes.append(bool(holes[r]))
        out = PlanarPolygons(rings, ring_rows, ring_holes, n_polygons=self.n_polygons)
        out.epsg = self.epsg
        out.last_simplify_stats = stats
        return out


def _geojson_epsg(crs):
    """The EPSG code of a GeoJSON `crs` member ({"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::32610"}} or
    "EPSG:32610"); None for anything else."""
    import re

    name = ((crs.get("properties") or {}).get("name") if isinstance(crs, dict) else None)
    match = re.fullmatch(r"(?:urn:ogc:def:crs:)?EPSG:(?:[\d.]*:)?(\d+)", name.strip(), re.I) if isinstance(name, str) else None
    return int(match.group(1)) if match else None


# -- region of interest (DESIGN.md "Region of interest") ----------------------------------------------------------------------------
def snap_with_polygons(verts, polygons):
    """Rule P3 / V2: (snapped points (N, 2) int64, the polygons' snapped ring table), both on the 1e-6 m grid behind ONE integer
    origin, the middle of their joint bounds."""
    vq = snap_to_grid(verts[:, :2])
    lo, hi = (vq.min(axis=0), vq.max(axis=0)) if len(vq) else (np.zeros(2, np.int64), np.zeros(2, np.int64))
    ring_bounds = polygons.bounds_snapped()
    if ring_bounds is not None:
        lo, hi = np.minimum(lo, ring_bounds[0]), np.maximum(hi, ring_bounds[1])
    origin = lo + (hi - lo) // 2
    vq = vq - origin
    if len(vq) and np.abs(vq).max() > SNAP_LIMIT:
        raise ValueError("a mesh vertex lies more than 2^40 grid steps (1 099 512 m) from the common origin of mesh and "
                         "polygons")
    return vq, polygons.snapped(origin)


def region_polygons(ROI) -> "PlanarPolygons":
    """Rule Q1: a `PlanarPolygons`, a `.geojson` path (`PlanarPolygons.from_geojson`) or anything `PlanarPolygons.from_sequence`
    takes.  All rows together are the region."""
    import os

    if isinstance(ROI, PlanarPolygons):
        return ROI
    if isinstance(ROI, (str, os.PathLike)):
        if os.path.splitext(os.fspath(ROI))[1] != ".geojson":
            raise NotImplementedError(f"ROI file {ROI}: files other than .geojson need geopandas, which is outside the projection "
                                      "path")
        return PlanarPolygons.from_geojson(ROI)[0]
    return PlanarPolygons.from_sequence(ROI)


def region_buffer_steps(buffer_meters) -> int:
    """Rule Q2: the buffer in grid steps, D = rint(buffer_meters / 1e-6), 0 <= D < 2^40 or ValueError."""
    steps = np.rint(float(buffer_meters) / SNAP_GRID_METERS)
    if not (0 <= steps < SNAP_LIMIT):
        raise ValueError(f"buffer of {buffer_meters} m is outside [0, {SNAP_LIMIT * SNAP_GRID_METERS:.0f}) m")
    return int(steps)


def points_in_region(backend, ROI, points, buffer_meters=0):
    """Rules Q1-Q4 through `backend.points_in_region`: (mask (N,) bool -- a device tensor from a device backend --, stats).  points:
    (N, 2) or (N, 3) float64 in the ROI's planar CRS; a point is in the region iff it lies in the closed region of some row of the
    ROI or within `buffer_meters` of one of its rings, decided exactly on the 1e-6 m grid."""
    polygons = region_polygons(ROI)
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] not in (2, 3):
        raise ValueError(f"points must be (N, 2) or (N, 3), got {points.shape}")
    steps = region_buffer_steps(buffer_meters)
    vq, table = snap_with_polygons(points, polygons)
    return backend.points_in_region(vq, *table, steps)


# -- ring simplification: exact Douglas-Peucker -------------------------------------------------------------
SIMPLIFY_METHODS = ("douglas-peucker",)
SIMPLIFY_STAT_NAMES = ("kept_vertices", "collapsed_rings", "passes", "wide_comparisons", "short_rings")   # GR_SIMPLIFY_STAT_*


def check_simplify_method(method, what: str = "simplify_method"):
    """The one simplification this package has is asked for by name: anything but "douglas-peucker" is a ValueError."""
    if method not in SIMPLIFY_METHODS:
        raise ValueError(f"{what} must be one of {SIMPLIFY_METHODS} (or None: no simplification), got {method!r}")
    return method


def simplify_rings(backend, ring_vertices, ring_offsets, tol_meters, fixed=None):
    """Rules S1-S7 through `backend.ring_simplifier()`: ring_vertices (N, 2) int64 on the 1e-6 m grid and ring_offsets (R + 1,) as
    `PlanarPolygons.snapped` gives them, fixed (N,) flags or None -> (keep (N,) uint8, kept_index (M,) int32: the kept vertices,
    ring after ring in input order, out_offsets (R + 1,) int64, stats: a dict over SIMPLIFY_STAT_NAMES), all on the host.
    `backend`: a `HipRaster` (None: the shared one) or an object with its `ring_simplifier` method."""
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    keep, kept_index, out_offsets, stats = backend.ring_simplifier().simplify(ring_vertices, ring_offsets, tol_meters, fixed)
    keep, kept_index, out_offsets, stats = (_host(a) for a in (keep, kept_index, out_offsets, stats))
    return (keep.astype(np.uint8), kept_index.astype(np.int32), out_offsets.astype(np.int64),
            {name: int(stats[k]) for k, name in enumerate(SIMPLIFY_STAT_NAMES)})


def shared_border_fixed(ring_q, ring_offsets) -> np.ndarray:
    """Rule S9: (N,) uint8, 1 at every ring vertex whose POSITION must stay when the rings of a class map are simplified: over
    all its occurrences in all rings, the position has more than one distinct unordered pair of neighbour positions.  The interior
    vertices of a border that two classes share have the same two neighbours in both rings and stay free; where a third class
    joins, or a ring touches another in one point, the position is fixed.  A host sort over (position, neighbour pair) keys."""
    q = np.asarray(ring_q, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
    N = len(q)
    if N == 0:
        return np.zeros(0, dtype=np.uint8)
    n = np.diff(off)
    idx = np.arange(N, dtype=np.int64)
    start, length = np.repeat(off[:-1], n), np.repeat(n, n)
    a, b = q[start + (idx - start - 1) % length], q[start + (idx - start + 1) % length]
    swap = (a[:, 0] > b[:, 0]) | ((a[:, 0] == b[:, 0]) & (a[:, 1] > b[:, 1]))
    keys = np.column_stack([q, np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)])
    order = np.lexsort(keys.T[::-1])
    s = keys[order]
    new_position, new_key = np.ones(N, dtype=bool), np.ones(N, dtype=bool)
    new_position[1:] = np.any(s[1:, :2] != s[:-1, :2], axis=1)
    new_key[1:] = np.any(s[1:] != s[:-1], axis=1)
    group = np.cumsum(new_position) - 1
    distinct = np.bincount(group, weights=new_key)
    fixed = np.zeros(N, dtype=np.uint8)
    fixed[order] = distinct[group] > 1
    return fixed


# -- the face sieve: components of equally labelled faces, small ones merged into their greatest neighbour --------
SIEVE_STAT_NAMES = ("rounds", "components_before", "components_after", "faces_changed", "small_left", "degenerate", "fan_edges",
                    "round_cap", "bad_faces")   # GR_SIEVE_STAT_*
SIEVE_AREA_UNITS_PER_M2 = 1e6   # face_area_weights counts mm^2


def face_area_weights(points, faces) -> np.ndarray:
    """(F,) int64: the area of every face in mm^2, w = floor(0.5 * |(p1 - p0) x (p2 - p0)| * 1e6 + 0.5) -- ONE float64 expression,
    computed once on the host; the device sees the integers only (I5)."""
    p = np.asarray(_host(points), dtype=np.float64).reshape(-1, 3)
    f = np.asarray(_host(faces), dtype=np.int64).reshape(-1, 3)
    p0, p1, p2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    return np.floor(0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1) * SIEVE_AREA_UNITS_PER_M2 + 0.5).astype(np.int64)


def weld_canon(points) -> np.ndarray:
    """(V,) int32 for I1's `vertex_canon`: vertices whose float64 coordinates are bit-equal map to the smallest index of their
    group (-0.0 and 0.0 differ in a bit and are not welded; neither are NaNs of different payloads).  A host sort."""
    p = np.ascontiguousarray(np.asarray(_host(points), dtype=np.float64).reshape(-1, 3))
    V = len(p)
    if V == 0:
        return np.zeros(0, dtype=np.int32)
    bits = p.view(np.uint64).reshape(V, 3)
    order = np.lexsort((np.arange(V), bits[:, 2], bits[:, 1], bits[:, 0]))
    s = bits[order]
    head = np.ones(V, dtype=bool)
    head[1:] = np.any(s[1:] != s[:-1], axis=1)
    first = order[head][np.cumsum(head) - 1]      # the group's first vertex in the sorted order: its smallest index
    canon = np.empty(V, dtype=np.int32)
    canon[order] = first
    return canon


def sieve_face_classes(faces, classes, weights=None, min_measure=0, fill_unlabelled: bool = False, vertex_canon=None, max_rounds: int = 64,
                       backend=None, n_vertices=None, return_tensor: bool = False):
    """Rules I1-I10 through `backend.face_sieve`: faces (F, 3), classes (F,) integers (< 0: unlabelled), weights (F,) int64 >= 0 or
    None for 1 per face, arrays or device tensors -> (class_out (F,) int32, comp (F,) int32: the smallest face of the face's
    component in the final labelling, -1 for a face that takes no part, stats: a dict over SIEVE_STAT_NAMES).  A component whose
    measure is below `min_measure` joins its greatest labelled neighbour; min_measure = 0 only labels the components.  A face that
    names a vertex outside the mesh is a ValueError.  `backend`: a `HipRaster` (None: the shared one) or an object with its
    `face_sieve` method.  With `return_tensor` the two arrays stay on the device."""
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    classes_flat = classes.reshape(-1)
    n_faces = int(faces.shape[0])
    if int(classes_flat.shape[0]) != n_faces:
        raise ValueError(f"{int(classes_flat.shape[0])} face classes for {n_faces} faces")
    class_out, comp, stats = backend.face_sieve(faces, classes_flat, weights, min_measure, fill_unlabelled, vertex_canon, max_rounds,
                                                **({} if n_vertices is None else {"n_vertices": n_vertices}))
    stats_h = _host(stats)
    named = {name: int(stats_h[k]) for k, name in enumerate(SIEVE_STAT_NAMES)}
    if named["bad_faces"]:
        raise ValueError(f"gr_face_sieve: {named['bad_faces']} faces name a vertex (or a vertex_canon entry) outside the mesh")
    if return_tensor:
        return class_out, comp, named
    return _host(class_out).astype(np.int32), _host(comp).astype(np.int32), named


def face_components(faces, classes, backend=None, vertex_canon=None, n_vertices=None, return_tensor: bool = False):
    """Rule I4 alone: (comp (F,) int32: the smallest face of the face's component of edge-neighbours of equal class -- unlabelled,
    any class < 0, is a class here --, -1 for a degenerate face; stats: a dict over SIEVE_STAT_NAMES, `components_before` the
    number of components).  `sieve_face_classes` with min_measure = 0."""
    _, comp, stats = sieve_face_classes(faces, classes, None, 0, False, vertex_canon, 64, backend, n_vertices, return_tensor)
    return comp, stats


# -- nearest points: for every query row the nearest ref row, exact -----------------------------------------------
NEAREST_STAT_NAMES = ("ref_nonfinite", "query_nonfinite", "no_answer", "levels", "carried", "cells_probed", "candidates", "cell_bits",
                      "ring_cap")   # GR_NN_STAT_*


def points_3d(points, name: str = "points"):
    """(n, 3) float64 of an (n, 3) array, or of an (n, 2) one with z = 0; numpy stays numpy, a tensor stays a tensor on its
    device.  Any other shape is a ValueError naming `name`."""
    shape = tuple(points.shape) if hasattr(points, "shape") else np.asarray(points).shape
    if len(shape) != 2 or shape[1] not in (2, 3):
        raise ValueError(f"{name} must be (n, 3), or (n, 2) for z = 0, got {shape}")
    if hasattr(points, "detach"):
        import torch

        p = points.to(torch.float64)
        return p if shape[1] == 3 else torch.cat([p, torch.zeros((shape[0], 1), dtype=torch.float64, device=p.device)], dim=1)
    p = np.asarray(points, dtype=np.float64)
    return np.ascontiguousarray(p if shape[1] == 3 else np.concatenate([p, np.zeros((shape[0], 1))], axis=1))


def named_nearest_stats(stats) -> dict:
    """The statistics block of gr_nearest_points as a dict over NEAREST_STAT_NAMES, and `cell`: the cell side as a float."""
    stats_h = np.asarray(_host(stats)).astype(np.int64)
    named = {name: int(stats_h[k]) for k, name in enumerate(NEAREST_STAT_NAMES)}
    named["cell"] = float(np.array([named["cell_bits"]], dtype=np.int64).view(np.float64)[0])
    return named


def nearest_points(backend, ref, query, *, max_distance=None, cell: float = 0.0, max_rings: int = 2, return_dist2: bool = False,
                   return_tensor: bool = False):
    """Rules K1-K9 through `backend.nearest_points`: ref (R, 3), query (Q, 3) -- or (n, 2) for z = 0 --, arrays or device tensors
    -> (index (Q,) int32: for every query row the row of the nearest ref, the lowest among equally near ones, -1 where there
    is none (a non-finite query, no finite ref, none within `max_distance`); [dist2 (Q,) float64 with `return_dist2`: the squared
    distance ((dx dx + dy dy) + dz dz), NaN beside -1;] stats: a dict over NEAREST_STAT_NAMES and `cell`).  The answer is the
    brute-force argmin, bit for bit; `cell` and `max_rings` steer the search only.  `backend`: a `HipRaster` (None: the shared
    one) or an object with its `nearest_points` method.  With `return_tensor` the arrays stay where the backend left them."""
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    ref, query = points_3d(ref, "ref"), points_3d(query, "query")
    out = backend.nearest_points(ref, query, max_distance=max_distance, cell=cell, max_rings=max_rings, return_dist2=return_dist2)
    arrays, named = out[:-1], named_nearest_stats(out[-1])
    if not return_tensor:
        arrays = tuple(np.asarray(_host(a)) for a in arrays)
    return (*arrays, named)


def gather_rows(values, index, fill):
    """out[i] = values[index[i]] where index[i] >= 0, `fill` elsewhere; the dtype and the trailing axes of `values`.  With a
    device `index` the gather runs on that device and the result comes back as numpy."""
    values = np.asarray(_host(values))
    if hasattr(index, "detach"):
        import torch

        vals_t = torch.as_tensor(np.ascontiguousarray(values)).to(index.device)
        idx = index.to(torch.int64)
        if vals_t.shape[0] == 0:
            out = torch.full((idx.shape[0],) + tuple(vals_t.shape[1:]), fill, dtype=vals_t.dtype, device=index.device)
        else:
            out = vals_t[idx.clamp(min=0)]
            out[idx < 0] = fill
        return out.cpu().numpy()
    idx = np.asarray(index, dtype=np.int64)
    if values.shape[0] == 0:
        return np.full((idx.shape[0],) + values.shape[1:], fill, dtype=values.dtype)
    out = values[np.maximum(idx, 0)]
    out[idx < 0] = fill
    return out


# -- mesh decimation by vertex clustering ---------------------------------------------------------------------
CLUSTER_COORD_LIMIT = 1 << 41   # D1: snapped coordinates behind their minimum stay below this
CLUSTER_CELLS_PER_AXIS = 1 << 21   # D2: a cell component fits 21 bits of the key
CLUSTER_MAX_CELL_SIDE = 1 << 30    # D2: ... and the doubled offset to the cell's centre 31


def snap_points_3d(points) -> np.ndarray:
    """Rule D1: (V, 3) float64 metres -> (V, 3) int64 on the 1e-6 m grid (`snap_to_grid`, all three columns) behind the per-axis
    minimum, so every value is >= 0.  A coordinate of 2^41 steps (2 199 023 m) or more behind the minimum is a ValueError."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (V, 3), got {points.shape}")
    q = snap_to_grid(points)
    if len(q):
        q = q - q.min(axis=0)
        if int(q.max()) >= CLUSTER_COORD_LIMIT:
            raise ValueError("the mesh spans 2^41 grid steps (2 199 023 m) or more along an axis: too large to decimate on the 1e-6 m grid")
    return np.ascontiguousarray(q)


def cluster_cell_range(verts_q) -> typing.Tuple[int, int]:
    """Rule D2: (s_min, s_max), the cell sides in grid steps the snapped vertices of `snap_points_3d` allow: s_min keeps every cell
    component below 2^21, s_max is a cell that holds the whole mesh, at most 2^30."""
    verts_q = np.asarray(verts_q)
    extent = int(verts_q.max()) if verts_q.size else 0
    s_min = max(1, -(-(extent + 1) // CLUSTER_CELLS_PER_AXIS))
    return s_min, max(s_min, min(extent + 1, CLUSTER_MAX_CELL_SIDE))


def cluster_cell_size(backend, verts_q, target: float, held=None) -> typing.Tuple[int, int, int]:
    """Rule D4 through `backend.cluster_count`: the cell side for a target fraction of the vertices -> (s, cells(s), probes).
    T = max(1, floor(target V)); s_min when it already gives at most T cells, else the bisection of [s_min, s_max] as D4
    states it (cells(s) is not strictly monotone: the rule is the procedure).  One probe per step: the first at s_min, at most 30
    of the bisection, and one at s_max when no step reached it.  The vertices go to the device once (`backend.to_device`; `held`:
    the caller's copy of them there)."""
    verts_q = np.asarray(verts_q)
    V = int(verts_q.shape[0])
    want = max(1, int(math.floor(float(target) * V)))
    lo, hi = cluster_cell_range(verts_q)
    if held is not None:
        verts_q = held
    elif hasattr(backend, "to_device"):
        verts_q = backend.to_device(verts_q, "int64")
    probes = 1
    cells = int(backend.cluster_count(verts_q, lo))
    if cells <= want:
        return lo, cells, probes
    cells_hi = None   # cells(hi) once hi has been probed
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes += 1
        cells_mid = int(backend.cluster_count(verts_q, mid))
        if cells_mid <= want:
            hi, cells_hi = mid, cells_mid
        else:
            lo = mid
    if cells_hi is None:   # s_max was never probed (one cell, unless the mesh is wider than 2^30 steps)
        probes += 1
        cells_hi = int(backend.cluster_count(verts_q, hi))
    return hi, cells_hi, probes


# -- class outlines ---------------------------------------------------------------------------------------------
OUTLINE_MAX_CLASSES = 65535   # GR_OUTL_MAX_CLASSES: classes of one gr_class_outlines call
MEMBER_MAX_CLASSES = 2 ** 31 - 2   # GR_MEMBER_MAX_CLASSES: classes of one gr_member_outlines call


def is_sparse(labels) -> bool:
    """A scipy.sparse matrix or array (scipy is only imported where one can be about)."""
    if not type(labels).__module__.startswith("scipy.sparse"):
        return False
    import scipy.sparse

    return scipy.sparse.issparse(labels)


def csr_members(labels):
    """Rule Y1: a scipy.sparse (F, C) matrix or array of any format -> (face_ptr (F + 1,) int64, face_members (nnz,) int32): the
    face-major CSR of its entries > 0, duplicates summed first, the members of a row strictly ascending.  C must fit int32."""
    import scipy.sparse

    csr = scipy.sparse.csr_matrix(labels)   # a new header; COO input is summed here
    if csr is labels or csr.data is getattr(labels, "data", None):
        csr = csr.copy()
    csr.sum_duplicates()
    csr.sort_indices()
    keep = csr.data > 0   # NaN is not
    kept_before = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(keep, dtype=np.int64)])
    if csr.shape[1] > MEMBER_MAX_CLASSES:
        raise ValueError(f"{csr.shape[1]} columns: a member table takes at most {MEMBER_MAX_CLASSES}")
    return kept_before[csr.indptr], np.ascontiguousarray(csr.indices[keep], dtype=np.int32)


def snap_points(points):
    """Rule X1: (V, 2 | 3) float64 metres -> (V, 2) int64 on the 1e-6 m grid behind the integer middle of their bounds; z is not
    used.  A vertex more than 2^40 steps from that origin is a ValueError."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] not in (2, 3):
        raise ValueError(f"points must be (V, 2) or (V, 3), got {points.shape}")
    vq = snap_to_grid(points[:, :2])
    if len(vq):
        lo, hi = vq.min(axis=0), vq.max(axis=0)
        vq = vq - (lo + (hi - lo) // 2)
        if np.abs(vq).max() > SNAP_LIMIT:
            raise ValueError("a mesh vertex lies more than 2^40 grid steps (1 099 512 m) from the middle of the mesh")
    return np.ascontiguousarray(vq)


class FaceLabelOutlines:
    """What `TexturedPhotogrammetryMesh.face_label_outlines` returns: R rings over E ring vertices, in the order of rule X6.
    ring_offsets (R + 1,) int64; ring_class (R,) float64, the label of the ring's faces (NaN: the class of the unlabelled faces, with
    drop_nan=False; the column for many-hot labels); ring_vertex_ids (E,) int32 ORIGINAL vertex indices, the smallest of every group
    of vertices that share a snapped (x, y); ring_xy (E, 2) float64, the coordinates of those vertices as they were passed in;
    ring_is_hole (R,) bool, the exact signed area of the snapped ring is negative; stats: a dict of counters."""

    def __init__(self, ring_offsets, ring_class, ring_vertex_ids, ring_xy, ring_is_hole, stats, snapped=None):
        self.ring_offsets, self.ring_class, self.ring_vertex_ids = ring_offsets, ring_class, ring_vertex_ids
        self.ring_xy, self.ring_is_hole, self.stats = ring_xy, ring_is_hole, stats
        self.snapped = snapped   # (snapped ring vertices (E, 2) int64, twice the exact signed area per ring: Python integers), or None

    def __len__(self):
        return int(self.ring_offsets.shape[0]) - 1

    def simplified(self, tol_meters, backend, shared_borders: bool = True) -> "FaceLabelOutlines":
        """These outlines with every ring simplified by the exact Douglas-Peucker of DESIGN.md section 8q at `tol_meters`, on the
        device (host arrays out).  The R rings keep their numbers, classes and hole flags: a ring that collapses (S6) has no
        vertices left.  `ring_vertex_ids` and `ring_xy` are carried over through the kept indices.  shared_borders (S9): the
        positions where the borders of the class map meet are fixed (`shared_border_fixed`), so two classes keep the same
        vertices along the border they share.  `stats` gains the words of the call as simplify_<name> (SIMPLIFY_STAT_NAMES)."""
        if self.snapped is None:
            raise ValueError("these outlines carry no snapped rings to simplify")
        q = np.asarray(self.snapped[0], dtype=np.int64).reshape(-1, 2)
        off = _host(self.ring_offsets).astype(np.int64)
        fixed = shared_border_fixed(q, off) if shared_borders else None
        _, kept, out_off, words = simplify_rings(backend, q, off, tol_meters, fixed)
        kept = kept.astype(np.int64)
        alive = np.nonzero(np.diff(out_off) > 0)[0]
        areas2 = [0] * len(self)
        for r, a in zip(alive.tolist(), ring_areas2_exact(q[kept], np.concatenate([out_off[alive], out_off[-1:]]))):
            areas2[r] = a
        stats = dict(self.stats, **{f"simplify_{name}": value for name, value in words.items()})
        return FaceLabelOutlines(out_off, _host(self.ring_class), _host(self.ring_vertex_ids)[kept], _host(self.ring_xy)[kept],
                                 _host(self.ring_is_hole), stats, (q[kept], areas2))


def ring_areas2_exact(ring_q, ring_offsets):
    """Twice the exact signed area of every ring of an integer ring table: a list of Python integers.  Rings whose shoelace sum
    fits int64 (relative to their first vertex) are summed by numpy, the others in Python integers."""
    ring_q = np.asarray(ring_q, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64)
    R = len(off) - 1
    if R <= 0:
        return []
    n = np.diff(off)
    first = np.repeat(ring_q[off[:-1]], n, axis=0)
    d = ring_q - first                                  # |d| <= 2^41
    nxt = np.arange(len(ring_q)) + 1
    nxt[off[1:] - 1] = off[:-1]                         # the closing edge
    reach = np.maximum.reduceat(np.abs(d).max(axis=1), off[:-1]).astype(np.float64)
    small = reach * reach * 2.0 * n < 2.0 ** 62
    with np.errstate(over="ignore"):
        terms = d[:, 0] * d[nxt, 1] - d[nxt, 0] * d[:, 1]
    sums = np.add.reduceat(terms, off[:-1])
    out = [int(v) for v in sums]
    for r in np.nonzero(~small)[0]:
        out[r] = _signed_area2_exact(d[off[r]:off[r + 1]])
    return out


class _RingLocator:
    """The closed region of one integer ring -- on the ring, or a non-zero winding number -- asked point by point.  The edges are
    bucketed into horizontal slabs (about sqrt(n) of them), so a query reads the edges of one slab only; the arithmetic is int64 numpy
    where every product fits (|coordinate| < 2^30) and Python integers otherwise."""

    def __init__(self, ring):
        ring = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
        a, b = np.roll(ring, 1, axis=0), ring
        self.ax, self.ay, self.bx, self.by = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
        self.fits = int(np.abs(ring).max()) < 2 ** 30
        n = len(ring)
        self.y0, self.y1 = int(ring[:, 1].min()), int(ring[:, 1].max())
        n_slabs = min(4096, max(1, int(np.sqrt(n))))
        self.h = (self.y1 - self.y0) // n_slabs + 1
        lo = (np.minimum(self.ay, self.by) - self.y0) // self.h
        hi = (np.maximum(self.ay, self.by) - self.y0) // self.h
        count = hi - lo + 1
        edge = np.repeat(np.arange(n), count)
        slab = np.repeat(lo, count) + (np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count))
        order = np.argsort(slab, kind="stable")
        self.edges = edge[order]
        self.start = np.searchsorted(slab[order], np.arange((self.y1 - self.y0) // self.h + 2))

    def contains(self, px, py):
        if py < self.y0 or py > self.y1:
            return False
        k = (py - self.y0) // self.h
        e = self.edges[self.start[k]:self.start[k + 1]]
        ax, ay, bx, by = self.ax[e], self.ay[e], self.bx[e], self.by[e]
        if not self.fits:
            ax, ay, bx, by = (v.astype(object) for v in (ax, ay, bx, by))
            px, py = int(px), int(py)
        o = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        zero, up, down = (o == 0).astype(bool), (o > 0).astype(bool), (o < 0).astype(bool)
        ax, ay, bx, by = self.ax[e], self.ay[e], self.bx[e], self.by[e]
        if np.any(zero & (np.minimum(ax, bx) <= px) & (px <= np.maximum(ax, bx)) & (np.minimum(ay, by) <= py) & (py <= np.maximum(ay, by))):
            return True
        cross = (ay <= py) != (by <= py)
        return int(np.sum(cross & (by > ay) & up)) - int(np.sum(cross & (by < ay) & down)) != 0


NEST_CELL_SPREAD = 64   # an exterior whose box meets more cells of the candidate grid than this is kept on one list for every hole


def nest_outline_rings(ring_q, ring_offsets, ring_class_index, areas2=None):
    """Rule X8 on the snapped rings: (areas2: twice the exact signed area of every ring, a list of Python integers -- `areas2` when
    the caller has them already; home (R,) int64).  A ring of positive area is an exterior, one of negative area a hole.  home[r] of
    a hole is the exterior of its class with the smallest area (equal areas: the earlier ring) whose closed region -- non-zero
    winding, or on the ring -- holds ALL of the hole's vertices; -1 for a hole without one (an orphan) and for every exterior.
    The search is not quadratic: per class the exteriors' boxes go into a uniform grid of about as many cells as there are
    exteriors (those that spread over more than NEST_CELL_SPREAD cells onto one common list), a hole looks up the cell of its first
    vertex, one vectorised comparison keeps the candidates whose box holds the hole's box, and only those reach the exact test, in
    order of area, through a `_RingLocator` per exterior (built when first asked)."""
    ring_q = np.asarray(ring_q, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64)
    cls = np.asarray(ring_class_index, dtype=np.int64).reshape(-1)
    R = len(cls)
    if areas2 is None:
        areas2 = ring_areas2_exact(ring_q, off)
    home = np.full(R, -1, dtype=np.int64)
    if R == 0:
        return areas2, home
    lo = np.minimum.reduceat(ring_q, off[:-1], axis=0)
    hi = np.maximum.reduceat(ring_q, off[:-1], axis=0)
    sign = np.array([(a > 0) - (a < 0) for a in areas2], dtype=np.int64)
    locators = {}
    for c in np.unique(cls[sign < 0]):
        ext = np.nonzero((cls == c) & (sign > 0))[0]
        holes = np.nonzero((cls == c) & (sign < 0))[0]
        if not len(ext):
            continue
        ext = np.array(sorted(ext.tolist(), key=lambda r: (areas2[r], r)), dtype=np.int64)   # rank = position: area, then ring
        e_lo, e_hi = lo[ext], hi[ext]
        g_lo, g_hi = e_lo.min(axis=0), e_hi.max(axis=0)
        side = min(1024, max(1, int(np.sqrt(len(ext)))))
        cell = (g_hi - g_lo) // side + 1
        c_lo, c_hi = (e_lo - g_lo) // cell, (e_hi - g_lo) // cell
        spread = (c_hi - c_lo + 1).prod(axis=1)
        wide = np.nonzero(spread > NEST_CELL_SPREAD)[0]                                      # ranks, ascending
        small = np.nonzero(spread <= NEST_CELL_SPREAD)[0]
        nx = (c_hi[small, 0] - c_lo[small, 0] + 1)
        n = spread[small]
        k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        cx = np.repeat(c_lo[small, 0], n) + k % np.repeat(nx, n)
        cy = np.repeat(c_lo[small, 1], n) + k // np.repeat(nx, n)
        flat = cy * side + cx
        order = np.argsort(flat, kind="stable")                                              # ranks stay ascending within a cell
        listed = np.repeat(small, n)[order]
        start = np.searchsorted(flat[order], np.arange(side * side + 1))
        for r in holes.tolist():
            first = ring_q[off[r]]
            if np.any(first < g_lo) or np.any(first > g_hi):
                continue
            at = (first - g_lo) // cell
            f = int(at[1] * side + at[0])
            cand = np.concatenate([listed[start[f]:start[f + 1]], wide])
            cand = cand[np.all(e_lo[cand] <= lo[r], axis=1) & np.all(e_hi[cand] >= hi[r], axis=1)]
            points = ring_q[off[r]:off[r + 1]].tolist()
            for rank in np.sort(cand).tolist():
                e = int(ext[rank])
                if e not in locators:
                    locators[e] = _RingLocator(ring_q[off[e]:off[e + 1]])
                if all(locators[e].contains(px, py) for px, py in points):
                    home[r] = e
                    break
    return areas2, home


def write_geojson_multipolygons(path, polygons: "PlanarPolygons", properties: dict):
    """A FeatureCollection with one MultiPolygon feature per row of `polygons`, written with `json`: every exterior ring of the row
    starts a part, the holes follow the exterior they were stored behind; rings are closed; the coordinates are those stored.  A
    row without rings has a MultiPolygon without parts.  `PlanarPolygons.from_geojson` reads the file back."""
    import json

    rows = [[] for _ in range(polygons.n_polygons)]
    for ring, row, hole in zip(polygons.rings, polygons.ring_polygon, polygons.ring_is_hole):
        closed = [[float(x), float(y)] for x, y in ring] + [[float(ring[0][0]), float(ring[0][1])]]
        if hole and rows[row]:
            rows[row][-1].append(closed)
        else:
            rows[row].append([closed])

    def plain(v):
        if isinstance(v, (np.floating, float)):
            return None if np.isnan(v) else float(v)
        return int(v) if isinstance(v, np.integer) else v

    features = [{"type": "Feature", "properties": {k: plain(v[row]) for k, v in properties.items()},
                 "geometry": {"type": "MultiPolygon", "coordinates": parts}} for row, parts in enumerate(rows)]
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as file:
        json.dump({"type": "FeatureCollection", "features": features}, file)


# -- vector textures: a uniform cell index over the polygon boxes (DESIGN.md "Vector textures") ------------------------------------
CELL_GRID_MAX_SIDE = 1024      # cells a side of the chosen grid
CELL_LIST_BUDGET = 8           # list entries per polygon the chosen grid may spend (a floor of 4096 entries)


def _cell_ranges(boxes3, grid):
    """Per non-empty box the closed range of cells it meets on each axis: (rows, ix0, ix1, iy0, iy1)."""
    x0, y0, cw, ch, nx, ny = (int(v) for v in grid)
    rows = np.nonzero((boxes3[:, 0] <= boxes3[:, 2]) & (boxes3[:, 1] <= boxes3[:, 3]))[0]
    b = boxes3[rows]
    ix0, ix1 = np.floor_divide(b[:, 0] - x0, cw), np.floor_divide(b[:, 2] - x0, cw)
    iy0, iy1 = np.floor_divide(b[:, 1] - y0, ch), np.floor_divide(b[:, 3] - y0, ch)
    keep = (ix1 >= 0) & (ix0 < nx) & (iy1 >= 0) & (iy0 < ny)   # a box beside a grid the caller chose
    return (rows[keep], np.clip(ix0[keep], 0, nx - 1), np.clip(ix1[keep], 0, nx - 1), np.clip(iy0[keep], 0, ny - 1),
            np.clip(iy1[keep], 0, ny - 1))


def choose_cell_grid(polygon_boxes) -> np.ndarray:
    """The grid `polygon_cell_table` uses unless told otherwise, (x0, y0, cell_w, cell_h, nx, ny) int64 in units of a THIRD of a
    grid step (the units of 3 x centre): over the joint bounds of the non-empty boxes, square cells whose side is the median of
    the boxes' longer sides -- a typical polygon then meets about four cells and a cell about four polygons' boxes --, at most
    CELL_GRID_MAX_SIDE cells a side; the side is doubled while the lists would hold more than
    max(CELL_LIST_BUDGET x polygons, 4096) entries (a few polygons that span everything would otherwise be listed in every
    cell).  A cell is one unit wider than extent / n needs: n cells cover the closed bounds.  No box: one cell."""
    boxes3 = 3 * np.asarray(polygon_boxes, dtype=np.int64).reshape(-1, 4)
    live = boxes3[(boxes3[:, 0] <= boxes3[:, 2]) & (boxes3[:, 1] <= boxes3[:, 3])]
    if len(live) == 0:
        return np.array([0, 0, 1, 1, 1, 1], dtype=np.int64)
    x0, y0, x1, y1 = int(live[:, 0].min()), int(live[:, 1].min()), int(live[:, 2].max()), int(live[:, 3].max())
    side = max(int(np.median(np.maximum(live[:, 2] - live[:, 0], live[:, 3] - live[:, 1]))), 1)
    while True:
        nx = int(min(max(-(-(x1 - x0 + 1) // side), 1), CELL_GRID_MAX_SIDE))
        ny = int(min(max(-(-(y1 - y0 + 1) // side), 1), CELL_GRID_MAX_SIDE))
        grid = np.array([x0, y0, (x1 - x0) // nx + 1, (y1 - y0) // ny + 1, nx, ny], dtype=np.int64)
        _, ix0, ix1, iy0, iy1 = _cell_ranges(boxes3, grid)
        if int(np.sum((ix1 - ix0 + 1) * (iy1 - iy0 + 1))) <= max(CELL_LIST_BUDGET * len(live), 4096) or nx * ny == 1:
            return grid
        side *= 2


def polygon_cell_table(polygon_boxes, grid=None):
    """The cell index `HipRaster.face_polygon_index` takes, from the (P, 4) int64 boxes of `PlanarPolygons.snapped`:
    (grid (6,) int64 x0 y0 cell_w cell_h nx ny -- `choose_cell_grid` unless given --, cell_offsets (nx ny + 1,) int64,
    cell_polygons int32).  Cell (ix, iy) has index iy nx + ix and lists, in DESCENDING order, every row whose box meets it, the
    box closed on both sides; rows with the empty box are listed nowhere.  Work and memory are O(sum over polygons of the cells
    their box meets)."""
    boxes3 = 3 * np.asarray(polygon_boxes, dtype=np.int64).reshape(-1, 4)
    grid = choose_cell_grid(polygon_boxes) if grid is None else np.asarray(grid, dtype=np.int64).reshape(6)
    nx, ny = int(grid[4]), int(grid[5])
    if nx < 1 or ny < 1 or grid[2] < 1 or grid[3] < 1:
        raise ValueError(f"bad cell grid {grid.tolist()}: nx, ny and the cell size must be at least 1")
    rows, ix0, ix1, iy0, iy1 = _cell_ranges(boxes3, grid)
    w, h = ix1 - ix0 + 1, iy1 - iy0 + 1
    n = w * h
    owner = np.repeat(np.arange(len(rows)), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)      # position inside the polygon's block of cells
    cell = (iy0[owner] + k // w[owner]) * nx + ix0[owner] + k % w[owner]
    row = rows[owner]
    order = np.lexsort((-row, cell))                                    # by cell, the highest row first
    offsets = np.zeros(nx * ny + 1, dtype=np.int64)
    np.cumsum(np.bincount(cell, minlength=nx * ny), out=offsets[1:])
    return grid, offsets, np.ascontiguousarray(row[order], dtype=np.int32)


# -- the orthomosaic baseline: the bin table of the tile assembly, the work items of the zonal counts ----------------
ORTHO_BIN_SIDE = 64            # pixels a side of a bin of `tile_bin_table` unless told otherwise
ZONAL_BLOCK = (64, 16)         # cells (width, height) of a work item of `zonal_work_items` unless told otherwise


def tile_bin_table(windows, width: int, height: int, bin_side: int = ORTHO_BIN_SIDE):
    """The bin table `HipRaster.assemble_tiles` takes, by count-then-fill as `polygon_cell_table`: windows (T, 4) int col_off
    row_off width height inside a `height` x `width` extent -> (bin_ptr (bins_x bins_y + 1,) int64, bin_tiles int32, bin_side,
    bins_x, bins_y).  Bin (bx, by) has index by bins_x + bx, covers the pixels [bx side, (bx + 1) side) x [by side, (by + 1) side)
    and lists, in ASCENDING tile index, every tile whose window meets it.  Empty windows are listed nowhere."""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 4)
    side = int(bin_side)
    if side < 1:
        raise ValueError(f"bin_side must be at least 1, got {bin_side}")
    bins_x, bins_y = max(-(-int(width) // side), 1), max(-(-int(height) // side), 1)
    tiles = np.nonzero((windows[:, 2] > 0) & (windows[:, 3] > 0))[0]
    col, row, w, h = windows[tiles].T
    ix0, ix1 = np.clip(col // side, 0, bins_x - 1), np.clip((col + w - 1) // side, 0, bins_x - 1)
    iy0, iy1 = np.clip(row // side, 0, bins_y - 1), np.clip((row + h - 1) // side, 0, bins_y - 1)
    nw, nh = ix1 - ix0 + 1, iy1 - iy0 + 1
    n = nw * nh
    owner = np.repeat(np.arange(len(tiles)), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    cell = (iy0[owner] + k // nw[owner]) * bins_x + ix0[owner] + k % nw[owner]
    tile = tiles[owner]
    order = np.lexsort((tile, cell))
    bin_ptr = np.zeros(bins_x * bins_y + 1, dtype=np.int64)
    np.cumsum(np.bincount(cell, minlength=bins_x * bins_y), out=bin_ptr[1:])
    return bin_ptr, np.ascontiguousarray(tile[order], dtype=np.int32), side, bins_x, bins_y


def zonal_work_items(ring_vertices, ring_offsets, ring_polygon, n_polygons: int, height: int, width: int, block=ZONAL_BLOCK):
    """The work items `HipRaster.zonal_class_counts` takes (rule Z6), by count-then-fill from the rows' boxes: the ring table in
    cell units (1 / 65536 of a cell, `utils.geospatial.rings_to_cell_units`) -> (n, 7) int32 rows (polygon row, col0, row0, width,
    height, first ring, one past the last ring).  A row's box is the box of its rings of 3 or more vertices, clamped to the cells
    whose CENTRE it can hold inside the `height` x `width` raster, and is cut into blocks of at most block = (width <= 64,
    height <= 128) cells.  Rows whose box holds no centre have no item."""
    bw, bh = int(block[0]), int(block[1])
    if not (1 <= bw <= 64 and 1 <= bh <= 128):
        raise ValueError(f"a block is at most 64 x 128 cells, got {bw} x {bh}")
    rv = np.asarray(ring_vertices, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
    rp = np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
    P = int(n_polygons)
    big = np.iinfo(np.int64).max
    lo = np.full((P, 2), big, dtype=np.int64)
    hi = np.full((P, 2), -big, dtype=np.int64)
    live = np.nonzero(np.diff(off) >= 3)[0]
    if len(live) and len(rv):
        owner = np.repeat(rp[live], np.diff(off)[live])
        v = np.concatenate([rv[off[r]:off[r + 1]] for r in live])
        np.minimum.at(lo, owner, v)
        np.maximum.at(hi, owner, v)
    ring_lo, ring_hi = np.searchsorted(rp, np.arange(P), "left"), np.searchsorted(rp, np.arange(P), "right")
    rows = np.nonzero(lo[:, 0] <= hi[:, 0])[0]
    # a centre 65536 c + 32768 lies in [lo, hi] iff ceil((lo - 32768) / 65536) <= c <= floor((hi - 32768) / 65536)
    c0 = np.maximum(-((32768 - lo[rows, 0]) // 65536), 0)
    c1 = np.minimum((hi[rows, 0] - 32768) // 65536, int(width) - 1)
    r0 = np.maximum(-((32768 - lo[rows, 1]) // 65536), 0)
    r1 = np.minimum((hi[rows, 1] - 32768) // 65536, int(height) - 1)
    keep = (c0 <= c1) & (r0 <= r1)
    rows, c0, c1, r0, r1 = rows[keep], c0[keep], c1[keep], r0[keep], r1[keep]
    nx, ny = -(-(c1 - c0 + 1) // bw), -(-(r1 - r0 + 1) // bh)
    n = nx * ny
    owner = np.repeat(np.arange(len(rows)), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    bx, by = k % nx[owner], k // nx[owner]
    col0, row0 = c0[owner] + bx * bw, r0[owner] + by * bh
    items = np.stack([rows[owner], col0, row0, np.minimum(bw, c1[owner] + 1 - col0), np.minimum(bh, r1[owner] + 1 - row0),
                      ring_lo[rows[owner]], ring_hi[rows[owner]]], axis=1) if len(owner) else np.zeros((0, 7))
    return np.ascontiguousarray(items, dtype=np.int32)


# -- polygon rows burned into windows of a raster grid ---------------------------------------------------------
def row_centre_boxes(ring_vertices, ring_offsets, ring_polygon, n_polygons: int) -> np.ndarray:
    """(P, 4) int64 col0, row0, col1, row1: the inclusive, UNCLAMPED box of the cell indices whose centre the row's rings of 3 or
    more vertices can hold, from the ring table in cell units (`utils.geospatial.rings_to_cell_units`); a row that can hold none
    has the empty box (1, 1, 0, 0).  Computed once per ring table: `burn_work_items` cuts it to each window."""
    rv = np.asarray(ring_vertices, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
    rp = np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
    P = int(n_polygons)
    big = np.iinfo(np.int64).max
    lo = np.full((P, 2), big, dtype=np.int64)
    hi = np.full((P, 2), -big, dtype=np.int64)
    n = np.diff(off)
    if len(rv) and len(n):
        of_ring = np.repeat(np.arange(len(n)), n)          # the ring of every vertex
        live = n[of_ring] >= 3
        np.minimum.at(lo, rp[of_ring[live]], rv[live])
        np.maximum.at(hi, rp[of_ring[live]], rv[live])
    boxes = np.tile(np.array([1, 1, 0, 0], dtype=np.int64), (P, 1))
    rows = np.nonzero(lo[:, 0] <= hi[:, 0])[0]
    # a centre 65536 c + 32768 lies in [lo, hi] iff ceil((lo - 32768) / 65536) <= c <= floor((hi - 32768) / 65536)
    c0, c1 = -((32768 - lo[rows, 0]) // 65536), (hi[rows, 0] - 32768) // 65536
    r0, r1 = -((32768 - lo[rows, 1]) // 65536), (hi[rows, 1] - 32768) // 65536
    keep = (c0 <= c1) & (r0 <= r1)
    boxes[rows[keep]] = np.stack([c0, r0, c1, r1], axis=1)[keep]
    return boxes


def row_ring_ranges(ring_polygon, n_polygons: int) -> np.ndarray:
    """(P, 2) int64: the first ring of every row and one past its last, from the non-decreasing `ring_polygon`."""
    rp = np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
    rows = np.arange(int(n_polygons))
    return np.stack([np.searchsorted(rp, rows, "left"), np.searchsorted(rp, rows, "right")], axis=1).astype(np.int64)


def burn_work_items(boxes, ring_ranges, window, block=ZONAL_BLOCK) -> np.ndarray:
    """The work items `PolygonBurner.window` takes for one window (rule B5), by count-then-fill: boxes (P, 4) of
    `row_centre_boxes`, ring_ranges (P, 2) of `row_ring_ranges`, window = (col_off, row_off, width, height) in cells of the parent
    grid -> (n, 7) int32 rows (polygon row, col0, row0, width, height, first ring, one past the last ring) in PARENT coordinates:
    every row's box cut to the window and then into blocks of at most block = (width <= 64, height <= 128) cells.  Rows whose box
    misses the window have no item; no vertex is looked at."""
    bw, bh = int(block[0]), int(block[1])
    if not (1 <= bw <= 64 and 1 <= bh <= 128):
        raise ValueError(f"a block is at most 64 x 128 cells, got {bw} x {bh}")
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    ring_ranges = np.asarray(ring_ranges, dtype=np.int64).reshape(-1, 2)
    col_off, row_off, width, height = (int(v) for v in window)
    c0, c1 = np.maximum(boxes[:, 0], col_off), np.minimum(boxes[:, 2], col_off + width - 1)
    r0, r1 = np.maximum(boxes[:, 1], row_off), np.minimum(boxes[:, 3], row_off + height - 1)
    rows = np.nonzero((c0 <= c1) & (r0 <= r1))[0]
    c0, c1, r0, r1 = c0[rows], c1[rows], r0[rows], r1[rows]
    nx, ny = -(-(c1 - c0 + 1) // bw), -(-(r1 - r0 + 1) // bh)
    n = nx * ny
    owner = np.repeat(np.arange(len(rows)), n)
    if not len(owner):
        return np.zeros((0, 7), dtype=np.int32)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    bx, by = k % nx[owner], k // nx[owner]
    col0, row0 = c0[owner] + bx * bw, r0[owner] + by * bh
    items = np.stack([rows[owner], col0, row0, np.minimum(bw, c1[owner] + 1 - col0), np.minimum(bh, r1[owner] + 1 - row0),
                      ring_ranges[rows[owner], 0], ring_ranges[rows[owner], 1]], axis=1)
    return np.ascontiguousarray(items, dtype=np.int32)


def ring_edges(ring_vertices, ring_offsets, ring_polygon):
    """(edges (E, 4) int64 ax ay bx by, edge_row (E,) int64): every edge, the closing one included, of the rings of 3 or more
    vertices of a ring table, and the row each belongs to -- what `rectangle_meets_rows` walks."""
    rv = np.asarray(ring_vertices, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64).reshape(-1)
    rp = np.asarray(ring_polygon, dtype=np.int64).reshape(-1)
    edges, rows = [], []
    for r in range(len(rp)):
        ring = rv[off[r]:off[r + 1]]
        if len(ring) >= 3:
            edges.append(np.concatenate([ring, np.roll(ring, -1, axis=0)], axis=1))
            rows.append(np.full(len(ring), rp[r], dtype=np.int64))
    if not edges:
        return np.zeros((0, 4), dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(edges), np.concatenate(rows)


def rectangle_meets_rows(edges, edge_row, rectangle) -> bool:
    """Whether the CLOSED rectangle (x0, y0, x1, y1), x0 <= x1, y0 <= y1, intersects the union of the polygon rows behind `edges`
    (`ring_edges`), touching included; every row is the even-odd region of all its rings (Z3), all in one integer unit.  Exact:
    the boxes are compared in int64, the determinants are Python integers.  The rectangle meets a row iff a ring edge meets it
    (which covers a ring vertex inside it: an edge meets a box iff their boxes overlap and the box's corners do not all lie
    strictly on one side of the edge's line) or, when no edge does, iff the rectangle lies inside the row whole -- then all four
    corners agree and the corner (x0, y0) is asked.  This is no centre test: a thin row selects every rectangle it crosses."""
    x0, y0, x1, y1 = (int(v) for v in rectangle)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
    ax, ay, bx, by = edges.T
    near = np.nonzero((np.minimum(ax, bx) <= x1) & (np.maximum(ax, bx) >= x0) & (np.minimum(ay, by) <= y1) & (np.maximum(ay, by) >= y0))[0]
    for k in near:
        axk, ayk, bxk, byk = (int(v) for v in edges[k])
        side = [(bxk - axk) * (cy - ayk) - (byk - ayk) * (cx - axk) for cx, cy in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
        if not (all(s > 0 for s in side) or all(s < 0 for s in side)):
            return True
    # no edge meets the rectangle: the parity of the corner (x0, y0) per row, half-open in y, strictly left of the upward edge
    inside = {}
    for k in np.nonzero((ay > y0) != (by > y0))[0]:
        axk, ayk, bxk, byk = (int(v) for v in edges[k])
        o = (bxk - axk) * (y0 - ayk) - (byk - ayk) * (x0 - axk)
        if (o > 0) if byk > ayk else (o < 0):
            row = int(edge_row[k])
            inside[row] = not inside.get(row, False)
    return any(inside.values())


# -- polygon-on-polygon overlap areas --------------------------------------------------------------------------
OVERLAP_TILE = (256, 4096)   # GR_OVERLAP_TILE_A, GR_OVERLAP_TILE_B: the edge slots of row a and of row b in one work item


def snap_polygon_pair(polygons_a, polygons_b):
    """Rule A1: (table_a, table_b, origin) -- the snapped ring tables (`PlanarPolygons.snapped`) of two `PlanarPolygons`, both on the
    1e-6 m grid behind ONE integer origin, the middle of their joint bounds, as `snap_with_polygons` does for points and polygons.
    ValueError (from `snapped`) when a vertex lies more than 2^40 grid steps from it."""
    bounds = [b for b in (polygons_a.bounds_snapped(), polygons_b.bounds_snapped()) if b is not None]
    if bounds:
        lo, hi = np.min([b[0] for b in bounds], axis=0), np.max([b[1] for b in bounds], axis=0)
        origin = lo + (hi - lo) // 2
    else:
        origin = np.zeros(2, dtype=np.int64)
    return polygons_a.snapped(origin), polygons_b.snapped(origin), origin


def overlap_work_items(offsets_a, rows_a, offsets_b, rows_b, pairs, tile=OVERLAP_TILE) -> np.ndarray:
    """The work items `PolygonOverlap.areas` takes (rule A8), by count-then-fill: the ring offsets (R + 1,) and the non-decreasing
    ring rows (R,) of both tables, pairs (n, 2) rows (a, b) -> (m, 5) int32 rows (pair index, first edge slot and slots of row a,
    first slot and slots of row b).  The edge slots of a row are its ring vertices, consecutive because its rings are; they are
    cut into tiles of at most tile = (slots of a <= 256, slots of b <= 4096), a tile may start or end inside a ring, and a pair
    gets one item per (tile of a, tile of b), the tiles of b running fastest.  Pairs are listed in their own order; a pair with a
    row without vertices has no item (its area is 0)."""
    ta, tb = int(tile[0]), int(tile[1])
    if not (1 <= ta <= OVERLAP_TILE[0] and 1 <= tb <= OVERLAP_TILE[1]):
        raise ValueError(f"a tile is at most {OVERLAP_TILE[0]} x {OVERLAP_TILE[1]} edge slots, got {ta} x {tb}")
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)

    def spans(offsets, rows, which):
        off = np.asarray(offsets, dtype=np.int64).reshape(-1)
        rp = np.asarray(rows, dtype=np.int64).reshape(-1)
        return off[np.searchsorted(rp, which, "left")], off[np.searchsorted(rp, which, "right")]

    a_lo, a_hi = spans(offsets_a, rows_a, pairs[:, 0])
    b_lo, b_hi = spans(offsets_b, rows_b, pairs[:, 1])
    n_a, n_b = -(-(a_hi - a_lo) // ta), -(-(b_hi - b_lo) // tb)
    n = n_a * n_b
    owner = np.repeat(np.arange(len(pairs)), n)
    if not len(owner):
        return np.zeros((0, 5), dtype=np.int32)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    ka, kb = k // n_b[owner], k % n_b[owner]
    a0, b0 = a_lo[owner] + ka * ta, b_lo[owner] + kb * tb
    items = np.stack([owner, a0, np.minimum(ta, a_hi[owner] - a0), b0, np.minimum(tb, b_hi[owner] - b0)], axis=1)
    return np.ascontiguousarray(items, dtype=np.int32)
