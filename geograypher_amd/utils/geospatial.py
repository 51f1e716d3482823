"""WGS84 coordinate reference systems and the reprojection of points between them on the device (DESIGN.md "CRS
reprojection"; reference: utils/geospatial.py:51-71, which goes through pyproj).

One ellipsoid, three coordinate kinds, no datum shift: EPSG:4978 (ECEF), EPSG:4326 / EPSG:4979 (geographic) and the WGS84 UTM
zones EPSG:32601-32660 (north) and EPSG:32701-32760 (south), or a transverse Mercator with explicit parameters.  Everything
else -- another datum such as NAD83 (EPSG:26910), Web Mercator, a WKT string -- needs pyproj and is refused."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

KIND_ECEF, KIND_GEOGRAPHIC, KIND_TM = 0, 1, 2   # GR_CRS_ECEF, GR_CRS_GEOGRAPHIC, GR_CRS_TM of include/geograster.h
UTM_K0 = 0.9996
UTM_FALSE_EASTING = 500000.0
UTM_FALSE_NORTHING_SOUTH = 10000000.0


@dataclass(frozen=True)
class WGS84CRS:
    """A CRS on the WGS84 ellipsoid.  kind: KIND_ECEF (X, Y, Z), KIND_GEOGRAPHIC (degrees and ellipsoidal height) or KIND_TM
    (easting, northing, height; lon0 in degrees, k0, false easting and northing in metres).  `lat_first`: the authority's axis
    order is (lat, lon, h) -- EPSG:4326 and EPSG:4979, as pyproj hands them out.  `epsg`: the code it was parsed from, or None."""
    kind: int
    lon0: float = 0.0
    k0: float = 1.0
    false_easting: float = 0.0
    false_northing: float = 0.0
    epsg: Optional[int] = None
    lat_first: bool = False

    @staticmethod
    def transverse_mercator(lon0: float, k0: float = UTM_K0, false_easting: float = UTM_FALSE_EASTING,
                            false_northing: float = 0.0) -> "WGS84CRS":
        if not (np.isfinite(lon0) and np.isfinite(false_easting) and np.isfinite(false_northing)) or not k0 > 0:
            raise ValueError(f"transverse Mercator needs finite parameters and k0 > 0, got lon0={lon0} k0={k0} "
                             f"FE={false_easting} FN={false_northing}")
        return WGS84CRS(KIND_TM, float(lon0), float(k0), float(false_easting), float(false_northing))

    @staticmethod
    def utm(zone: int, south: bool = False) -> "WGS84CRS":
        if not 1 <= int(zone) <= 60:
            raise ValueError(f"UTM zones are 1 ... 60, got {zone}")
        return WGS84CRS(KIND_TM, 6.0 * int(zone) - 183.0, UTM_K0, UTM_FALSE_EASTING, UTM_FALSE_NORTHING_SOUTH if south else 0.0,
                        (32700 if south else 32600) + int(zone))

    @staticmethod
    def parse(designator) -> "WGS84CRS":
        """"EPSG:4978", "EPSG:4326", "EPSG:4979", "EPSG:32601" ... "EPSG:32660", "EPSG:32701" ... "EPSG:32760", the same as
        integers, or a WGS84CRS.  Anything else: NotImplementedError."""
        if isinstance(designator, WGS84CRS):
            return designator
        code = None
        if isinstance(designator, (int, np.integer)) and not isinstance(designator, bool):
            code = int(designator)
        elif isinstance(designator, str):
            text = designator.upper().replace(" ", "")
            if text.startswith("EPSG:") and text[5:].isdigit():
                code = int(text[5:])
        if code == 4978:
            return WGS84CRS(KIND_ECEF, epsg=4978)
        if code in (4326, 4979):
            return WGS84CRS(KIND_GEOGRAPHIC, epsg=code, lat_first=True)
        if code is not None and (32601 <= code <= 32660 or 32701 <= code <= 32760):
            return WGS84CRS.utm(code % 100, south=code >= 32700)
        raise NotImplementedError(
            f"CRS {designator!r}: only the WGS84 systems EPSG:4978, EPSG:4326, EPSG:4979 and the UTM zones EPSG:32601-32660 / "
            "EPSG:32701-32760 are reprojected here; any other CRS needs pyproj and is outside the projection path")

    def __str__(self):
        if self.epsg is not None:
            return f"EPSG:{self.epsg}"
        return ("WGS84 ECEF", "WGS84 lon/lat", f"WGS84 TM(lon0={self.lon0}, k0={self.k0}, FE={self.false_easting}, "
                f"FN={self.false_northing})")[self.kind]


def is_CRS_designator(value) -> bool:
    """What the `points_in_*_CRS` keywords take in place of an array: a string, an integer or a WGS84CRS."""
    return isinstance(value, (str, WGS84CRS)) or (isinstance(value, (int, np.integer)) and not isinstance(value, bool))


def crs_tuple(crs):
    """(kind, lon0, k0, false easting, false northing): the fields of the C ABI's gr_crs."""
    c = WGS84CRS.parse(crs)
    return (c.kind, c.lon0, c.k0, c.false_easting, c.false_northing)


def get_projected_CRS(lat, lon, assume_western_hem: bool = True) -> int:
    """The EPSG code of the WGS84 UTM zone of a position, by the reference's formula (utils/geospatial.py:51-57; Python's
    `round`, halves to even).  The reference wraps the code in a pyproj.CRS; every CRS argument here takes the code."""
    if assume_western_hem and lon > 0:
        lon = -lon
    return int(32700 - round((45 + lat) / 90) * 100 + round((183 + lon) / 6))


def _default_backend():
    from geograypher_amd._hip import HipRaster

    return HipRaster()


def reproject_points(backend, points, from_CRS, to_CRS, *, faces=None, pre_transform=None, force_easting_northing: bool = False,
                     return_tensor: bool = False):
    """points (V, 3) in `from_CRS`, in ITS axis order -> (N, 3) in `to_CRS` through `backend.reproject_points` (N = V, or the
    faces' count: their centres).  The result is in the axis order of `to_CRS` -- (lat, lon, h) for EPSG:4326 / 4979 -- unless
    `force_easting_northing`.  A host array unless `return_tensor`.  Returns (points, stats)."""
    src, dst = WGS84CRS.parse(from_CRS), WGS84CRS.parse(to_CRS)
    if src.lat_first:
        points = points[:, [1, 0, 2]]
    out, stats = backend.reproject_points(points, src, dst, faces=faces, pre_transform=pre_transform)
    if dst.lat_first and not force_easting_northing:
        out = out[:, [1, 0, 2]]
    if not return_tensor and hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    elif not return_tensor:
        out = np.asarray(out)
    return out, stats


def convert_CRS_3D_points(points, input_CRS, output_CRS, backend=None):
    """(n, 3) points of `input_CRS` in `output_CRS`, both in the CRS's own axis order (reference: utils/geospatial.py:60-71),
    computed on the device.  `backend`: an object with `HipRaster.reproject_points` (default: a HipRaster on the current device)."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (n, 3), got {points.shape}")
    out, _ = reproject_points(backend if backend is not None else _default_backend(), points, input_CRS, output_CRS)
    return np.array(out, dtype=np.float64)


def points_or_CRS(file_name: str, points_file, crs_name: str, crs):
    """What an entry point hands a `points_in_*_CRS` keyword: the array of `points_file` (a `.npy` path or the array itself), or
    the designator `crs` -- checked here, so that a CRS that cannot be reprojected fails before any work --, or None when neither
    is given.  Both is a ValueError."""
    from pathlib import Path

    if points_file is not None and crs is not None:
        raise ValueError(f"{file_name} and {crs_name} are both given: the points are either read or computed, not both")
    if crs is not None:
        if isinstance(crs, str) and crs.strip().isdigit():   # "32610" from a command line
            crs = int(crs)
        return WGS84CRS.parse(crs)
    return np.load(points_file) if isinstance(points_file, (str, Path)) else points_file


# -- the class counts of the raster cells under polygons (reference: utils/geospatial.py:150-211) ------------
def points_to_cell_units(xy, inverse, what: str = "point"):
    """THE arithmetic of rule Z1 (and N2): xy (n, 2) float64 in the raster's CRS -> (n, 2) int64 pixel coordinates times 65536,
    with the raster's `inverse` (ia, ib, ic, id, ie, if) in float64, every operation rounded on its own in the order of rule T2:
    col = (ia x + ib y) + ic, row = (id x + ie y) + if, q = rint(65536 value).  ValueError naming `what` for a value that is
    not finite or has |q| >= 2^40."""
    ia, ib, ic, id_, ie, if_ = (np.float64(v) for v in inverse)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    col = (x * ia + y * ib) + ic
    row = (x * id_ + y * ie) + if_
    q = np.rint(np.stack([col, row], axis=1) * 65536.0)
    if q.size and not np.all(np.abs(q) < 2.0 ** 40):
        raise ValueError(f"a {what} is not finite or lies 2^40 / 65536 cells or more from the raster's corner")
    return q.astype(np.int64)


def rings_to_cell_units(rings, inverse):
    """Rule Z1: ring vertices (x, y) in the raster's CRS -> int64 pixel coordinates times 65536, with the raster's `inverse`
    (ia, ib, ic, id, ie, if) in float64, every operation rounded on its own in the order of rule T2: col = (ia x + ib y) + ic,
    row = (id x + ie y) + if, q = rint(65536 value).  rings: a list of (n, 2) arrays -> (ring_vertices (N, 2) int64, ring_offsets
    (R + 1,) int64).  ValueError for a value that is not finite or has |q| >= 2^40."""
    verts, offsets = [], [0]
    for ring in rings:
        q = points_to_cell_units(np.asarray(ring, dtype=np.float64).reshape(-1, 2), inverse, "polygon vertex")
        verts.append(q)
        offsets.append(offsets[-1] + len(q))
    ring_vertices = np.concatenate(verts) if verts else np.zeros((0, 2), dtype=np.int64)
    return np.ascontiguousarray(ring_vertices.reshape(-1, 2)), np.asarray(offsets, dtype=np.int64)


def raster_to_uint8(data, nodata):
    """Rule Z5: a band of a `PlanarRaster` -> (uint8 array, the nodata value as gr_zonal_class_counts takes it: an int in
    [0, 255] or None).  ValueError for a value that is not an integer in [0, 255] and not `nodata`."""
    from geograypher_amd._hip import zonal_nodata

    data = np.asarray(data)
    if data.dtype == np.uint8:
        cells = data
    else:
        values = data.astype(np.float64)
        is_nodata = np.zeros(values.shape, dtype=bool) if nodata is None else ((values == nodata) | (np.isnan(values) & bool(np.isnan(nodata))))
        with np.errstate(invalid="ignore"):
            fits = (values >= 0) & (values <= 255) & (values == np.floor(values))
        if not np.all(fits | is_nodata):
            raise ValueError(f"{int(np.sum(~(fits | is_nodata)))} raster cells hold a value that is not an integer in [0, 255] and not nodata")
        cells = np.where(fits, values, 0).astype(np.uint8)
        if zonal_nodata(nodata) < 0 and np.any(is_nodata):
            # a nodata value no uint8 cell can hold: park those cells on a value the raster does not use
            free = np.setdiff1d(np.arange(256), np.unique(cells[fits]))
            if not len(free):
                raise ValueError("the raster uses all 256 values and has nodata cells beside them")
            cells[is_nodata] = free[-1]
            return np.ascontiguousarray(cells), int(free[-1])
    nd = zonal_nodata(nodata)
    return np.ascontiguousarray(cells), None if nd < 0 else nd


def _as_planar_polygons(polygons):
    from geograypher_amd.utils.geometric import PlanarPolygons

    if isinstance(polygons, PlanarPolygons):
        return polygons
    if isinstance(polygons, (str, bytes)) or hasattr(polygons, "__fspath__"):
        if not str(polygons).lower().endswith((".geojson", ".json")):
            raise NotImplementedError(f"{polygons}: polygon files are read as .geojson only")
        return PlanarPolygons.from_geojson(polygons)[0]
    return PlanarPolygons.from_sequence(polygons)


def _as_planar_raster(raster):
    from geograypher_amd.utils.raster import PlanarRaster

    return raster if isinstance(raster, PlanarRaster) else PlanarRaster.from_geotiff(raster)


def zonal_class_counts(polygons, classes_raster, num_classes=None, backend=None, block=None):
    """The cells of every value under every polygon row, counted on the device (`HipRaster.zonal_class_counts`): polygons a
    `PlanarPolygons`, a `.geojson` path or a sequence of ring arrays, in the raster's CRS; classes_raster a path or a
    `PlanarRaster` whose band 0 holds integers in [0, 255] -> (counts (P, C) int64, stats dict).  num_classes=None: 1 + the
    largest counted value (at least 1).  A counted value >= num_classes is a ValueError naming how many cells hold one.  A cell
    belongs to a row iff its CENTRE lies in it under the half-open even-odd rule Z3 over all rings of the row; what GDAL's
    rasterize(all_touched=False), behind rasterstats, decides for a centre exactly ON a boundary is not measured (GDAL is not
    available here): the two can differ on those cells only."""
    from geograypher_amd import _hip
    from geograypher_amd.utils.geometric import ZONAL_BLOCK, zonal_work_items

    polygons = _as_planar_polygons(polygons)
    raster = _as_planar_raster(classes_raster)
    cells, nodata = raster_to_uint8(raster.data[0], raster.nodata)
    H, W = cells.shape
    rv, off = rings_to_cell_units(polygons.rings, raster.inverse)
    rp = np.asarray(polygons.ring_polygon, dtype=np.int32)
    P = len(polygons)
    items = zonal_work_items(rv, off, rp, P, H, W, ZONAL_BLOCK if block is None else block)
    backend = backend if backend is not None else _default_backend()
    C = _hip.GR_ZONAL_MAX_CLASSES if num_classes is None else int(num_classes)
    counts, stats = backend.zonal_class_counts(cells, nodata, rv, off, rp, P, items, C)
    counts = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts, dtype=np.int64)
    stats = np.asarray(stats.cpu() if hasattr(stats, "cpu") else stats, dtype=np.int64)
    names = ("tested", "inside", "nodata", "over", "largest_plus_1", "largest_ring", "rings_ignored")
    stats = {k: int(stats[i]) for i, k in enumerate(names)}
    if num_classes is None:
        counts = counts[:, :max(stats["largest_plus_1"], 1)]
    elif stats["over"]:
        raise ValueError(f"{stats['over']} counted cells hold a value >= num_classes={C} (the largest is {stats['largest_plus_1'] - 1})")
    return counts, stats


def get_overlap_raster(unlabeled_df, classes_raster, num_classes=None, normalize: bool = False, backend=None):
    """The class counts of the raster cells under every polygon (reference: utils/geospatial.py:150-211, which calls
    rasterstats.zonal_stats per polygon) -> (counts_matrix (n_valid, C) float64, valid_IDs (n_valid,) int64): one row per VALID
    polygon -- a polygon with at least one counted cell --, in ascending polygon index; `normalize` divides every row by its
    sum.  The reference writes the counts of valid polygon k into row valid_IDs[k] of its n_valid-row matrix, which is out of
    place (or out of bounds) whenever an invalid polygon precedes a valid one; this builds the matrix that was meant, row k for
    valid polygon k.  Inputs, num_classes and the boundary rule as `zonal_class_counts`."""
    counts, _ = zonal_class_counts(unlabeled_df, classes_raster, num_classes, backend=backend)
    valid = np.nonzero(counts.sum(axis=1) > 0)[0].astype(np.int64)
    matrix = counts[valid].astype(np.float64)
    if normalize:
        matrix = matrix / np.sum(matrix, axis=1, keepdims=True)
    return matrix, valid


# -- polygon rows burned into a label raster (reference: rasterio.features.rasterize in write_chips) ------------
def _to_host(x) -> np.ndarray:
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x)


def rings_in_raster_CRS(polygons, raster_epsg, backend=None):
    """The rings of a `PlanarPolygons` in the CRS of a raster: as they stand unless `polygons.epsg` and `raster_epsg` are both
    known and differ; then every vertex is reprojected on its own with `backend.reproject_points` at height 0 (what geopandas'
    to_crs does: edges are not densified).  GeoJSON coordinates are (easting, northing) / (lon, lat) whatever the authority's
    axis order.  NotImplementedError where `WGS84CRS.parse` refuses one of the two."""
    if polygons.epsg is None or raster_epsg is None or int(polygons.epsg) == int(raster_epsg) or not polygons.rings:
        return polygons.rings
    src, dst = WGS84CRS.parse(int(polygons.epsg)), WGS84CRS.parse(int(raster_epsg))
    xy = np.concatenate(polygons.rings)
    points = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1)
    out, _ = (backend if backend is not None else _default_backend()).reproject_points(points, src, dst)
    out = _to_host(out).astype(np.float64)[:, :2]
    return np.split(out, np.cumsum([len(r) for r in polygons.rings])[:-1])


def burn_values(values, n_polygons: int) -> np.ndarray:
    """(P,) uint8 from one value per polygon row: every value must be an integer in [0, 255], else ValueError (the reference's
    astype(np.uint8) wraps such values silently)."""
    values = list(values) if not isinstance(values, np.ndarray) else values.tolist()
    if len(values) != int(n_polygons):
        raise ValueError(f"{n_polygons} polygon rows need as many values, got {len(values)}")
    out = np.zeros(len(values), dtype=np.uint8)
    for k, v in enumerate(values):
        is_number = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
        if not is_number or not np.isfinite(v) or v != int(v) or not 0 <= int(v) <= 255:
            raise ValueError(f"the value {v!r} of polygon row {k} is not an integer in [0, 255]")
        out[k] = int(v)
    return out


def _grid_like(like):
    """(height, width, transform, epsg) of a `PlanarRaster`, a GeoTIFF path (header only) or ((height, width), transform)."""
    from geograypher_amd.utils.raster import PlanarRaster, read_geotiff_header

    if isinstance(like, PlanarRaster):
        return like.data.shape[1], like.data.shape[2], like.transform, like.epsg
    if isinstance(like, (str, bytes)) or hasattr(like, "__fspath__"):
        transform, _nodata, epsg, height, width = read_geotiff_header(like)
        return height, width, transform, epsg
    (height, width), transform = like
    return int(height), int(width), tuple(float(v) for v in transform), None


def burn_polygons(polygons, values, like, fill: int = 255, backend=None, max_device_bytes=None, rows: bool = False):
    """Polygon rows burned into a raster grid on the device (`HipRaster.polygon_burner`, gr_burn_polygons; rules B1-B7 of
    DESIGN.md 8m), in place of rasterio.features.rasterize(zip(shapes, values), out_shape, transform=..., fill=fill).

    polygons: a `PlanarPolygons`, a `.geojson` path or a sequence of ring arrays; when their EPSG code and the raster's are both
    known and differ the vertices are reprojected (`rings_in_raster_CRS`).  values: one integer in [0, 255] per row (ValueError
    otherwise); may be None with `rows`.  like: the grid -- a `PlanarRaster`, a GeoTIFF path (only its header is read) or
    ((height, width), transform).  A cell takes the value of the HIGHEST row that holds its centre (later rows overwrite earlier
    ones, rasterize's merge_alg=replace) and `fill` where none does; the centre rule is Z3 of `zonal_class_counts`, so a burned
    raster and its zonal counts agree cell for cell, and what GDAL decides for a centre exactly ON a boundary is as unmeasured
    here as there.  Returns the (height, width) uint8 raster, or with `rows` the int32 plane of winning rows (-1: none).
    The grid is burned in bands of rows that take at most `max_device_bytes` of device memory, 5 bytes a cell (default: the
    assembly's); the bands do not change a byte."""
    from geograypher_amd.predictors.ortho_segmentor import DEFAULT_MAX_DEVICE_BYTES, MAX_BAND_ROWS
    from geograypher_amd.utils.geometric import burn_work_items, row_centre_boxes, row_ring_ranges
    from geograypher_amd.utils.raster import invert_affine

    polygons = _as_planar_polygons(polygons)
    height, width, transform, epsg = _grid_like(like)
    P = len(polygons)
    if values is None and not rows:
        raise ValueError("burn_polygons needs one value per polygon row unless the row plane is asked for (rows=True)")
    values = None if values is None else burn_values(values, P)
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"fill={fill} does not fit the uint8 raster")
    backend = backend if backend is not None else _default_backend()
    rv, off = rings_to_cell_units(rings_in_raster_CRS(polygons, epsg, backend), invert_affine(transform))
    rp = np.asarray(polygons.ring_polygon, dtype=np.int32)
    burner = backend.polygon_burner(rv, off, rp, P, values)
    boxes, ranges = row_centre_boxes(rv, off, rp, P), row_ring_ranges(rp, P)
    budget = DEFAULT_MAX_DEVICE_BYTES if max_device_bytes is None else int(max_device_bytes)
    band = int(max(1, min(height, MAX_BAND_ROWS, budget // (5 * max(width, 1)))))
    result = np.empty((height, width), dtype=np.int32 if rows else np.uint8)
    for row0 in range(0, height, band):
        n = min(band, height - row0)
        window = (0, row0, width, n)
        rows_t, out_t, _stats = burner.window(*window, burn_work_items(boxes, ranges, window), fill=int(fill), want_values=not rows)
        result[row0:row0 + n] = _to_host(rows_t if rows else out_t)
    return result


# -- the mesh seen from above on a raster grid (the reference has no counterpart) ------------------------------
TOP_DOWN_STAT_NAMES = ("faces", "bad_index", "zero_area", "nonfinite_z", "empty_box", "items", "tests", "inside", "skipped", "covered")
GRID_SIDE_LIMIT = 1 << 23   # Z2: H, W stay below it


def grid_from_bounds(points_xy, resolution):
    """A north-up grid of square cells of `resolution` CRS units that holds the points (n, 2+): ((H, W), transform) with transform
    (a, b, c, d, e, f) = (res, 0, floor(xmin / res) res, 0, -res, ceil(ymax / res) res), W = ceil((xmax - c) / res), H =
    ceil((f - ymin) / res), both at least 1.  ValueError for a resolution that is not positive and finite, points that are not
    finite (or none), or H, W >= 2^23."""
    res = float(resolution)
    if not np.isfinite(res) or res <= 0:
        raise ValueError(f"resolution={resolution!r} is not a positive, finite cell size")
    xy = np.asarray(points_xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] < 2 or xy.shape[0] < 1 or not np.all(np.isfinite(xy[:, :2])):
        raise ValueError("grid_from_bounds needs at least one point, (n, 2) or (n, 3), all finite")
    xmin, xmax, ymin, ymax = xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()
    c, f = float(np.floor(xmin / res) * res), float(np.ceil(ymax / res) * res)
    W, H = max(int(np.ceil((xmax - c) / res)), 1), max(int(np.ceil((f - ymin) / res)), 1)
    if H >= GRID_SIDE_LIMIT or W >= GRID_SIDE_LIMIT:
        raise ValueError(f"resolution={res}: the grid would have {H} x {W} cells, not below 2^23 on both sides")
    return (H, W), (res, 0.0, c, 0.0, -res, f)


def top_down_raster(points, faces, like, backend=None, max_device_bytes=None, return_tensor: bool = False):
    """The mesh seen from above on a raster grid, on the device (`HipRaster.nadir_rasterizer`, gr_nadir_raster; rules N1-N9 of
    DESIGN.md 8r): points (V, 3) float64 in the grid's CRS, faces (F, 3) integers, like: the grid -- a `PlanarRaster`, a GeoTIFF
    path (only its header is read) or ((height, width), transform) -> (face_ids (height, width) int32: the face whose surface is
    HIGHEST at the cell's centre, -1 where no face holds it; heights (height, width) float64: that height, NaN there; stats: a
    dict of `TOP_DOWN_STAT_NAMES`, summed over the bands).  A centre exactly on an edge or a vertex belongs to one face (rule
    Z3 of `zonal_class_counts`, on the triangle), so faces that tile a region partition its cells; vertical faces take no part.
    Equal heights go to the lower face index.  ValueError for a vertex that is not finite or lies 2^40 / 65536 cells or more from
    the grid's corner, a face that names no vertex, H or W >= 2^23.  The grid is rastered in bands of rows that take at most
    `max_device_bytes` of device memory, 12 bytes a cell (default: the assembly's); the bands do not change a byte.  Host
    arrays unless `return_tensor` (then the two planes are tensors on the backend's device)."""
    from geograypher_amd.predictors.ortho_segmentor import DEFAULT_MAX_DEVICE_BYTES, MAX_BAND_ROWS
    from geograypher_amd.utils.raster import invert_affine

    height, width, transform, _epsg = _grid_like(like)
    if not (1 <= height < GRID_SIDE_LIMIT and 1 <= width < GRID_SIDE_LIMIT):
        raise ValueError(f"the grid has {height} x {width} cells, not inside [1, 2^23) on both sides")
    points = np.asarray(points.cpu() if hasattr(points, "cpu") else points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (V, 3), got {points.shape}")
    faces = np.asarray(faces.cpu() if hasattr(faces, "cpu") else faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
        raise ValueError(f"faces must be an (F, 3) integer array, got {faces.shape} {faces.dtype}")
    verts_q = points_to_cell_units(points[:, :2], invert_affine(transform), "mesh vertex")
    backend = backend if backend is not None else _default_backend()
    rasterizer = backend.nadir_rasterizer(verts_q, np.ascontiguousarray(points[:, 2]), faces.astype(np.int32))
    budget = DEFAULT_MAX_DEVICE_BYTES if max_device_bytes is None else int(max_device_bytes)
    band = int(max(1, min(height, MAX_BAND_ROWS, budget // (12 * max(width, 1)))))
    face_parts, z_parts, totals = [], [], np.zeros(len(TOP_DOWN_STAT_NAMES), dtype=np.int64)
    for row0 in range(0, height, band):
        face_t, z_t, stats = rasterizer.window(0, row0, width, min(band, height - row0))
        if not return_tensor:
            face_t, z_t = _to_host(face_t), _to_host(z_t)
        face_parts.append(face_t)
        z_parts.append(z_t)
        s = _to_host(stats).astype(np.int64)
        totals += s[:len(totals)]
        # the words about the faces themselves are the same in every band
        totals[:4] = s[:4]
    if len(face_parts) == 1:
        face_ids, heights = face_parts[0], z_parts[0]
    elif return_tensor and hasattr(face_parts[0], "device"):
        import torch

        face_ids, heights = torch.cat(face_parts), torch.cat(z_parts)
    else:
        face_ids, heights = np.concatenate(face_parts), np.concatenate(z_parts)
    return face_ids, heights, {k: int(v) for k, v in zip(TOP_DOWN_STAT_NAMES, totals)}


# -- raster -> raster: any raster on any grid in any supported CRS (reference: utils/geospatial.py:333-392) ----
WARP_OUTLINE_POINTS = 21   # points per edge of the source outline, corners aside, that `default_warp_grid` reprojects


def _crs_or_none(crs):
    return None if crs is None else WGS84CRS.parse(crs)


def _crs_epsg(crs):
    return None if crs is None else crs.epsg


def default_warp_grid(raster, src_crs, dst_crs, backend=None):
    """The grid a raster takes in another CRS when nothing else is asked for -> ((H', W'), transform).  The source outline -- its
    corners and `WARP_OUTLINE_POINTS` points along every edge -- goes through `backend.reproject_points`; with its bounds xmin, xmax, ymin,
    ymax: res = hypot(xmax - xmin, ymax - ymin) / hypot(W, H), W' = max(1, floor((xmax - xmin) / res + 0.5)), H' likewise, the grid
    north-up with its corner at (xmin, ymax).  This is the rule GDAL documents for its suggested warp output (the diagonal keeps
    its count of cells); parity with GDAL's numbers is not measured.  raster: a `PlanarRaster` or ((H, W), transform).  Geographic
    grids are (lon, lat): x is the longitude."""
    from geograypher_amd.utils.raster import PlanarRaster

    if isinstance(raster, PlanarRaster):
        H, W, transform = raster.data.shape[1], raster.data.shape[2], raster.transform
    else:
        (H, W), transform = raster
    a, b, c, d, e, f = (float(v) for v in transform)
    n = WARP_OUTLINE_POINTS + 1
    t = np.arange(n, dtype=np.float64) / n
    cols = np.concatenate([t * W, np.full(n, float(W)), (1.0 - t) * W, np.zeros(n)])
    rows = np.concatenate([np.zeros(n), t * H, np.full(n, float(H)), (1.0 - t) * H])
    outline = np.stack([(a * cols + b * rows) + c, (d * cols + e * rows) + f, np.zeros(4 * n)], axis=1)
    # (the backend's own call: rows are (x, y) = (lon, lat) on both sides, whatever the authority's axis order)
    out, _ = (backend if backend is not None else _default_backend()).reproject_points(outline, WGS84CRS.parse(src_crs),
                                                                                       WGS84CRS.parse(dst_crs))
    out = _to_host(out).astype(np.float64)
    if not np.all(np.isfinite(out[:, :2])):
        raise ValueError(f"default_warp_grid: the raster's outline cannot be taken from {src_crs} to {dst_crs}")
    xmin, xmax, ymin, ymax = out[:, 0].min(), out[:, 0].max(), out[:, 1].min(), out[:, 1].max()
    res = float(np.hypot(xmax - xmin, ymax - ymin) / np.hypot(float(W), float(H)))
    if not res > 0.0:
        raise ValueError("default_warp_grid: the reprojected outline has no extent")
    Wd, Hd = max(1, int(np.floor((xmax - xmin) / res + 0.5))), max(1, int(np.floor((ymax - ymin) / res + 0.5)))
    if Hd >= GRID_SIDE_LIMIT or Wd >= GRID_SIDE_LIMIT:
        raise ValueError(f"default_warp_grid: the grid would have {Hd} x {Wd} cells, not below 2^23 on both sides")
    return (Hd, Wd), (res, 0.0, float(xmin), 0.0, -res, float(ymax))


def _warp_sides(src_crs, dst_crs):
    """The CRS-known/unknown matrix of `warp_raster` -> (src, dst) as WGS84CRS for a cross-CRS warp, (None, None) for a same-CRS one."""
    if (src_crs is None) != (dst_crs is None):
        missing, known = ("src_crs=", "dst_crs=") if src_crs is None else ("dst_crs=", "src_crs=")
        raise ValueError(f"warp_raster: {known[:-1]} is known and {missing[:-1]} is not; name the other CRS with {missing} (or neither: "
                         "both grids are then taken to share one CRS)")
    src, dst = _crs_or_none(src_crs), _crs_or_none(dst_crs)   # NotImplementedError for a CRS that is not reprojected here
    if src is None or src == dst or (src.epsg is not None and src.epsg == dst.epsg):
        return None, None
    if KIND_ECEF in (src.kind, dst.kind):
        raise ValueError(f"warp_raster: {src} -> {dst}: an ECEF side: a raster is planar or geographic")
    return src, dst


def warp_raster(raster, like=None, *, resolution=None, dst_crs=None, src_crs=None, resampling: str = "nearest", dst_nodata=None,
                backend=None, max_device_bytes=None, return_tensor: bool = False):
    """A raster on another grid, in the same or in another WGS84 CRS, resampled on the device (`HipRaster.warp_raster`,
    gr_warp_raster; rules W1-W9 of DESIGN.md 8t), in place of rasterio.warp.reproject -> a `PlanarRaster` of the source's dtype (with
    `return_tensor` its `.data` is the (B, H', W') tensor on the backend's device).

    raster: a `PlanarRaster` or a single-band GeoTIFF path.  like: the destination grid -- a `PlanarRaster`, a GeoTIFF path (only its
    header is read) or ((height, width), transform); None: `default_warp_grid` in `dst_crs`, or with `resolution` a north-up grid of
    square cells of that size over the reprojected outline (`grid_from_bounds`).  src_crs defaults to `raster.epsg`, dst_crs to the
    EPSG code of `like`.  Both known and different: a cross-CRS warp; both known and equal, or both unknown: the grids share a CRS;
    exactly one known: ValueError naming the keyword to give.  A CRS that `WGS84CRS.parse` refuses: NotImplementedError.
    resampling: "nearest" (the cell the centre falls into) or "bilinear" (four taps; GDAL widens its kernel when it decimates, this
    does not).  dst_nodata: default the source's, else NaN.  The source goes to the device once; the destination is produced in
    bands of rows that take at most `max_device_bytes` (default: the assembly's); the bands do not change a byte.
    `.last_warp_stats` of the result: the statistics summed over the bands (`_hip.WARP_STAT_NAMES`)."""
    from geograypher_amd import _hip
    from geograypher_amd.predictors.ortho_segmentor import DEFAULT_MAX_DEVICE_BYTES, MAX_BAND_ROWS
    from geograypher_amd.utils.raster import PlanarRaster

    raster = _as_planar_raster(raster)
    backend = backend if backend is not None else _default_backend()
    like_epsg = None
    if like is not None:
        height, width, transform, like_epsg = _grid_like(like)
    src_crs = raster.epsg if src_crs is None else src_crs
    dst_crs = like_epsg if dst_crs is None else dst_crs
    src, dst = _warp_sides(src_crs, dst_crs)
    if like is None:
        if src is None and resolution is None:
            raise ValueError("warp_raster: no destination: give like=, resolution= or a dst_crs= that differs from the source's")
        if src is None:
            (height, width), transform = default_warp_grid_same(raster, resolution)
        elif resolution is None:
            (height, width), transform = default_warp_grid(raster, src, dst, backend)
        else:
            (Hd, Wd), t = default_warp_grid(raster, src, dst, backend)
            corners = np.array([[t[2], t[5]], [t[2] + Wd * t[0], t[5] + Hd * t[4]]])
            (height, width), transform = grid_from_bounds(corners, resolution)
    elif resolution is not None:
        raise ValueError("warp_raster: like= and resolution= are both given: the grid is either named or built, not both")
    if not (1 <= height < GRID_SIDE_LIMIT and 1 <= width < GRID_SIDE_LIMIT):
        raise ValueError(f"the grid has {height} x {width} cells, not inside [1, 2^23) on both sides")
    B = raster.data.shape[0]
    item = raster.data.dtype.itemsize
    nd = _hip.warp_dst_nodata(dst_nodata, raster.nodata, raster.data.dtype)
    budget = DEFAULT_MAX_DEVICE_BYTES if max_device_bytes is None else int(max_device_bytes)
    band = int(max(1, min(height, MAX_BAND_ROWS, budget // (B * item * max(width, 1)))))
    data_t = backend.to_device(raster.data, raster.data.dtype.name) if hasattr(backend, "to_device") else raster.data
    parts, totals = [], np.zeros(len(_hip.WARP_STAT_NAMES), dtype=np.int64)
    for row0 in range(0, height, band):
        out_t, stats = backend.warp_raster(data_t, raster.inverse, raster.nodata, transform, (0, row0, width, min(band, height - row0)),
                                           src_crs=src, dst_crs=dst, resampling=resampling, dst_nodata=nd)
        parts.append(out_t if return_tensor else _to_host(out_t))
        totals += _to_host(stats).astype(np.int64)[:len(totals)]
    if len(parts) == 1:
        data = parts[0]
    elif return_tensor and hasattr(parts[0], "device"):
        import torch

        data = torch.cat(parts, dim=1)
    else:
        data = np.concatenate(parts, axis=1)
    epsg = _crs_epsg(dst) if dst is not None else (like_epsg if like_epsg is not None else raster.epsg)
    result = PlanarRaster(np.zeros((1, 1, 1), dtype=raster.data.dtype), transform, None if np.isnan(nd) else nd, epsg)
    result.data = data   # (set behind the constructor, which widens uint8: the warp keeps the source's dtype)
    result.last_warp_stats = {k: int(v) for k, v in zip(_hip.WARP_STAT_NAMES, totals)}
    return result


def default_warp_grid_same(raster, resolution):
    """The north-up grid of square cells of `resolution` over the outline of a raster, in the raster's own CRS."""
    H, W = raster.data.shape[1], raster.data.shape[2]
    a, b, c, d, e, f = raster.transform
    cols, rows = np.array([0.0, W, W, 0.0]), np.array([0.0, 0.0, H, H])
    return grid_from_bounds(np.stack([(a * cols + b * rows) + c, (d * cols + e * rows) + f], axis=1), resolution)


def read_raster_bands(path):
    """All bands of a GeoTIFF as a `PlanarRaster` whose data keep the file's sample type where the warp takes it (uint8, float32;
    anything else becomes float64): (raster, the file's numpy dtype).  Read with PIL: single-band files of `GEOTIFF_MODES`, RGB and
    RGBA."""
    from PIL import Image

    from geograypher_amd.utils.raster import PlanarRaster, georeference_from_tags

    limit, Image.MAX_IMAGE_PIXELS = Image.MAX_IMAGE_PIXELS, None
    try:
        with Image.open(path) as image:
            tags = image.tag_v2 if hasattr(image, "tag_v2") else {}
            transform, nodata, epsg = georeference_from_tags(path, tags)
            data = np.array(image)
    finally:
        Image.MAX_IMAGE_PIXELS = limit
    file_dtype = data.dtype
    data = data[None] if data.ndim == 2 else np.ascontiguousarray(np.moveaxis(data, 2, 0))
    raster = PlanarRaster(np.zeros((1, 1, 1)), transform, nodata, epsg)
    raster.data = np.ascontiguousarray(data if data.dtype in (np.uint8, np.float32, np.float64) else data.astype(np.float64))
    return raster, file_dtype


def reproject_raster(in_path, out_path, out_crs="EPSG:4326", *, resampling: str = "nearest", like=None, resolution=None, backend=None):
    """A GeoTIFF in another CRS, all bands, file to file (reference: utils/geospatial.py:333-359, rasterio.warp.reproject with
    nearest resampling on calculate_default_transform's grid).  The grid is `default_warp_grid` unless `like` or `resolution` names
    one; a geographic grid is (lon, lat).  The file is written with `write_tiff_deflate` and records the destination's EPSG code,
    transform and nodata.  NotImplementedError for a CRS `WGS84CRS.parse` refuses, a file that names no CRS, and a sample type or
    band count the writer cannot hold (it names them).  Returns the `PlanarRaster` that was written."""
    from geograypher_amd.utils.tiff import _TYPES, write_tiff_deflate

    raster, file_dtype = read_raster_bands(in_path)
    if raster.epsg is None:
        raise NotImplementedError(f"{in_path}: the file names no EPSG code; its CRS cannot be told")
    if np.dtype(file_dtype) not in _TYPES or raster.data.dtype != file_dtype:
        raise NotImplementedError(f"{in_path}: samples of dtype {file_dtype} are not written by the TIFF writer here "
                                  f"({', '.join(str(t) for t in _TYPES)} that the warp keeps: uint8, float32)")
    if raster.data.shape[0] not in (1, 3):
        raise NotImplementedError(f"{in_path}: {raster.data.shape[0]} bands are not written by the TIFF writer here (1 or 3)")
    dst = WGS84CRS.parse(out_crs)
    out = warp_raster(raster, like, resolution=resolution, dst_crs=dst, resampling=resampling, backend=backend)
    out.epsg = dst.epsg if dst.epsg is not None else out.epsg
    image = out.data[0] if out.data.shape[0] == 1 else np.moveaxis(out.data, 0, 2)
    write_tiff_deflate(out_path, np.ascontiguousarray(image), transform=out.transform, nodata=out.nodata, epsg=out.epsg)
    return out


def load_downsampled_raster_data(dataset_filename, downsample_factor: float, *, backend=None):
    """A raster read at 1 / downsample_factor of its size (reference: utils/geospatial.py:362-392, a rasterio read with
    out_shape and bilinear resampling) -> (data (B, H', W'), the `PlanarRaster` of the source as the file holds it, the updated
    transform): H' = int(H / factor), W' = int(W / factor), the transform scaled by (W / W', H / H').  Sampling is the four-tap
    bilinear rule W6 at the centres of the new cells; GDAL widens its kernel when it decimates, this does not, so at factors above
    2 the two differ (this one aliases where GDAL averages)."""
    factor = float(downsample_factor)
    if not np.isfinite(factor) or factor <= 0:
        raise ValueError(f"downsample_factor={downsample_factor!r} is not a positive, finite number")
    raster, _ = read_raster_bands(dataset_filename)
    H, W = raster.data.shape[1], raster.data.shape[2]
    Hd, Wd = int(H / factor), int(W / factor)
    if Hd < 1 or Wd < 1:
        raise ValueError(f"downsample_factor={factor}: a raster of {H} x {W} cells would have no cell left")
    a, b, c, d, e, f = raster.transform
    sx, sy = W / Wd, H / Hd
    updated = (a * sx, b * sy, c, d * sx, e * sy, f)
    src_epsg, raster.epsg = raster.epsg, None     # the grids share the file's CRS, whatever it is
    try:
        out = warp_raster(raster, ((Hd, Wd), updated), resampling="bilinear", backend=backend)
    finally:
        raster.epsg = src_epsg
    return out.data, raster, updated


# -- polygon-on-polygon overlap areas (reference: utils/geospatial.py:221-329, gpd.overlay) ------------------------
# A6: the device's area of a pair lies within OVERLAP_BOUND_K 2^-53 area_abs of the exact one.  K = 4 x the largest ratio the numpy
# restatement of A5 reached over every pair of every scene of the tests, rounded up to a power of two (tests/overlap_standin.py
# holds the measurement and the largest ratio the device reached).
OVERLAP_BOUND_K = 32.0
GRID_STEP_AREA = 1e-12     # m^2 of one square grid step (SNAP_GRID_METERS squared)


def overlap_bound(area_abs):
    """A6: the error bound of a pair's area from its area_abs, in the same unit."""
    return OVERLAP_BOUND_K * 2.0 ** -53 * np.asarray(area_abs, dtype=np.float64)


def polygon_source(source):
    """A `.geojson` path or a (PlanarPolygons, {column: values}) pair -> (PlanarPolygons, properties): the convention of
    `get_values_for_faces_from_vector`.  A bare PlanarPolygons has no properties."""
    from geograypher_amd.utils.geometric import PlanarPolygons

    if isinstance(source, PlanarPolygons):
        return source, {}
    if isinstance(source, tuple) and len(source) == 2 and isinstance(source[0], PlanarPolygons):
        return source[0], {k: np.asarray(v) for k, v in dict(source[1]).items()}
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        if not str(source).lower().endswith((".geojson", ".json")):
            raise NotImplementedError(f"{source}: polygon files are read as .geojson only")
        return PlanarPolygons.from_geojson(source)
    raise TypeError("a polygon source is a .geojson path or a (PlanarPolygons, {column: values}) pair")


def _same_planar_CRS(a, b, what: str):
    if a.epsg is not None and b.epsg is not None and int(a.epsg) != int(b.epsg):
        raise ValueError(f"{what}: the two sources are in EPSG:{a.epsg} and EPSG:{b.epsg}; polygons are not reprojected here, "
                         "bring both into one planar CRS first")


def overlap_pairs(A, B, backend=None):
    """The candidate pairs of two `PlanarPolygons` and their overlap on the device (`HipRaster.polygon_overlap`): (pairs (n, 2) int64
    ascending by (row of A, row of B), area (n,), area_abs (n,) float64 in m^2).  The table with the longer rows goes to the lane
    side of the kernel (table b of the call) and the answer is transposed back."""
    from geograypher_amd.utils.geometric import overlap_work_items, snap_polygon_pair

    backend = backend if backend is not None else _default_backend()
    table_a, table_b, _ = snap_polygon_pair(A, B)
    mean_row = lambda t, P: len(t[0]) / max(P, 1)   # noqa: E731
    swap = mean_row(table_a, len(A)) > mean_row(table_b, len(B))
    if swap:
        table_a, table_b = table_b, table_a
    overlap = backend.polygon_overlap(table_a, table_b)
    pairs = _to_host(overlap.pairs()).astype(np.int64).reshape(-1, 2)
    items = overlap_work_items(table_a[1], table_a[2], table_b[1], table_b[2], pairs)
    area, area_abs, _stats = overlap.areas(pairs.astype(np.int32), items)
    area, area_abs = _to_host(area).astype(np.float64) * GRID_STEP_AREA, _to_host(area_abs).astype(np.float64) * GRID_STEP_AREA
    if swap:
        pairs = pairs[:, ::-1]
        order = np.lexsort((pairs[:, 1], pairs[:, 0]))
        pairs, area, area_abs = pairs[order], area[order], area_abs[order]
    return np.ascontiguousarray(pairs), area, area_abs


def polygon_overlap_areas(A, B, backend=None):
    """area(row a of A n row b of B) for every pair of rows, on the device (gr_polygon_overlap_areas; rules A1-A9 of DESIGN.md 8o)
    -> a scipy CSR matrix (n_A, n_B) in m^2.  A, B: `PlanarPolygons` in one planar CRS (a differing `.epsg` is a ValueError).  An
    entry whose area does not exceed its bound (`overlap_bound` of its area_abs: rounding alone could have produced it) is dropped,
    so rows that only touch, or lie in each other's holes, have no entry."""
    import scipy.sparse

    _same_planar_CRS(A, B, "polygon_overlap_areas")
    pairs, area, area_abs = overlap_pairs(A, B, backend)
    keep = area > overlap_bound(area_abs)
    return scipy.sparse.csr_matrix((area[keep], (pairs[keep, 0], pairs[keep, 1])), shape=(len(A), len(B)))


def get_overlap_vector(unlabeled, classes, class_column: str, normalize: bool = False, backend=None):
    """For every unlabeled polygon its overlap area with every class (reference: utils/geospatial.py:221-329, which goes through
    gpd.overlay) -> (counts_matrix (n_valid, n_classes) float64 in m^2, intersection_IDs (n_valid,) int64, unique_class_names: the
    sorted distinct values of `class_column`).

    unlabeled, classes: a `.geojson` path or a (PlanarPolygons, {column: values}) pair.  counts_matrix[k][c] is the sum of
    area(unlabeled row intersection_IDs[k] n class row) over the class rows of class c -- what the reference's overlay of the
    UNDISSOLVED class rows sums; class rows of one class that overlap each other count twice there and here.  intersection_IDs
    are the unlabeled rows with a pair area above its bound (`polygon_overlap_areas`).  `normalize` divides every row by its sum.
    Differences from the reference: its simplify(0.01) of both sources is not applied; rows that only touch do not count as
    intersecting (GEOS' intersects counts them, with rows of zeros); nothing is reprojected: both sources share one planar CRS,
    and a differing `.epsg` is a ValueError."""
    A, _ = polygon_source(unlabeled)
    B, properties = polygon_source(classes)
    if class_column not in properties:
        raise ValueError(f"Class column `{class_column}` not in {sorted(properties)}")
    _same_planar_CRS(A, B, "get_overlap_vector")
    names = np.asarray(properties[class_column]).tolist()
    if len(names) != len(B):
        raise ValueError(f"{len(B)} class rows need as many values of {class_column!r}, got {len(names)}")
    unique_class_names = sorted(set(names))
    class_of_row = np.array([unique_class_names.index(v) for v in names], dtype=np.int64)
    pairs, area, area_abs = overlap_pairs(A, B, backend)
    keep = area > overlap_bound(area_abs)
    pairs, area = pairs[keep], area[keep]
    intersection_IDs = np.unique(pairs[:, 0])
    counts_matrix = np.zeros((len(intersection_IDs), len(unique_class_names)), dtype=np.float64)
    np.add.at(counts_matrix, (np.searchsorted(intersection_IDs, pairs[:, 0]), class_of_row[pairs[:, 1]]), area)
    if normalize:
        counts_matrix = counts_matrix / np.sum(counts_matrix, axis=1, keepdims=True)
    return counts_matrix, intersection_IDs, unique_class_names


def row_areas(polygons) -> np.ndarray:
    """(P,) float64 m^2: the area of every row of a `PlanarPolygons` on the 1e-6 m grid, exteriors minus holes, from the exact
    integer shoelace sums of its snapped rings."""
    from geograypher_amd.utils.geometric import _signed_area2_exact

    bounds = polygons.bounds_snapped()
    rv, off, rp, rh, _ = polygons.snapped((0, 0) if bounds is None else bounds[0] + (bounds[1] - bounds[0]) // 2)
    twice = [0] * len(polygons)
    for r in range(len(rp)):
        a2 = _signed_area2_exact(rv[off[r]:off[r + 1]])
        twice[int(rp[r])] += -a2 if rh[r] else a2
    return np.array([t / 2 for t in twice], dtype=np.float64) * GRID_STEP_AREA
