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
def rings_to_cell_units(rings, inverse):
    """Rule Z1: ring vertices (x, y) in the raster's CRS -> int64 pixel coordinates times 65536, with the raster's `inverse`
    (ia, ib, ic, id, ie, if) in float64, every operation rounded on its own in the order of rule T2: col = (ia x + ib y) + ic,
    row = (id x + ie y) + if, q = rint(65536 value).  rings: a list of (n, 2) arrays -> (ring_vertices (N, 2) int64, ring_offsets
    (R + 1,) int64).  ValueError for a value that is not finite or has |q| >= 2^40."""
    ia, ib, ic, id_, ie, if_ = (np.float64(v) for v in inverse)
    verts, offsets = [], [0]
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
        x, y = ring[:, 0], ring[:, 1]
        col = (x * ia + y * ib) + ic
        row = (x * id_ + y * ie) + if_
        q = np.rint(np.stack([col, row], axis=1) * 65536.0)
        if q.size and not np.all(np.abs(q) < 2.0 ** 40):
            raise ValueError("a polygon vertex is not finite or lies 2^40 / 65536 cells or more from the raster's corner")
        verts.append(q.astype(np.int64))
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
