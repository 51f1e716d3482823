"""A georeferenced raster in one planar CRS, as the raster-sample call takes it (DESIGN.md "Raster samples", T1-T2).

`PlanarRaster` holds the bands, the affine transform in the order of rasterio's `Affine` and the nodata value; `inverse` is the
inverse transform in Python floats, in the order of operations of the `affine` package.  `from_geotiff` reads single-band GeoTIFFs
with PIL (there is no rasterio / GDAL here): the transform from the ModelPixelScale + ModelTiepoint or ModelTransformation tags,
the PixelIsPoint half-pixel shift from the GeoKeyDirectory, the nodata value from GDAL_NODATA.  The EPSG code of the file's CRS
is recorded as `.epsg` (ProjectedCSTypeGeoKey, else GeographicTypeGeoKey, else None) and nothing consults it: the caller supplies
the query points in the raster's CRS, or names that CRS (`points_in_raster_CRS=dtm.epsg`)."""
import math
from pathlib import Path

import numpy as np

TAG_MODEL_PIXEL_SCALE = 33550
TAG_MODEL_TIEPOINT = 33922
TAG_MODEL_TRANSFORMATION = 34264
TAG_GEO_KEY_DIRECTORY = 34735
TAG_GDAL_NODATA = 42113
GEO_KEY_RASTER_TYPE = 1025
GEO_KEY_GEOGRAPHIC_TYPE = 2048
GEO_KEY_PROJECTED_CS_TYPE = 3072
GEO_KEY_USER_DEFINED = 32767
RASTER_PIXEL_IS_POINT = 2
GEOTIFF_MODES = ("F", "I", "I;16", "L")


def invert_affine(transform):
    """(ia, ib, ic, id, ie, if) of the inverse of (a, b, c, d, e, f) (rule T2: Python floats, the `affine` package's order)."""
    a, b, c, d, e, f = (float(v) for v in transform)
    det = a * e - b * d
    if det == 0.0 or not math.isfinite(det):
        raise ValueError(f"the raster transform {(a, b, c, d, e, f)} cannot be inverted (determinant {det})")
    idet = 1.0 / det
    ia = e * idet
    ib = -b * idet
    id_ = -d * idet
    ie = a * idet
    return (ia, ib, -c * ia - f * ib, id_, ie, -c * id_ - f * ie)


class PlanarRaster:
    """data (B, H, W) (a 2-D array is one band), transform (a, b, c, d, e, f): x = a col + b row + c, y = d col + e row + f,
    nodata a float or None.  float32 and float64 data stay what they are; any other dtype becomes float64 (exact for uint8,
    uint16, int16 and int32)."""

    def __init__(self, data, transform, nodata=None, epsg=None):
        data = np.asarray(data)
        if data.ndim == 2:
            data = data[None]
        if data.ndim != 3 or min(data.shape) < 1:
            raise ValueError(f"raster data must be (B, H, W) or (H, W) with no empty axis, got {data.shape}")
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        self.data = np.ascontiguousarray(data)
        transform = tuple(float(v) for v in np.asarray(transform, dtype=np.float64).reshape(-1))
        if len(transform) != 6:
            raise ValueError(f"the transform has six coefficients (a, b, c, d, e, f), got {len(transform)}")
        self.transform = transform
        self.inverse = invert_affine(transform)
        self.nodata = None if nodata is None else float(nodata)
        self.epsg = None if epsg is None else int(epsg)   # read only: the CRS the file names, if it names one

    @property
    def shape(self):
        return self.data.shape

    @classmethod
    def from_array(cls, data, transform, nodata=None):
        return cls(data, transform, nodata)

    def warped(self, like=None, **kwargs):
        """This raster on another grid, in the same or in another WGS84 CRS: `utils.geospatial.warp_raster(self, like, ...)`, which
        documents the keywords (resolution, dst_crs, src_crs, resampling, dst_nodata, backend, max_device_bytes, return_tensor)."""
        from geograypher_amd.utils.geospatial import warp_raster

        return warp_raster(self, like, **kwargs)

    @classmethod
    def from_geotiff(cls, path):
        """A single-band GeoTIFF of mode F (float32), I (int32), I;16 (uint16) or L (uint8); strips or tiles, deflate / LZW as
        PIL's libtiff reads them.  ValueError for a file without georeferencing tags, or with several tiepoints and no scale."""
        from PIL import Image

        with Image.open(Path(path)) as image:
            if image.mode not in GEOTIFF_MODES:
                raise ValueError(f"{path}: image mode {image.mode!r} is not one of {GEOTIFF_MODES} (float64 and multi-band "
                                 "rasters go through PlanarRaster.from_array)")
            tags = image.tag_v2 if hasattr(image, "tag_v2") else {}
            transform, nodata, epsg = georeference_from_tags(path, tags)
            data = np.array(image)
        raster = cls(data, transform, nodata)
        raster.epsg = epsg
        return raster


def georeference_from_tags(path, tags):
    """(transform (a, b, c, d, e, f), nodata or None, epsg or None) from the TIFF tags of a GeoTIFF: no pixel is decoded.
    ValueError for a file without georeferencing tags, or with several tiepoints and no scale."""
    scale = tags.get(TAG_MODEL_PIXEL_SCALE)
    tie = tags.get(TAG_MODEL_TIEPOINT)
    matrix = tags.get(TAG_MODEL_TRANSFORMATION)
    keys = tags.get(TAG_GEO_KEY_DIRECTORY)
    nodata = tags.get(TAG_GDAL_NODATA)
    if scale is not None and tie is not None:
        if len(tie) != 6:
            raise ValueError(f"{path}: {len(tie) // 6} tiepoints beside a pixel scale: one is expected")
        sx, sy = float(scale[0]), float(scale[1])
        i, j, _k, X, Y, _Z = (float(v) for v in tie)
        transform = [sx, 0.0, X - i * sx, 0.0, -sy, Y + j * sy]
    elif matrix is not None:
        if len(matrix) != 16:
            raise ValueError(f"{path}: ModelTransformation has {len(matrix)} values, not 16")
        transform = [float(matrix[k]) for k in (0, 1, 3, 4, 5, 7)]
    elif tie is not None:
        raise ValueError(f"{path}: tiepoints without a pixel scale (a warp through several tiepoints is not supported)")
    else:
        raise ValueError(f"{path}: no georeferencing (ModelPixelScale + ModelTiepoint or ModelTransformation)")
    if keys is not None and _geo_key(keys, GEO_KEY_RASTER_TYPE) == RASTER_PIXEL_IS_POINT:
        a, b, c, d, e, f = transform   # the tags place the CENTRE of pixel (0, 0): its corner lies half a pixel before
        transform = [a, b, c - (0.5 * a + 0.5 * b), d, e, f - (0.5 * d + 0.5 * e)]
    if nodata is not None:
        if isinstance(nodata, bytes):
            nodata = nodata.decode("ascii", "replace")
        if isinstance(nodata, (tuple, list)):
            nodata = nodata[0]
        nodata = float(str(nodata).strip().rstrip("\x00").strip())
    epsg = None
    if keys is not None:
        for key in (GEO_KEY_PROJECTED_CS_TYPE, GEO_KEY_GEOGRAPHIC_TYPE):
            code = _geo_key(keys, key)
            if code is not None and 0 < code < GEO_KEY_USER_DEFINED:
                epsg = code
                break
    return transform, nodata, epsg


def read_geotiff_header(path):
    """(transform, nodata, epsg, height, width) of a GeoTIFF of ANY band count and sample type -- an RGB(A) orthomosaic, which
    `PlanarRaster.from_geotiff` refuses, included: only the tags are read."""
    from PIL import Image

    limit, Image.MAX_IMAGE_PIXELS = Image.MAX_IMAGE_PIXELS, None   # an orthomosaic is large; nothing is decoded here
    try:
        with Image.open(Path(path)) as image:
            tags = image.tag_v2 if hasattr(image, "tag_v2") else {}
            transform, nodata, epsg = georeference_from_tags(path, tags)
            width, height = image.size
    finally:
        Image.MAX_IMAGE_PIXELS = limit
    return tuple(transform), nodata, epsg, int(height), int(width)


def _geo_key(directory, key):
    """The SHORT value of `key` stored in a GeoKeyDirectory itself (TIFFTagLocation 0), or None."""
    directory = [int(v) for v in directory]
    for k in range(4, min(len(directory), 4 + 4 * directory[3]) - 3, 4):
        if directory[k] == key and directory[k + 1] == 0:
            return directory[k + 3]
    return None
