"""Minimal baseline-TIFF writer with deflate compression for the `save_renders` writer pool (row f2).

The reference saves every render with `PIL.Image.save(..., compression="tiff_deflate")` (meshes.py:2390-2397).  PIL's TIFF
encoder holds the interpreter lock while it compresses: eight writer threads produce exactly as many files per second as
one (4.2 views/s at 4000 x 3000).  `zlib.compress` releases the lock, so this writer -- TIFF 6.0, little endian,
Compression = 8 (Adobe deflate, what PIL writes for "tiff_deflate"), strips of about 1 MiB, chunky planar configuration,
unsigned samples -- scales with the threads.  Any TIFF reader (PIL, skimage.io, tifffile, GDAL) reads the files."""
import struct
import zlib
from pathlib import Path

import numpy as np

_TYPES = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(np.uint32): 32, np.dtype(np.float32): 32}


def write_tiff_deflate(path, array: np.ndarray, level: int = 6, strip_bytes: int = 1 << 20, transform=None, nodata=None,
                       epsg=None) -> None:
    """(H, W) or (H, W, C) uint8 / uint16 / uint32 / float32 array -> deflate-compressed TIFF at `path` (SampleFormat 1, unsigned
    integer, or 3, IEEE floating point: a height raster).

    Optional georeferencing makes it a GeoTIFF that `PlanarRaster.from_geotiff` and GDAL read: transform (a, b, c, d, e, f) with
    x = a col + b row + c, y = d col + e row + f of pixel CORNERS -- ModelPixelScale + ModelTiepoint when b = d = 0 and a > 0 > e,
    the 16-value ModelTransformation otherwise --, nodata (GDAL_NODATA, ASCII) and epsg (a GeoKeyDirectory with PixelIsArea and
    the code as ProjectedCSTypeGeoKey, or GeographicTypeGeoKey for the codes 4000-4999)."""
    a = np.ascontiguousarray(array)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.dtype not in _TYPES or a.shape[2] not in (1, 3):
        raise ValueError(f"unsupported image for the TIFF writer: shape {array.shape}, dtype {array.dtype}")
    a = a.astype(a.dtype.newbyteorder("<"), copy=False)
    h, w, c = a.shape
    bits = _TYPES[np.dtype(array.dtype)]
    sample_format = 3 if a.dtype.kind == "f" else 1               # IEEE floating point / unsigned integer
    row_bytes = w * c * (bits // 8)
    rows_per_strip = max(1, min(h, strip_bytes // max(row_bytes, 1)))
    strips = [zlib.compress(a[r0 : r0 + rows_per_strip].tobytes(), level) for r0 in range(0, h, rows_per_strip)]
    n = len(strips)
    offsets, pos = [], 8
    for s in strips:
        offsets.append(pos)
        pos += len(s) + (len(s) & 1)  # word alignment
    extra = bytearray()  # out-of-line arrays, placed behind the strips
    extra_base = pos

    def out_of_line(fmt, values):
        off = extra_base + len(extra)
        extra.extend(struct.pack("<" + fmt * len(values), *values))
        if len(extra) & 1:
            extra.append(0)
        return off

    def entry(tag, typ, count, value):
        return struct.pack("<HHII", tag, typ, count, value)

    SHORT, LONG = 3, 4
    tags = [entry(256, LONG, 1, w), entry(257, LONG, 1, h)]
    if c == 1:
        tags.append(entry(258, SHORT, 1, bits))
    elif c == 2:
        tags.append(struct.pack("<HHIHH", 258, SHORT, 2, bits, bits))
    else:
        tags.append(entry(258, SHORT, c, out_of_line("H", [bits] * c)))
    tags.append(entry(259, SHORT, 1, 8))                          # Compression: Adobe deflate
    tags.append(entry(262, SHORT, 1, 2 if c == 3 else 1))         # Photometric: RGB / BlackIsZero
    tags.append(entry(273, LONG, n, offsets[0] if n == 1 else out_of_line("I", offsets)))
    tags.append(entry(277, SHORT, 1, c))
    tags.append(entry(278, LONG, 1, rows_per_strip))
    counts = [len(s) for s in strips]
    tags.append(entry(279, LONG, n, counts[0] if n == 1 else out_of_line("I", counts)))
    tags.append(entry(284, SHORT, 1, 1))                          # PlanarConfiguration: chunky
    if c == 1:
        tags.append(entry(339, SHORT, 1, sample_format))          # SampleFormat
    elif c == 2:
        tags.append(struct.pack("<HHIHH", 339, SHORT, 2, sample_format, sample_format))
    else:
        tags.append(entry(339, SHORT, c, out_of_line("H", [sample_format] * c)))
    DOUBLE, ASCII = 12, 2
    if transform is not None:
        ta, tb, tc, td, te, tf = (float(v) for v in transform)
        if tb == 0.0 and td == 0.0 and ta > 0.0 and te < 0.0:
            tags.append(entry(33550, DOUBLE, 3, out_of_line("d", [ta, -te, 0.0])))                    # ModelPixelScale
            tags.append(entry(33922, DOUBLE, 6, out_of_line("d", [0.0, 0.0, 0.0, tc, tf, 0.0])))      # ModelTiepoint
        else:
            matrix = [ta, tb, 0.0, tc, td, te, 0.0, tf, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
            tags.append(entry(34264, DOUBLE, 16, out_of_line("d", matrix)))                           # ModelTransformation
    if transform is not None or epsg is not None:
        keys = [(1025, 0, 1, 1)]                                                                      # GTRasterType: PixelIsArea
        if epsg is not None:
            geographic = 4000 <= int(epsg) <= 4999
            keys = [(1024, 0, 1, 2 if geographic else 1)] + keys + [(2048 if geographic else 3072, 0, 1, int(epsg))]
        directory = [1, 1, 0, len(keys)] + [v for key in keys for v in key]
        tags.append(entry(34735, SHORT, len(directory), out_of_line("H", directory)))                 # GeoKeyDirectory
    if nodata is not None:
        text = (repr(int(nodata)) if float(nodata) == int(nodata) else repr(float(nodata))).encode("ascii") + b"\0"
        if len(text) <= 4:
            tags.append(struct.pack("<HHI4s", 42113, ASCII, len(text), text.ljust(4, b"\0")))         # GDAL_NODATA, in line
        else:
            tags.append(entry(42113, ASCII, len(text), out_of_line("B", list(text))))
    tags.sort(key=lambda e: struct.unpack("<H", e[:2])[0])
    ifd_offset = extra_base + len(extra)
    with open(Path(path), "wb") as f:
        f.write(struct.pack("<2sHI", b"II", 42, ifd_offset))
        for s in strips:
            f.write(s)
            if len(s) & 1:
                f.write(b"\0")
        f.write(bytes(extra))
        f.write(struct.pack("<H", len(tags)))
        for e in tags:
            f.write(e)
        f.write(struct.pack("<I", 0))
