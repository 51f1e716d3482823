"""Rules Z1-Z5 of DESIGN.md 8m in Python integers, written independently of the device code: the stand-in the device's zonal class
counts are compared with.  Exact: every comparison is between products of Python integers.

Z3 in words: shoot a ray from the cell centre along +x.  An edge a -> b is a candidate when exactly one of its ends lies strictly
above the ray (y > py), so a horizontal edge never is and a vertex on the ray belongs to one of its two edges.  A candidate
counts when its crossing with the ray lies STRICTLY right of the centre: x* > px with x* = ax + (py - ay) (bx - ax) / (by - ay),
compared without the division.  The centre belongs to the row iff an odd number of the edges of all its rings count."""
import numpy as np

HALF, ONE = 32768, 65536


def to_cell_units(rings, inverse):
    """Z1: float64, every operation rounded on its own, then rint(65536 v) -> list of lists of (qx, qy) Python integers."""
    ia, ib, ic, id_, ie, if_ = (np.float64(v) for v in inverse)
    out = []
    for ring in rings:
        q = []
        for x, y in np.asarray(ring, dtype=np.float64).reshape(-1, 2):
            col = (x * ia + y * ib) + ic
            row = (x * id_ + y * ie) + if_
            qx, qy = np.rint(np.float64(65536.0) * col), np.rint(np.float64(65536.0) * row)
            if not (abs(qx) < 2.0 ** 40 and abs(qy) < 2.0 ** 40):
                raise ValueError("vertex outside the 2^40 range")
            q.append((int(qx), int(qy)))
        out.append(q)
    return out


def centre_in_rings(px, py, rings_q):
    inside = False
    for ring in rings_q:
        n = len(ring)
        if n < 3:
            continue
        for k in range(n):
            (ax, ay), (bx, by) = ring[k], ring[(k + 1) % n]
            if (ay > py) == (by > py):
                continue
            # x* > px  <=>  (py - ay) (bx - ax) > (px - ax) (by - ay) when by > ay, the reverse when by < ay
            lhs, rhs = (py - ay) * (bx - ax), (px - ax) * (by - ay)
            if (lhs > rhs) if by > ay else (lhs < rhs):
                inside = not inside
    return inside


def zonal_counts(raster, nodata, rings_q, ring_polygon, n_polygons, num_classes):
    """raster (H, W) uint8, nodata an int or None, rings_q: a list of rings of (qx, qy) integer vertices in cell units, ring_polygon
    their rows -> (counts (P, C) int64, stats (8,) int64 as GR_ZONAL_STAT_*; word 0, the cells tested, is left 0: it depends on
    the work decomposition)."""
    raster = np.asarray(raster)
    H, W = raster.shape
    counts = np.zeros((n_polygons, num_classes), dtype=np.int64)
    stats = np.zeros(8, dtype=np.int64)
    stats[5] = max([len(r) for r in rings_q], default=0)
    stats[6] = sum(1 for r in rings_q if len(r) < 3)
    for p in range(n_polygons):
        mine = [r for r, row in zip(rings_q, ring_polygon) if row == p and len(r) >= 3]
        if not mine:
            continue
        xs = [v[0] for r in mine for v in r]
        ys = [v[1] for r in mine for v in r]
        c0, c1 = max(-((HALF - min(xs)) // ONE), 0), min((max(xs) - HALF) // ONE, W - 1)
        r0, r1 = max(-((HALF - min(ys)) // ONE), 0), min((max(ys) - HALF) // ONE, H - 1)
        for row in range(r0, r1 + 1):
            for col in range(c0, c1 + 1):
                if not centre_in_rings(ONE * col + HALF, ONE * row + HALF, mine):
                    continue
                v = int(raster[row, col])
                stats[1] += 1
                if nodata is not None and v == nodata:
                    stats[2] += 1
                    continue
                stats[4] = max(stats[4], v + 1)
                if v >= num_classes:
                    stats[3] += 1
                    continue
                counts[p, v] += 1
    return counts, stats


class StandInBackend:
    """`HipRaster.zonal_class_counts` on the host, from the same tables, through `zonal_counts`: for the host tests of the layers
    above it (get_overlap_raster, compute_confusion_matrix_from_geospatial)."""

    def zonal_class_counts(self, raster, nodata, ring_vertices, ring_offsets, ring_polygon, n_polygons, items, num_classes):
        from geograypher_amd import _hip

        raster = np.asarray(raster)
        _hip.check_zonal_tables(raster.shape[0], raster.shape[1], nodata, ring_vertices, ring_offsets, ring_polygon, n_polygons, items,
                                num_classes)
        rings = [[(int(x), int(y)) for x, y in ring_vertices[ring_offsets[r]:ring_offsets[r + 1]]] for r in range(len(ring_polygon))]
        counts, stats = zonal_counts(raster, nodata, rings, [int(p) for p in ring_polygon], n_polygons, num_classes)
        stats[0] = int((np.asarray(items)[:, 3].astype(np.int64) * np.asarray(items)[:, 4]).sum())
        return counts, stats
