"""numpy stand-in for the two device calls behind the covering meshes (gr_points_bounds, gr_cover_grid), written from the rule
of DESIGN.md "Covering meshes": a visited row belongs to grid point (xi, yi) iff x_lo[xi] <= x <= x_hi[xi] and
y_lo[yi] <= y <= y_hi[yi], both ends included, in float64; per grid point the largest and the smallest member z and the number of
members.  Membership is the two comparisons against EVERY column of the tables and nothing else: no arithmetic finds a cell
here, so an axis of zero extent, cells that share, overlap or miss each other by an ulp and points that belong to one, two or
four cells all fall out of the same lines.  Rows with a NaN or infinite coordinate are counted by `points_bounds_np` and take
part in nothing.

`tests/test_covering_meshes_host.py` pins it to cases worked by hand; the GPU tests then hold the device to it bit for bit."""
import numpy as np


def _visited(points, stride):
    p = np.asarray(points, dtype=np.float64)[:: int(stride)]
    return p, np.isfinite(p).all(axis=1)


def points_bounds_np(points, stride=1):
    """(bounds (6,) float64 xmin xmax ymin ymax zmin zmax over the visited finite rows -- +inf / -inf without any --, the number
    of visited rows that are not finite)."""
    p, ok = _visited(points, stride)
    q = p[ok]
    bounds = np.array([np.inf, -np.inf] * 3)
    if len(q):
        bounds = np.array([q[:, 0].min(), q[:, 0].max(), q[:, 1].min(), q[:, 1].max(), q[:, 2].min(), q[:, 2].max()])
    return bounds, int((~ok).sum())


def cover_grid_np(points, x_lo, x_hi, y_lo, y_hi, stride=1):
    """(z_max (N, N), z_min (N, N), count (N, N) int64), indexed [xi, yi]; NaN where count is 0."""
    p, ok = _visited(points, stride)
    x, y, z = p[ok, 0], p[ok, 1], p[ok, 2]
    x_lo, x_hi, y_lo, y_hi = (np.asarray(t, dtype=np.float64) for t in (x_lo, x_hi, y_lo, y_hi))
    N = len(x_lo)
    in_row = (y_lo[None, :] <= y[:, None]) & (y[:, None] <= y_hi[None, :])     # (points, yi)
    z_max, z_min = np.full((N, N), np.nan), np.full((N, N), np.nan)
    count = np.zeros((N, N), dtype=np.int64)
    for xi in range(N):
        in_col = (x_lo[xi] <= x) & (x <= x_hi[xi])
        if not in_col.any():
            continue
        member = in_row[in_col]                                                # (points of this column, yi)
        zc = z[in_col][:, None]
        count[xi] = member.sum(axis=0)
        have = count[xi] > 0
        z_max[xi, have] = np.where(member, zc, -np.inf).max(axis=0)[have]
        z_min[xi, have] = np.where(member, zc, np.inf).min(axis=0)[have]
    return z_max, z_min, count


def bound_tables(bounds, N):
    """The four tables as the reference forms its operands: np.linspace over the extent, minus / plus half a grid step."""
    x_min, x_max, y_min, y_max = (np.float64(v) for v in bounds[:4])
    x_grid, y_grid = np.linspace(x_min, x_max, N), np.linspace(y_min, y_max, N)
    hx, hy = (x_max - x_min) / (N - 1) / 2, (y_max - y_min) / (N - 1) / 2
    return x_grid - hx, x_grid + hx, y_grid - hy, y_grid + hy


class CoverStandIn:
    """The two covering-mesh calls of HipRaster, on the host."""

    def points_bounds(self, points, stride=1):
        bounds, bad = points_bounds_np(points, stride)
        return bounds, np.array([bad], dtype=np.int64)

    def cover_grid(self, points, x_lo, x_hi, y_lo, y_hi, stride=1):
        return cover_grid_np(points, x_lo, x_hi, y_lo, y_hi, stride)
