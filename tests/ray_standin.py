"""numpy stand-in for the two device calls of the multiview-detection workflow (gr_ray_pairs, gr_rays_clip), written for the
tests: a per-pair restatement of the clamped segment distance and a brute-force Moller-Trumbore, generic in the float type
(float64, or np.longdouble to measure float64's own error).  tests/test_triangulation_host.py pins it to the reference's
`dist` arrays in tests/golden/reference_triangulation.npz; the GPU tests then use it where no golden exists.

Keep this copy: geograypher_amd/utils/numeric.py has a host form of the same mathematics (`segment_closest_points`), and this
module must not be "simplified" to import it -- the tests would then compare the package with itself wherever no golden exists.
Both are pinned to the reference's goldens separately."""
import numpy as np


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _clip0(x, hi):
    return np.minimum(np.maximum(x, 0), hi)


def pair_distance(starts, ends, i, j, dtype=np.float64):
    """Clamped distance between segments i[k] and j[k] for every k: (K,) of `dtype`."""
    s, e = np.asarray(starts, dtype=dtype), np.asarray(ends, dtype=dtype)
    with np.errstate(all="ignore"):
        seg = e - s
        mag = np.sqrt((seg[:, 0] * seg[:, 0] + seg[:, 1] * seg[:, 1]) + seg[:, 2] * seg[:, 2])
        unit = seg / mag[:, None]
        a0, a1, uA, mA = s[i], e[i], unit[i], mag[i]
        b0, b1, uB, mB = s[j], e[j], unit[j], mag[j]
        n = _cross(uA, uB)
        cn = np.sqrt(_dot(n, n))
        denom = cn * cn
        par = denom == 0
        denom = np.where(par, dtype(1), denom)
        t = b0 - a0
        t0 = _dot(_cross(t, uB), n) / denom
        t1 = _dot(_cross(t, uA), n) / denom
        pA = a0 + _clip0(t0, mA)[:, None] * uA
        pB = b0 + _clip0(t1, mB)[:, None] * uB
        oobA = (t0 < 0) | (t0 > mA)
        oobB = (t1 < 0) | (t1 > mB)
        pB = np.where(oobA[:, None], b0 + _clip0(_dot(pA - b0, uB), mB)[:, None] * uB, pB)
        pA = np.where(oobB[:, None], a0 + _clip0(_dot(pB - a0, uA), mA)[:, None] * uA, pA)
        # exactly parallel
        base = _dot(uA, a0)
        d0 = _dot(uA, b0) - base
        d1 = _dot(uA, b1) - base
        before = (d0 <= 0) & (d1 <= 0)
        after = (d0 >= mA) & (d1 >= mA)
        near = np.where((np.abs(d0) < np.abs(d1))[:, None], b0, b1)
        midA = a0 + _clip0(d0, mA)[:, None] * uA
        g = b0 - midA
        midB = midA + (g - _dot(g, uA)[:, None] * uA)
        qA = np.where(after[:, None], a1, np.where(before[:, None], a0, midA))
        qB = np.where((before | after)[:, None], near, midB)
        pA = np.where(par[:, None], qA, pA)
        pB = np.where(par[:, None], qB, pB)
        d = pA - pB
        return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def all_pairs_distance(starts, ends, dtype=np.float64):
    """(N, N) clamped distances, rows = A."""
    n = len(starts)
    i, j = np.divmod(np.arange(n * n), n)
    return pair_distance(starts, ends, i, j, dtype).reshape(n, n)


def rows_distance(starts, ends, rows, dtype=np.float64):
    """(len(rows), N) distances of the given rows against every ray."""
    n = len(starts)
    i = np.repeat(np.asarray(rows), n)
    j = np.tile(np.arange(n), len(rows))
    return pair_distance(starts, ends, i, j, dtype).reshape(len(rows), n)


def ray_pair_edges_np(starts, ends, ray_ids, threshold, block=512):
    """(i, j, d) sorted by (i, j): what gr_ray_pairs returns."""
    starts, ends, ids = np.asarray(starts, np.float64), np.asarray(ends, np.float64), np.asarray(ray_ids)
    n = len(starts)
    out_i, out_j, out_d = [], [], []
    for r0 in range(0, n, block):
        rows = np.arange(r0, min(r0 + block, n))
        d = rows_distance(starts, ends, rows)
        cols = np.arange(n)
        with np.errstate(invalid="ignore"):
            keep = (rows[:, None] < cols[None, :]) & (ids[rows][:, None] != ids[None, :]) & (d <= threshold)
        ii, jj = np.nonzero(keep)
        out_i.append(rows[ii]); out_j.append(jj); out_d.append(d[ii, jj])
    if not out_i:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
    return np.concatenate(out_i).astype(np.int32), np.concatenate(out_j).astype(np.int32), np.concatenate(out_d)


def clip_rays_np(origins, directions, points, faces, dtype=np.float64):
    """Nearest double-sided hit with t >= 0 (first face wins a tie): hit (N,) bool, t (N,), points (N, 3), and the barycentric
    margin min(u, v, 1 - u - v) of the winning hit (how far from the triangle's edges it is)."""
    o, d = np.asarray(origins, dtype=dtype), np.asarray(directions, dtype=dtype)
    p, f = np.asarray(points, dtype=dtype), np.asarray(faces)
    n = len(o)
    best = np.full(n, np.inf, dtype=dtype)
    margin = np.full(n, np.nan, dtype=dtype)
    hit = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(len(f)):
            v0, v1, v2 = p[f[k, 0]], p[f[k, 1]], p[f[k, 2]]
            e1, e2 = (v1 - v0)[None, :], (v2 - v0)[None, :]
            pv = _cross(d, e2)
            det = _dot(e1, pv)
            inv = 1 / det
            s = o - v0[None, :]
            u = _dot(s, pv) * inv
            q = _cross(s, e1)
            v = _dot(d, q) * inv
            t = _dot(e2, q) * inv
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t < best)
            best = np.where(ok, t, best)
            margin = np.where(ok, np.minimum(np.minimum(u, v), 1 - (u + v)), margin)
            hit |= ok
        t_out = np.where(hit, best, np.nan)
        pts = np.where(hit[:, None], o + best[:, None] * d, np.nan)
    return hit, t_out, pts, margin


class StandInBackend:
    """The two device calls of HipRaster, on the host."""

    def ray_pair_edges(self, starts, ends, ray_ids, threshold):
        return ray_pair_edges_np(starts, ends, ray_ids, threshold)

    def clip_rays(self, origins, directions, points, faces):
        hit, t, pts, _ = clip_rays_np(origins, directions, points, faces)
        return hit, t, pts
