"""numpy float64 stand-in of the CRS reprojection stage (DESIGN.md "CRS reprojection", rules G1-G9): the operations of
csrc/crs.hip in the same order, each rounded on its own.  numpy's sin, atan2, atanh ... and the device library's are not the same
functions to the last bit, so the two agree within the tolerance of G9, not bit for bit.  `CrsStandinBackend` offers the
`reproject_points` of `HipRaster` for the host tests.

Kinds and the parameter tuple of a CRS: (kind, lon0 degrees, k0, false easting, false northing); the last four are read for
TM only."""
import numpy as np

ECEF, GEOGRAPHIC, TM = 0, 1, 2

A_WGS84 = 6378137.0
F_WGS84 = 1.0 / 298.257223563
E2 = F_WGS84 * (2.0 - F_WGS84)
ECC = np.sqrt(E2)
B_WGS84 = A_WGS84 * (1.0 - F_WGS84)
EP2B = E2 / (1.0 - E2) * B_WGS84     # e'^2 b
E2A = E2 * A_WGS84
ONE_F = 1.0 - F_WGS84
ONE_E2 = 1.0 - E2
DEG = np.pi / 180.0
RAD = 180.0 / np.pi
POLE_R = 2.0 ** -51

# the header's 13 doubles (read, not typed: the header is what the kernel compiles)
import re as _re
from pathlib import Path as _Path

_text = (_Path(__file__).resolve().parents[1] / "geograypher_amd" / "csrc" / "crs_constants.hpp").read_text()
RECT_RADIUS = float(_re.search(r"#define GR_CRS_RECT_RADIUS (\S+)", _text).group(1))
ALPHA = [float(v) for v in _re.search(r"#define GR_CRS_ALPHA \{(.*?)\}", _text).group(1).split(",")]
BETA = [float(v) for v in _re.search(r"#define GR_CRS_BETA \{(.*?)\}", _text).group(1).split(",")]

OK, NONFINITE, BEYOND, BAD_FACE = 0, 1, 2, 3


def _wrap(d):
    """G6: an angle in radians into (-pi, pi]."""
    d = d - (2.0 * np.pi) * np.floor((d + np.pi) / (2.0 * np.pi))
    return np.where(d <= -np.pi, d + 2.0 * np.pi, np.where(d > np.pi, d - 2.0 * np.pi, d))


def _clenshaw(coef, sign, x, y):
    """G5: sum_j sign coef_j sin(2 j (x + i y)) in real arithmetic -> (real, imaginary)."""
    s0, c0 = np.sin(2.0 * x), np.cos(2.0 * x)
    sh0, ch0 = np.sinh(2.0 * y), np.cosh(2.0 * y)
    ar, ai = 2.0 * (c0 * ch0), -2.0 * (s0 * sh0)
    y1r = np.zeros_like(x); y1i = np.zeros_like(x); y2r = np.zeros_like(x); y2i = np.zeros_like(x)
    for j in range(5, -1, -1):
        tr = ((ar * y1r - ai * y1i) - y2r) + sign * coef[j]
        ti = (ar * y1i + ai * y1r) - y2i
        y2r, y2i, y1r, y1i = y1r, y1i, tr, ti
    zr, zi = s0 * ch0, c0 * sh0
    return zr * y1r - zi * y1i, zr * y1i + zi * y1r


def _taup(tau):
    """tan of the conformal latitude from tan of the geodetic one."""
    tau1 = np.sqrt(1.0 + tau * tau)
    sig = np.sinh(ECC * np.arctanh(ECC * (tau / tau1)))
    return tau * np.sqrt(1.0 + sig * sig) - sig * tau1


def ecef_to_geo(X, Y, Z):
    """G3 -> (phi, lam, h, status)."""
    with np.errstate(all="ignore"):
        p = np.sqrt(X * X + Y * Y)
        bad = ~(np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)) | ((p == 0.0) & (Z == 0.0))
        u, v = Z * A_WGS84, p * B_WGS84
        r = np.sqrt(u * u + v * v)
        sb, cb = u / r, v / r
        for _ in range(3):
            s = Z + EP2B * ((sb * sb) * sb)
            c = p - E2A * ((cb * cb) * cb)
            u, v = ONE_F * s, c
            r = np.sqrt(u * u + v * v)
            sb, cb = u / r, v / r
        r = np.sqrt(s * s + c * c)
        sp, cp = s / r, c / r
        phi = np.arctan2(s, c)
        lam = np.where(p == 0.0, 0.0, np.arctan2(Y, X))
        h = (p * cp + Z * sp) - A_WGS84 * np.sqrt(1.0 - E2 * (sp * sp))
    return phi, lam, h, np.where(bad, NONFINITE, OK)


def geo_to_ecef(phi, lam, h):
    """G4"""
    with np.errstate(all="ignore"):
        sp, cp, sl, cl = np.sin(phi), np.cos(phi), np.sin(lam), np.cos(lam)
        n = A_WGS84 / np.sqrt(1.0 - E2 * (sp * sp))
        q = (n + h) * cp
        return q * cl, q * sl, (n * ONE_E2 + h) * sp


def geo_to_tm(phi, lam, h, crs):
    """G5, G6 -> (E, N, h, status)"""
    _, lon0, k0, fe, fn = crs
    with np.errstate(all="ignore"):
        d = _wrap(lam - lon0 * DEG)
        beyond = ~(np.abs(d) < np.pi / 2.0)
        taup = _taup(np.tan(phi))
        cd = np.cos(d)
        xi = np.arctan2(taup, cd)
        eta = np.arcsinh(np.sin(d) / np.sqrt(taup * taup + cd * cd))
        dr, di = _clenshaw(ALPHA, 1.0, xi, eta)
        ka = k0 * RECT_RADIUS
        return fe + ka * (eta + di), fn + ka * (xi + dr), h, np.where(beyond, BEYOND, OK)


def tm_to_geo(E, N, h, crs):
    """G7 -> (phi, lam, h, status)"""
    _, lon0, k0, fe, fn = crs
    with np.errstate(all="ignore"):
        ka = k0 * RECT_RADIUS
        xi, eta = (N - fn) / ka, (E - fe) / ka
        dr, di = _clenshaw(BETA, -1.0, xi, eta)
        xip, etap = xi + dr, eta + di
        sh, cx, sx = np.sinh(etap), np.cos(xip), np.sin(xip)
        r = np.sqrt(sh * sh + cx * cx)
        pole = r <= POLE_R
        beyond = ~pole & ~(cx > 0.0)
        taup = sx / r
        tau = taup / ONE_E2
        for _ in range(3):
            tau1 = np.sqrt(1.0 + tau * tau)
            sig = np.sinh(ECC * np.arctanh(ECC * (tau / tau1)))
            ti = tau * np.sqrt(1.0 + sig * sig) - sig * tau1
            tau = tau + ((taup - ti) / np.sqrt(1.0 + ti * ti)) * ((1.0 + ONE_E2 * (tau * tau)) / (ONE_E2 * tau1))
        phi = np.where(pole, np.where(sx < 0.0, -np.pi / 2.0, np.pi / 2.0), np.arctan(tau))
        lam = _wrap(lon0 * DEG + np.where(pole, 0.0, np.arctan2(sh, cx)))
    return phi, lam, h, np.where(beyond, BEYOND, OK)


def reproject(points, from_crs, to_crs, pre=None):
    """(P, 3) float64 -> ((P, 3), status (P,)): G1-G8 for one row each.  Geographic rows are (lon, lat, h) in degrees."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
    with np.errstate(all="ignore"):
        if pre is not None:
            m = np.asarray(pre, dtype=np.float64).reshape(4, 4)
            x, y, z = (((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3))
        status = np.where(np.isfinite(x) & np.isfinite(y) & np.isfinite(z), OK, NONFINITE)
        kind = from_crs[0]
        if kind == ECEF:
            phi, lam, h, st = ecef_to_geo(x, y, z)
        elif kind == GEOGRAPHIC:
            st = np.where(np.abs(y) <= 90.0, OK, NONFINITE)
            phi, lam, h = y * DEG, x * DEG, z
        else:
            phi, lam, h, st = tm_to_geo(x, y, z, from_crs)
        status = np.where(status == OK, st, status)
        kind = to_crs[0]
        if kind == ECEF:
            ox, oy, oz = geo_to_ecef(phi, lam, h)
        elif kind == GEOGRAPHIC:
            ox, oy, oz = _wrap(lam) * RAD, phi * RAD, h
        else:
            ox, oy, oz, st = geo_to_tm(phi, lam, h, to_crs)
            status = np.where(status == OK, st, status)
    out = np.stack([ox, oy, oz], axis=1)
    out[status != OK] = np.nan
    return out, status


def reproject_faces(points, faces, from_crs, to_crs, pre=None):
    """G8: one row per face, ((p0 + p1) + p2) / 3 of its reprojected vertices; a face naming a missing vertex is NaN, BAD_FACE."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    V = pts.shape[0]
    good = ((faces >= 0) & (faces < V)).all(axis=1)
    out = np.full((faces.shape[0], 3), np.nan)
    status = np.full(faces.shape[0], BAD_FACE)
    if good.any():
        rp, st = reproject(pts, from_crs, to_crs, pre)
        f = faces[good]
        with np.errstate(all="ignore"):
            out[good] = ((rp[f[:, 0]] + rp[f[:, 1]]) + rp[f[:, 2]]) / 3.0
        s3 = st[f]
        status[good] = np.where((s3 == NONFINITE).any(axis=1), NONFINITE, np.where((s3 == BEYOND).any(axis=1), BEYOND, OK))
        out[status != OK] = np.nan
    return out, status


def stats_of(status):
    return np.array([(status == NONFINITE).sum(), (status == BEYOND).sum(), (status == BAD_FACE).sum(), 0], dtype=np.int64)


class CrsStandinBackend:
    """The `reproject_points` of `HipRaster`, on the host: (points, from, to, faces, pre_transform, out) -> (array, stats)."""

    def reproject_points(self, points, from_crs, to_crs, faces=None, pre_transform=None, out=None, check=True):
        from geograypher_amd.utils.geospatial import crs_tuple

        f, t = crs_tuple(from_crs), crs_tuple(to_crs)
        if pre_transform is not None and f[0] != ECEF:
            raise ValueError("pre_transform needs an ECEF source")
        if faces is None:
            res, st = reproject(points, f, t, pre_transform)
        else:
            res, st = reproject_faces(points, faces, f, t, pre_transform)
        if out is not None:
            out[...] = res
            res = out
        return res, stats_of(st)


# -- what the host and the device tests share: the golden file and the error measure of G9 -------------------------------------------
KIND_NAMES = ("ecef", "geo", "tm")
PAIRS = [(s, d) for s in KIND_NAMES for d in KIND_NAMES if s != d]
DEVICE_CAP_M = 5e-7   # half of the 1e-6 m snapping grid


def load_golden():
    path = _Path(__file__).resolve().parent / "golden" / "crs_wgs84.npz"
    with np.load(path, allow_pickle=False) as d:
        g = {k: d[k] for k in d.files}
    for v in g.values():
        v.setflags(write=False)
    return g


def golden_crs(g, kind: str, group: int):
    return (KIND_NAMES.index(kind), *(float(v) for v in g["tm_params"][group]))


def bounds(g, factor: float):
    """(planar / ECEF, h, lon / lat as radians x a) in metres: `factor` x what the golden script measured of this stand-in,
    never above DEVICE_CAP_M."""
    return np.minimum(np.asarray(g["standin_err_m"], dtype=np.float64) * factor, DEVICE_CAP_M)


def worst_errors(got, want, dst: str, from_ecef: bool = False):
    """The largest errors of unflagged rows, in the three classes of `bounds`.  Longitudes are compared around the circle; at a
    pole the longitude means nothing, except that an ECEF point on the axis has longitude 0 exactly (G3)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rows = ~np.isnan(want).any(axis=1)
    got, want = got[rows], want[rows]
    if not len(got):
        return np.zeros(3)
    assert np.isfinite(got).all()
    d = np.abs(got - want)
    if dst == "geo":
        dl = np.abs((got[:, 0] - want[:, 0] + 180.0) % 360.0 - 180.0)
        pole = np.abs(want[:, 1]) == 90.0
        dl[pole] = np.where(got[pole, 0] == 0.0, 0.0, np.inf) if from_ecef else 0.0
        return np.array([0.0, d[:, 2].max(), max(dl.max(), d[:, 1].max()) * DEG * A_WGS84])
    if dst == "tm":
        return np.array([d[:, :2].max(), d[:, 2].max(), 0.0])
    return np.array([d.max(), 0.0, 0.0])


def utm_grid_scene(n: int = 7, m: int = 8):
    """(vertices (n m, 3) in UTM zone 10 north, faces (2 (n - 1)(m - 1), 3)): a 60 m square of gently rolling ground."""
    e, nn = np.meshgrid(552000.0 + np.linspace(0, 60, m), 4182000.0 + np.linspace(0, 60, n))
    h = 20.0 + 3.0 * np.sin(e / 9.0) + 2.0 * np.cos(nn / 7.0)
    utm = np.stack([e.ravel(), nn.ravel(), h.ravel()], axis=1)
    idx = np.arange(n * m).reshape(n, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return utm, np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)])
