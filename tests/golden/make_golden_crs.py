#!/usr/bin/env python
"""tests/golden/crs_wgs84.npz: the oracle of the CRS reprojection stage (DESIGN.md "CRS reprojection", G9).

An mpmath restatement that shares no arithmetic with the kernel or with tests/crs_standin.py: Fourier coefficients of the
Krueger series to 8 terms by quadrature (tools/make_crs_constants.py) at 40 digits, the complex series
xi + i eta = zeta' + sum_j alpha_j sin 2 j zeta' evaluated with complex sines, the conformal latitude inverted by root finding,
ECEF inverted by Newton's method on p tan(phi) = Z + e^2 N sin(phi).  Every expected output is computed from the FLOAT64-ROUNDED
input of its direction.  On the central meridian the northing is also checked against k0 M(phi), the meridian arc by direct
quadrature, and one published position (43 38 33.24 N 79 23 13.7 W -> zone 17, E 630084.31, N 4833438.55) is asserted.

The file holds, for P points and G transverse Mercator systems (every point belongs to one):
  tm_params (G, 4) lon0, k0, FE, FN;  group (P,)
  in_ecef, in_geo, in_tm (P, 3): the inputs of the three kinds; geographic rows are (lon, lat, h) in degrees
  exp_<from>_<to> (P, 3), flag_<from>_<to> (P,) for the six ordered pairs: expected rows (NaN where flagged) and the flag
      (0 fine, 1 non-finite / origin / latitude outside [-90, 90], 2 beyond 90 degrees of the central meridian)
  constants (13,): A, alpha_1..6, beta_1..6 as doubles
  standin_err_m (3,): the largest error of tests/crs_standin.py over all of the above, in metres: E and N and ECEF
      components; h; lon and lat as radians times a
Run from the repository root:  python tests/golden/make_golden_crs.py"""
import sys
from pathlib import Path

import mpmath as mp
import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import make_crs_constants as consts  # noqa: E402

mp.mp.dps = 40
A_, F_, E2_ = consts.ellipsoid(mp)
E_ = mp.sqrt(E2_)
RECT, ALPHA8, BETA8 = consts.compute(8, 40)
DEG = mp.pi / 180
NAN3 = (mp.nan, mp.nan, mp.nan)
KINDS = ("ecef", "geo", "tm")


def wrap(d):
    d = d - 2 * mp.pi * mp.floor((d + mp.pi) / (2 * mp.pi))
    return d + 2 * mp.pi if d <= -mp.pi else d


def geo_to_ecef(phi, lam, h):
    if abs(phi) == mp.pi / 2:   # cos(pi / 2) is not 0 at any finite precision: the axis, exactly
        return mp.mpf(0), mp.mpf(0), (A_ * (1 - F_) + h) * mp.sign(phi)
    n = A_ / mp.sqrt(1 - E2_ * mp.sin(phi) ** 2)
    return (n + h) * mp.cos(phi) * mp.cos(lam), (n + h) * mp.cos(phi) * mp.sin(lam), (n * (1 - E2_) + h) * mp.sin(phi)


def ecef_to_geo(X, Y, Z):
    p = mp.sqrt(X * X + Y * Y)
    if p == 0:
        return (mp.pi / 2 if Z > 0 else -mp.pi / 2), mp.mpf(0), abs(Z) - A_ * (1 - F_)
    phi = mp.atan2(Z, p * (1 - E2_))
    for _ in range(60):   # Newton on g(phi) = p tan(phi) - Z - e^2 a sin(phi) / sqrt(1 - e^2 sin^2 phi)
        s, c = mp.sin(phi), mp.cos(phi)
        w = 1 - E2_ * s * s
        g = p * s / c - Z - E2_ * A_ * s / mp.sqrt(w)
        step = g / (p / (c * c) - E2_ * A_ * c / w ** mp.mpf(1.5))
        phi -= step
        if abs(step) < mp.mpf(10) ** -36:
            break
    else:
        raise RuntimeError("Newton did not converge")
    s, c = mp.sin(phi), mp.cos(phi)
    n = A_ / mp.sqrt(1 - E2_ * s * s)
    return phi, mp.atan2(Y, X), p * c + Z * s - n * (1 - E2_ * s * s)


def isometric(phi):
    return mp.asinh(mp.tan(phi)) - E_ * mp.atanh(E_ * mp.sin(phi))


def geo_to_tm(phi, lam, h, prm):
    lon0, k0, fe, fn = prm
    d = wrap(lam - lon0 * DEG)
    if abs(d) >= mp.pi / 2:
        return None
    if abs(phi) == mp.pi / 2:
        zeta = mp.mpc(phi, 0)
    else:
        t = mp.sinh(isometric(phi))   # tan of the conformal latitude
        zeta = mp.mpc(mp.atan2(t, mp.cos(d)), mp.asinh(mp.sin(d) / mp.sqrt(t * t + mp.cos(d) ** 2)))
    z = zeta + sum(ALPHA8[j] * mp.sin(2 * (j + 1) * zeta) for j in range(8))
    return fe + k0 * RECT * z.imag, fn + k0 * RECT * z.real, h


def tm_to_geo(E, N, h, prm):
    lon0, k0, fe, fn = prm
    z = mp.mpc((N - fn) / (k0 * RECT), (E - fe) / (k0 * RECT))
    zp = z - sum(BETA8[j] * mp.sin(2 * (j + 1) * z) for j in range(8))
    sh, cx, sx = mp.sinh(zp.imag), mp.cos(zp.real), mp.sin(zp.real)
    r = mp.sqrt(sh * sh + cx * cx)
    if r <= mp.mpf(2) ** -51:   # G7: the pole
        return (mp.pi / 2 if sx > 0 else -mp.pi / 2), wrap(lon0 * DEG), h
    if cx <= 0:
        return None
    psi = mp.asinh(sx / r)
    phi = mp.findroot(lambda p: isometric(p) - psi, mp.atan(sx / r), tol=mp.mpf(10) ** -70)
    return phi, wrap(lon0 * DEG + mp.atan2(sh, cx)), h


def convert(row, src, dst, prm):
    """One float64 row of kind `src` -> (mp triple, flag) in kind `dst`."""
    if not all(np.isfinite(row)):
        return NAN3, 1
    prm = tuple(mp.mpf(float(v)) for v in prm)
    x, y, z = (mp.mpf(float(v)) for v in row)
    if src == "ecef":
        if x == 0 and y == 0 and z == 0:
            return NAN3, 1
        geo = ecef_to_geo(x, y, z)
    elif src == "geo":
        if abs(y) > 90:
            return NAN3, 1
        geo = (y * DEG, x * DEG, z)
    else:
        geo = tm_to_geo(x, y, z, prm)
        if geo is None:
            return NAN3, 2
    if dst == "ecef":
        return geo_to_ecef(*geo), 0
    if dst == "geo":
        return (wrap(geo[1]) / DEG, geo[0] / DEG, geo[2]), 0
    out = geo_to_tm(*geo, prm)
    return (NAN3, 2) if out is None else (out, 0)


def points():
    """(geographic rows (lon, lat, h), group) and the systems."""
    utm = lambda zone, south=False: (6.0 * zone - 183.0, 0.9996, 500000.0, 10000000.0 if south else 0.0)  # noqa: E731
    systems = [utm(10), utm(17), utm(1), utm(60), utm(33, True), (12.5, 1.0, 0.0, -5000000.0)]
    rng = np.random.default_rng(20240611)
    rows, group = [], []

    def add(g, lon, lat, h):
        rows.append((lon, lat, h)); group.append(g)

    for _ in range(160):   # the working range of a zone
        g = int(rng.integers(0, len(systems)))
        add(g, systems[g][0] + rng.uniform(-3.5, 3.5), rng.uniform(-80, 84), rng.uniform(-500, 9000))
    add(1, -(79 + 23 / 60 + 13.7 / 3600), 43 + 38 / 60 + 33.24 / 3600, 0.0)   # the published position
    for g in (0, 4):
        lon0 = systems[g][0]
        for lat in (0.0, 1e-9, -1e-9, 30.0, -47.25, 80.0, -80.0, 84.0, -84.0, 89.0, 90.0, -90.0):   # the central meridian
            add(g, lon0, lat, 120.0)
        for dlon in (-3.0, 3.0, 6.0, -6.0, 20.0, -20.0):   # the equator and a mid latitude, off the meridian
            add(g, lon0 + dlon, 0.0, 0.0)
            add(g, lon0 + dlon, 38.5, -60.0)
        for dlon in (91.0, -91.0, 100.0, 179.0, 180.0, -135.0):   # beyond
            add(g, lon0 + dlon, 12.0, 5.0)
    for g, lons in ((2, (179.9, -179.9, 180.0, -180.0, 178.0, -176.5, 185.0)), (3, (179.9, -179.9, 180.0, 176.0, -178.5, -183.0))):
        for lon in lons:   # zones 1 and 60 across the antimeridian
            add(g, lon, 52.0, 10.0)
            add(g, lon, -17.0, -30.0)
    for lat, h in ((90.0, 0.0), (-90.0, 0.0), (90.0, 2500.0), (-90.0, -100.0)):   # the poles, the axis
        add(0, -123.0, lat, h)
        add(5, 40.0, lat, h)
    for lon, lat, h in ((10.0, 45.0, -6000.0), (5.0, -33.0, -420.0), (35.5, 31.5, -430.5)):   # h < 0
        add(5, lon, lat, h)
    special = len(rows)
    for bad in ((np.nan, 10.0, 0.0), (10.0, np.inf, 0.0), (10.0, 10.0, -np.inf), (20.0, 91.0, 0.0), (20.0, -90.5, 0.0)):
        add(1, *bad)
    add(1, -80.0, 0.0, 0.0)   # its ECEF row is replaced by the origin below
    return np.array(rows, dtype=np.float64), np.array(group, dtype=np.int32), np.array(systems, dtype=np.float64), special


def to_f64(triple):
    return [float(v) for v in triple]


def main():
    geo, group, systems, special = points()
    P = len(geo)
    ins = {"geo": geo, "ecef": np.full((P, 3), np.nan), "tm": np.full((P, 3), np.nan)}
    for i in range(P):   # the inputs of the other two kinds: the oracle's image of the geographic row, rounded
        for kind in ("ecef", "tm"):
            out, flag = convert(geo[i], "geo", kind, systems[group[i]])
            if flag == 0:
                ins[kind][i] = to_f64(out)
    ins["ecef"][P - 1] = 0.0                       # the origin
    ins["ecef"][special] = (np.inf, 1.0, 1.0)
    ins["tm"][special + 1] = (500000.0, np.inf, 1.0)
    ins["ecef"][special + 3] = (0.0, 0.0, 7.0e6)   # the axis, given directly
    ins["ecef"][special + 4] = (0.0, 0.0, -6.3e6)
    result = {"tm_params": systems, "group": group, "in_ecef": ins["ecef"], "in_geo": ins["geo"], "in_tm": ins["tm"]}
    oracle = {}
    for src in KINDS:
        for dst in KINDS:
            if src == dst:
                continue
            exp = np.full((P, 3), np.nan)
            flag = np.zeros(P, dtype=np.uint8)
            exact = []
            for i in range(P):
                out, flag[i] = convert(ins[src][i], src, dst, systems[group[i]])
                exact.append(out)
                if flag[i] == 0:
                    exp[i] = to_f64(out)
            result[f"exp_{src}_{dst}"] = exp
            result[f"flag_{src}_{dst}"] = flag
            oracle[(src, dst)] = exact

    # independent identities
    for i in range(P):
        lon0, k0, fe, fn = (mp.mpf(float(v)) for v in systems[group[i]])
        if result["flag_geo_tm"][i] == 0 and geo[i, 0] == float(lon0) and abs(geo[i, 1]) < 90:
            arc = mp.quad(lambda t: A_ * (1 - E2_) * (1 - E2_ * mp.sin(t) ** 2) ** mp.mpf(-1.5), [0, mp.mpf(float(geo[i, 1])) * DEG])
            north = oracle[("geo", "tm")][i][1]
            assert abs(north - (fn + k0 * arc)) < mp.mpf(10) ** -12, (i, north, fn + k0 * arc)
    landmark = 160
    e, n, _ = result["exp_geo_tm"][landmark]
    assert abs(e - 630084.31) < 0.25 and abs(n - 4833438.55) < 0.25, (e, n)   # published to 0.1 arc second of longitude
    assert consts.as_doubles(RECT, ALPHA8, BETA8) == consts.read_header(), "run tools/make_crs_constants.py --write first"
    assert abs(ALPHA8[6]) * float(RECT) < 1e-12 and abs(BETA8[6]) * float(RECT) < 1e-12   # six terms truncate below 1e-12 m

    # the stand-in's error against the unrounded oracle
    sys.path.insert(0, str(ROOT / "tests"))
    import crs_standin

    worst = np.zeros(3)
    kind_id = {"ecef": 0, "geo": 1, "tm": 2}
    for (src, dst), exact in oracle.items():
        for g in range(len(systems)):
            rows = np.nonzero(group == g)[0]
            crs = lambda k: (kind_id[k], *systems[g])  # noqa: E731
            got, status = crs_standin.reproject(ins[src][rows], crs(src), crs(dst))
            want_flag = result[f"flag_{src}_{dst}"][rows]
            assert np.array_equal(status, want_flag), (src, dst, g, rows[status != want_flag])
            for k, i in enumerate(rows):
                if want_flag[k]:
                    assert np.isnan(got[k]).all()
                    continue
                err = [abs(mp.mpf(float(got[k, c])) - exact[i][c]) for c in range(3)]
                if dst == "geo":
                    dl = abs(wrap((mp.mpf(float(got[k, 0])) - exact[i][0]) * DEG))
                    lat = exact[i][1]
                    if abs(lat) == 90:   # the longitude of a pole means nothing; the axis rule of G3 is exact
                        dl = mp.mpf(0) if src != "ecef" or got[k, 0] == 0.0 else mp.inf
                    worst[2] = max(worst[2], float(dl * A_), float(err[1] * DEG * A_))
                    worst[1] = max(worst[1], float(err[2]))
                else:
                    worst[0] = max(worst[0], float(err[0]), float(err[1]), float(err[2]) if dst == "ecef" else 0.0)
                    if dst == "tm":
                        worst[1] = max(worst[1], float(err[2]))
    result["standin_err_m"] = worst
    result["constants"] = np.array(consts.as_doubles(RECT, ALPHA8, BETA8))
    out = Path(__file__).with_name("crs_wgs84.npz")
    np.savez_compressed(out, **result)
    print(f"{P} points, stand-in worst error [planar / ECEF, h, lon / lat x a] = {worst} m -> {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
