#!/usr/bin/env python
"""The 13 doubles of the CRS reprojection stage (DESIGN.md "CRS reprojection", rule G2), computed, not looked up.

WGS84: a = 6378137, 1/f = 298.257223563.  chi is the conformal latitude, mu the rectifying latitude (meridian arc / A), A the
quarter meridian times 2 / pi.  On the central meridian

    mu - chi = sum_j alpha_j sin 2 j chi,        chi = mu - sum_j beta_j sin 2 j mu,

so alpha_j = (4 / pi) int_0^{pi/2} (mu - chi) sin 2 j chi dchi and beta_j = (4 / pi) int_0^{pi/2} (mu - chi) sin 2 j mu dmu are
exact Fourier coefficients.  mu - chi vanishes at both ends, so one integration by parts turns them into integrals over the
GEODETIC latitude phi that need no root finding:

    alpha_j =  (2 / (j pi)) int_0^{pi/2} cos(2 j chi(phi)) mu'(phi)  dphi
    beta_j  = -(2 / (j pi)) int_0^{pi/2} cos(2 j mu(phi))  chi'(phi) dphi

with mu'(phi) = a (1 - e^2) (1 - e^2 sin^2 phi)^(-3/2) / A, chi(phi) = gd(asinh(tan phi) - e atanh(e sin phi)),
chi'(phi) = cos chi (1 - e^2) / ((1 - e^2 sin^2 phi) cos phi) and mu(phi) through the incomplete elliptic integral of the second
kind.  Evaluated with mpmath's tanh-sinh quadrature at `DIGITS` digits.

    python tools/make_crs_constants.py            # print the constants
    python tools/make_crs_constants.py --write    # rewrite geograypher_amd/csrc/crs_constants.hpp

(tests/golden/make_golden_crs.py imports `compute` and stores the same doubles in the golden file.)"""
import argparse
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "geograypher_amd" / "csrc" / "crs_constants.hpp"
DIGITS = 40
WGS84_A = 6378137
WGS84_INV_F = "298.257223563"


def ellipsoid(mp):
    a = mp.mpf(WGS84_A)
    f = 1 / mp.mpf(WGS84_INV_F)
    return a, f, f * (2 - f)


def rectifying_radius(mp):
    a, _, e2 = ellipsoid(mp)
    return 2 / mp.pi * mp.quad(lambda p: a * (1 - e2) * (1 - e2 * mp.sin(p) ** 2) ** mp.mpf(-1.5), [0, mp.pi / 2])


def conformal_latitude(mp, phi):
    _, _, e2 = ellipsoid(mp)
    e = mp.sqrt(e2)
    return mp.atan(mp.sinh(mp.asinh(mp.tan(phi)) - e * mp.atanh(e * mp.sin(phi))))


def meridian_arc(mp, phi):
    """M(phi) = a (1 - e^2) int_0^phi (1 - e^2 sin^2 t)^(-3/2) dt, through the incomplete integral E(phi | e^2)."""
    a, _, e2 = ellipsoid(mp)
    s, c = mp.sin(phi), mp.cos(phi)
    return a * (mp.ellipe(phi, e2) - e2 * s * c / mp.sqrt(1 - e2 * s * s))


def alpha(mp, j, A):
    a, _, e2 = ellipsoid(mp)

    def g(p):
        return mp.cos(2 * j * conformal_latitude(mp, p)) * a * (1 - e2) * (1 - e2 * mp.sin(p) ** 2) ** mp.mpf(-1.5) / A

    return 2 / (j * mp.pi) * mp.quad(g, [0, mp.pi / 4, mp.pi / 2])


def beta(mp, j, A):
    _, _, e2 = ellipsoid(mp)

    def g(p):
        chi = conformal_latitude(mp, p)
        return mp.cos(2 * j * meridian_arc(mp, p) / A) * mp.cos(chi) * (1 - e2) / ((1 - e2 * mp.sin(p) ** 2) * mp.cos(p))

    return -2 / (j * mp.pi) * mp.quad(g, [0, mp.pi / 4, mp.pi / 2])


def compute(terms: int = 6, digits: int = DIGITS):
    """(A, [alpha_1 ... alpha_terms], [beta_1 ... beta_terms]) as mpmath numbers."""
    import mpmath as mp

    with mp.workdps(digits):
        A = rectifying_radius(mp)
        return +A, [+alpha(mp, j, A) for j in range(1, terms + 1)], [+beta(mp, j, A) for j in range(1, terms + 1)]


def as_doubles(A, alphas, betas):
    return [float(A)] + [float(v) for v in alphas[:6]] + [float(v) for v in betas[:6]]


def header_text(doubles) -> str:
    A, al, be = doubles[0], doubles[1:7], doubles[7:13]
    row = lambda vs: ", ".join(repr(v) for v in vs)  # noqa: E731  (repr of a float reads back to the same double)
    return (
        "#pragma once\n"
        "// geograypher_amd/csrc/crs_constants.hpp -- WRITTEN BY tools/make_crs_constants.py, do not edit: the rectifying radius and the\n"
        "// six Krueger coefficients per direction of the WGS84 transverse Mercator series (DESIGN.md \"CRS reprojection\", rule G2),\n"
        "// Fourier coefficients evaluated by quadrature at %d digits and rounded once.  tests/test_reproject_host.py compares them\n"
        "// with tests/golden/crs_wgs84.npz to the last bit.\n"
        "#define GR_CRS_RECT_RADIUS %r\n"
        "#define GR_CRS_ALPHA { %s }\n"
        "#define GR_CRS_BETA { %s }\n" % (DIGITS, A, row(al), row(be)))


def read_header(path: Path = HEADER):
    """The 13 doubles of the committed header, in the order of `as_doubles`."""
    import re

    text = path.read_text()
    A = float(re.search(r"#define GR_CRS_RECT_RADIUS (\S+)", text).group(1))
    al = [float(v) for v in re.search(r"#define GR_CRS_ALPHA \{(.*?)\}", text).group(1).split(",")]
    be = [float(v) for v in re.search(r"#define GR_CRS_BETA \{(.*?)\}", text).group(1).split(",")]
    return [A] + al + be


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help=f"rewrite {HEADER.relative_to(ROOT)}")
    ap.add_argument("--terms", type=int, default=7, help="terms to print (the header keeps six)")
    args = ap.parse_args()
    A, al, be = compute(max(args.terms, 6))
    print(f"A = {float(A)!r}")
    for j, (x, y) in enumerate(zip(al, be), 1):
        print(f"alpha_{j} = {float(x)!r:>26}   beta_{j} = {float(y)!r:>26}")
    if args.write:
        HEADER.write_text(header_text(as_doubles(A, al, be)))
        print("wrote", HEADER)
