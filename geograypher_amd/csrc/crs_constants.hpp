#pragma once
// geograypher_amd/csrc/crs_constants.hpp -- WRITTEN BY tools/make_crs_constants.py, do not edit: the rectifying radius and the
// six Krueger coefficients per direction of the WGS84 transverse Mercator series (DESIGN.md "CRS reprojection", rule G2),
// Fourier coefficients evaluated by quadrature at 40 digits and rounded once.  tests/test_reproject_host.py compares them
// with tests/golden/crs_wgs84.npz to the last bit.
#define GR_CRS_RECT_RADIUS 6367449.145823415
#define GR_CRS_ALPHA { 0.0008377318206244698, 7.60852777357249e-07, 1.197645503242492e-09, 2.4291706803973133e-12, 5.711818369154105e-15, 1.4799980270526208e-17 }
#define GR_CRS_BETA { 0.0008377321640579486, 5.9058701522203654e-08, 1.673482665343825e-10, 2.1647981104903862e-13, 3.787930968839601e-16, 7.236769287965758e-19 }
