"""tests/image_edge_cases.py -- the case tables shared by tests/test_image_oracles.py (CPU: the host restatements against live
scipy) and tests/test_image_stage_edges.py (GPU: the kernels of warp.hip and resize.hip against those restatements), so that
every shape and coordinate a kernel is held to is one the yardstick itself was held to.  Test-only."""
import numpy as np

# ---- warp: sampling coordinates --------------------------------------------------------------------------------------------
HUGE = [1e300, -1e300, 2.0**31, -(2.0**31), 2.0**63, -(2.0**63)]
NON_FINITE = [np.inf, -np.inf, np.nan]


def edge_coordinates(n, finite_only=False, quarters_only=False):
    """The coordinates of one axis of length n where nearest / bilinear sampling decides something: ties of floor(x + 0.5),
    both borders and the half pixel around them, and values no integer conversion survives.
    quarters_only: only multiples of 1/4 (and the huge / non-finite ones, which read `fill`), for which bilinear weights and
    products of small integers are exact in float64."""
    lo = [-1.5, -1.0, -0.75, -0.5, np.nextafter(-0.5, 0.0), -0.25, -0.0, 0.0, 0.25, 0.49999999999999994, 0.5, 1.5, 2.5]
    hi = [n - 1.5, n - 1.0, n - 0.75, np.nextafter(n - 0.5, -np.inf), n - 0.5, n - 0.25, float(n), n + 0.5]
    vals = lo + hi
    if quarters_only:
        vals = [v for v in vals if v * 4 == np.floor(v * 4)]
    vals = vals + HUGE
    if not finite_only:
        vals = vals + NON_FINITE
    return np.array(vals, dtype=np.float64)


def edge_map(h_in, w_in, **kw):
    """(2, R, K) map: every combination of an edge row coordinate with an edge column coordinate."""
    rr, cc = np.meshgrid(edge_coordinates(h_in, **kw), edge_coordinates(w_in, **kw), indexing="ij")
    return np.stack([rr, cc])


def random_map(rng, h_in, w_in, h_out, w_out, non_finite=True, quarters_only=False):
    """(2, h_out, w_out) map over and around the input: uniform positions, a third snapped to halves (quarters_only: all
    snapped to quarters), a tenth replaced by edge coordinates of their axis."""
    m = np.stack([rng.uniform(-2, h_in + 1, (h_out, w_out)), rng.uniform(-2, w_in + 1, (h_out, w_out))])
    if quarters_only:
        m = np.round(m * 4) / 4
    else:
        m = np.where(rng.random(m.shape) < 0.3, np.round(m * 2) / 2, m)
    for axis, n in enumerate((h_in, w_in)):
        e = edge_coordinates(n, finite_only=not non_finite, quarters_only=quarters_only)
        pick = rng.random((h_out, w_out)) < 0.1
        m[axis] = np.where(pick, e[rng.integers(0, e.size, (h_out, w_out))], m[axis])
    return m


# one pixel, one row, one column, and widths around a workgroup
WARP_IN_SHAPES = [(1, 1), (1, 7), (5, 1), (2, 2), (6, 9), (2, 255), (1, 256), (3, 257)]
# output shapes: 1 x 1, pixel counts around one and 256 workgroups of 256, and 91 pixels (x C never a multiple of 256 for C < 256)
WARP_OUT_SHAPES = [(1, 1), (7, 13), (1, 255), (16, 16), (257, 1), (1, 65535), (256, 256), (65537, 1)]
WARP_CHANNELS = [1, 2, 3, 4, 5, 7]

# ---- resize: (h_in, w_in) -> (h_out, w_out) -----------------------------------------------------------------------------------
RESIZE_SHAPES = [
    # the filter radius exceeds the image: the mirror index wraps more than one period
    ((1, 300), (1, 7)), ((300, 1), (7, 1)), ((2, 2), (1, 1)), ((3, 5), (1, 1)), ((200, 260), (1, 1)), ((9, 9), (2, 2)),
    # one axis shrinks while the other grows; one axis unchanged (radius 0 on rows only)
    ((5, 7), (2, 20)), ((40, 3), (3, 9)), ((7, 513), (7, 3)),
    # near identity
    ((64, 64), (63, 65)), ((100, 100), (99, 99)),
    # single row / column growing
    ((1, 5), (1, 12)), ((4, 1), (9, 1)),
]
RESIZE_CHANNELS = [None, 1, 2, 3, 4, 5]


def resize_block_shapes():
    """((h_in, w_in), (h_out, w_out), C) with w_in * C and w_out * C at 255 / 256 / 257: both kernels run 256-wide blocks over
    col * C + channel."""
    out = []
    for C, w_lo, w_mid, w_hi in ((None, 255, 256, 257), (1, 255, 256, 257), (3, 85, None, None), (2, None, 128, None),
                                 (4, None, 64, None), (5, 51, None, None)):
        for w in (w_lo, w_mid, w_hi):
            if w is None:
                continue
            out.append(((6, w), (4, max(1, w // 3)), C))   # w_in * C on the boundary
            out.append(((5, 2 * w + 3), (3, w), C))        # w_out * C on the boundary (down-scale)
            out.append(((3, w // 2 + 1), (4, w), C))       # w_out * C on the boundary (up-scale)
    out.append(((4, 257), (3, 100), 1))
    return out


# the largest filter the library takes (radius int(4 sigma + 0.5) <= 1024): factor 513 -> sigma 256 -> radius 1024, and
# factor 512.5 -> radius 1023 just under it; factor 513.33 -> sigma 256.17 -> radius 1025 is refused
RESIZE_LARGEST_RADIUS = [((6150, 4), (12, 4)), ((6156, 4), (12, 4)), ((3, 6156), (3, 12))]
RESIZE_RADIUS_TOO_LARGE = [((6160, 4), (12, 4)), ((4, 6160), (4, 12))]


def resize_image_values(rng, shape, dtype):
    if dtype == "uint8":
        return rng.integers(0, 256, shape).astype(np.uint8)
    return (rng.normal(0, 1, shape) * 50).astype(dtype)


def with_channels(hw, C):
    return tuple(hw) if C is None else tuple(hw) + (C,)


# ---- lens inverse ------------------------------------------------------------------------------------------------------------
def lens(f, W, H, cx=0.0, cy=0.0, **coeffs):
    return {"f": float(f), "cx": float(cx), "cy": float(cy), "image_width": W, "image_height": H, **coeffs}


# magnitudes of a photogrammetry lens (the golden camera XML: k1 -0.09, k2 -0.08, k3 0.12, k4 -0.08, p ~ 1e-4, b ~ 0.5)
LENS_COEFFS = {"k1": 0.09, "k2": 0.08, "k3": 0.12, "k4": 0.08, "p1": 3e-3, "p2": 2e-3, "b1": 0.5, "b2": 0.3}
FULL_LENS = {"k1": -0.0919367147, "k2": -0.0762807468, "k3": 0.1162639394, "k4": -0.0761413904, "p1": -0.0003134847,
             "p2": 0.0001164035, "b1": 0.5262024073, "b2": -0.3058334293}


def one_coefficient_lenses():
    out = {}
    for name, mag in LENS_COEFFS.items():
        for sign in (1, -1):
            out[f"{name}{'+' if sign > 0 else '-'}"] = {name: sign * mag}
    out["all8"] = dict(FULL_LENS)
    return out
