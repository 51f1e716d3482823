"""Rule-set checks for the C rasterizer oracle: fast == spec, and coverage == the exact geometric predicate on the
snapped vertices (evaluated with Python integers / fractions, independent of the C code) -- under rule R1 and under R1-GL
(vertex_order="gl": the vertex stage in an OpenGL pipeline's order of operations), the latter also on rounding ties, at the guard
band and on a vertex that tells the fused viewport multiply-add from an unfused one."""
import math
from fractions import Fraction

import numpy as np
import pytest

from geograypher_amd.utils import synthetic
from oracle import oracle_c
from tests import raster_scenes


def _cam(h, w, f=None, pos=(0, 0, 5.0), near=1e-3):
    T = synthetic.downward_view(1, pos[2], 1)  # looks down from z = pos[2]
    T[:3, 3] = pos
    rec = np.zeros(16, dtype=np.float32)
    rec[0:9] = T[:3, :3].reshape(9)
    rec[9:12] = T[:3, 3]
    rec[12] = f if f is not None else h
    rec[13], rec[14], rec[15] = w / 2, h / 2, near
    return rec


def _round_f32(x):
    """The float32 nearest to an exact rational, ties to even, found with integer arithmetic alone (one rounding: no detour
    through float64)."""
    x = Fraction(x)
    if x == 0:
        return np.float32(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^e <= a < 2^(e + 1), give or take one
    if Fraction(2) ** e > a:
        e -= 1
    elif Fraction(2) ** (e + 1) <= a:
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)                       # subnormals keep the spacing of the smallest normals
    n, r = divmod(a / ulp, 1)
    if 2 * r > 1 or (2 * r == 1 and n % 2 == 1):
        n += 1
    a = n * ulp
    if a >= Fraction(2) ** 128:
        return np.float32(-np.inf if x < 0 else np.inf)
    return np.float32(-float(a) if x < 0 else float(a))            # n < 2^25: exact in a double, and representable in float32


def _snap_gl(qx, qy, iz, cam, size, rounding="even", fused=True):
    """The second half of R1-GL as DESIGN.md section 2 and include/geograster.h (GR_OPT_VERTEX_ORDER) state it, float32 unless
    said otherwise: P = ((2 f) / w, -((2 f) / h)); clip = P q; ndc = clip (1 / q_z); win = fma(ndc, size / 2, size / 2), rounded
    ONCE; valid iff |win| < 16384; fixed = round-half-to-even(256 (win - 0.5)); X = fixed_x + 128, Y = 256 h - 128 - fixed_y
    (GL rows run bottom-up).  Returns (X, Y), None for an invalid vertex.
    `rounding="floor"` (floor(x + 0.5) in place of half-to-even) and `fused=False` (the product rounded before the sum) are the
    two mistakes a scene must be able to tell from the rule: tests compute both pictures and require them to differ."""
    f32 = np.float32
    h, w = size
    two_f = f32(2.0) * cam[12]
    P = (two_f / f32(w), -(two_f / f32(h)))
    half = (f32(0.5) * f32(w), f32(0.5) * f32(h))
    fixed = []
    with np.errstate(all="ignore"):
        for c, q in enumerate((f32(qx), f32(qy))):
            clip = f32(P[c] * q)
            ndc = f32(clip * iz)
            if not np.isfinite(ndc):
                return None
            if fused:
                win = _round_f32(Fraction(float(ndc)) * Fraction(float(half[c])) + Fraction(float(half[c])))
            else:
                win = f32(f32(ndc * half[c]) + half[c])
            if not abs(win) < 16384:
                return None
            x = Fraction(float(f32(f32(win - f32(0.5)) * f32(256.0))))
            fixed.append(round(x) if rounding == "even" else math.floor(x + Fraction(1, 2)))   # round(Fraction): half to even
    return fixed[0] + 128, 256 * h - 128 - fixed[1]


def _project_f32(p, cam, vertex_order="r1", size=None, **gl):
    """R1 (or, vertex_order="gl" with size = (h, w), R1-GL) in numpy float32, op for op."""
    f32 = np.float32
    d = [f32(p[i]) - cam[9 + i] for i in range(3)]
    q = []
    for c in range(3):
        m0, m1, m2 = cam[c] * d[0], cam[3 + c] * d[1], cam[6 + c] * d[2]
        q.append(f32(f32(m0 + m1) + m2))
    if not q[2] > cam[15]:
        return None
    iz = f32(1.0) / q[2]
    if vertex_order == "gl":
        XY = _snap_gl(q[0], q[1], iz, cam, size, **gl)
        return None if XY is None else (XY[0], XY[1], iz)
    sx = cam[13] + f32(f32(cam[12] * q[0]) * iz)
    sy = cam[14] + f32(f32(cam[12] * q[1]) * iz)
    if not (abs(sx) < 16384 and abs(sy) < 16384):
        return None
    return int(np.floor(f32(sx * f32(256.0)) + f32(0.5))), int(np.floor(f32(sy * f32(256.0)) + f32(0.5))), iz


def _clip_python(pts, cam, vertex_order="r1", size=None, **gl):
    """R7 in Python floats (IEEE doubles, one rounding per operation): the clipped polygon of a face as snapped
    (X, Y, iz) vertices, [] when the face is dropped.  The guard planes bound the coordinate the snap's guard tests: R1's s, or
    the GL window coordinate."""
    f32 = np.float32
    q = []
    for p in pts:
        d = [f32(p[i]) - cam[9 + i] for i in range(3)]
        q.append([f32(f32(cam[c] * d[0] + cam[3 + c] * d[1]) + cam[6 + c] * d[2]) for c in range(3)])
    fe, cxp, cyp, near = cam[12], cam[13], cam[14], cam[15]
    if not (near > 0 and fe > 0 and np.isfinite(fe) and np.isfinite(cxp) and np.isfinite(cyp)):
        return []
    if not all(np.isfinite(c) for v in q for c in v) or not any(v[2] > near for v in q):
        return []
    G = 16383.0
    ccx, ccy = float(cxp), float(cyp)
    if vertex_order == "gl":     # the planes bound the GL window coordinate: win_x = w / 2 + f x / z, win_y = h / 2 - f y / z
        ccx, ccy = 0.5 * size[1], -0.5 * size[0]
    planes = [(0.0, 0.0, 1.0, -float(near)), (-float(fe), 0.0, G - ccx, 0.0), (float(fe), 0.0, G + ccx, 0.0),
              (0.0, -float(fe), G - ccy, 0.0), (0.0, float(fe), G + ccy, 0.0)]
    poly = [tuple(float(c) for c in v) for v in q]

    def dist(pl, P):
        return ((pl[0] * P[0] + pl[1] * P[1]) + pl[2] * P[2]) + pl[3]

    def cross(inside, din, outside, dout):
        t = din / (din - dout)
        return tuple(inside[k] + t * (outside[k] - inside[k]) for k in range(3))

    for pl in planes:
        out = []
        for i in range(len(poly)):
            S, E = poly[i], poly[(i + 1) % len(poly)]
            dS, dE = dist(pl, S), dist(pl, E)
            if dS >= 0 and dE >= 0:
                out.append(E)
            elif dS >= 0:
                out.append(cross(S, dS, E, dE))
            elif dE >= 0:
                out.append(cross(E, dE, S, dS))
                out.append(E)
        poly = out
        if not poly:
            return []
    if len(poly) < 3:
        return []
    snapped = []
    for P in poly:
        qx, qy, qz = f32(P[0]), f32(P[1]), f32(P[2])
        if not qz > 0:
            return []
        iz = f32(1.0) / qz
        if vertex_order == "gl":
            XY = _snap_gl(qx, qy, iz, cam, size, **gl)
            if XY is None:
                return []
            snapped.append((XY[0], XY[1], iz))
            continue
        sx = cxp + f32(f32(fe * qx) * iz)
        sy = cyp + f32(f32(fe * qy) * iz)
        if not (abs(sx) < 16384 and abs(sy) < 16384):
            return []
        snapped.append((int(np.floor(f32(sx * f32(256.0)) + f32(0.5))), int(np.floor(f32(sy * f32(256.0)) + f32(0.5))), iz))
    return snapped


def _spec_python(verts, faces, cam, h, w, vertex_order="r1", want_depth=False, **gl):
    """Exact coverage + top-left rule + R4 depth (+ R7 clipping), straight from DESIGN.md, with Python ints.  want_depth: also
    the camera-space depth image the oracle returns (1 / the winning key's float, +inf background)."""
    f32 = np.float32
    ids = np.full((h, w), -1, dtype=np.int64)
    zb = np.zeros((h, w), dtype=np.int64)
    work = []
    for f, tri in enumerate(faces):
        v = [_project_f32(verts[i], cam, vertex_order, (h, w), **gl) for i in tri]
        if any(x is None for x in v):
            poly = _clip_python([verts[i] for i in tri], cam, vertex_order, (h, w), **gl)
            work += [(f, [poly[0], poly[k], poly[k + 1]]) for k in range(1, len(poly) - 1)]
        else:
            work.append((f, v))
    for f, v in work:
        (X0, Y0, z0), (X1, Y1, z1), (X2, Y2, z2) = v
        area2 = (X1 - X0) * (Y2 - Y0) - (X2 - X0) * (Y1 - Y0)
        if area2 == 0:
            continue
        if area2 < 0:
            (X1, Y1, z1), (X2, Y2, z2) = (X2, Y2, z2), (X1, Y1, z1)
            area2 = -area2
        d1, d2 = float(z1) - float(z0), float(z2) - float(z0)
        A = f32((d1 * float(Y2 - Y0) - d2 * float(Y1 - Y0)) / float(area2))
        B = f32((d2 * float(X1 - X0) - d1 * float(X2 - X0)) / float(area2))
        P = [(X0, Y0), (X1, Y1), (X2, Y2)]
        for i in range(h):
            for j in range(w):
                px, py = 256 * j + 128, 256 * i + 128
                ok = True
                for k in range(3):
                    (xa, ya), (xb, yb) = P[k], P[(k + 1) % 3]
                    dx, dy = xb - xa, yb - ya
                    e = dx * (py - ya) - dy * (px - xa)
                    owns = dy < 0 or (dy == 0 and dx < 0)
                    if not (e > 0 or (e == 0 and owns)):
                        ok = False
                if not ok:
                    continue
                z = f32(z0 + f32(f32(A * f32(px - X0)) + f32(B * f32(py - Y0))))
                bits = int(np.array(z, dtype=np.float32).view(np.int32))
                bits = max(bits, 1)
                if bits > zb[i, j] or (bits == zb[i, j] and f < ids[i, j]):
                    zb[i, j], ids[i, j] = bits, f
    if want_depth:
        with np.errstate(divide="ignore"):
            depth = np.where(ids >= 0, f32(1.0) / zb.astype(np.int32).view(f32), f32(np.inf)).astype(f32)
        return ids, depth
    return ids


def _random_soup(rng, n_tri, spread=3.0, zspread=1.5):
    verts = rng.uniform(-spread, spread, (3 * n_tri, 3))
    verts[:, 2] = rng.uniform(-zspread, zspread, 3 * n_tri)
    faces = np.arange(3 * n_tri).reshape(n_tri, 3)
    return verts.astype(np.float32), faces.astype(np.int32)


@pytest.mark.parametrize("seed", range(4))
def test_c_oracle_equals_python_spec(seed):
    rng = np.random.default_rng(seed)
    verts, faces = _random_soup(rng, 25)
    h, w = 20, 28
    cam = _cam(h, w, f=18.0)
    got = oracle_c.raster(verts, faces, cam, h, w, spec=True)
    want = _spec_python(verts, faces, cam, h, w)
    np.testing.assert_array_equal(got, want)
    assert (got >= 0).sum() > 50


@pytest.mark.parametrize("seed", range(6))
def test_fast_equals_spec(seed):
    rng = np.random.default_rng(100 + seed)
    verts, faces = _random_soup(rng, 400, spread=6.0)
    h, w = 97, 131
    cam = _cam(h, w, f=60.0 + 10 * seed)
    a, da = oracle_c.raster(verts, faces, cam, h, w, want_depth=True, spec=True)
    b, db = oracle_c.raster(verts, faces, cam, h, w, want_depth=True, spec=False)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(da, db)


def test_shared_edges_are_watertight_and_exclusive():
    """A nadir view of a jittered grid: every pixel inside the footprint gets exactly one face, no holes on edges."""
    (points, faces), cams = synthetic.config1_scene()
    cam = cams[0]
    h, w = cam.get_image_size(1.0)
    ids = oracle_c.raster(points, faces, cam.get_raster_record(1.0, near=0.1), h, w)
    assert ids.min() >= 0 and ids.max() < faces.shape[0]  # the 100 m plane covers the 51 x 38 m footprint entirely


def test_pixel_centres_on_edges_follow_top_left_rule():
    """Two triangles of one square whose diagonal passes exactly through pixel centres (the situation of the
    reference's own simple-mesh fixture): every pixel is claimed exactly once and the split is the top-left rule."""
    verts = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    h = w = 8
    cam = _cam(h, w, f=20.0)  # 4 px per unit at depth 5: the square fills the 8 x 8 window, diagonal on centres
    ids = oracle_c.raster(verts, faces, cam, h, w, spec=True)
    assert ids.min() >= 0
    # each pixel centre on the shared diagonal belongs to exactly one triangle, and both triangles own pixels
    assert set(np.unique(ids)) == {0, 1}


@pytest.mark.parametrize("seed", range(4))
def test_clipping_c_oracle_equals_python_spec(seed):
    """R7: a camera in the middle of the soup -- faces straddle the near plane and run far outside the guard band; the C
    oracle (both forms) and the Python restatement agree pixel for pixel."""
    rng = np.random.default_rng(100 + seed)
    verts, faces = _random_soup(rng, 40, spread=4.0, zspread=2.5)
    h, w = 20, 28
    cam = _cam(h, w, f=14.0, pos=(0.3, -0.2, 0.4), near=0.05 if seed % 2 else 0.6)
    got = oracle_c.raster(verts, faces, cam, h, w, spec=True)
    want = _spec_python(verts, faces, cam, h, w)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(oracle_c.raster(verts, faces, cam, h, w), got)
    clipped = sum(1 for tri in faces if any(_project_f32(verts[i], cam) is None for i in tri) and _clip_python([verts[i] for i in tri], cam))
    assert clipped >= 5 and (got >= 0).sum() > 100


def test_clipping_ground_plane_to_the_horizon():
    """Two 1 km triangles seen from 2 m above them, looking at the horizon: every vertex is behind the camera or outside
    the guard band; clipped, the ground fills the picture below the horizon with the analytic depth."""
    pts = np.array([[-500, -500, 0], [500, -500, 0], [500, 500, 0], [-500, 500, 0]], dtype=np.float64)
    quad = np.array([[0, 1, 2], [0, 2, 3]])
    pose = synthetic.look_at((0.0, 0.0, 2.0), (0.0, 100.0, 2.0), up_hint=(0, 0, 1))
    cams = synthetic.camera_set_from_poses([pose], f=300.0, width=320, height=240)
    rec = cams.get_raster_records(1.0, near=0.1)[0]
    ids, dep = oracle_c.raster(pts, quad, rec, 240, 320, want_depth=True)
    np.testing.assert_array_equal(oracle_c.raster(pts, quad, rec, 240, 320, spec=True), ids)
    assert (ids[121:] >= 0).all() and (ids[:120] == -1).all()
    for row in (130, 180, 239):
        assert abs(dep[row, 160] - 2.0 * 300.0 / (row + 0.5 - 120.0)) < 2e-3 * dep[row, 160]


def test_background_degenerate_and_behind_camera():
    h, w = 16, 16
    cam = _cam(h, w, f=8.0)
    verts = np.array(
        [[0, 0, 0], [1, 0, 0], [2, 0, 0],  # collinear -> zero area
         [0, 0, 6], [1, 0, 6], [0, 1, 6],  # behind the camera (camera at z=5 looking down)
         [-0.4, -0.4, 0], [0.4, -0.4, 0], [0, 0.4, 0]],
        dtype=np.float32,
    )
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32)
    ids, depth = oracle_c.raster(verts, faces, cam, h, w, want_depth=True)
    assert set(np.unique(ids)) <= {-1, 2}
    assert (ids == 2).sum() > 0
    assert np.all(np.isinf(depth[ids == -1]))
    np.testing.assert_allclose(depth[ids == 2], 5.0, rtol=1e-6)


def test_nearest_face_wins_and_ties_go_to_lower_id():
    h, w = 12, 12
    cam = _cam(h, w, f=6.0)
    big = [[-3, -3], [3, -3], [0, 4]]
    verts = np.array([[x, y, 0.0] for x, y in big] + [[x, y, 1.0] for x, y in big] + [[x, y, 0.0] for x, y in big],
                     dtype=np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32)
    ids = oracle_c.raster(verts, faces, cam, h, w)
    assert set(np.unique(ids)) <= {-1, 1}  # z = 1 is nearer to the camera at z = 5
    ids2 = oracle_c.raster(verts, faces[[0, 2]], cam, h, w)  # two coincident faces: lower id
    assert set(np.unique(ids2)) <= {-1, 0}


# ---- R1-GL: vertex_order="gl" ---------------------------------------------------------------------------------------------------
# sizes at which size / 2 is a half-integer or 2 f / w is inexact, each with a focal length that is no dyadic number
GL_SIZES = {(20, 28): 18.3, (1, 1): 0.7, (3, 7): 5.3, (21, 29): 17.1, (17, 64): 41.9}


@pytest.mark.parametrize("inside", [False, True], ids=["above", "inside"])
@pytest.mark.parametrize("size", list(GL_SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_gl_order_c_oracle_equals_python_spec(size, inside):
    """oracle_raster.c's R1-GL branch (orc_snap) against the restatement above, written from DESIGN.md's prose: random soups seen
    from above and from a camera in the middle of the soup, where faces cross the near plane and the clip path snaps its new
    vertices in the same order."""
    h, w = size
    rng = np.random.default_rng(200 + 7 * h + w + (1000 if inside else 0))
    if inside:
        verts, faces = _random_soup(rng, 40, spread=4.0, zspread=2.5)
        cam = _cam(h, w, f=GL_SIZES[size], pos=(0.3, -0.2, 0.4), near=0.05 if h % 2 else 0.6)
    else:
        verts, faces = _random_soup(rng, 25)
        cam = _cam(h, w, f=GL_SIZES[size])
    assert cam[13] == w / 2 and cam[14] == h / 2      # the GL order's viewport: principal point at the window centre
    got = oracle_c.raster(verts, faces, cam, h, w, spec=True, vertex_order="gl")
    want = _spec_python(verts, faces, cam, h, w, "gl")
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(oracle_c.raster(verts, faces, cam, h, w, vertex_order="gl"), got)
    assert (got >= 0).sum() > min(50, h * w // 2)
    if inside:
        clipped = sum(1 for tri in faces if any(_project_f32(verts[i], cam, "gl", size) is None for i in tri)
                      and _clip_python([verts[i] for i in tri], cam, "gl", size))
        assert clipped >= 5


@pytest.mark.parametrize("seed", range(6))
def test_gl_order_fast_equals_spec(seed):
    """test_fast_equals_spec in the GL order: ids and depth bits."""
    rng = np.random.default_rng(100 + seed)
    verts, faces = _random_soup(rng, 400, spread=6.0)
    h, w = 97, 131
    cam = _cam(h, w, f=60.0 + 10 * seed)
    a, da = oracle_c.raster(verts, faces, cam, h, w, want_depth=True, spec=True, vertex_order="gl")
    b, db = oracle_c.raster(verts, faces, cam, h, w, want_depth=True, spec=False, vertex_order="gl")
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(da.view(np.int32), db.view(np.int32))


def test_gl_order_rounds_ties_to_even():
    """raster_scenes.tie_scene: every vertex is an exact tie of the snap, 256 (win - 0.5) = k + 0.5, with k even and odd, positive
    and negative, in x and -- through the bottom-up row flip -- in y.  The vertex stage itself first: R1 gives k + 129 always,
    R1-GL k + 128 for even k and k + 129 for odd k.  Then the picture: the oracle's equals the restatement's, and the scene tells
    half-to-even from floor(x + 0.5) -- the restatement with that rounding draws another picture, on every face but the
    all-odd one."""
    h = w = 64
    cam = raster_scenes.pinhole_record(h, w, raster_scenes.TIE_F)[0]
    for k in (-1024, -1001, -2, -1, 0, 1, 2560, 2561, 16382, 16383, 17000):
        p = [raster_scenes.tie_x(k, w), raster_scenes.tie_y(k, h), 1.0]
        assert _project_f32(p, cam)[:2] == (k + 129, 256 * h - 128 - k)
        assert _project_f32(p, cam, "gl", (h, w))[:2] == (k + 128 + k % 2, 256 * h - 128 - (k + k % 2))
    verts, faces, recs = raster_scenes.tie_scene(h, w)
    want = _spec_python(verts, faces, recs[0], h, w, "gl")
    for spec in (True, False):
        np.testing.assert_array_equal(oracle_c.raster(verts, faces, recs[0], h, w, spec=spec, vertex_order="gl"), want)
    floor = _spec_python(verts, faces, recs[0], h, w, "gl", rounding="floor")
    assert (floor != want).sum() > 0
    for f in range(faces.shape[0]):
        differs = ((floor == f) != (want == f)).sum()
        assert (differs == 0) if f == 6 else (differs >= 20), (f, differs)
    assert (want != oracle_c.raster(verts, faces, recs[0], h, w)).sum() > 0


def test_gl_order_viewport_multiply_add_is_fused():
    """raster_scenes.fma_scene: a coordinate whose exact ndc * size / 2 + size / 2 lies between the fused and the unfused result,
    on a snap tie.  The restatement with the product rounded on its own draws another picture of both faces; the oracle draws
    the fused one."""
    verts, faces, recs = raster_scenes.fma_scene()
    cam = recs[0]
    assert _snap_gl(verts[0, 0], verts[3, 1], np.float32(1.0), cam, (6, 6)) == (513 + 128, 256 * 6 - 128 - 513)
    assert _snap_gl(verts[0, 0], verts[3, 1], np.float32(1.0), cam, (6, 6), fused=False) == (512 + 128, 256 * 6 - 128 - 512)
    want = _spec_python(verts, faces, cam, 6, 6, "gl")
    unfused = _spec_python(verts, faces, cam, 6, 6, "gl", fused=False)
    for f in range(2):
        assert ((unfused == f) != (want == f)).sum() >= 2
    for spec in (True, False):
        np.testing.assert_array_equal(oracle_c.raster(verts, faces, cam, 6, 6, spec=spec, vertex_order="gl"), want)


@pytest.mark.parametrize("size", [(64, 64), (64, 128), (128, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gl_order_guard_band_is_taken_on_the_window_coordinate(size):
    """raster_scenes.guard_scene: vertices whose window coordinate lies within three float32 steps of the coordinate on either
    side of +-16384, in x and in y.  On the inner side the vertex is valid, at +-16384 and beyond the face is clipped; ids and
    depth bits (the clipped fan has its own 1/z planes) equal the restatement's."""
    h, w = size
    verts, faces, recs = raster_scenes.guard_scene(h, w)
    cam = recs[0]
    n = len(raster_scenes.GUARD_STEPS)
    valid = [_project_f32(verts[tri[2]], cam, "gl", size) is not None for tri in faces]
    inner_first = [s < 0 for s in raster_scenes.GUARD_STEPS]       # towards +x and +y (window y -> -16384) the steps run outwards
    assert valid == inner_first + inner_first[::-1] + inner_first + inner_first[::-1]
    assert all(_clip_python([verts[i] for i in tri], cam, "gl", size) for tri, ok in zip(faces, valid) if not ok)
    want, wdep = _spec_python(verts, faces, cam, h, w, "gl", want_depth=True)
    assert len(np.unique(want)) == 4 * n and want.min() == 0       # every strip is seen
    for spec in (True, False):
        got, dep = oracle_c.raster(verts, faces, cam, h, w, want_depth=True, spec=spec, vertex_order="gl")
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(dep.view(np.int32), wdep.view(np.int32))


def test_gl_order_differs_from_r1_on_config1():
    """The two orders are two rule-sets: on a C1 view they put some vertices on neighbouring 1/256 px steps, which decides a few
    pixels (if this counted zero, every GL test here would pass with the switch ignored)."""
    (points, faces), cams = synthetic.config1_scene()
    h, w = cams[0].get_image_size(1.0)
    rec = cams[0].get_raster_record(1.0, near=0.1)
    gl = oracle_c.raster(points, faces, rec, h, w, vertex_order="gl")
    assert 0 < (gl != oracle_c.raster(points, faces, rec, h, w)).sum() < 0.001 * h * w
    assert gl.min() >= 0
