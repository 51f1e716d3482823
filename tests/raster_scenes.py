"""tests/raster_scenes.py -- scene builders shared by the raster tests: tests/test_hip_parity.py runs them under rule R1,
tests/test_gl_order_edges.py under R1-GL (GR_OPT_VERTEX_ORDER = 1), tests/test_oracle_raster.py runs the tie and guard scenes
through the Python restatement of the rule-set.  Builders only: what a test asserts stays in the test."""
import numpy as np

from geograypher_amd.utils import synthetic


def pinhole_record(h, w, f, near=0.05):
    """Identity rotation, camera at the origin, principal point at the window centre: q = p, (x, y, z) -> (f x / z + w / 2,
    f y / z + h / 2)."""
    rec = np.zeros((1, 16), dtype=np.float32)
    rec[0, [0, 4, 8]] = 1.0
    rec[0, 12], rec[0, 13], rec[0, 14], rec[0, 15] = f, 0.5 * w, 0.5 * h, near
    return rec


# ---- R1-GL: rounding ties and the guard band (f = 32, q_z = 1, even sizes: every operation of the vertex stage is exact) --------
TIE_F = 32.0


def tie_x(k, w):
    """The camera-space x (at q_z = 1, f = 32, width w) whose GL window coordinate has 256 (win - 0.5) = k + 0.5 exactly:
    win = 32 x + w / 2.  R1 snaps it to X = k + 129 always, R1-GL to k + 128 for even k and k + 129 for odd k."""
    return (k + 0.5 - 128.0 * w + 128.0) / 8192.0


def tie_y(m, h):
    """The same in y: win = h / 2 - 32 y (GL rows run bottom-up), 256 (win - 0.5) = m + 0.5 exactly, Y = 256 h - 128 - fixed:
    R1 gives Y = 256 h - 128 - m always, R1-GL the same for even m and one less for odd m."""
    return (128.0 * h - 128.0 - (m + 0.5)) / 8192.0


def tie_scene(h=64, w=64):
    """Triangles whose vertices are rounding ties of the R1-GL snap (tie_x / tie_y).  Vertex (j, i, even) below lands EXACTLY on
    the centre of pixel (row i, column j) under round-half-to-even; with even = True (k, m even) floor(x + 0.5) puts it one
    1/256 px step beside it (right and up), with even = False (k, m odd) both roundings agree.  Edges between such vertices run
    through pixel centres under the one rounding and beside them under the other: left (owning) and right vertical edges, top and
    bottom horizontal ones, diagonals, in all four quadrants of the window; the last two faces leave the image to the left and
    the top (negative window x, window y above h) and to the right and the bottom (negative window y).
    Returns (points float32 (V, 3), faces int32 (F, 3), camera records (1, 16))."""
    assert h % 2 == 0 and w % 2 == 0 and h >= 64 and w >= 64

    def vtx(j, i, even=True):
        k = 256 * j - (0 if even else 1)
        m = 256 * (h - 1 - i) - (0 if even else 1)
        return [tie_x(k, w), tie_y(m, h), 1.0]

    J, I = w - 64, h - 64      # offsets of the right / lower quadrants
    tris = [
        # upper left quadrant: a vertical LEFT edge through the centres of column 5 (owned: covered under half-even only)
        [vtx(5, 3), vtx(5, 27), vtx(25, 14, even=False)],
        # upper right quadrant: a vertical RIGHT edge through the centres of column 58 (not owned: covered under floor only)
        [vtx(J + 58, 4), vtx(J + 58, 28), vtx(J + 36, 15, even=False)],
        # lower left quadrant: horizontal edges through the centres of rows 36 (top) and 60 (bottom)
        [vtx(4, I + 36), vtx(28, I + 36), vtx(15, I + 50, even=False)],
        [vtx(3, I + 60), vtx(29, I + 60), vtx(17, I + 52, even=False)],
        # lower right quadrant: both diagonals through pixel centres, one odd-k vertex each
        [vtx(J + 36, I + 36), vtx(J + 60, I + 60), vtx(J + 36, I + 60, even=False)],
        [vtx(J + 60, I + 34), vtx(J + 38, I + 56), vtx(J + 60, I + 56)],
        # all vertices odd: the two roundings agree (and equal R1)
        [vtx(30, 30, even=False), vtx(34, 30, even=False), vtx(32, 34, even=False)],
        # leaving the image to the left and the top: a vertex on the centre of pixel (row -3, column -4), negative window x
        [vtx(-4, -3), vtx(20, 21), vtx(-4, 21)],
        # leaving it to the right and the bottom: negative window y
        [vtx(w + 3, h + 2), vtx(w - 21, h - 22), vtx(w + 3, h - 22)],
    ]
    points = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(points.astype(np.float32).astype(np.float64), points)      # dyadic: exact in float32
    faces = np.arange(points.shape[0], dtype=np.int32).reshape(-1, 3)
    return points.astype(np.float32), faces, pinhole_record(h, w, TIE_F)


GUARD_STEPS = (-3, -2, -1, 0, 1, 2, 3)


def _stepped(x, steps):
    x = np.float32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, np.float32(np.inf if steps > 0 else -np.inf), dtype=np.float32)
    return float(x)


def guard_scene(h=64, w=64):
    """Faces with one vertex (at q_z = 1) whose GL window coordinate lies within three float32 steps of the coordinate on either
    side of +-16384 px, in x and in y: win_x = 32 x + w / 2 is exactly +-16384 at step 0 (invalid: the guard is |win| < 16384),
    valid on the inner side, invalid on the outer one, where the face is clipped (R7).  The other two vertices lie just outside the
    opposite image border at another depth, so every face is a strip across the image with a sloped 1/z plane: which of the two
    paths a face took shows in its depth bits.  Strips towards +-x lie behind (z = 1.25) and are seen in the right half of the
    image, strips towards +-y in front (z = 0.8) cover the left half.
    Returns (points float32, faces int32, camera records (1, 16))."""
    ax, ay = 0.5 * w / TIE_F, 0.5 * h / TIE_F        # the image spans |x| <= ax, |y| <= ay at q_z = 1
    n = len(GUARD_STEPS)
    tris = []
    for sign in (1.0, -1.0):                          # towards +x, then -x: horizontal strips, upper / lower half
        x0 = (sign * 16384.0 - 0.5 * w) / TIE_F
        for s, step in enumerate(GUARD_STEPS):
            y_lo = (-ay if sign > 0 else 0.0) + ay * s / n
            y_hi = y_lo + ay / n
            zb = 1.25
            tris.append([[-sign * 1.1 * ax * zb, y_lo * zb, zb], [-sign * 1.1 * ax * zb, y_hi * zb, zb],
                         [_stepped(x0, step), 0.5 * (y_lo + y_hi), 1.0]])
    for sign in (1.0, -1.0):                          # towards +y (window y -16384), then -y: vertical strips in the left half
        y0 = (0.5 * h + sign * 16384.0) / TIE_F       # win_y = h / 2 - 32 y = -+16384
        for s, step in enumerate(GUARD_STEPS):
            x_lo = (-ax if sign > 0 else -0.5 * ax) + 0.5 * ax * s / n
            x_hi = x_lo + 0.5 * ax / n
            zb = 0.8
            tris.append([[x_lo * zb, -sign * 1.1 * ay * zb, zb], [x_hi * zb, -sign * 1.1 * ay * zb, zb],
                         [0.5 * (x_lo + x_hi), _stepped(y0, step), 1.0]])
    points = np.asarray(tris, dtype=np.float32).reshape(-1, 3)
    faces = np.arange(points.shape[0], dtype=np.int32).reshape(-1, 3)
    return points, faces, pinhole_record(h, w, TIE_F)


FMA_NDC = float.fromhex("-0x1.53fffap-3")


def fma_scene():
    """A 6 x 6 window with f = 3 (P = (1, -1), size / 2 = 3, q_z = 1: ndc = (x, -y) exactly) and the coordinate FMA_NDC, found by
    a search with the Python restatement: the exact value of ndc * 3 + 3 lies between two float32 neighbours such that the fused
    multiply-add gives 256 (win - 0.5) just above 512.5 (fixed = 513) and a product rounded on its own gives 512.5 exactly
    (a tie: fixed = 512).  Face 0 has a vertical left edge on that x -- through the centres of column 2 when unfused, one step to
    the right of them when fused --, face 1 a horizontal edge on the same value in y (row 3).
    Returns (points float32, faces int32, camera records (1, 16))."""
    c = FMA_NDC
    tris = [[[c, -0.9, 1.0], [c, 0.1, 1.0], [0.9, -0.4, 1.0]],
            [[-0.9, -c, 1.0], [0.2, -c, 1.0], [-0.3, 0.9, 1.0]]]
    points = np.asarray(tris, dtype=np.float32).reshape(-1, 3)
    assert float(points[0, 0]) == c
    return points, np.arange(6, dtype=np.int32).reshape(2, 3), pinhole_record(6, 6, 3.0)


# ---- the scenes of tests/test_hip_parity.py ---------------------------------------------------------------------------------------
def boundary_93_scene():
    """Triangles of every size from 1 to 130 px centred on the corners of the 64 x 32 tiles (all three extra slots), on vertical and
    on horizontal tile borders, at many orientations and depths, overlapping.  Returns (points, faces, records, h, w)."""
    rng = np.random.default_rng(93)
    h, w, f = 448, 640, 500.0
    pts, fcs = [], []
    k = 0
    for size in list(range(1, 20)) + list(range(20, 131, 3)) + [91, 92, 93, 94, 95]:
        for rep in range(3):
            cx = 64.0 * rng.integers(1, 9) + (rng.random() - 0.5) * (0.0 if rep == 0 else 0.4 * size)
            cy = 32.0 * rng.integers(1, 13) + (rng.random() - 0.5) * (0.0 if rep == 1 else 0.4 * size)
            ang = rng.random(3) * 0.6 + np.array([0.0, 2.1, 4.2]) + rng.random() * 6.28
            r = 0.5 * size * (0.6 + 0.4 * rng.random(3))
            z = 8.0 + 4.0 * rng.random(3)      # camera-space depth of each corner: tilted faces, overlapping in depth
            px = cx + r * np.cos(ang) * (1.6 if rep == 2 else 1.0)
            py = cy + r * np.sin(ang) * (0.4 if rep == 2 else 1.0)
            for i in range(3):     # pinhole at the origin looking down -z ... the record maps (x, y, z) -> (f x / z + cx0, f y / z + cy0)
                pts.append([(px[i] - 0.5 * w) * z[i] / f, (py[i] - 0.5 * h) * z[i] / f, z[i]])
            fcs.append([k, k + 1, k + 2])
            k += 3
    points = np.asarray(pts, dtype=np.float64)
    faces = np.asarray(fcs, dtype=np.int64)
    return points, faces, pinhole_record(h, w, f), h, w      # identity rotation, camera at the origin: q = p


def broken_vertices_scene(points, faces):
    """Three faces with a NaN, a +inf and a -inf vertex appended to a mesh."""
    broken = np.vstack([points, [[np.nan, 0.0, 0.0], [np.inf, 1.0, 2.0], [0.0, -np.inf, 0.0]]])
    extra = np.array([[0, 1, len(points)], [2, len(points) + 1, 3], [len(points) + 2, 4, 5]], dtype=faces.dtype)
    return broken, np.vstack([faces, extra])


def ragged_cameras(width=613, height=457):
    """C1 with photos of a size that is no multiple of the tile.  Returns ((points, faces), cams)."""
    (points, faces), cams = synthetic.config1_scene()
    for c in cams.cameras:
        c.image_width, c.image_height, c.image_size = width, height, (height, width)
    return (points, faces), cams


def tile_sized_faces_scene(pitch):
    """A grid of faces about `pitch` tile widths large under two cameras of 900 x 1600.  Returns (points, faces, cams)."""
    nx, ny = 24, 24
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    rng = np.random.default_rng(int(pitch * 10))
    z = rng.uniform(0.0, 0.4, xs.shape)
    f = 300.0
    height = 30.0
    step = pitch * 64.0 * height / f  # world size of a cell that projects to `pitch` tile widths
    points = np.stack([(xs - nx / 2) * step + 0.013, (ys - ny / 2) * step * 0.5 + 0.007, z], axis=-1).reshape(-1, 3)
    idx = lambda i, j: j * (nx + 1) + i
    faces = np.array([[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for j in range(ny) for i in range(nx)] +
                     [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for j in range(ny) for i in range(nx)])
    poses = [synthetic.nadir_pose(0.0, 0.0, height), synthetic.nadir_pose(3.0, -2.0, height, yaw_deg=23.0)]
    cams = synthetic.camera_set_from_poses(poses, f=f, width=1600, height=900)
    return points, faces, cams


def degenerate_soup_scene(seed, n=3000):
    """Random overlapping triangles of every size; faces behind and across the camera plane, zero-area and coincident faces; two
    cameras of 251 x 333.  Returns (points, faces, cams)."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-30, 30, (n, 1, 3)) * np.array([1, 1, 0.3])
    size = np.exp(rng.uniform(np.log(0.02), np.log(40.0), (n, 1, 1)))
    tri = centers + rng.normal(0, 1, (n, 3, 3)) * size
    tri[:50, :, 2] = 45.0                       # behind the camera (camera at z = 40 looking down)
    tri[50:100, 0, 2] = 45.0                    # straddling the camera plane -> clipped at the near plane (R7)
    tri[100:120, 2] = tri[100:120, 1]           # zero area
    tri[120:140] = tri[140:160]                 # coincident faces: lower id wins
    points = tri.reshape(-1, 3)
    faces = np.arange(3 * n).reshape(n, 3)
    poses = [synthetic.nadir_pose(0, 0, 40.0, yaw_deg=17.0 * seed, tilt_x_deg=3.0 * seed),
             synthetic.look_at((60, 10, 25), (0, 0, 0), up_hint=(0, 0, 1))]
    cams = synthetic.camera_set_from_poses(poses, f=300.0, width=333, height=251)
    return points, faces, cams


def ground_plane_scene():
    """Two 1 km triangles seen from 2 m above them, looking at the horizon (240 x 320).  Returns (points, faces, cams)."""
    pts = np.array([[-500, -500, 0], [500, -500, 0], [500, 500, 0], [-500, 500, 0]], dtype=np.float64)
    quad = np.array([[0, 1, 2], [0, 2, 3]])
    pose = synthetic.look_at((0.0, 0.0, 2.0), (0.0, 100.0, 2.0), up_hint=(0, 0, 1))
    cams = synthetic.camera_set_from_poses([pose], f=300.0, width=320, height=240)
    return pts, quad, cams


def cameras_inside_terrain():
    """C1's mesh with two cameras in the middle of it and one whose near plane cuts it obliquely (251 x 333).
    Returns (points, faces, cams)."""
    (points, faces), _ = synthetic.config1_scene()
    poses = [synthetic.look_at((1.0, 2.0, 0.9), (30.0, 20.0, 0.0), up_hint=(0, 0, 1)),
             synthetic.look_at((-3.0, 0.5, 0.7), (0.0, 40.0, 5.0), up_hint=(0, 0, 1)),
             synthetic.nadir_pose(0.0, 0.0, 0.8, tilt_x_deg=70.0)]
    cams = synthetic.camera_set_from_poses(poses, f=250.0, width=333, height=251)
    return points, faces, cams


STRESS_SIZES = [(1, 1), (3, 70), (65, 33), (64, 64), (97, 131), (200, 257)]


def _full_size(n, image_scale):
    """The smallest photo size N with int(N * image_scale) == n (the truncation of get_image_size)."""
    N = int(n / image_scale)
    while int(N * image_scale) < n:
        N += 1
    assert int(N * image_scale) == n
    return N


def random_stress_scene(seed, size=None, principal_point=None, image_scale=1.0):
    """The randomised scene of test_random_stress: lattices with exact ties, soups with faces far larger than the image, cameras
    inside the scene.  `size` (h, w) and `principal_point` override what the seed would draw (the R1-GL tests need "center"); with
    `image_scale` the photos are larger and (h, w) is the size they are rendered at (f_eff = f h / H, no dyadic number).
    Returns (points, faces, records, h, w)."""
    rng = np.random.default_rng(1000 + seed)
    h, w = STRESS_SIZES[seed % 6] if size is None else size
    n = [50, 400, 3000, 9000][seed % 4]
    if seed % 3 == 0:  # axis-aligned lattice of small quads plus noise-free coordinates -> exact ties and A/B == 0
        g = int(np.sqrt(n / 2)) + 1
        xs, ys = np.meshgrid(np.linspace(-3, 3, g + 1), np.linspace(-3, 3, g + 1))
        points = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1)
        faces = synthetic.grid_faces(g + 1, g + 1)
    else:
        centers = rng.uniform(-4, 4, (n, 1, 3)) * np.array([1, 1, 0.2])
        size_ = np.exp(rng.uniform(np.log(0.01), np.log(30.0 if seed % 2 else 0.3), (n, 1, 1)))
        points = (centers + rng.normal(0, 1, (n, 3, 3)) * size_).reshape(-1, 3)
        faces = np.arange(3 * n).reshape(n, 3)
    z_cam = [6.0, 1.0, 0.05][seed % 3]  # the last one sits inside the scene's bounding box
    poses = [synthetic.nadir_pose(rng.uniform(-1, 1), rng.uniform(-1, 1), z_cam, yaw_deg=rng.uniform(0, 360),
                                  tilt_x_deg=rng.uniform(-20, 20), tilt_y_deg=rng.uniform(-20, 20)) for _ in range(3)]
    H, W = _full_size(h, image_scale), _full_size(w, image_scale)
    cams = synthetic.camera_set_from_poses(poses, f=float(max(H, W)) * rng.uniform(0.3, 2.0), width=W, height=H)
    assert cams[0].get_image_size(image_scale) == (h, w)
    for c in cams.cameras:
        c.cx, c.cy = rng.uniform(-5, 5), rng.uniform(-5, 5)
    if principal_point is None:
        principal_point = "intrinsics" if seed % 2 else "center"
    recs = cams.get_raster_records(image_scale, near=0.02, principal_point=principal_point)
    return points, faces, recs, h, w


def many_views_scene(n_views=70):
    """C1's mesh under more views than one launch group holds (200 x 320).  Returns (points, faces, cams)."""
    (points, faces), _ = synthetic.config1_scene()
    poses = [synthetic.nadir_pose(3.0 * k - 30, 2.0 * k - 20, 35.0 + k, yaw_deg=11.0 * k) for k in range(n_views)]
    cams = synthetic.camera_set_from_poses(poses, f=260.0, width=320, height=200)
    return points, faces, cams
