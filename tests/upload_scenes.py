"""TEST INFRASTRUCTURE ONLY: the meshes, cameras and sliver blocks shared by tests/test_mesh_upload_host.py and
tests/test_mesh_upload_gpu.py.  Everything is float32 / int32 as the library takes it, and seeded."""
import numpy as np

F32 = np.float32


# ---- meshes ----------------------------------------------------------------------------------------------------------
def grid(nx: int, ny: int, spacing: float = 1.0, relief: float = 0.25, seed: int = 1):
    """A manifold nx x ny grid of quads cut into 2 nx ny triangles, row by row, with a little relief."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    verts = np.stack([ii * spacing, jj * spacing, relief * rng.standard_normal(ii.shape)], axis=-1).reshape(-1, 3)
    v00 = (jj[:-1, :-1] * (nx + 1) + ii[:-1, :-1]).reshape(-1)
    v10, v01, v11 = v00 + 1, v00 + nx + 1, v00 + nx + 2
    faces = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], axis=1).reshape(-1, 3)
    return verts.astype(F32), faces.astype(np.int32)


def grid_faces(F: int, seed: int = 1):
    """The first F faces of a grid that has at least F (its other vertices stay, unreferenced)."""
    n = 1
    while 2 * n * n < F:
        n += 1
    verts, faces = grid(n, n, seed=seed)
    return verts, faces[:F].copy()


def soup(F: int, scale=(10.0, 10.0, 10.0), size: float = 0.5, seed: int = 2):
    """F triangles with three vertices of their own each."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (F, 1, 3)) * np.asarray(scale)
    verts = (centres + size * rng.standard_normal((F, 3, 3))).reshape(-1, 3)
    return verts.astype(F32), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def fan(n: int = 64):
    """n faces (0, k + 1, k + 2) around vertex 0, the rim rising along x: their codes rise with k, so orig is the identity."""
    verts = np.zeros((n + 2, 3), dtype=F32)
    verts[1:, 0] = np.arange(n + 1)
    verts[1:, 1] = 1.0
    faces = np.stack([np.zeros(n, dtype=np.int32), np.arange(1, n + 1), np.arange(2, n + 2)], axis=-1)
    return verts, faces.astype(np.int32)


def upload_cases():
    """{name: (verts, faces)}: every mesh the upload is pinned at (the issue's list)."""
    rng = np.random.default_rng(7)
    cases = {}
    for F in (1, 2, 63, 64, 65, 128, 129, 257):
        cases[f"grid_F{F}"] = grid_faces(F)
        cases[f"soup_F{F}"] = soup(F)
    cases["fan64"] = fan(64)
    v, f = grid_faces(65)
    f = f.copy()
    f[3] = (f[3, 0], f[3, 0], f[3, 1])                       # (a, a, b)
    f[40] = (f[40, 2], f[40, 2], f[40, 2])                   # (a, a, a)
    f[64] = (f[64, 1], f[64, 0], f[64, 0])                   # (b, a, a), alone in the second block
    cases["degenerate_faces"] = (v, f)
    v, f = grid_faces(64)
    cases["duplicated_faces"] = (v, np.concatenate([f, f[::-1]]).astype(np.int32))
    v, f = grid_faces(257)
    cases["shuffled_order"] = (v, f[rng.permutation(257)])
    tri = np.array([[1, 2, 3], [4, 6, 5], [7, 7, 9]], dtype=F32)
    cases["equal_centroids"] = (np.tile(tri, (129, 1)), np.arange(387, dtype=np.int32).reshape(129, 3))
    line = np.zeros((67, 3), dtype=F32)
    line[:, 0], line[:, 1], line[:, 2] = np.arange(67) * 0.37, 5.0, -2.0
    cases["on_a_line"] = (line, np.stack([np.arange(65), np.arange(1, 66), np.arange(2, 67)], -1).astype(np.int32)[rng.permutation(65)])
    cases["single_point"] = (np.full((3, 3), 4.25, dtype=F32), np.array([[0, 1, 2], [2, 1, 0]], dtype=np.int32))
    v, f = soup(129, scale=(1, 1, 1), size=0.02, seed=3)
    cube = np.array([[0, 0, 0], [1, 1, 1]], dtype=F32)
    cases["equal_extents"] = (np.concatenate([np.clip(v, 0, 1), cube]), f)
    for k, scale in enumerate([(1, 2, 3), (1, 3, 2), (2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1)]):
        cases["extents_%d%d%d" % scale] = soup(129, scale=scale, size=0.01, seed=10 + k)
    v, f = grid_faces(129)
    cases["unreferenced_stretch"] = (np.concatenate([v, np.array([[-50, 3, 900], [4, 700, -900]], dtype=F32)]), f)
    cases["unreferenced_nonfinite"] = (np.concatenate([v, np.array([[np.nan, np.inf, -np.inf], [np.inf, 1, np.nan], [-np.inf, np.nan, 2]],
                                                                   dtype=F32)]), f)
    for name, bad in (("nan", np.nan), ("posinf", np.inf), ("neginf", -np.inf)):
        v2 = v.copy()
        v2[f[5, 0], 0] = bad
        v2[f[70, 1], 1] = bad
        v2[f[100, 2], 2] = bad
        cases[f"referenced_{name}"] = (v2, f)
    v2 = v.copy()
    v2[f[5, 0]], v2[f[70, 1], 2], v2[f[100, 2], 1] = np.nan, np.inf, -np.inf
    cases["referenced_mixed_nonfinite"] = (v2, f)
    v2, f2 = soup(65, scale=(4, 4, 0), size=0.3, seed=5)
    v2[:, :2] -= 2.0
    v2[::5, 2], v2[1::5, 2], v2[2::7, 0], v2[3::7, 0] = -0.0, 0.0, -0.0, 0.0
    cases["negative_zero"] = (v2, f2)
    V = 128 * 256 + 65
    big = (rng.uniform(-30, 30, (V, 3))).astype(F32)
    fb = rng.integers(0, V, (65, 3)).astype(np.int32)
    fb[0], fb[1] = (V - 1, 0, V - 2), (128 * 256, 128 * 256 - 1, 128 * 256 + 1)
    cases["stride_loop_V32833"] = (big, fb)
    return cases


# ---- cameras -----------------------------------------------------------------------------------------------------------
def rotation(yaw: float, pitch: float, roll: float) -> np.ndarray:
    """cam_to_world: the columns are the image's x axis, its y axis and the viewing direction, in world coordinates."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Ry @ Rx @ Rz


def camera(R, t, f, cx, cy, near=0.1) -> np.ndarray:
    """The 16-float camera record (include/geograster.h), float32."""
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3), [f, cx, cy, near]]).astype(F32)


def camera_space64(cam, p) -> np.ndarray:
    """q = R^T (p - t) in float64 from the float32 record: (..., 3)"""
    cam = np.asarray(cam, dtype=np.float64)
    return (np.asarray(p, dtype=np.float64) - cam[9:12]) @ cam[:9].reshape(3, 3)


def planes64(cam, h: int, w: int):
    """The five planes of the cull in camera space, float64, with their 2-pixel margin: rows (a, b, c, d), a point q is inside
    where a qx + b qy + c qz + d >= 0.  Near, left, right, top, bottom."""
    cam = np.asarray(cam, dtype=np.float64)
    f, cx, cy, near = cam[12:16]
    return np.array([[0, 0, 1, -near], [f, 0, cx + 2, 0], [-f, 0, w - cx + 2, 0], [0, f, cy + 2, 0], [0, -f, h - cy + 2, 0]])


def fixture_cameras():
    """[(cam16, h, w)]: principal point inside, left of 0 and right of w; rolled and tilted; 1 x 1 and 613 x 457 windows."""
    out = []
    for k, (yaw, pitch, roll, f, cx, cy, h, w) in enumerate([
            (0.0, 0.0, 0.0, 4000.0, 320.0, 240.0, 480, 640),
            (0.4, -0.3, 0.0, 800.0, 306.5, 228.5, 457, 613),
            (2.5, 0.7, 1.1, 300.0, -40.0, 20.0, 48, 64),
            (-1.2, 0.2, -2.0, 300.0, 90.0, 70.0, 48, 64),
            (3.0, -1.0, 0.5, 50.0, 0.5, 0.5, 1, 1),
            (0.1, 1.4, 3.0, 1200.0, 100.0, -300.0, 457, 613)]):
        t = np.array([3.0 * k - 7, 5 - 2.0 * k, 1.5 * k])
        out.append((camera(rotation(yaw, pitch, roll), t, f, cx, cy, near=0.1 + 0.3 * k), h, w))
    return out


# ---- slivers -------------------------------------------------------------------------------------------------------------
SLIVER_H, SLIVER_W, SLIVER_F = 480, 640, 4000.0
ULP_1E5 = 2.0 ** -7   # of a float32 at 1e5


def sliver_scene(n_per_edge: int = 40, offset: float = 1e5, seed: int = 11):
    """[(verts (3, 3) float32, cam16)]: one-face meshes (one block each) at x, y = `offset`, in the plane y = const, 2 .. 20 cm
    long on x and 0.5 .. 4 mm wide on z, seen from 0.5 m along +y through a 640 x 480 window at f = 4000 (8 px per mm), so
    that one END of the sliver reaches 3 .. 24 px into the window across one of its four edges (the image's x axis is the
    world's x axis for the left and right edge, its y axis for the top and bottom edge) and the rest lies outside.  The
    block's box is thin on y and z: nothing but the radius' own slack covers the rounding of the centre's x."""
    rng = np.random.default_rng(seed)
    out = []
    for edge in range(4):   # left, right, top, bottom
        for _ in range(n_per_edge):
            steps = int(rng.integers(3, 26))                       # length in ulps of x (odd: lo + hi is rounded)
            steps += 1 - steps % 2
            x0 = offset + ULP_1E5 * int(rng.integers(-2000, 2000))
            length, width = steps * ULP_1E5, rng.uniform(0.0005, 0.004)
            y0, z0 = offset + ULP_1E5 * int(rng.integers(-2000, 2000)), rng.uniform(-1, 1)
            low_edge = edge in (0, 2)                              # the window's edge at coordinate 0
            x_in, x_out = (x0 + length, x0) if low_edge else (x0, x0 + length)   # the blunt end points into the window
            verts = np.array([[x_in, y0, z0], [x_in, y0, z0 + width], [x_out, y0, z0 + 0.5 * width]]).astype(F32)
            reach = rng.uniform(3, 24)                             # pixels of the sliver inside the window
            along = edge >= 2                                      # the sliver runs along the image's y axis
            size = SLIVER_H if along else SLIVER_W
            per_m = SLIVER_F / 0.5                                 # pixels per metre at 0.5 m
            # The camera stands on the float32 lattice (62.5 px a step), about half a window from the sliver's inner end; the
            # principal point takes the rest, so that the end lies `reach` pixels inside the edge.
            x_end = float(verts[0, 0])
            cam_x = float(F32(x_end + (0.5 * size / per_m if low_edge else -0.5 * size / per_m)))
            pp = (reach if low_edge else size - reach) - per_m * (x_end - cam_x)
            if along:   # image y = world x, image x = world z  (columns: x axis, y axis, viewing direction)
                R = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float64)
                cxy = (SLIVER_W / 2, pp)
            else:       # image x = world x, image y = -world z
                R = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float64)
                cxy = (pp, SLIVER_H / 2)
            out.append((verts, camera(R, [cam_x, y0 - 0.5, z0], SLIVER_F, cxy[0], cxy[1], near=0.01)))
    return out
