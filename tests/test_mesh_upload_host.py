"""CPU: anchors tests/upload_standin.py -- the numpy restatement of gr_mesh_upload and k_cull_blocks that
tests/test_mesh_upload_gpu.py compares the library with bit for bit -- WITHOUT the library: hand-worked uploads, containment of
every block's vertices in its sphere in exact arithmetic, and the cull against float64 geometry (conservative, and not
vacuous)."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle_c
from tests import upload_scenes as scenes
from tests import upload_standin as su

F32 = np.float32


def interleave(u0: int, u1: int) -> int:
    """bit k of u0 -> bit 2k, bit k of u1 -> bit 2k + 1, one bit at a time"""
    code = 0
    for k in range(16):
        code |= ((u0 >> k) & 1) << (2 * k) | ((u1 >> k) & 1) << (2 * k + 1)
    return code


# ---- hand-worked uploads -------------------------------------------------------------------------------------------------
def test_two_by_two_grid_morton_order_written_out():
    """Vertices (i, j, 0), i, j in 0..2; cell (i, j) holds A = (v00, v10, v11), centroid (i + 2/3, j + 1/3), and
    B = (v00, v11, v01), centroid (i + 1/3, j + 2/3).  Extents (2, 2, 0): the axes are x, y; inv = 32767.5, and the 16-bit
    coordinates of 1/3, 2/3, 4/3, 5/3 are 10922 = 0x2AAA, 21845 = 0x5555, 43690 = 0xAAAA, 54612 = 0xD554.  x takes the even
    bits, y the odd ones: the cells come in the order (0,0) (1,0) (0,1) (1,1), and in every cell A (bits x1 y0) before B."""
    verts = np.array([[i, j, 0] for j in range(3) for i in range(3)], dtype=F32)
    v = lambda i, j: 3 * j + i
    A = lambda i, j: (v(i, j), v(i + 1, j), v(i + 1, j + 1))
    B = lambda i, j: (v(i, j), v(i + 1, j + 1), v(i, j + 1))
    # the caller's order, scrambled:   0        1        2        3        4        5        6        7
    faces = np.array([B(1, 1), A(0, 1), B(0, 0), A(1, 0), A(1, 1), B(1, 0), A(0, 0), B(0, 1)], dtype=np.int32)
    up = su.upload_np(verts, faces)
    assert up["axes"] == (0, 1)
    u = {1: 0x2AAA, 2: 0x5555, 4: 0xAAAA, 5: 0xD554}   # thirds -> 16-bit coordinate
    want = {0: (4, 5), 1: (2, 4), 2: (1, 2), 3: (5, 1), 4: (5, 4), 5: (4, 2), 6: (2, 1), 7: (1, 5)}   # face -> thirds of (x, y)
    assert up["codes"].tolist() == [interleave(u[a], u[b]) for a, b in want.values()]
    assert up["orig"].tolist() == [6, 2, 3, 5, 1, 7, 4, 0]
    # one block of 8 faces over all 9 vertices, first use in soup order: A(0,0) = (0, 1, 4), B(0,0) = (0, 4, 3), A(1,0) = (1, 2, 5), ...
    assert up["counts"].tolist() == [9]
    assert [(w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24) for w in up["bidx"][:3].tolist()] == [(0, 1, 2, 8), (0, 2, 3, 8), (1, 4, 5, 8)]
    np.testing.assert_array_equal(up["bvert"][0, :6], verts[[0, 1, 4, 3, 2, 5]])
    assert np.isnan(up["bvert"][0, 9:]).all()
    # box (0,0,0) .. (2,2,0): centre (1, 1, 0), radius sqrt(2) (1.0001) + 1e-6 + 2 * 2^-23
    assert up["blk"][0, :3].tolist() == [1, 1, 0]
    assert abs(float(up["blk"][0, 3]) - (np.sqrt(2) * 1.0001 + 1e-6 + 2.0 ** -22)) < 1e-6


def test_equal_codes_keep_the_callers_order():
    verts, faces = scenes.upload_cases()["equal_centroids"]
    up = su.upload_np(verts, faces)
    assert len(set(up["codes"].tolist())) == 1
    assert up["orig"].tolist() == list(range(129))
    # two codes, interleaved in the caller's order: each group keeps its order
    verts = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [8, 0, 0], [8, 0, 0], [8, 0, 0]], dtype=F32)
    faces = np.array([[3, 4, 5], [0, 1, 2], [4, 5, 3], [1, 2, 0], [5, 3, 4], [2, 0, 1]], dtype=np.int32)
    up = su.upload_np(verts, faces)
    assert up["codes"].tolist() == [0x55555555, 0] * 3
    assert up["orig"].tolist() == [1, 3, 5, 0, 2, 4]


def test_the_fan_shares_its_hub():
    """64 faces (0, k + 1, k + 2): codes rise with k, the hub is vertex 0 of the block's list, 66 distinct vertices."""
    verts, faces = scenes.fan(64)
    up = su.upload_np(verts, faces)
    assert (np.diff(up["codes"].astype(np.int64)) > 0).all()
    assert up["orig"].tolist() == list(range(64))
    assert up["bidx"].tolist() == [0 | (k + 1) << 8 | (k + 2) << 16 | 65 << 24 for k in range(64)]
    np.testing.assert_array_equal(up["bvert"][0, :66], verts)


def test_degenerate_faces_number_a_vertex_once():
    """x = 0, 3, 6 on a line (extents (6, 0, 0): the second axis codes 0).  Centroids 1, 3, 3: faces 1 and 2 tie and keep their
    order.  (0, 0, 1) -> positions (0, 0, 1); (1, 1, 1) -> (1, 1, 1); (2, 1, 0) -> (2, 1, 0); three distinct vertices."""
    verts = np.array([[0, 0, 0], [3, 0, 0], [6, 0, 0]], dtype=F32)
    faces = np.array([[0, 0, 1], [1, 1, 1], [2, 1, 0]], dtype=np.int32)
    up = su.upload_np(verts, faces)
    assert up["axes"] == (0, 1)
    assert up["codes"].tolist() == [interleave(65535 // 6, 0), interleave(32767, 0), interleave(32767, 0)]
    assert up["orig"].tolist() == [0, 1, 2]
    assert up["bidx"].tolist() == [0 | 0 << 8 | 1 << 16 | 2 << 24, 1 | 1 << 8 | 1 << 16 | 2 << 24, 2 | 1 << 8 | 0 << 16 | 2 << 24]
    assert up["blk"][0, :3].tolist() == [3, 0, 0]
    assert 3.0003 <= float(up["blk"][0, 3]) <= 3.00031


def test_axis_choice_and_bounds_words():
    """The two swaps: extents (1,2,3) -> axes (2, 1); (3,2,1) -> (0, 1); (3,1,2) -> (0, 2); (1,3,2) -> (2, 1) -- the smallest
    extent is left out, ties keep x, y.  Bounds skip non-finite coordinates one by one, unreferenced vertices count."""
    assert su.morton_axes(np.array([1, 2, 3], dtype=F32)) == (2, 1)
    assert su.morton_axes(np.array([3, 2, 1], dtype=F32)) == (0, 1)
    assert su.morton_axes(np.array([3, 1, 2], dtype=F32)) == (0, 2)
    assert su.morton_axes(np.array([1, 3, 2], dtype=F32)) == (2, 1)
    assert su.morton_axes(np.array([2, 1, 3], dtype=F32)) == (2, 0)
    assert su.morton_axes(np.array([2, 3, 1], dtype=F32)) == (0, 1)
    assert su.morton_axes(np.array([5, 5, 5], dtype=F32)) == (0, 1)
    assert su.morton_axes(np.array([0, 0, 0], dtype=F32)) == (0, 1)
    cases = scenes.upload_cases()
    got = {su.upload_np(*cases["extents_%d%d%d" % s])["axes"] for s in [(1, 2, 3), (1, 3, 2), (2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1)]}
    assert {frozenset(a) for a in got} == {frozenset((0, 1)), frozenset((0, 2)), frozenset((1, 2))}
    verts = np.array([[np.nan, 2, -np.inf], [1, np.inf, 5], [-3, -0.0, np.nan], [np.inf, 0.0, 7]], dtype=F32)
    words = su.mesh_bounds_words(verts)
    lo, hi = su.ordered_float(words[:3]), su.ordered_float(words[3:])
    assert lo.tolist() == [-3, 0, 5] and hi.tolist() == [1, 2, 7]
    assert np.signbit(lo[1])                                    # -0 is the smaller zero
    lo, ext = su.extents(su.mesh_bounds_words(np.full((2, 3), np.nan, dtype=F32)))
    assert ext.tolist() == [0, 0, 0]                            # no finite vertex
    lo, ext = su.extents(su.mesh_bounds_words(np.array([[-3e38, 0, 0], [3e38, 0, 1]], dtype=F32)))
    assert ext.tolist() == [0, 0, 1]                            # hi - lo overflows
    assert len({su.mesh_sig(64, 40, words), su.mesh_sig(65, 40, words), su.mesh_sig(64, 41, words), su.mesh_sig(64, 40, words[::-1])}) == 4
    assert 0 < su.mesh_sig(1, 3, words) < 2 ** 64


def test_codes_of_non_finite_centroids():
    """NaN -> 0, +inf -> 65535, -inf -> 0 on the axis that carries them; an axis without extent codes 0."""
    verts = np.array([[0, 0, 0], [4, 4, 0], [np.nan, 1, 0], [np.inf, 1, 0], [-np.inf, 1, 0], [1, 1, 0]], dtype=F32)
    faces = np.array([[2, 5, 5], [3, 5, 5], [4, 5, 5], [5, 5, 5]], dtype=np.int32)
    up = su.upload_np(verts, faces)
    y = 65535 // 4   # (1 - 0) * (65535 / 4) = 16383.75
    assert up["codes"].tolist() == [interleave(0, y), interleave(65535, y), interleave(0, y), interleave(y, y)]
    assert up["orig"].tolist() == [0, 2, 3, 1]


# ---- containment in exact arithmetic ------------------------------------------------------------------------------------------
CONTAINED = ["grid_F257", "soup_F129", "fan64", "degenerate_faces", "on_a_line", "single_point", "equal_extents", "extents_123",
             "extents_312", "negative_zero", "stride_loop_V32833"]
OFFSETS = [0.0, 1e3, 1e4, 1e5]


def _outside(verts, faces, up):
    """The (block, vertex) pairs whose vertex lies farther from the block's centre than its radius, in exact arithmetic."""
    bad = []
    for b in range(up["blk"].shape[0]):
        c, r = [Fraction(float(x)) for x in up["blk"][b, :3]], Fraction(float(up["blk"][b, 3]))
        members = up["orig"][b * 64:(b + 1) * 64]
        for g in np.unique(faces[members]):
            if sum((Fraction(float(x)) - cd) ** 2 for x, cd in zip(verts[g], c)) > r * r:
                bad.append((b, int(g)))
    return bad


def _moved(verts, offset):
    out = np.asarray(verts, dtype=np.float64).copy()
    out[:, :2] += offset
    return out.astype(F32)


@pytest.mark.parametrize("offset", OFFSETS)
def test_every_vertex_lies_within_the_radius_of_the_stored_centre(offset):
    cases = scenes.upload_cases()
    for name in CONTAINED:
        verts, faces = cases[name]
        verts = _moved(verts, offset)
        assert np.isfinite(verts[np.unique(faces)]).all()
        assert _outside(verts, faces, su.upload_np(verts, faces)) == [], name
    one = np.array([[0, 1, 2]], dtype=np.int32)
    for k, (verts, _cam) in enumerate(scenes.sliver_scene(60, offset)):
        assert _outside(verts, one, su.upload_np(verts, one)) == [], f"sliver {k}"


def test_without_the_centre_term_slivers_at_1e5_stick_out():
    """What the term in k_block_bounds is for: the radius 1.0001 r + 1e-6 alone holds every fixture up to 1e4, and at 1e5 every
    compact block, but not the blocks that are thin on two axes -- the centre is rounded by up to 2^-8 (3.9 mm) there."""
    cases = scenes.upload_cases()
    one = np.array([[0, 1, 2]], dtype=np.int32)
    for name in ("grid_F257", "soup_F129"):
        verts = _moved(cases[name][0], 1e5)
        assert _outside(verts, cases[name][1], su.upload_np(verts, cases[name][1], centre_slack=False)) == []
    out = [bool(_outside(verts, one, su.upload_np(verts, one, centre_slack=False))) for verts, _cam in scenes.sliver_scene(60, 1e5)]
    assert sum(out) >= len(out) // 4
    verts, faces = _moved(cases["on_a_line"][0], 1e5), cases["on_a_line"][1]
    assert _outside(verts, faces, su.upload_np(verts, faces, centre_slack=False)) != []


# ---- the cull against float64 ----------------------------------------------------------------------------------------------
def _random_blocks(n, seed):
    """n blocks of six points within 100 units of the origin: (points (n, 6, 3) float32, spheres (n, 4) float32)"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-60, 60, (n, 1, 3))
    radii = 10 ** rng.uniform(-2, 1.3, (n, 1, 1))
    pts = (centres + radii * rng.uniform(-1, 1, (n, 6, 3))).astype(F32)
    blk = np.stack([su.block_sphere(su.fmin_all(p, axis=0), su.fmax_all(p, axis=0)) for p in pts])
    return pts, blk


@pytest.mark.parametrize("k", range(6))
def test_standin_cull_is_conservative_and_not_vacuous(k):
    cam, h, w = scenes.fixture_cameras()[k]
    pts, blk = _random_blocks(3000, 100 + k)
    # half of the blocks are moved in front of the camera, so that every camera sees some
    q_front = np.random.default_rng(k).uniform([-1, -1, 0.2], [1, 1, 40], (1500, 3)) * [w / cam[12], h / cam[12], 1]
    q_front[:, :2] *= q_front[:, 2:]
    shift = (cam[9:12].astype(np.float64) + q_front @ cam[:9].reshape(3, 3).astype(np.float64).T) - blk[:1500, :3]
    pts[:1500] = (pts[:1500] + shift[:, None, :]).astype(F32)
    pts = pts[np.abs(pts).max(axis=(1, 2)) <= 100]
    blk = np.stack([su.block_sphere(su.fmin_all(p, axis=0), su.fmax_all(p, axis=0)) for p in pts])
    keep = su.cull_np(blk, cam, h, w)
    # (a) a vertex in front of the near plane that projects at least 2 px inside the window: the block is kept
    q = scenes.camera_space64(cam, pts)
    f, cx, cy, near = (float(x) for x in cam[12:16])
    with np.errstate(all="ignore"):
        sx, sy = cx + f * q[..., 0] / q[..., 2], cy + f * q[..., 1] / q[..., 2]
    seen = ((q[..., 2] > near) & (sx >= 2) & (sx <= w - 2) & (sy >= 2) & (sy <= h - 2)).any(axis=1)
    if min(h, w) > 4:
        assert seen.sum() >= 30
        assert keep[seen].all()
    # (b) a sphere beyond one of the five planes by more than 1.002 r + 1e-5 is rejected.  The cull measures the distance with
    # the normal's 1-norm |f| + |m| (no square root, conservative): in Euclidean terms the threshold grows by
    # (|f| + |m|) / hypot(f, m) in [1, sqrt 2], which is 1 for the near plane.
    planes = scenes.planes64(cam, h, w)
    qc = scenes.camera_space64(cam, blk[:, :3])
    n2 = np.linalg.norm(planes[:, :3], axis=1)
    dist = (qc @ planes[:, :3].T + planes[:, 3]) / n2
    factor = np.abs(planes[:, :3]).sum(axis=1) / n2
    assert factor[0] == 1 and (factor >= 1).all() and (factor <= np.sqrt(2) + 1e-12).all()
    far_out = (dist < -factor * (1.002 * blk[:, 3:].astype(np.float64) + 1e-5)).any(axis=1)
    assert far_out.sum() >= 100
    assert not keep[far_out].any()
    assert not (seen & far_out).any()
    for p in range(5):   # every plane rejects something on its own
        assert (dist[:, p] < -factor[p] * (1.002 * blk[:, 3] + 1e-5)).sum() >= 5, p


def test_standin_cull_keeps_non_finite_spheres():
    cam, h, w = scenes.fixture_cameras()[0]
    for sphere in ([np.nan, 0, 0, 1], [0, 0, 0, np.nan], [np.inf, 0, 0, np.inf], [0, 0, -50, np.inf], [np.nan, np.nan, np.nan, np.inf],
                   [-np.inf, np.inf, 0, np.nan]):
        assert su.cull_np(np.array([sphere], dtype=F32), cam, h, w).tolist() == [True], sphere
    assert su.cull_np(np.array([[0, 0, -50, 1]], dtype=F32), cam, h, w).tolist() == [False]   # behind this camera
    # a block with a NaN and an infinite vertex: NaN is dropped from the box, the infinite one makes the radius infinite
    pts = np.array([[1, 2, 3], [np.nan, 2, 3], [1, np.inf, 3], [2, 2, 2]], dtype=F32)
    s = su.block_sphere(su.fmin_all(pts, axis=0), su.fmax_all(pts, axis=0))
    assert s[0] == 1.5 and np.isinf(s[1]) and s[2] == 2.5 and np.isinf(s[3])
    s = su.block_sphere(su.fmin_all(pts[:2], axis=0), su.fmax_all(pts[:2], axis=0))
    assert s[:3].tolist() == [1, 2, 3] and 0 < s[3] < 1e-5


# ---- the sliver scene has teeth ----------------------------------------------------------------------------------------------
def test_sliver_scene_shows_faces_the_old_radius_would_have_culled():
    """The oracle draws pixels of slivers whose sphere, without the centre term, k_cull_blocks rejects; with it, every sliver
    the oracle draws is kept."""
    one = np.array([[0, 1, 2]], dtype=np.int32)
    dropped = shown = 0
    for verts, cam in scenes.sliver_scene():
        visible = (oracle_c.raster(verts, one, cam, scenes.SLIVER_H, scenes.SLIVER_W) >= 0).any()
        shown += int(visible)
        if visible:
            assert su.cull_np(su.upload_np(verts, one)["blk"], cam, scenes.SLIVER_H, scenes.SLIVER_W).all()
            dropped += int(not su.cull_np(su.upload_np(verts, one, centre_slack=False)["blk"], cam, scenes.SLIVER_H, scenes.SLIVER_W).all())
    assert shown >= 120 and dropped >= 8, (shown, dropped)
