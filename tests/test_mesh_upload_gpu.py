"""-m gpu: what gr_mesh_upload leaves behind (read back with gr_debug_read_upload) and what k_cull_blocks decides (seen in
`last_stats["blocks"]`) against tests/upload_standin.py, bit for bit, and against properties that need no stand-in; the id
images against the C oracle.  The stand-in itself is anchored on the CPU by tests/test_mesh_upload_host.py."""
import numpy as np
import pytest

from geograypher_amd._hip import HipRaster
from oracle import oracle_c
from tests import upload_scenes as scenes
from tests import upload_standin as su

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = scenes.upload_cases()
_STANDIN = {}   # case -> upload_np of it, computed once and never changed


def _standin(name):
    if name not in _STANDIN:
        _STANDIN[name] = su.upload_np(*CASES[name])
    return _STANDIN[name]


def _read(hip) -> dict:
    d = hip.debug_upload()
    return {"orig": d["orig"].cpu().numpy(), "blk": d["blk"].cpu().numpy(), "bvert": d["bvert"].cpu().numpy(),
            "bidx": d["bidx"].cpu().numpy().view(np.uint32), "mesh_sig": d["mesh_sig"]}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _assert_same_products(got, want, counts):
    """orig, blk, bidx, mesh_sig and the first count rows of every block's bvert, bit for bit"""
    np.testing.assert_array_equal(got["orig"], want["orig"])
    np.testing.assert_array_equal(got["bidx"], want["bidx"])
    bad = np.argwhere(_bits(got["blk"]) != _bits(want["blk"]))
    assert bad.size == 0, f"block spheres differ at {bad[:4].tolist()}: {got['blk'][bad[0, 0]]} != {want['blk'][bad[0, 0]]}"
    assert got["mesh_sig"] == want["mesh_sig"]
    for b, n in enumerate(counts):
        np.testing.assert_array_equal(_bits(got["bvert"][b, :n]), _bits(want["bvert"][b, :n]), err_msg=f"block {b}")


def _assert_properties(got, verts, faces):
    """Without the stand-in: orig is a permutation; a block's count byte is its number of distinct vertex indices - 1; bidx
    decodes to bvert rows that are the bits of verts[faces[orig[f]]]."""
    F = faces.shape[0]
    assert sorted(got["orig"].tolist()) == list(range(F))
    for b in range((F + 63) // 64):
        members = got["orig"][64 * b:64 * b + 64]
        words = got["bidx"][64 * b:64 * b + 64]
        n = len(np.unique(faces[members]))
        assert n <= 192 and ((words >> np.uint32(24)) == n - 1).all(), (b, n)
        local = np.stack([words & np.uint32(255), (words >> np.uint32(8)) & np.uint32(255), (words >> np.uint32(16)) & np.uint32(255)], axis=-1)
        assert local.max() < n
        np.testing.assert_array_equal(_bits(got["bvert"][b][local]), _bits(verts[faces[members]]), err_msg=f"block {b}")


@pytest.mark.parametrize("name", list(CASES))
def test_upload_products_equal_the_standin(hip, name):
    verts, faces = CASES[name]
    want = _standin(name)
    hip.upload_mesh(verts, faces)
    got = _read(hip)
    _assert_properties(got, verts, faces)
    _assert_same_products(got, want, want["counts"])
    if name.startswith("soup_F"):   # a full block of a soup has 192 distinct vertices: top byte 191
        F = faces.shape[0]
        assert (got["bidx"][:64 * (F // 64)] >> np.uint32(24) == 191).all()
        assert (got["bidx"][64 * (F // 64):] >> np.uint32(24) == 3 * (F % 64) - 1).all()
    if name == "equal_centroids":
        assert got["orig"].tolist() == list(range(faces.shape[0]))
    if name == "fan64":
        assert int(got["bidx"][0] >> np.uint32(24)) == 65 and (got["bidx"] & np.uint32(255) == 0).all()


def test_reupload_on_one_context_leaves_what_a_fresh_context_does():
    """large, small, large again on ONE context: buffers that are kept, reused and (for the stage scratch) shrunk in use"""
    ctx = HipRaster(0)
    try:
        with pytest.raises(RuntimeError, match=r"code -4"):
            ctx.debug_upload()                                   # no mesh yet
        for name in ("grid_F257", "soup_F2", "grid_F257", "stride_loop_V32833", "soup_F129"):
            verts, faces = CASES[name]
            ctx.upload_mesh(verts, faces)
            got = _read(ctx)
            fresh = HipRaster(0)
            try:
                fresh.upload_mesh(verts, faces)
                _assert_same_products(got, _read(fresh), _standin(name)["counts"])
            finally:
                fresh.close()
            _assert_same_products(got, _standin(name), _standin(name)["counts"])
        # an upload refused for a bad index: the mesh before it stays in use (include/geograster.h) ...
        verts, faces = CASES["soup_F129"]
        bad = faces.copy()
        bad[77, 1] = verts.shape[0]
        with pytest.raises(IndexError):
            ctx.upload_mesh(verts, bad)
        _assert_same_products(_read(ctx), _standin("soup_F129"), _standin("soup_F129")["counts"])
    finally:
        ctx.close()
    # ... and a context that never had one still has none
    ctx = HipRaster(0)
    try:
        with pytest.raises(IndexError):
            ctx.upload_mesh(verts, bad)
        with pytest.raises(RuntimeError, match=r"code -4"):
            ctx.debug_upload()
    finally:
        ctx.close()


# ---- the cull decision of ONE block ------------------------------------------------------------------------------------
def _patch():
    """A compact one-block mesh, 64 faces of the grid (a few units across), and its sphere by the stand-in."""
    verts, faces = scenes.grid_faces(64, seed=4)
    verts = (verts + F32([11.0, -7.0, 3.0])).astype(F32)
    return verts, faces


# deltas around the rejection threshold, in radii: the smallest are a few ulps of the camera's position
DELTAS = [s * d for d in (3e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.5, 1.5, 3.0) for s in (-1, 1)]

#            yaw  pitch  roll    f      cx     cy     h    w
SCENARIOS = {"pp_inside_613x457": (0.3, -0.2, 0.0, 900.0, 306.5, 228.5, 457, 613),
             "pp_left_of_0": (2.0, 0.4, 0.0, 300.0, -40.0, 30.0, 48, 64),
             "pp_right_of_w": (-1.0, 0.1, 0.0, 300.0, 110.0, 10.0, 48, 64),
             "rolled_tilted": (0.7, 1.2, 2.3, 500.0, 75.0, 50.0, 96, 160),
             "window_1x1": (-2.5, -0.8, 0.9, 50.0, 0.5, 0.5, 1, 1)}


def _walk(sphere, R, f, cx, cy, h, w, near=0.5):
    """[(plane or None, cam16)]: per plane the sphere's centre is put on the plane, in the middle of the window at ten radii
    of depth (the near plane: on the axis), and moved along the plane's normal through the cull's rejection threshold,
    DELTAS radii around it; then a camera inside the sphere and one with the sphere wholly behind it."""
    C, r = sphere[:3].astype(np.float64), float(sphere[3])
    cam0 = scenes.camera(R, [0, 0, 0], f, cx, cy, near)
    planes = scenes.planes64(cam0, h, w)
    out = []
    z0 = 10 * r
    mid = np.array([(w / 2 - cx) / f * z0, (h / 2 - cy) / f * z0, z0])
    for p, (a, b, c, d) in enumerate(planes):
        n = np.array([a, b, c])
        norm2, norm1 = np.linalg.norm(n), np.abs(n).sum()
        base = np.array([0, 0, near]) if p == 0 else mid - n * (n @ mid) / norm2 ** 2
        threshold = -1.001 * r * norm1 / norm2          # Euclidean distance at which the cull starts to reject
        for delta in DELTAS:
            q = base + (threshold + delta * r) * n / norm2
            out.append((p, scenes.camera(R, C - R @ q, f, cx, cy, near)))
    out.append((None, scenes.camera(R, C - R @ np.array([0.1 * r, -0.2 * r, 0.3 * r]), f, cx, cy, near)))   # inside the sphere
    out.append((None, scenes.camera(R, C - R @ np.array([0.0, 0.0, -5 * r]), f, cx, cy, near)))            # sphere behind
    return out


def _check_walk(hip, verts, faces, sphere, walk, h, w, expect_both=True):
    hip.upload_mesh(verts, faces)
    blk = _read(hip)["blk"]
    assert blk.shape == (1, 4)
    np.testing.assert_array_equal(_bits(blk), _bits(su.upload_np(verts, faces)["blk"]))
    assert len(walk) < 300
    seen = {p: set() for p, _ in walk}
    shown = 0
    for p, cam in walk:
        ids = hip.raster_face_ids(cam[None], h, w).cpu().numpy()[0]
        blocks = int(hip.last_stats["blocks"])
        want = oracle_c.raster(verts, faces, cam, h, w)
        keep = bool(su.cull_np(blk, cam, h, w)[0])
        print(f"plane {p}: blocks {blocks}, stand-in {int(keep)}, oracle pixels {int((want >= 0).sum())}")
        assert blocks == int(keep), (p, cam.tolist())
        bad = np.argwhere(ids != want)
        assert bad.size == 0, f"plane {p}: {bad.shape[0]} pixels differ, first {bad[:5].tolist()}, camera {cam.tolist()}"
        if (want >= 0).any():
            assert blocks == 1
            shown += 1
        seen[p].add(blocks)
    if expect_both:
        for p in range(5):
            assert seen[p] == {0, 1}, (p, seen[p])
        # A thousandth of the radius or more from the threshold the decision is the geometry's: the float32 error of the
        # camera-space centre is a few ulps of its size, ten radii -- 1e-5 radii.
        for (p, cam), delta in zip(walk, DELTAS * 5):
            if abs(delta) >= 1e-3:
                assert bool(su.cull_np(blk, cam, h, w)[0]) == (delta > 0), (p, delta)
    return seen, shown


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_cull_of_one_block_follows_the_standin_through_every_plane(hip, name):
    yaw, pitch, roll, f, cx, cy, h, w = SCENARIOS[name]
    verts, faces = _patch()
    sphere = su.upload_np(verts, faces)["blk"][0]
    walk = _walk(sphere, scenes.rotation(yaw, pitch, roll), f, cx, cy, h, w)
    seen, shown = _check_walk(hip, verts, faces, sphere, walk, h, w)
    assert seen[None] == {0, 1}          # inside the sphere: kept; the sphere behind the camera: rejected
    assert shown >= 5


def test_block_with_nan_and_inf_vertex_is_never_culled_and_shows_its_finite_faces(hip):
    yaw, pitch, roll, f, cx, cy, h, w = SCENARIOS["rolled_tilted"]
    clean, faces = _patch()
    sphere = su.upload_np(clean, faces)["blk"][0]
    verts = clean.copy()
    verts[faces[10, 0], 1] = np.nan
    verts[faces[50, 2], 0] = np.inf
    got = su.upload_np(verts, faces)["blk"][0]
    assert not np.isfinite(got[3])
    walk = _walk(sphere, scenes.rotation(yaw, pitch, roll), f, cx, cy, h, w)
    seen, shown = _check_walk(hip, verts, faces, sphere, walk, h, w, expect_both=False)
    assert all(s == {1} for s in seen.values())
    # the faces without a broken vertex are drawn wherever the clean mesh draws them
    broken = np.isin(faces, [faces[10, 0], faces[50, 2]]).any(axis=1)
    p, cam = walk[19]   # the near plane's last step: three radii inside
    ids = hip.raster_face_ids(cam[None], h, w).cpu().numpy()[0]
    assert len(np.setdiff1d(np.unique(ids[ids >= 0]), np.nonzero(broken)[0])) >= 10


# ---- many blocks ---------------------------------------------------------------------------------------------------------
MANY_H, MANY_W = 120, 160


def _many_block_scene(offset):
    """A 40-block grid (32 x 40 cells, F = 2560) and three cameras: one over its middle looking down at a part of it, one
    tilted over a corner, one high enough to see it all; translated by `offset` on x and y, rounded to float32."""
    verts, faces = scenes.grid(32, 40, seed=9)
    assert faces.shape[0] == 2560
    verts = verts.astype(np.float64)
    verts[:, :2] += offset
    down = scenes.rotation(0.0, np.pi, 0.0)   # the viewing direction is -z
    cams = [scenes.camera(down, [16.0 + offset, 20.0 + offset, 12.0], 200.0, 80.0, 60.0, near=0.5),
            scenes.camera(down @ scenes.rotation(0.5, 0.4, 0.3), [3.0 + offset, 36.0 + offset, 9.0], 150.0, 80.0, 60.0, near=0.5),
            scenes.camera(down, [16.0 + offset, 20.0 + offset, 80.0], 200.0, 80.0, 60.0, near=0.5)]
    return verts.astype(F32), faces, cams


@pytest.mark.parametrize("offset", [0.0, 1e4, 1e5])
def test_many_blocks_counted_like_the_standin_ids_like_the_oracle(hip, offset):
    verts, faces, cams = _many_block_scene(offset)
    want = su.upload_np(verts, faces)
    hip.upload_mesh(verts, faces)
    got = _read(hip)
    _assert_same_products(got, want, want["counts"])
    counts = []
    for v, cam in enumerate(cams):
        ids = hip.raster_face_ids(cam[None], MANY_H, MANY_W).cpu().numpy()[0]
        blocks = int(hip.last_stats["blocks"])
        keep = su.cull_np(got["blk"], cam, MANY_H, MANY_W)
        print(f"offset {offset:g} view {v}: blocks {blocks}, stand-in {int(keep.sum())} of {keep.shape[0]}")
        assert blocks == int(keep.sum())
        ref = oracle_c.raster(verts, faces, cam, MANY_H, MANY_W)
        bad = np.argwhere(ids != ref)
        assert bad.size == 0, f"view {v}: {bad.shape[0]} pixels differ, first {bad[:5].tolist()}"
        assert (ref >= 0).sum() > 1000
        # every block the oracle shows a face of was kept
        block_of = np.empty(faces.shape[0], dtype=np.int64)
        block_of[got["orig"]] = np.arange(faces.shape[0]) // 64
        assert keep[np.unique(block_of[ref[ref >= 0]])].all()
        counts.append(blocks)
    assert any(0 < c < 40 for c in counts), counts
    assert counts[2] == 40


def test_slivers_at_1e5_hugging_the_window_edges_are_drawn(hip):
    """One-face blocks that are thin on two axes, at x, y = 1e5, one end a few pixels inside a window edge
    (tests/upload_scenes.py): the oracle is the judge.  With a radius that does not cover the rounding of the centre the cull
    drops slivers that the oracle draws (tests/test_mesh_upload_host.py counts them)."""
    one = np.array([[0, 1, 2]], dtype=np.int32)
    shown = kept = 0
    for k, (verts, cam) in enumerate(scenes.sliver_scene()):
        hip.upload_mesh(verts, one)
        ids = hip.raster_face_ids(cam[None], scenes.SLIVER_H, scenes.SLIVER_W).cpu().numpy()[0]
        blocks = int(hip.last_stats["blocks"])
        want = oracle_c.raster(verts, one, cam, scenes.SLIVER_H, scenes.SLIVER_W)
        assert blocks == int(su.cull_np(su.upload_np(verts, one)["blk"], cam, scenes.SLIVER_H, scenes.SLIVER_W)[0]), k
        assert np.array_equal(ids, want), f"sliver {k}: device {int((ids >= 0).sum())} pixels, oracle {int((want >= 0).sum())}, blocks {blocks}"
        shown += int((want >= 0).any())
        kept += blocks
    print(f"slivers: {shown} drawn by the oracle, {kept} kept by the cull")
    assert shown >= 120
