"""gr_class_outlines on the device against the exact stand-in of tests/outline_standin.py (dictionaries of edge counts, a plain ring
walk): EVERY output array -- canonical ids, ring vertices, offsets, classes, the statistics words and the two host counts -- must be
bit-equal.  The sizes that matter are the 64 lanes of a wave and the 256 threads of a workgroup (one vertex, face, run or slot per
lane), and the device-wide sorts and scans between the kernels."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import outline_standin as osn  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils.geometric import PlanarPolygons  # noqa: E402

pytestmark = pytest.mark.gpu


def same(hip, verts_q, faces, classes, n_classes, **kw):
    """Run the device and the stand-in on one scene; compare everything; return the stand-in's answer."""
    want = osn.outlines_np(verts_q, faces, classes, n_classes)
    canon, ring_vertices, ring_offsets, ring_class, stats = hip.class_outlines(verts_q, faces, classes, n_classes, check=False, **kw)
    got = dict(canon=canon, ring_vertices=ring_vertices, ring_offsets=ring_offsets, ring_class=ring_class, stats=stats)
    for name, dtype in (("canon", np.int32), ("ring_vertices", np.int32), ("ring_offsets", np.int64), ("ring_class", np.int32),
                        ("stats", np.int64)):
        g = got[name].cpu().numpy()
        assert g.dtype == dtype and g.shape == want[name].shape and np.array_equal(g, want[name]), name
    return want


def test_minimal_scenes(hip):
    verts, faces, quad = osn.grid_mesh(1, 1)
    want = same(hip, verts, faces, [0, 0], 1)
    assert want["n_rings"] == 1 and want["ring_offsets"].tolist() == [0, 4] and want["stats"][3] == 1
    verts, faces, quad = osn.grid_mesh(2, 1)
    want = same(hip, verts, faces, osn.quad_classes(quad, [0, 1]), 2)
    assert want["ring_class"].tolist() == [0, 1] and want["ring_offsets"].tolist() == [0, 4, 8]
    want = same(hip, verts, np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32), 3)   # F = 0
    assert want["n_edges"] == 0 and want["ring_offsets"].tolist() == [0]
    want = same(hip, verts, faces, [-1, 7, 3, -5], 3)                                            # no face has a class
    assert want["n_edges"] == 0 and want["stats"][0] == 4
    want = same(hip, verts, faces, [4, 4, 5, 5], 5)                                              # class C - 1 is one, class C is none
    assert want["ring_class"].tolist() == [4] and want["stats"][0] == 2
    same(hip, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32), 1)   # V = 0


def test_pinch_vertices(hip):
    verts, faces, quad = osn.grid_mesh(4, 4, jitter=100_000)
    want = same(hip, verts, faces, osn.quad_classes(quad, [(i + j) % 2 for j in range(4) for i in range(4)]), 2)
    assert want["n_edges"] == 64   # every inner vertex has two incoming and two outgoing copies per class
    verts3, faces3, quad3 = osn.grid_mesh(3, 3)
    want = same(hip, verts3, faces3, osn.quad_classes(quad3, [0, 0, 0, 0, 1, 0, 0, 0, 0]), 2)
    areas2, home = osn.nest_np(verts3, want)
    assert want["ring_class"].tolist() == [0, 0, 1] and sorted(a < 0 for a in areas2) == [False, False, True] and 0 in home
    touching = np.zeros(16, dtype=np.int32)
    touching[5], touching[0] = 1, -1    # the hole at quad (1, 1) meets the notch at quad (0, 0) in one vertex
    want = same(hip, verts, faces, osn.quad_classes(quad, touching), 2)
    assert want["n_rings"] == 3


def test_folds(hip):
    verts, faces = osn.fold_scene()
    want = same(hip, verts, faces, [0, 0], 1)
    assert want["stats"][4] == 1 and want["n_edges"] == 6 and want["stats"][3] == 0   # the shared edge twice, nothing cancels
    want = same(hip, verts, faces, [0, 1], 2)
    assert want["stats"][4] == 0 and want["n_rings"] == 2


def test_canonical_vertices_and_face_rules(hip):
    verts, faces = osn.seam_scene()
    want = same(hip, verts, faces, [0, 0, 0, 0], 1)
    assert want["canon"].tolist() == [0, 1, 2, 3, 1, 5, 6, 2] and want["n_rings"] == 1 and want["n_edges"] == 6
    verts, faces = osn.wall_scene()
    want = same(hip, verts, faces, [0] * 6, 1)
    assert want["stats"][1] == 2 and want["n_rings"] == 1 and want["n_edges"] == 6
    verts, faces, quad = osn.grid_mesh(3, 2, jitter=100_000)
    want = same(hip, verts, osn.reversed_faces(faces), osn.quad_classes(quad, [0, 1, 0, 1, 1, 0]), 2)
    assert want["stats"][2] == len(faces)
    verts, faces = osn.unit_area_scene()
    want = same(hip, verts, faces, [0] * 7, 1)
    assert want["stats"][1] == 1 and want["stats"][2] == 1 and want["n_rings"] == 6   # neither 2^64 dropped nor 2^63 turned


@pytest.mark.parametrize("n_faces", (63, 64, 65, 257, 5003))
def test_block_and_wave_borders(hip, n_faces):
    verts, faces = osn.delaunay_scene(n_faces, seed=n_faces)
    rng = np.random.default_rng(n_faces)
    want = same(hip, verts, faces, rng.integers(-1, 3, n_faces).astype(np.int32), 3)
    assert want["n_rings"] > 3 and want["stats"][0] > 0
    coherent = osn.disk_classes(verts, faces, seed=n_faces)
    want = same(hip, verts, faces, coherent, 3)
    if n_faces == 5003:
        assert want["n_rings"] >= 3 and want["stats"][3] > 1000
        sparse = np.where(coherent < 0, -1, np.array([3, 40_000, 65_534], dtype=np.int32)[np.clip(coherent, 0, 2)])
        want = same(hip, verts, faces, sparse, 65535)
        assert set(want["ring_class"].tolist()) <= {3, 40_000, 65_534} and len(set(want["ring_class"].tolist())) >= 2


def test_capacity_and_bad_faces(hip):
    verts, faces = osn.delaunay_scene(257, seed=5)
    classes = np.random.default_rng(5).integers(-1, 3, 257).astype(np.int32)
    want = osn.outlines_np(verts, faces, classes, 3)
    E, R = want["n_edges"], want["n_rings"]
    vq, f_t, c_t = (torch.as_tensor(a).to(hip.device) for a in (verts, faces, classes))
    stats = torch.empty(_hip.GR_OUTL_STAT_WORDS, dtype=torch.int64, device=hip.device)

    def call(cap, buffers):
        n_edges, n_rings = ctypes.c_int64(-1), ctypes.c_int64(-1)
        with torch.cuda.device(hip.device):
            rc = hip.lib.gr_class_outlines(hip._ctx, vq.data_ptr(), len(verts), f_t.data_ptr(), len(faces), c_t.data_ptr(), 3,
                                           *(b.data_ptr() if b is not None else None for b in buffers), cap, ctypes.byref(n_edges),
                                           ctypes.byref(n_rings), stats.data_ptr(), hip._stream())
        return rc, n_edges.value, n_rings.value

    sentinel = -77
    buffers = [torch.full((n,), sentinel, dtype=dt, device=hip.device)
               for n, dt in ((len(verts), torch.int32), (E, torch.int32), (E // 3 + 1, torch.int64), (E // 3 + 1, torch.int32))]
    assert call(E - 1, buffers) == (_hip.GR_EOVERFLOW, E, R)                      # too small: the totals, nothing written
    assert all(bool((b == sentinel).all()) for b in buffers)
    assert np.array_equal(stats.cpu().numpy(), want["stats"])
    assert call(0, [None] * 4) == (_hip.GR_OK, E, R)                              # capacity 0: the counts alone
    assert call(E, buffers) == (_hip.GR_OK, E, R)                                 # exactly enough
    assert np.array_equal(buffers[1].cpu().numpy(), want["ring_vertices"])
    assert np.array_equal(buffers[2].cpu().numpy()[:R + 1], want["ring_offsets"])
    canon, rv, ro, rcls, _ = hip.class_outlines(verts, faces, classes, 3, capacity=5)   # the binding repeats the call once
    assert hip.last_outline_calls == 2 and np.array_equal(rv.cpu().numpy(), want["ring_vertices"])
    # a face that names vertex V is reported and reads nothing
    broken = faces.copy()
    broken[100, 2] = len(verts)
    broken[7, 0] = -1
    want_bad = same(hip, verts, broken, classes, 3)
    assert want_bad["stats"][5] == 2
    with pytest.raises(ValueError, match=rf"gr_class_outlines: 2 faces name a vertex outside \[0, {len(verts)}\)"):
        hip.class_outlines(verts, broken, classes, 3)
    for bad_call in (lambda: hip.class_outlines(verts, faces, classes, 65536),
                     lambda: hip._call("gr_class_outlines", None, 4, f_t.data_ptr(), 1, c_t.data_ptr(), 1, None, None, None, None, 0,
                                       ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()), stats.data_ptr(), hip._stream()),
                     lambda: hip._call("gr_class_outlines", vq.data_ptr(), 4, f_t.data_ptr(), -1, c_t.data_ptr(), 1, None, None, None,
                                       None, 0, ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()), stats.data_ptr(),
                                       hip._stream()),
                     lambda: hip._call("gr_class_outlines", vq.data_ptr(), 4, f_t.data_ptr(), 1, c_t.data_ptr(), 70000, None, None, None,
                                       None, 0, ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()), stats.data_ptr(),
                                       hip._stream())):
        with pytest.raises(ValueError, match="gr_class_outlines"):
            bad_call()


def test_end_to_end_equals_the_host_path(hip, tmp_path):
    points, faces, labels = osn.height_field()
    results = {}
    for name, backend in (("device", hip), ("host", osn.StandInBackend())):
        mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=backend)
        outlines = mesh.face_label_outlines(labels, points_in_export_CRS=points, drop_nan=False)
        polygons, columns = mesh.export_face_labels_vector(labels, tmp_path / f"{name}.geojson", label_names=["a", "b", "c"],
                                                           points_in_export_CRS=points)
        results[name] = (outlines, polygons, columns, mesh.last_outline_stats)
    dev, host = results["device"], results["host"]
    for field in ("ring_offsets", "ring_class", "ring_vertex_ids", "ring_xy", "ring_is_hole"):
        assert np.array_equal(getattr(dev[0], field), getattr(host[0], field), equal_nan=True), field
    assert dev[0].stats == host[0].stats and dev[3] == host[3] and len(dev[0]) > 6
    assert len(dev[1].rings) == len(host[1].rings) and all(np.array_equal(a, b) for a, b in zip(dev[1].rings, host[1].rings))
    assert np.array_equal(dev[1].ring_polygon, host[1].ring_polygon) and np.array_equal(dev[1].ring_is_hole, host[1].ring_is_hole)
    assert (tmp_path / "device.geojson").read_text() == (tmp_path / "host.geojson").read_text()
    tensors = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=hip).face_label_outlines(
        torch.as_tensor(labels).to(hip.device), points_in_export_CRS=points, drop_nan=False, return_tensor=True)
    assert tensors.ring_vertex_ids.is_cuda and np.array_equal(tensors.ring_vertex_ids.cpu().numpy(), host[0].ring_vertex_ids)
    back, _ = PlanarPolygons.from_geojson(tmp_path / "device.geojson")
    assert len(back) == 3
