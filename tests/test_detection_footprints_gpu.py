"""gr_member_outlines on the device against the exact stand-in of tests/member_outline_standin.py (one dictionary of edge counts per
class, a plain ring walk): EVERY output array -- canonical ids, ring vertices, offsets, classes and the statistics words -- must be
bit-equal.  The sizes that matter are the 64 faces a wave owns, the 64 members it writes per step and the 256 threads of a
workgroup in `k_outline_member_edges`, rows longer than a wave and than a workgroup, and the 31 class bits of both sort keys."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import member_outline_standin as msn  # noqa: E402
import outline_standin as osn  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = (("canon", np.int32), ("ring_vertices", np.int32), ("ring_offsets", np.int64), ("ring_class", np.int32), ("stats", np.int64))


def same(hip, verts_q, faces, rows, n_classes, table=None, **kw):
    """Run the device and the stand-in on one membership; compare everything; return the stand-in's answer."""
    face_ptr, face_members = msn.csr_of_rows(rows) if table is None else table
    want = msn.members_np(verts_q, faces, face_ptr, face_members, n_classes)
    got = dict(zip((name for name, _ in FIELDS), hip.member_outlines(verts_q, faces, face_ptr, face_members, n_classes, check=False, **kw)))
    for name, dtype in FIELDS:
        g = got[name].cpu().numpy()
        assert g.dtype == dtype and g.shape == want[name].shape and np.array_equal(g, want[name]), name
    return want


def test_minimal_scenes(hip):
    verts, faces, quad = osn.grid_mesh(1, 1)
    want = same(hip, verts, faces[:1], [[0]], 1)                         # one face in one class
    assert want["ring_offsets"].tolist() == [0, 3] and want["ring_class"].tolist() == [0]
    want = same(hip, verts, faces[:1], [[0, 4]], 5)                      # ... in two
    assert want["ring_offsets"].tolist() == [0, 3, 6] and want["ring_class"].tolist() == [0, 4]
    want = same(hip, verts, faces, [[0, 1], [0, 2]], 3)                  # two adjacent faces share class 0 and differ in another
    assert want["ring_class"].tolist() == [0, 1, 2] and want["ring_offsets"].tolist() == [0, 4, 7, 10] and want["stats"][3] == 1
    want = same(hip, verts, faces, [[], []], 3)                          # nnz = 0
    assert want["n_edges"] == 0 and want["ring_offsets"].tolist() == [0]
    want = same(hip, verts, np.zeros((0, 3), dtype=np.int32), [], 3)     # F = 0
    assert want["n_edges"] == 0 and want["ring_offsets"].tolist() == [0]
    same(hip, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3), dtype=np.int32), [], 1)   # V = 0
    verts, faces, quad = osn.grid_mesh(3, 1)
    for empty in (0, 3, 5):                                              # an empty row first, inside, last
        rows = [[0, 1] if f != empty else [] for f in range(6)]
        want = same(hip, verts, faces, rows, 2)
        assert want["n_rings"] == 2 and want["stats"][:3].tolist() == [0, 0, 0]
    want = same(hip, verts, faces, [[-1, 0, 2]] * 6, 2)                  # class -1 and class n_classes are counted and dropped
    assert want["stats"][0] == 12 and want["ring_class"].tolist() == [0]


@pytest.mark.parametrize("n_faces", (63, 64, 65, 257, 5003))
def test_block_and_wave_borders(hip, n_faces):
    verts, faces = osn.delaunay_scene(n_faces, seed=n_faces)
    want = same(hip, verts, faces, msn.random_rows(n_faces, 5, seed=n_faces), 5)
    assert want["n_rings"] > 3
    rows = msn.random_rows(n_faces, 400, seed=n_faces + 1)
    rows[n_faces // 2] = list(range(3, 73))           # a row longer than a wave
    rows[n_faces - 1] = list(range(50, 350))          # ... and longer than a workgroup, in the last face
    want = same(hip, verts, faces, rows, 400)
    assert len(set(want["ring_class"].tolist())) > 300


@pytest.mark.parametrize("nnz", (63, 64, 65, 255, 256, 257))
def test_member_counts_at_the_borders(hip, nnz):
    verts, faces = osn.delaunay_scene(257, seed=9)
    rows = msn.rows_with_nnz(257, 4, nnz, seed=nnz)
    want = same(hip, verts, faces, rows, 4)
    assert sum(len(r) for r in rows) == nnz and want["n_rings"] >= 4


def test_class_range(hip):
    verts, faces = osn.delaunay_scene(5003, seed=5003)
    coherent = osn.disk_classes(verts, faces, seed=5003)
    names = np.array([3, 40_000, 69_999])
    rows = [[] if c < 0 else sorted({int(names[c]), int(names[(c + 1) % 3])}) for c in coherent.tolist()]
    want = same(hip, verts, faces, rows, 70_000)       # above the 65 535 of gr_class_outlines
    assert set(want["ring_class"].tolist()) == {3, 40_000, 69_999}
    top = _hip.GR_MEMBER_MAX_CLASSES                    # 31 class bits in both sort keys
    assert top == 2 ** 31 - 2
    rows = [[] for _ in range(5003)]
    rows[17] = [top - 1]
    rows[18] = [5, top - 1]
    rows[19] = [-1, top]                               # outside [0, n_classes) on both sides
    want = same(hip, verts, faces, rows, top)
    assert want["ring_class"].tolist() == [5] + [top - 1] * (want["n_rings"] - 1) and want["stats"][0] == 2


def test_identity_with_the_per_class_calls(hip):
    """Y5 on the device: the one call equals the per-column calls of gr_class_outlines, concatenated."""
    verts, faces = osn.delaunay_scene(257, seed=21)
    rows = msn.random_rows(257, 9, seed=21, most=4)
    face_ptr, face_members = msn.csr_of_rows(rows)
    canon, rv, ro, rc, _ = (t.cpu().numpy() for t in hip.member_outlines(verts, faces, face_ptr, face_members, 9))
    assert hip.last_outline_calls == 1
    vertices, offsets, classes = [], [np.zeros(1, dtype=np.int64)], []
    for column in range(9):
        alone = msn.column_classes(face_ptr, face_members, column, 257)
        c1, v1, o1, k1, _ = (t.cpu().numpy() for t in hip.class_outlines(verts, faces, alone, 1))
        assert np.array_equal(c1, canon) and len(o1) > 1
        offsets.append(o1[1:] + offsets[-1][-1])
        vertices.append(v1)
        classes.append(np.full(len(k1), column, dtype=np.int32))
    assert np.array_equal(rv, np.concatenate(vertices)) and np.array_equal(ro, np.concatenate(offsets))
    assert np.array_equal(rc, np.concatenate(classes))


def test_pinch_vertices_folds_seams_and_walls(hip):
    verts, faces, quad = osn.grid_mesh(4, 4, jitter=100_000)
    checker = [(i + j) % 2 for j in range(4) for i in range(4)]
    rows = [[checker[q], 2] if q != 5 else [checker[q]] for q in quad.tolist()]      # class 2 overlaps both, with a hole
    want = same(hip, verts, faces, rows, 3)
    assert want["n_rings"] >= 4 and 2 in want["ring_class"].tolist()
    verts, faces = osn.fold_scene()
    want = same(hip, verts, faces, [[0, 1], [0]], 2)
    assert want["stats"][4] == 1 and want["n_edges"] == 9
    verts, faces = osn.seam_scene()
    want = same(hip, verts, faces, [[0, 1], [0, 1], [0], [0, 1]], 2)
    assert want["canon"].tolist() == [0, 1, 2, 3, 1, 5, 6, 2] and want["ring_class"].tolist() == [0, 1] and want["n_edges"] == 11
    verts, faces = osn.wall_scene()
    want = same(hip, verts, faces, [[0, 1]] * 6, 2)
    assert want["stats"][1] == 4 and want["n_rings"] == 2 and want["n_edges"] == 12
    verts, faces, quad = osn.grid_mesh(3, 2, jitter=100_000)
    want = same(hip, verts, osn.reversed_faces(faces), [[0, 1]] * len(faces), 2)
    assert want["stats"][2] == 2 * len(faces)
    verts, faces = osn.unit_area_scene()                                              # vertices at +-(2^40 - 1), areas of 0 and +-1
    want = same(hip, verts, faces, [[0, 3]] * 7, 4)
    assert want["stats"][1] == 2 and want["stats"][2] == 2 and want["n_rings"] == 12


def _raw_call(hip, verts, faces, face_ptr, face_members, n_classes, cap, buffers, stats):
    tensors = [torch.as_tensor(np.ascontiguousarray(a)).to(hip.device) for a in (verts, faces, face_ptr, face_members)]
    n_edges, n_rings = ctypes.c_int64(-1), ctypes.c_int64(-1)
    with torch.cuda.device(hip.device):
        rc = hip.lib.gr_member_outlines(hip._ctx, tensors[0].data_ptr(), len(verts), tensors[1].data_ptr(), len(faces),
                                        tensors[2].data_ptr(), tensors[3].data_ptr() if len(face_members) else None, len(face_members),
                                        n_classes, *(b.data_ptr() if b is not None else None for b in buffers), cap,
                                        ctypes.byref(n_edges), ctypes.byref(n_rings), stats.data_ptr(), hip._stream())
        torch.cuda.synchronize()
    return rc, n_edges.value, n_rings.value


def _sentinel_buffers(hip, n_verts, E, sentinel=-77):
    return [torch.full((n,), sentinel, dtype=dt, device=hip.device)
            for n, dt in ((n_verts, torch.int32), (max(E, 1), torch.int32), (E // 3 + 1, torch.int64), (E // 3 + 1, torch.int32))]


def test_malformed_tables_are_counted_and_rejected(hip):
    """Y2: rejected by the count of the violations; nothing but the statistics is written."""
    verts, faces = osn.delaunay_scene(65, seed=3)
    rows = msn.random_rows(65, 6, seed=3)
    rows[10], rows[40] = [1, 2, 5], [0, 3, 4]
    face_ptr, face_members = msn.csr_of_rows(rows)
    nnz = len(face_members)

    def edited(ptr_edit=None, member_edit=None):
        ptr, members = face_ptr.copy(), face_members.copy()
        if ptr_edit:
            ptr_edit(ptr)
        if member_edit:
            member_edit(members)
        return ptr, members

    def descending(m): m[face_ptr[10]:face_ptr[10] + 3] = [5, 2, 1]
    def duplicated(m): m[face_ptr[40]:face_ptr[40] + 3] = [0, 3, 3]
    def first_not_zero(p): p[0] = 1
    def last_not_nnz(p): p[-1] = nnz - 1
    def last_beyond(p): p[-1] = nnz + 1000
    def decreasing(p): p[30] = p[29] - 1 if p[29] > 0 else p[31] + 1
    def negative(p): p[20] = -5
    cases = {"descending": edited(member_edit=descending), "duplicated": edited(member_edit=duplicated),
             "first": edited(first_not_zero), "last": edited(last_not_nnz), "beyond": edited(last_beyond),
             "decreasing": edited(decreasing), "negative": edited(negative)}
    stats = torch.empty(_hip.GR_OUTL_STAT_WORDS, dtype=torch.int64, device=hip.device)
    for name, (ptr, members) in cases.items():
        n_ptr, n_bad = msn.bad_ptr(ptr, nnz, 65), msn.bad_rows(ptr, members, 65)
        assert n_bad > 0, name
        buffers = _sentinel_buffers(hip, len(verts), 3 * nnz)
        assert _raw_call(hip, verts, faces, ptr, members, 6, 3 * nnz, buffers, stats) == (_hip.GR_OK, 0, 0), name
        assert all(bool((b == -77).all()) for b in buffers), name
        counted = int(stats[_hip.GR_OUTL_STAT_BAD_ROWS])
        assert counted == n_bad if n_ptr == 0 else counted >= n_ptr, name    # rows that overlap: the offsets' share is exact
        with pytest.raises(ValueError, match=rf"gr_member_outlines: {counted} violations"):
            hip.member_outlines(verts, faces, ptr, members, 6)
        canon, rv, ro, rc, st = hip.member_outlines(verts, faces, ptr, members, 6, check=False)   # an empty table and the count
        assert rv.numel() == 0 and rc.numel() == 0 and ro.cpu().tolist() == [0] and int(st[_hip.GR_OUTL_STAT_BAD_ROWS]) == counted
    same(hip, verts, faces, rows, 6)                                        # the well-formed table still traces


def test_capacity_and_bad_faces(hip):
    verts, faces = osn.delaunay_scene(257, seed=5)
    rows = msn.random_rows(257, 3, seed=5)
    face_ptr, face_members = msn.csr_of_rows(rows)
    want = msn.members_np(verts, faces, face_ptr, face_members, 3)
    E, R = want["n_edges"], want["n_rings"]
    stats = torch.empty(_hip.GR_OUTL_STAT_WORDS, dtype=torch.int64, device=hip.device)
    buffers = _sentinel_buffers(hip, len(verts), E)
    call = lambda cap, bufs: _raw_call(hip, verts, faces, face_ptr, face_members, 3, cap, bufs, stats)
    assert call(E - 1, buffers) == (_hip.GR_EOVERFLOW, E, R)                      # too small: the totals, nothing written
    assert all(bool((b == -77).all()) for b in buffers)
    assert np.array_equal(stats.cpu().numpy(), want["stats"])
    assert call(0, [None] * 4) == (_hip.GR_OK, E, R)                              # capacity 0: the counts alone
    assert call(E, buffers) == (_hip.GR_OK, E, R)                                 # exactly enough
    assert np.array_equal(buffers[1].cpu().numpy(), want["ring_vertices"])
    assert np.array_equal(buffers[2].cpu().numpy()[:R + 1], want["ring_offsets"])
    assert np.array_equal(buffers[3].cpu().numpy()[:R], want["ring_class"])
    _, rv, _, _, _ = hip.member_outlines(verts, faces, face_ptr, face_members, 3, capacity=5)   # the binding repeats the call once
    assert hip.last_outline_calls == 2 and np.array_equal(rv.cpu().numpy(), want["ring_vertices"])
    same(hip, verts, faces, rows, 3, capacity=0)
    # a face that names vertex V is reported and reads nothing
    broken = faces.copy()
    broken[100, 2] = len(verts)
    broken[7, 0] = -1
    want_bad = same(hip, verts, broken, rows, 3)
    assert want_bad["stats"][5] == 2
    with pytest.raises(ValueError, match=rf"gr_member_outlines: 2 faces name a vertex outside \[0, {len(verts)}\)"):
        hip.member_outlines(verts, broken, face_ptr, face_members, 3)
    with pytest.raises(ValueError, match="gr_member_outlines: n_classes"):
        hip.member_outlines(verts, faces, face_ptr, face_members, 2 ** 31 - 1)
    with pytest.raises(ValueError, match="gr_member_outlines: face_ptr must hold"):
        hip.member_outlines(verts, faces, face_ptr[:-1], face_members, 3)
    # the library's own argument checks: GR_EINVAL naming the call, before any device work (the statistics keep their sentinel)
    vq, f_t, p_t, m_t = (torch.as_tensor(np.ascontiguousarray(a)).to(hip.device) for a in (verts, faces, face_ptr, face_members))
    counts = lambda: (ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()))
    nnz = len(face_members)
    stats.fill_(-77)
    for bad_call in (
            lambda: hip._call("gr_member_outlines", None, 4, f_t.data_ptr(), 1, p_t.data_ptr(), m_t.data_ptr(), 1, 1, None, None, None, None,
                              0, *counts(), stats.data_ptr(), hip._stream()),                                        # no vertices
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), 4, f_t.data_ptr(), 1, None, m_t.data_ptr(), 1, 1, None, None, None, None,
                              0, *counts(), stats.data_ptr(), hip._stream()),                                        # no face_ptr
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), 4, f_t.data_ptr(), 1, p_t.data_ptr(), None, 1, 1, None, None, None, None,
                              0, *counts(), stats.data_ptr(), hip._stream()),                                        # no members
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), 4, f_t.data_ptr(), -1, p_t.data_ptr(), m_t.data_ptr(), 1, 1, None, None,
                              None, None, 0, *counts(), stats.data_ptr(), hip._stream()),                            # F < 0
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), 4, f_t.data_ptr(), 1, p_t.data_ptr(), m_t.data_ptr(), -1, 1, None, None,
                              None, None, 0, *counts(), stats.data_ptr(), hip._stream()),                            # nnz < 0
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), 4, f_t.data_ptr(), 1, p_t.data_ptr(), m_t.data_ptr(), (2 ** 31 + 2) // 3,
                              1, None, None, None, None, 0, *counts(), stats.data_ptr(), hip._stream()),            # 3 nnz >= 2^31
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), 4, f_t.data_ptr(), 1, p_t.data_ptr(), m_t.data_ptr(), 1, -1, None, None,
                              None, None, 0, *counts(), stats.data_ptr(), hip._stream()),                            # n_classes < 0
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), 4, f_t.data_ptr(), 1, p_t.data_ptr(), m_t.data_ptr(), 1, 2 ** 31 - 1, None,
                              None, None, None, 0, *counts(), stats.data_ptr(), hip._stream()),                      # n_classes > 2^31 - 2
            lambda: hip._call("gr_member_outlines", vq.data_ptr(), len(verts), f_t.data_ptr(), len(faces), p_t.data_ptr(), m_t.data_ptr(), nnz,
                              3, None, None, None, None, 8, *counts(), stats.data_ptr(), hip._stream())):            # room without buffers
        with pytest.raises(ValueError, match="gr_member_outlines"):
            bad_call()
    torch.cuda.synchronize()
    assert bool((stats == -77).all())


def test_end_to_end_equals_the_host_path(hip, tmp_path):
    """`face_label_outlines` and `export_face_labels_vector` on the CSR of a real `aggregate_projected_images` call."""
    from geograypher_amd.cameras.segmentor import SegmentorPhotogrammetryCameraSet
    from geograypher_amd.meshes.derived_meshes import TexturedPhotogrammetryMeshIndexPredictions
    from geograypher_amd.predictors.derived_segmentors import TabularRectangleSegmentor
    from geograypher_amd.utils import synthetic

    (points, faces), cams = synthetic.config1_scene()
    sub = cams[0:2]
    for i, c in enumerate(sub.cameras):
        c.image_filename = Path(tmp_path, "images", f"img{i}.png")
    detector = TabularRectangleSegmentor(Path(__file__).parent / "golden" / "tabular" / "cols", (480, 640), split_bbox=False)
    mesh = TexturedPhotogrammetryMeshIndexPredictions((points, faces), log_level="ERROR", backend=hip)
    _, info = mesh.aggregate_projected_images(SegmentorPhotogrammetryCameraSet(sub, segmentor=detector), n_classes=detector.num_classes)
    matrix = info["summed_projections"]
    assert matrix.nnz > 50 and matrix.shape == (len(faces), detector.num_classes)
    results = {}
    for name, backend in (("device", hip), ("host", msn.StandInBackend())):
        m = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=backend)
        outlines = m.face_label_outlines(matrix, points_in_export_CRS=points)
        polygons, columns = m.export_face_labels_vector(matrix, tmp_path / f"{name}.geojson", points_in_export_CRS=points)
        results[name] = (outlines, polygons, columns, m.last_outline_stats)
    dev, host = results["device"], results["host"]
    for field in ("ring_offsets", "ring_class", "ring_vertex_ids", "ring_xy", "ring_is_hole"):
        assert np.array_equal(getattr(dev[0], field), getattr(host[0], field)), field
    assert dev[0].stats == host[0].stats and dev[0].stats["calls"] == 1 and dev[3] == host[3] and len(dev[0]) >= 3
    assert np.array_equal(dev[2]["class_ID"], host[2]["class_ID"]) and len(dev[2]["class_ID"]) >= 3
    assert (tmp_path / "device.geojson").read_text() == (tmp_path / "host.geojson").read_text()
