"""gr_face_sieve on the device against the numpy stand-in of tests/face_sieve_standin.py: every scene of
tests/face_sieve_scenes.py, all three outputs, byte for byte; repeatability, a fresh context against a long-lived one, in place,
fenced outputs over a poisoned stage arena, every GR_EINVAL case, and the mesh methods and `aggregate_images` on the C1 scene."""
import ctypes
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import face_sieve_scenes as sc  # noqa: E402
import face_sieve_standin as fs  # noqa: E402
from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import geometric, synthetic  # noqa: E402
from tests.fenced_backend import FencedHipRaster, fenced  # noqa: E402
from tests.test_mesh_vis_host import aggregate_scene  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = sc.HAND + [sc.border_scene(n) for n in sc.BORDER_SIZES] + [sc.spiral_scene(), dict(sc.spiral_scene(), name="spiral_sieved", min_measure=3000)]


@pytest.fixture(scope="module")
def ctx():
    backend = FencedHipRaster(0)
    yield backend
    backend.close()


_wanted = {}


def standin(s):
    """The stand-in's answer for a scene: computed once, shared, not modified."""
    if s["name"] not in _wanted:
        class_out, comp, stats, _ = fs.sieve(s["faces"], s["classes"], s["weights"], s["min_measure"], s["fill"], s["canon"], n_vertices=s["V"])
        for a in (class_out, comp, stats):
            a.setflags(write=False)
        _wanted[s["name"]] = (class_out, comp, stats)
    return _wanted[s["name"]]


def device(backend, s, **kw):
    class_out, comp, stats = backend.face_sieve(s["faces"], s["classes"], s["weights"], s["min_measure"], s["fill"], s["canon"],
                                                n_vertices=s["V"], **kw)
    return class_out.cpu().numpy(), comp.cpu().numpy(), stats.cpu().numpy()


def assert_same(got, want, name):
    for g, w, what in zip(got, want, ("class_out", "comp", "stats")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, what, g[:16].tolist(), w[:16].tolist())


@pytest.mark.parametrize("s", SCENES, ids=lambda s: s["name"])
def test_scene_equals_the_standin(ctx, s):
    with fenced(ctx):
        got = device(ctx, s)
    assert_same(got, standin(s), s["name"])
    if "want_stats" in s:
        assert got[0].tolist() == s["want_class"].tolist() and got[1].tolist() == s["want_comp"].tolist() and got[2].tolist() == s["want_stats"]


def test_random_scenes_equal_the_standin(ctx):
    rounds = []
    for s in sc.random_scenes():
        with fenced(ctx):
            got = device(ctx, s)
        assert_same(got, standin(s), s["name"])
        rounds.append(int(got[2][fs.ROUNDS]))
    assert max(rounds) >= 2


@pytest.mark.parametrize("min_measure,fill", [(2, False), (3, True)])
def test_hand_scenes_merged_into_one_call(ctx, min_measure, fill):
    """Disconnected pieces do not see each other: the pieces whose own call has this threshold keep their hand answers."""
    s, at = sc.merged(sc.HAND, min_measure, fill)
    with fenced(ctx):
        got = device(ctx, s)
    assert_same(got, standin(s), s["name"])
    kept = 0
    for f0, piece in at:
        if piece["min_measure"] == min_measure and piece["fill"] == fill and piece["weights"] is None:
            n = len(piece["faces"])
            assert got[0][f0:f0 + n].tolist() == piece["want_class"].tolist(), piece["name"]
            assert got[1][f0:f0 + n].tolist() == np.where(piece["want_comp"] < 0, -1, piece["want_comp"] + f0).tolist(), piece["name"]
            kept += 1
    assert kept >= (6 if min_measure == 2 else 1)


def test_same_call_twice_and_fresh_context(ctx):
    fresh = _hip.HipRaster(0)
    try:
        for s in (sc.random_scene(1, 5, True), sc.border_scene(1025), sc.HAND[3]):
            first, again, other = device(ctx, s), device(ctx, s), device(fresh, s)
            assert_same(again, first, s["name"])
            assert_same(other, first, s["name"])
            assert_same(first, standin(s), s["name"])
    finally:
        fresh.close()


def test_in_place(ctx):
    s = sc.random_scene(2, 50, False)
    classes = torch.as_tensor(s["classes"]).to(ctx.device)
    class_out, comp, stats = ctx.face_sieve(s["faces"], classes, s["weights"], s["min_measure"], s["fill"], n_vertices=s["V"], out=classes)
    assert class_out.data_ptr() == classes.data_ptr()
    assert_same((classes.cpu().numpy(), comp.cpu().numpy(), stats.cpu().numpy()), standin(s), s["name"])
    with pytest.raises(ValueError, match="in place"):
        ctx.face_sieve(s["faces"], classes, out=torch.empty_like(classes))


@contextmanager
def poison(backend, bits):
    backend.set_option(_hip.GR_OPT_DEBUG, bits)
    try:
        yield
    finally:
        backend.set_option(_hip.GR_OPT_DEBUG, 0)


def test_fenced_outputs_over_a_poisoned_stage_arena(ctx):
    """The call writes every scratch word before it reads it and every output word: the same answers over an arena of 0xFF, of
    0x7F and as it was left, between intact fences."""
    scenes = [sc.random_scene(3, 5, True), sc.HAND[8], sc.border_scene(257), sc.HAND[0]]
    device(ctx, scenes[0])                                                    # grows the arena first
    for bits in (0, _hip.GR_DBG_POISON_STAGE, _hip.GR_DBG_POISON_STAGE_7F, 0):
        with poison(ctx, bits):
            for s in scenes:
                with fenced(ctx):
                    got = device(ctx, s)
                assert_same(got, standin(s), (s["name"], bits))
            if bits:
                tail, _ = ctx.debug_stage(0, -64, 64)
                assert bool((tail == (0xFF if bits == _hip.GR_DBG_POISON_STAGE else 0x7F)).all())


def test_every_einval_case(ctx):
    F, V = 4, 6
    faces = torch.as_tensor(sc.strip_faces(F)).to(ctx.device)
    classes = torch.zeros(F, dtype=torch.int32, device=ctx.device)
    weights = torch.ones(F, dtype=torch.int64, device=ctx.device)
    canon = torch.arange(V, dtype=torch.int32, device=ctx.device)
    out, comp = torch.empty_like(classes), torch.empty_like(classes)
    stats = torch.empty(_hip.GR_SIEVE_STAT_WORDS, dtype=torch.int64, device=ctx.device)
    both = torch.empty(2 * F, dtype=torch.int32, device=ctx.device)
    good = dict(faces=faces.data_ptr(), face_class=classes.data_ptr(), weights=weights.data_ptr(), vertex_canon=canon.data_ptr(),
                class_out=out.data_ptr(), comp=comp.data_ptr(), stats=stats.data_ptr(), stream=ctx._stream().value, F=F, V=V, min_measure=2,
                has_canon=1, fill_unlabelled=0, max_rounds=4, reserved=0)

    def call(**changed):
        args = _hip.FaceSieveArgs(**{**good, **changed})
        return ctx._rc("gr_face_sieve", ctypes.byref(args))

    assert call() == _hip.GR_OK and call(class_out=classes.data_ptr()) == _hip.GR_OK, "in place is the one overlap allowed"
    assert call(weights=None) == _hip.GR_OK and call(vertex_canon=None, has_canon=0) == _hip.GR_OK
    torch.cuda.synchronize(ctx.device)
    sentinel = torch.full_like(stats, 77)
    bad = [dict(faces=None), dict(face_class=None), dict(class_out=None), dict(comp=None), dict(stats=None), dict(vertex_canon=None),
           dict(F=-1), dict(V=-1), dict(F=2 ** 31 - 1), dict(V=2 ** 31 - 1), dict(F=(2 ** 31 - 1) // 3 + 1), dict(min_measure=-1),
           dict(max_rounds=0), dict(max_rounds=-3),
           dict(class_out=faces.data_ptr()), dict(comp=faces.data_ptr() + 16), dict(comp=classes.data_ptr()), dict(class_out=weights.data_ptr()),
           dict(comp=weights.data_ptr() + 8), dict(class_out=canon.data_ptr()), dict(comp=canon.data_ptr()), dict(stats=weights.data_ptr()),
           dict(comp=out.data_ptr()), dict(class_out=both.data_ptr(), comp=both.data_ptr() + 4)]
    for changed in bad:
        stats.copy_(sentinel)
        assert call(**changed) == _hip.GR_EINVAL, changed
        message = ctx.lib.gr_last_error(ctx._ctx).decode()
        assert message.startswith("gr_face_sieve: "), (changed, message)
        torch.cuda.synchronize(ctx.device)
        if "stats" not in changed:
            assert torch.equal(stats, sentinel), f"{changed}: device work before the refusal"
    assert ctx._rc("gr_face_sieve", None) == _hip.GR_EINVAL
    with pytest.raises(ValueError, match="a weight is negative"):
        ctx.face_sieve(faces, classes, torch.tensor([1, 1, -1, 1]), 2)
    with pytest.raises(ValueError, match="not below 2\\^62"):
        ctx.face_sieve(faces, classes, torch.full((F,), 1 << 60, dtype=torch.int64, device=ctx.device), 2)


def test_out_of_range_corners_are_counted_and_never_used(ctx):
    """Corners and vertex_canon entries outside [0, V): the face takes no part (comp -1, class kept), the word counts it, the
    fences stay intact; the Python layer raises."""
    faces = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 2 ** 31 - 1], [3, 2, -5], [2, 3, 4], [3, 4, 5]], dtype=np.int32)
    classes = np.array([1, 2, 2, 2, 2, 2], dtype=np.int32)
    with fenced(ctx):
        got = device(ctx, dict(faces=faces, classes=classes, weights=None, min_measure=2, fill=False, canon=None, V=6))
    assert got[0].tolist() == [2, 2, 2, 2, 2, 2] and got[1].tolist() == [0, 0, -1, -1, 0, 0]
    assert got[2].tolist() == [1, 2, 1, 1, 0, 0, 0, 0, 2]
    canon = np.array([0, 1, 2, 3, 6, -1], dtype=np.int32)
    with fenced(ctx):
        got = device(ctx, dict(faces=faces[[0, 1, 4, 5]], classes=classes[:4], weights=None, min_measure=0, fill=False, canon=canon, V=6))
    assert got[1].tolist() == [0, 1, -1, -1] and got[2][fs.BAD_FACES] == 2
    with pytest.raises(ValueError, match="2 faces name a vertex"):
        geometric.sieve_face_classes(faces, classes, None, 2, backend=ctx, n_vertices=6)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1():
    (points, faces), cams = synthetic.config1_scene()
    rng = np.random.default_rng(5)
    labels = (np.arange(len(faces)) // 700 % 3).astype(np.float64)
    flip = rng.random(len(faces)) < 0.1
    labels[flip] = rng.integers(0, 3, int(flip.sum()))
    labels[rng.random(len(faces)) < 0.03] = np.nan
    return points, faces, labels


def test_mesh_methods_on_c1(ctx, c1):
    points, faces, labels = c1
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=ctx)
    classes = np.where(np.isnan(labels), -1, labels).astype(np.int32)
    weights = geometric.face_area_weights(mesh.points, mesh.faces)      # (known answers: tests/test_face_sieve_host.py)
    canon = geometric.weld_canon(mesh.points)
    assert np.array_equal(mesh.faces, faces) and len(mesh.points) == len(points)
    as_tensor = torch.as_tensor(labels).to(ctx.device)
    for kw, standin_kw in ((dict(min_faces=6), dict(weights=None, min_measure=6)),
                           (dict(min_area_m2=float(np.median(weights)) * 4e-6, fill_unseen=True, weld_vertices=True),
                            dict(weights=weights, min_measure=int(np.ceil(float(np.median(weights)) * 4e-6 * 1e6)), fill_unlabelled=True,
                                 vertex_canon=canon))):
        want, _, want_stats, _ = fs.sieve(faces, classes, n_vertices=len(points), **standin_kw)
        want_labels = np.where(want < 0, np.nan, want.astype(np.float64))
        got = mesh.sieve_face_labels(labels, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.tobytes() == want_labels.tobytes()
        assert list(mesh.last_sieve_stats.values()) == want_stats.tolist() and want_stats[fs.CHANGED] > 100
        got_t = mesh.sieve_face_labels(as_tensor.reshape(-1, 1), return_tensor=True, **kw)
        assert isinstance(got_t, torch.Tensor) and got_t.shape == (len(faces), 1) and got_t.is_cuda
        assert got_t.cpu().numpy().tobytes() == want_labels.tobytes()
    _, want_comp, want_stats, _ = fs.sieve(faces, classes, n_vertices=len(points))
    for given in (labels, as_tensor):
        comp, stats = mesh.face_label_components(given)
        assert comp.dtype == np.int32 and comp.tobytes() == want_comp.tobytes() and list(stats.values()) == want_stats.tolist()
    comp_t, _ = mesh.face_label_components(as_tensor, return_tensor=True)
    assert comp_t.is_cuda and comp_t.cpu().numpy().tobytes() == want_comp.tobytes()
    same = mesh.sieve_face_labels(labels, min_faces=1)
    assert same.tobytes() == labels.tobytes() and mesh.last_sieve_stats["rounds"] == 0


def test_aggregate_images_defaults_write_the_same_bytes(ctx, tmp_path):
    from geograypher_amd.entrypoints.aggregate_images import aggregate_images

    args, kw, _ = aggregate_scene(tmp_path)
    (points, _faces), _ = synthetic.config1_scene()
    written = {}
    for name, extra in (("plain", {}), ("defaults", dict(sieve_min_area_m2=None, sieve_min_faces=None, sieve_fill_unseen=False)),
                        ("sieved", dict(sieve_min_faces=30))):
        folder = tmp_path / name
        aggregate_images(*args, backend=ctx, aggregated_face_values_savefile=folder / "values.npy",
                         predicted_face_classes_savefile=folder / "classes.npy", top_down_vector_projection_savefile=str(folder / "map.geojson"),
                         top_down_points_file=points[:, :2].copy(), **extra, **kw)
        written[name] = {p.name: p.read_bytes() for p in sorted(folder.iterdir())}
    assert set(written["plain"]) == {"values.npy", "classes.npy", "map.geojson"}
    assert written["defaults"] == written["plain"]
    assert written["sieved"]["values.npy"] == written["plain"]["values.npy"]
    assert written["sieved"]["classes.npy"] != written["plain"]["classes.npy"]
    assert len(written["sieved"]["map.geojson"]) < len(written["plain"]["map.geojson"]), "the sieved map has fewer ring vertices"
