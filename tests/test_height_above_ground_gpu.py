"""gr_sample_raster / raster samples on the device against the numpy restatement of tests/raster_standin.py: every comparison is
`np.array_equal(..., equal_nan=True)` on EVERY query -- the rules round every float64 operation on its own, so there is no tolerance.

The kernel stages nothing (each lane reads its indices, its vertices and its samples straight from memory), so the sizes that
matter are the 64 lanes of a wave, the 256 threads of a workgroup and the degenerate rasters of one row, one column, one cell."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_standin as rs  # noqa: E402
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.raster import PlanarRaster  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = np.nan


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def host(t):
    return None if t is None else t.cpu().numpy()


def device_sample(hip, points, faces, raster, fill=NAN, **kw):
    kw.setdefault("want_values", True)
    kw.setdefault("want_height", True)
    values, height, labels, stats = hip.sample_raster(points, faces, raster.data, raster.inverse, raster.nodata, fill, **kw)
    return host(values), host(height), host(labels), host(stats)


def check_against_standin(hip, points, faces, raster, fill=NAN, **kw):
    """All outputs and the statistics of one device call equal the stand-in's; returns the stand-in's record."""
    want = rs.sample_raster_np(points, faces, raster.data, raster.inverse, raster.nodata, fill, **kw)
    values, height, labels, stats = device_sample(hip, points, faces, raster, fill, check=False, **kw)
    assert values.dtype == np.float64 and values.shape == want["values"].shape and same(values, want["values"])
    assert height.shape == want["height"].shape and same(height, want["height"])
    assert (labels is None) == (want["labels"] is None) and (labels is None or same(labels, want["labels"]))
    assert stats.tolist() == want["stats"].tolist()
    return want


@pytest.fixture(scope="module")
def scene():
    """The random scene with the stand-in's answer: computed once, shared, not modified."""
    points, faces, data, transform, nodata = rs.random_scene()
    raster = PlanarRaster(data, transform, nodata)
    want = rs.sample_raster_np(points, faces, raster.data, raster.inverse, nodata, NAN)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return points, faces, raster, want


@pytest.mark.parametrize("vertex_mode", [False, True])
def test_hand_worked_scene(hip, vertex_mode):
    cases = rs.hand_cases()
    if vertex_mode:
        points, faces = np.array([[c[0], c[1], 7.0] for c, _, _ in cases]), None
    else:
        points, faces = rs.centred_faces([c for c, _, _ in cases], 7.0)
    raster = PlanarRaster(rs.HAND_DATA, rs.HAND_TRANSFORM, rs.HAND_NODATA)
    values, height, _, stats = device_sample(hip, points, faces, raster)
    want = np.array([NAN if v is None else v for _, v, _ in cases])
    for (centre, _, what), g, w in zip(cases, values[:, 0], want):
        assert same(g, w), (centre, what, g)
    assert values.shape == (30, 1) and same(height, 7.0 - want) and stats.tolist() == [23, 7, 0, 0]
    check_against_standin(hip, points, faces, raster)
    check_against_standin(hip, points, faces, PlanarRaster(rs.HAND_DATA, rs.HAND_TRANSFORM), fill=-1.0)   # no nodata: outside reads 0.0
    sheared = PlanarRaster(rs.HAND_DATA, (0.5, 0.25, 10.0, 0.5, -0.25, 20.0), rs.HAND_NODATA)
    a, b, c, d, e, f = sheared.transform
    centres = [(a * cc + b * rr + c, d * cc + e * rr + f) for cc, rr in ((0.5, 0.5), (1.0, 0.5), (2.5, 2.0), (0.0, 0.0), (5.0, 1.5), (2.5, 3.0))]
    got = device_sample(hip, *rs.centred_faces(centres, 0.0), sheared)[0][:, 0]
    assert same(got, [101.0, 102.0, 303.0, 101.0, NAN, NAN])


def test_random_scene_has_the_hard_cases_and_matches_on_every_face(hip, scene):
    points, faces, raster, want = scene
    edge = rs.on_cell_edge(points, faces, raster.inverse)
    counts = dict(on_edge=int((edge & want["inside"]).sum()), outside=int((~want["inside"]).sum()),
                  nodata_inside=int((want["nodata_hit"] & want["inside"]).sum()))
    print(f"[raster_samples] random scene: {len(faces)} faces on a {raster.shape} raster, {counts}")
    assert len(faces) == 4000 and raster.shape == (1, 30, 40) and raster.data.dtype == np.float32
    assert counts["on_edge"] >= 200 and counts["outside"] >= 200 and counts["nodata_inside"] >= 50
    values, height, _, stats = device_sample(hip, points, faces, raster)
    assert same(values, want["values"]) and same(height, want["height"]) and stats.tolist() == want["stats"].tolist()
    # the second way, on the inside queries of the first 300 faces: a loop per point with math.floor
    loop = rs.sample_by_loop(want["queries"][:300, :2], raster.data, raster.transform, raster.nodata, NAN)
    assert same(values[:300], loop)
    # vertex mode on the same points
    check_against_standin(hip, points, None, raster)


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 257])
def test_face_counts_around_a_wave_and_a_workgroup(hip, scene, n_faces):
    points, faces, raster, want = scene
    values, height, _, stats = device_sample(hip, points, faces[:n_faces], raster)
    assert values.shape == (n_faces, 1) and same(values, want["values"][:n_faces]) and same(height, want["height"][:n_faces])
    assert stats[0] == want["inside"][:n_faces].sum() and stats[1] == want["nodata_hit"][:n_faces].sum()


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_degenerate_rasters_and_both_dtypes(hip, scene, shape, dtype):
    points, faces, _, _ = scene
    data = (np.arange(shape[0] * shape[1]).reshape(shape) + 0.125).astype(dtype)
    data.flat[-1] = -7.0
    # cells of 3 m over the middle of the scene: many queries inside, many beyond every side
    raster = PlanarRaster(data, (3.0, 0.0, 105.0, 0.0, -3.0, 212.0), nodata=-7.0)
    assert raster.data.dtype == dtype
    want = check_against_standin(hip, points, faces[:700], raster, fill=-2.5)
    assert 0 < want["stats"][0] < 700 and (want["values"] == -2.5).any()


def test_three_bands_and_float64_values_float32_cannot_hold(hip, scene):
    points, faces, raster, _ = scene
    band0 = raster.data[0].astype(np.float64)
    bands = np.stack([band0, band0 + 1.0 / 3.0, np.where(band0 > 55.0, rs.RANDOM_NODATA, 1e-300)])
    three = PlanarRaster(bands, raster.transform, rs.RANDOM_NODATA)
    want = check_against_standin(hip, points, faces, three)
    assert want["values"].shape == (4000, 3) and (want["values"][:, 2] == 1e-300).any() and np.isnan(want["values"][:, 2]).any()
    assert same(want["height"], rs.sample_raster_np(points, faces, bands[0], three.inverse, rs.RANDOM_NODATA, NAN)["height"])
    check_against_standin(hip, points, faces[:65], PlanarRaster(bands.astype(np.float32), raster.transform, rs.RANDOM_NODATA))


def test_non_finite_and_huge_coordinates_are_outside(hip):
    raster = PlanarRaster(rs.HAND_DATA, rs.HAND_TRANSFORM, rs.HAND_NODATA)
    specials = [NAN, np.inf, -np.inf, 1e300, -1e300]
    points = np.array([[x, 19.75, 1.0] for x in specials] + [[10.25, y, 1.0] for y in specials] + [[s, s, 1.0] for s in specials]
                      + [[10.25, 19.75, NAN], [10.25, 19.75, np.inf], [10.25, 19.75, 2.0]])
    want = check_against_standin(hip, points, None, raster, fill=-1.0)
    assert want["stats"].tolist() == [3, 15, 0, 0] and (want["values"][:15, 0] == -1.0).all() and want["height"][17] == -99.0
    # as corners of faces: the centre inherits the non-finite coordinate; 1e300 + (-1e300) is a finite centre again
    faces = np.array([[0, 17, 17], [3, 4, 17], [5, 17, 17], [16, 17, 17], [17, 17, 17], [3, 3, 3]], dtype=np.int32)
    want = check_against_standin(hip, points, faces, raster, fill=-1.0)
    assert want["inside"].tolist() == [False, False, False, True, True, False]


def test_last_vertex_and_bad_indices(hip, scene):
    points, faces, raster, want = scene
    V = len(points)
    last = np.array([[V - 1, V - 1, V - 1], [0, 1, V - 1]], dtype=np.int32)
    check_against_standin(hip, points, last, raster)
    bad = faces[:130].copy()
    bad[5, 1] = V
    bad[64, 0] = -1
    bad[129, 2] = np.iinfo(np.int32).max
    with pytest.raises(ValueError, match=f"3 faces name a vertex outside \\[0, {V}\\)"):
        hip.sample_raster(points, bad, raster.data, raster.inverse, raster.nodata, NAN)
    labels = np.zeros(130)
    got = check_against_standin(hip, points, bad, raster, labels=labels, threshold=1e9, ground_id=4.0)
    assert got["stats"][3] == 3 and np.isnan(got["height"][[5, 64, 129]]).all() and np.isnan(got["values"][[5, 64, 129], 0]).all()
    assert got["labels"][[5, 64, 129]].tolist() == [0.0, 0.0, 0.0]   # a face without a height keeps its label
    good = np.ones(130, dtype=bool)
    good[[5, 64, 129]] = False
    assert same(got["values"][good], want["values"][:130][good])
    # without a nodata the "outside" value of a bad face is 0.0
    plain = PlanarRaster(raster.data, raster.transform)
    assert check_against_standin(hip, points, bad, plain)["values"][[5, 64, 129], 0].tolist() == [0.0, 0.0, 0.0]


def test_each_output_alone_and_none(hip, scene):
    points, faces, raster, want = scene
    labels = np.where(np.arange(4000) % 7 == 0, NAN, np.arange(4000) % 3).astype(np.float64)
    relabel = rs.sample_raster_np(points, faces, raster.data, raster.inverse, raster.nodata, NAN, labels=labels, threshold=2.0,
                                  ground_id=9.0, only_existing=True)
    call = lambda **kw: hip.sample_raster(points, faces, raster.data, raster.inverse, raster.nodata, NAN, **kw)  # noqa: E731
    values, height, lab, stats = call(want_values=True, want_height=False)
    assert height is None and lab is None and same(host(values), want["values"]) and host(stats).tolist() == want["stats"].tolist()
    values, height, lab, stats = call(want_values=False, want_height=True)
    assert values is None and lab is None and same(host(height), want["height"])
    values, height, lab, stats = call(want_values=False, want_height=False, labels=labels, threshold=2.0, ground_id=9.0, only_existing=True)
    assert values is None and height is None and same(host(lab), relabel["labels"]) and host(stats).tolist() == relabel["stats"].tolist()
    values, height, lab, stats = call(want_values=False, want_height=False)
    assert values is None and height is None and lab is None and host(stats).tolist() == want["stats"].tolist()
    values, height, lab, stats = call(want_values=True, want_height=True, labels=labels, threshold=2.0, ground_id=9.0, only_existing=True)
    assert same(host(values), want["values"]) and same(host(height), want["height"]) and same(host(lab), relabel["labels"])
    assert same(labels[::7], np.full(len(labels[::7]), NAN))   # the caller's numpy labels were copied, not touched
    with pytest.raises(ValueError, match="threshold and ground_id"):
        call(labels=labels)


@pytest.mark.parametrize("only_existing", [False, True])
def test_relabel_in_place_on_a_device_tensor(hip, scene, only_existing):
    import torch

    points, faces, raster, want = scene
    start = np.where(np.arange(4000) % 5 == 0, NAN, np.arange(4000) % 4).astype(np.float64)
    start[7] = np.inf   # not finite: kept by "only existing"
    threshold = float(np.nanmedian(want["height"]))
    relabel = rs.sample_raster_np(points, faces, raster.data, raster.inverse, raster.nodata, NAN, labels=start, threshold=threshold,
                                  ground_id=NAN if only_existing else 11.0, only_existing=only_existing)
    tensor = torch.as_tensor(start.reshape(-1, 1).copy()).to(hip.device)
    _, _, got, stats = hip.sample_raster(points, faces, raster.data, raster.inverse, raster.nodata, NAN, want_values=False,
                                         labels=tensor, threshold=threshold, ground_id=NAN if only_existing else 11.0,
                                         only_existing=only_existing)
    assert got.data_ptr() == tensor.data_ptr() and got.shape == (4000, 1)
    assert same(host(tensor)[:, 0], relabel["labels"]) and host(stats).tolist() == relabel["stats"].tolist()
    assert 0 < relabel["stats"][2] < 4000 and not same(relabel["labels"], start)
    # height == threshold is not ground
    exact = float(want["height"][np.isfinite(want["height"])][0])
    at = rs.sample_raster_np(points, faces, raster.data, raster.inverse, raster.nodata, NAN, labels=np.zeros(4000), threshold=exact,
                             ground_id=1.0)
    lab = host(hip.sample_raster(points, faces, raster.data, raster.inverse, raster.nodata, NAN, want_values=False,
                                 labels=np.zeros(4000), threshold=exact, ground_id=1.0)[2])
    assert same(lab, at["labels"]) and lab[want["height"] == exact].tolist() == [0.0] * int((want["height"] == exact).sum())


def test_the_argmax_tensor_is_relabelled_without_leaving_the_device(hip, scene):
    points, faces, raster, want = scene
    votes = np.random.default_rng(2).integers(0, 3, (4000, 4)).astype(np.float64)
    votes[::9] = 0.0   # no votes: NaN
    mesh = TexturedPhotogrammetryMesh((np.ascontiguousarray(points), faces), IDs_to_labels={0: "a", 1: "b", 2: "c", 3: "d"},
                                      log_level="ERROR", backend=hip)
    classes = hip.argmax_nonzero(votes)
    before = host(classes).copy()
    got = mesh.label_ground_class(raster, 3.0, labels=classes, ground_class_name="GROUND", points_in_raster_CRS=points)
    assert got is classes and got.is_cuda and mesh.IDs_to_labels[4] == "GROUND"
    ground = (want["height"] < 3.0) & np.isfinite(before)
    assert same(host(classes), np.where(ground, 4.0, before)) and mesh.last_raster_stats["ground"] == ground.sum() > 0
    # the numpy path of the same method, and its boolean mask
    labels = before.copy()
    assert mesh.label_ground_class(raster, 3.0, labels=labels, ground_class_name="GROUND", points_in_raster_CRS=points) is labels
    assert same(labels, host(classes))
    assert same(mesh.get_height_above_ground(raster, threshold=3.0, points_in_raster_CRS=points), want["height"] < 3.0)
    values, q = mesh.get_values_from_raster_file(raster, return_mesh_points=True, points_in_raster_CRS=points)
    assert same(values, want["values"][:, 0]) and same(q, want["queries"]) and same(q[:, 2] - values, want["height"])


def test_errors_of_the_call(hip, scene):
    import ctypes

    points, faces, raster, _ = scene
    assert hip.sample_raster(points, faces[:0], raster.data, raster.inverse, raster.nodata, NAN)[0].shape == (0, 1)
    empty = hip.sample_raster(np.zeros((0, 3)), None, raster.data, raster.inverse, raster.nodata, NAN, want_height=True)
    assert empty[0].shape == (0, 1) and empty[1].shape == (0,) and host(empty[3]).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="points must be"):
        hip.sample_raster(points[:, :2], faces, raster.data, raster.inverse, raster.nodata, NAN)
    with pytest.raises(ValueError, match="six coefficients"):
        hip.sample_raster(points, faces, raster.data, raster.inverse[:5], raster.nodata, NAN)
    # the library's own checks, through the raw call
    import torch

    p = torch.as_tensor(points).to(hip.device)
    f = torch.as_tensor(faces).to(hip.device)
    r = torch.as_tensor(raster.data).to(hip.device)
    stats = torch.zeros(4, dtype=torch.int64, device=hip.device)
    inv = (ctypes.c_double * 6)(*raster.inverse)

    def raw(points_ptr=p.data_ptr(), F=len(faces), faces_ptr=f.data_ptr(), raster_ptr=r.data_ptr(), dtype=1, B=1, H=30, W=40,
            inv_ptr=ctypes.addressof(inv), stats_ptr=stats.data_ptr(), V=len(points)):
        hip._call("gr_sample_raster", points_ptr, V, faces_ptr, F, raster_ptr, dtype, B, H, W, inv_ptr, 0, 0.0, 0.0, None, None, None,
                  0.0, 0.0, 0, stats_ptr, hip._stream())

    raw()   # no output asked for: only the statistics
    assert stats.cpu().tolist()[0] > 0
    raw(F=0)   # N = 0 is fine
    for kw in (dict(points_ptr=None), dict(raster_ptr=None), dict(inv_ptr=None), dict(stats_ptr=None), dict(faces_ptr=None),
               dict(F=-1), dict(V=-1), dict(B=0), dict(H=0), dict(W=-3), dict(dtype=0), dict(dtype=7)):
        with pytest.raises(ValueError, match="gr_sample_raster"):
            raw(**kw)


def test_heights_become_a_texture_and_render(hip):
    (points, faces), cams = synthetic.config1_scene()
    lo, hi = points[:, :2].min(axis=0), points[:, :2].max(axis=0)
    nx, ny = int(np.ceil(hi[0] - lo[0])) + 1, int(np.ceil(hi[1] - lo[1])) + 1
    data = np.random.default_rng(4).uniform(-3.0, -1.0, (ny, nx)).astype(np.float32)
    raster = PlanarRaster(data, (1.0, 0.0, float(np.floor(lo[0])), 0.0, -1.0, float(np.floor(lo[1])) + ny))
    mesh = TexturedPhotogrammetryMesh((points, faces), log_level="ERROR", backend=hip)
    height = mesh.get_height_above_ground(raster, points_in_raster_CRS=points)
    want = rs.sample_raster_np(points, faces, raster.data, raster.inverse, None, NAN)
    assert same(height, want["height"]) and np.isfinite(height).all() and mesh.last_raster_stats["inside"] == len(faces)
    mesh.set_texture(height)
    render = next(mesh.render_flat(cams[0:1], render_img_scale=0.25, apply_distortion=False))
    ids = mesh.pix2face(cams[0:1], render_img_scale=0.25, apply_distortion=False)[0]
    assert (ids >= 0).any() and same(render[..., 0], np.where(ids >= 0, height[np.maximum(ids, 0)], NAN))
