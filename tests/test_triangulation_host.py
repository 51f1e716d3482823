"""Host layer of the multiview-detection workflow against the reference goldens (tests/golden/reference_triangulation.npz),
with the numpy stand-in of tests/ray_standin.py in place of the two device calls.  No GPU."""
import ctypes
import json

import numpy as np
import pytest

from geograypher_amd.cameras.cameras import PhotogrammetryCamera, PhotogrammetryCameraSet
from geograypher_amd.predictors.derived_segmentors import TabularRectangleSegmentor
from geograypher_amd.utils import geometric, numeric, synthetic
from tests.conftest import GOLDEN
from tests.ray_standin import StandInBackend, all_pairs_distance

BACKEND = StandInBackend()
SIGMA = 0.15   # detection_survey's default aim noise, metres per axis


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "reference_triangulation.npz", allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("scene", ["a", "b", "c"])
def test_stand_in_and_host_closest_points_are_pinned_to_the_reference(gold, scene):
    """The stand-in (and the package's host form of the same mathematics) against the reference's `dist`: within the bound the
    device is held to -- 4 e_ref of the reference's long-double run, e_ref being the reference's own float64 error -- on the
    survey and shared-origin scenes, where another order of the same operations moves the last bit (the reference sums its
    dot products inside einsum), and bit for bit on the integer scene, NaN pattern included."""
    starts, ends, want = gold[f"{scene}__starts"], gold[f"{scene}__ends"], gold[f"{scene}__dist64"]
    ref_ld = gold[f"{scene}__distld_hi"].astype(np.longdouble) + gold[f"{scene}__distld_lo"].astype(np.longdouble)
    fin = np.isfinite(want)
    for got in (all_pairs_distance(starts, ends), numeric.segment_closest_points(starts, ends, starts, ends)[2]):
        assert np.array_equal(np.isfinite(got), fin)
        if scene == "b":
            assert np.array_equal(got, want, equal_nan=True)
        err = float(np.abs(got.astype(np.longdouble) - ref_ld)[fin].max())
        print(f"scene {scene}: max |d - d_longdouble| {err:.3g}, e_ref {float(gold[f'{scene}__e_ref']):.3g}")
        assert err <= 4 * float(gold[f"{scene}__e_ref"])


@pytest.mark.parametrize("scene", ["a", "c"])
def test_edge_lists_equal_the_references_in_content_and_order(gold, scene, tmp_path):
    starts, ends, ids = gold[f"{scene}__starts"], gold[f"{scene}__ends"], gold[f"{scene}__ids"]
    n_lists = 0
    for k, t in enumerate(gold[f"{scene}__thresholds"]):
        for step in gold[f"{scene}__steps"]:
            for tag, tr in (("none", None), ("sq", lambda x: x ** 2)):
                key = f"{scene}__edges__t{k}__s{step}__{tag}"
                if key not in gold:
                    continue
                ref = gold[key]
                edges = numeric.calc_graph_weights(starts, ends, ids, float(t), step=int(step), transform=tr, backend=BACKEND)
                assert [(i, j) for i, j, _ in edges] == [(int(i), int(j)) for i, j, _ in ref]
                got_w = np.array([w["weight"] for _, _, w in edges])
                # w = 1 / f(d): 8 e_ref between two float64 evaluations of d (4 e_ref each against long double), carried
                # through f (|f'| = 1 or 2 d <= 2 * threshold) and the reciprocal (|dw| = w^2 |df|), plus the rounding of 1 / x
                df = 8 * float(gold[f"{scene}__e_ref"]) * (1.0 if tr is None else 2 * float(t))
                assert np.all(np.abs(got_w - ref[:, 2]) <= df * ref[:, 2] ** 2 + 4 * np.finfo(np.float64).eps * ref[:, 2])
                assert all(type(i) is int and type(j) is int and type(w["weight"]) is float for i, j, w in edges[:3])
                n_lists += 1
    assert n_lists >= 6
    path = numeric.calc_graph_weights(starts, ends, ids, float(t), out_dir=tmp_path, backend=BACKEND)
    assert path == tmp_path / "edge_weights.json"
    assert json.load(path.open()) == [[i, j, w] for i, j, w in numeric.calc_graph_weights(starts, ends, ids, float(t),
                                                                                          backend=BACKEND)]


def test_host_steps_after_the_device_call(gold):
    starts, ends, ids = gold["b__starts"], gold["b__ends"], gold["b__ids"]
    i, j, w = numeric.ray_pair_edges(starts, ends, ids, 0.0, backend=BACKEND)
    assert len(i) > 0 and np.all(w == 1 / 1e-6)                       # d = 0 -> min_dist
    i2, j2, w2 = numeric.ray_pair_edges(starts, ends, ids, 0.0, transform=lambda x: x ** 2, backend=BACKEND)
    assert np.array_equal(i2, i) and np.all(w2 == 1 / (1e-6 ** 2))     # the floor comes BEFORE the transform
    i3, _, _ = numeric.ray_pair_edges(starts, ends, ids, 2.5, transform=lambda x: np.where(x > 1, np.nan, x), backend=BACKEND)
    i4, _, _ = numeric.ray_pair_edges(starts, ends, ids, 1.0, backend=BACKEND)
    assert np.array_equal(i3, i4)                                      # non-finite after the transform: dropped
    with pytest.raises(ValueError, match="elementwise"):
        numeric.ray_pair_edges(starts, ends, ids, 1.0, transform=lambda x: x[:1], backend=BACKEND)
    assert numeric.calc_graph_weights(starts[:0], ends[:0], ids[:0], 1.0, backend=BACKEND) == []


def test_intersection_average_and_scale(gold):
    for scene in ("a", "b"):
        inds = gold[f"{scene}__avg_inds"]
        got = numeric.intersection_average(gold[f"{scene}__starts"][inds], gold[f"{scene}__ends"][inds])
        assert np.abs(got - gold[f"{scene}__avg"]).max() <= 1e-12 * 300   # a mean of ~10^2-10^3 float64 points up to 300
    T = np.diag([2.0, 2.0, 2.0, 1.0])
    assert geometric.get_scale_from_transform(None) == 1 and geometric.get_scale_from_transform(T) == pytest.approx(2.0)
    with pytest.raises(ValueError, match="Transform shape"):
        geometric.get_scale_from_transform(np.eye(3))


def test_communities_with_a_seed(gold, tmp_path):
    s = synthetic.detection_survey()
    starts, ends, ids = s["ray_starts"], s["ray_ends"], s["ray_IDs"]
    edges = numeric.calc_graph_weights(starts, ends, ids, 0.5, backend=BACKEND)
    res = numeric.calc_communities(starts, ends, edges, louvain_resolution=2.0, seed=0)
    labels, points = res["ray_IDs"], res["community_points"]
    nodes = sorted({i for i, _, _ in edges} | {j for _, j, _ in edges})
    assert np.array_equal(np.nonzero(~np.isnan(labels))[0], nodes)        # ids cover exactly the graph's nodes
    sizes = [int((labels == c).sum()) for c in range(len(points))]
    assert sizes == sorted(sizes, reverse=True) and min(sizes) >= 2 and sum(sizes) == len(nodes)
    for c in range(len(points)):
        inds = np.nonzero(labels == c)[0]
        # the community's node order is networkx's; the mean over all ordered pairs does not depend on it beyond rounding
        assert np.abs(points[c] - numeric.intersection_average(starts[inds], ends[inds])).max() <= 1e-9
    # Recovered points against the truth, for communities whose rays were all aimed at ONE object.  Every ray misses its
    # object by the aim noise, N(0, SIGMA) per axis: |miss| <= 4.5 SIGMA for all ~1200 rays (P(chi_3 > 4.5) = 1.5e-4 each is
    # the generator's own tail; seed 0 has no such ray).  Two rays that both pass within r of a point have their closest
    # points within r (1 + 2 / sin(angle)) of it; cameras 80-120 m up over a 200 m square see an object under angles whose
    # mean 1 / sin is below 3, and the community point is the mean over all pairs: bound 4.5 SIGMA (1 + 2 * 3) / 3 ~ 10 SIGMA,
    # the last 3 for the averaging of at least 10 independent pairs.  1.5 m, where objects are 26 m apart on average.
    pure = 0
    for c in range(len(points)):
        objs = np.unique(s["ray_objects"][labels == c])
        if len(objs) == 1:
            pure += 1
            assert np.linalg.norm(points[c] - s["objects"][objs[0]]) <= 10 * SIGMA
    # Seed 0 of the generator and of Louvain (networkx 3.4, resolution 2): 53 communities, 41 of them pure, every one of the
    # 1 240 rays labelled and every one of the 60 objects present.  (More communities than objects: Louvain at this resolution
    # splits the rays of some objects; the 12 mixed ones join objects whose rays pass within the threshold of each other.)
    assert (len(points), pure) == (53, 41)
    assert not np.isnan(labels).any() and len(np.unique(s["ray_objects"][~np.isnan(labels)])) == 60
    # the golden scene: the labelled rays are the nodes of the reference's graph
    ga = numeric.calc_graph_weights(gold["a__starts"], gold["a__ends"], gold["a__ids"], 0.5, backend=BACKEND)
    ra = numeric.calc_communities(gold["a__starts"], gold["a__ends"], ga, seed=1)
    assert np.array_equal(np.nonzero(~np.isnan(ra["ray_IDs"]))[0], gold["a__graph_nodes"])
    # files, the empty graph, the transform without pyproj
    path = numeric.calc_communities(starts, ends, edges, louvain_resolution=2.0, seed=0, out_dir=tmp_path)
    with np.load(path) as d:
        assert path.name == "communities.npz" and np.array_equal(d["community_points"], points)
    empty = numeric.calc_communities(starts, ends, [], transform_to_epsg_4978=np.eye(4))
    assert empty["ray_IDs"].shape == (0,) and empty["community_points"].shape == (0, 3)
    with_t = numeric.calc_communities(starts, ends, edges, seed=0, transform_to_epsg_4978=np.diag([2.0, 2.0, 2.0, 1.0]))
    try:
        import pyproj  # noqa: F401
    except ImportError:
        assert "community_points_latlon" not in with_t
        assert np.allclose(with_t["community_points_epsg_4978"], 2 * with_t["community_points"])
    else:
        assert with_t["community_points_latlon"].shape == with_t["community_points"].shape


def _golden_cameras(gold):
    with np.load(GOLDEN / "reference_cameras.npz") as g:
        kw = dict(f=float(g["f"]), cx=float(g["cx"]), cy=float(g["cy"]), image_width=int(g["image_width"]),
                  image_height=int(g["image_height"]))
        T0 = g["cam_to_world"].astype(np.float64)
    return T0, kw


def test_cast_rays_matches_the_reference(gold):
    T0, kw = _golden_cameras(gold)
    cam = PhotogrammetryCamera("img0.png", T0, **kw)
    pix = gold["cast__pixels"]
    for got, want in ((cam.cast_rays(pix), gold["cast__len10"]), (cam.cast_rays(pix, line_length=1e3), gold["cast__len1000"]),
                      (PhotogrammetryCamera("img0.png", gold["cast__scaled_transform"], **kw).cast_rays(pix, line_length=7.0),
                       gold["cast__scaled"])):
        assert got.shape == want.shape == (2 * len(pix), 3)
        assert np.abs(got - want).max() <= 16 * np.finfo(np.float64).eps * max(1.0, np.abs(want).max())
    assert cam.cast_rays(np.zeros((0, 2))) is None


def test_calc_line_segments_matches_the_reference(gold, tmp_path):
    _, kw = _golden_cameras(gold)
    cams = PhotogrammetryCameraSet(cameras=[PhotogrammetryCamera(nm, T, **kw)
                                            for nm, T in zip(("img0.png", "img1.png", "img2.png"), gold["seg__transforms"])])
    detector = TabularRectangleSegmentor(GOLDEN / "tabular" / "cols", (40, 60), split_bbox=False)
    seg = cams.calc_line_segments(detector, ray_length_local=25.0)
    lim = cams.calc_line_segments(detector, ray_length_local=25.0, limit_angle_from_vert=float(gold["seg__angle_limit"]))
    for got, prefix in ((seg, "seg__"), (lim, "seg__lim__")):
        assert np.array_equal(got["ray_IDs"], gold[prefix + "ray_IDs"])
        for k in ("ray_starts", "ray_ends"):
            assert np.abs(got[k] - gold[prefix + k]).max() <= 16 * np.finfo(np.float64).eps * np.abs(gold[prefix + k]).max()
    assert 0 < len(lim["ray_IDs"]) < len(seg["ray_IDs"])
    path = cams.calc_line_segments(detector, ray_length_local=25.0, out_dir=tmp_path)
    with np.load(path) as d:
        assert path.name == "line_segments.npz" and np.array_equal(d["ray_starts"], seg["ray_starts"])
    nothing = cams.calc_line_segments(synthetic.CenterDetector({}))
    assert nothing["ray_starts"].shape == (0, 3) and nothing["ray_IDs"].shape == (0,)


def _plane(z_fn):
    return synthetic.boundary_grid(4, z_fn, lo=-100.0, hi=100.0)


def test_clip_line_segments_closed_form():
    rng = np.random.default_rng(0)
    origins = np.column_stack([rng.uniform(-20, 20, 50), rng.uniform(-20, 20, 50), np.full(50, 80.0)])
    directions = np.column_stack([rng.uniform(-0.3, 0.3, 50), rng.uniform(-0.3, 0.3, 50), -np.ones(50)])
    directions /= np.linalg.norm(directions, axis=1, keepdims=True)
    ids = np.arange(50) % 7
    # two horizontal planes: z = 30 and z = -2
    s, e, d, k = geometric.clip_line_segments((_plane(lambda x, y: 30.0 + 0 * x), _plane(lambda x, y: -2.0 + 0 * x)),
                                              origins, directions, ids, backend=BACKEND)
    assert np.array_equal(k, ids)
    assert np.abs(s - (origins + ((30.0 - 80.0) / directions[:, 2])[:, None] * directions)).max() <= 1e-12
    assert np.abs(e - (origins + ((-2.0 - 80.0) / directions[:, 2])[:, None] * directions)).max() <= 1e-12
    assert np.abs(d - directions).max() <= 1e-13
    # a tilted pair: z = 30 + 0.1 x and z = 0.05 y -> t = (c - o_z + a o_x + b o_y) / (d_z - a d_x - b d_y)
    s, e, _, _ = geometric.clip_line_segments((_plane(lambda x, y: 30.0 + 0.1 * x), _plane(lambda x, y: 0.05 * y)),
                                              origins, directions, ids, backend=BACKEND)
    t0 = (30.0 - origins[:, 2] + 0.1 * origins[:, 0]) / (directions[:, 2] - 0.1 * directions[:, 0])
    t1 = (-origins[:, 2] + 0.05 * origins[:, 1]) / (directions[:, 2] - 0.05 * directions[:, 1])
    assert np.abs(s - (origins + t0[:, None] * directions)).max() <= 1e-12
    assert np.abs(e - (origins + t1[:, None] * directions)).max() <= 1e-12
    # ray_limit compares |origin - end|; rays that miss one boundary are dropped; ascending ray index
    far = np.linalg.norm(origins - e, axis=1)
    limit = float(np.median(far))
    _, e2, _, k2 = geometric.clip_line_segments((_plane(lambda x, y: 30.0 + 0.1 * x), _plane(lambda x, y: 0.05 * y)),
                                                origins, directions, ids, ray_limit=limit, backend=BACKEND)
    assert np.array_equal(e2, e[far <= limit]) and np.array_equal(k2, ids[far <= limit]) and 0 < len(k2) < 50
    small = synthetic.boundary_grid(2, lambda x, y: -2.0 + 0 * x, lo=0.0, hi=20.0)   # a floor under some rays only
    s3, e3, _, k3 = geometric.clip_line_segments((_plane(lambda x, y: 30.0 + 0 * x), small), origins, directions, ids,
                                                 backend=BACKEND)
    inside = np.all((e3[:, :2] >= 0) & (e3[:, :2] <= 20), axis=1)
    assert 0 < len(k3) < 50 and inside.all()
    up = geometric.clip_line_segments((_plane(lambda x, y: 30.0 + 0 * x), _plane(lambda x, y: -2.0 + 0 * x)), origins,
                                      -directions, ids, backend=BACKEND)
    assert all(len(x) == 0 for x in up)


def test_clip_line_segments_errors_and_empty():
    plane = _plane(lambda x, y: 0 * x)
    o, d = np.zeros((3, 3)), np.ones((3, 3))
    with pytest.raises(ValueError, match="2 boundaries required, not 1"):
        geometric.clip_line_segments((plane,), o, d, [0, 1, 2], backend=BACKEND)
    with pytest.raises(ValueError, match="pairs required"):
        geometric.clip_line_segments((plane, "mesh"), o, d, [0, 1, 2], backend=BACKEND)
    with pytest.raises(ValueError, match="origins and directions mismatched"):
        geometric.clip_line_segments((plane, plane), o, d[:2], [0, 1, 2], backend=BACKEND)
    with pytest.raises(ValueError, match=r"\(N, 3\) input arrays required"):
        geometric.clip_line_segments((plane, plane), np.zeros((3, 2)), np.zeros((3, 2)), [0, 1, 2], backend=BACKEND)
    with pytest.raises(ValueError, match="origins and image indices mismatched"):
        geometric.clip_line_segments((plane, plane), o, d, [0, 1], backend=BACKEND)
    s, e, dd, k = geometric.clip_line_segments((plane, plane), o[:0], d[:0], [], backend=BACKEND)
    assert s.shape == e.shape == dd.shape == (0, 3) and k.shape == (0,)


def test_triangulate_detections_stages_and_resumption(tmp_path):
    s = synthetic.detection_survey(n_objects=12, n_cameras=20, seed=2)
    cams, det = synthetic.detection_survey_cameras(s)
    bounds = (synthetic.boundary_grid(5, lambda x, y: 30.0 + 0 * x), synthetic.boundary_grid(5, lambda x, y: -2.0 + 0 * x))
    kw = dict(boundaries=bounds, similarity_threshold_meters=0.5, louvain_resolution=2.0, seed=1)
    seg = cams.calc_line_segments(det, boundaries=bounds, backend=BACKEND)
    assert np.array_equal(seg["ray_IDs"], s["ray_IDs"])
    assert np.abs(seg["ray_starts"] - s["ray_starts"]).max() <= 1e-11 and np.abs(seg["ray_ends"] - s["ray_ends"]).max() <= 1e-11
    want = cams.triangulate_detections(det, backend=BACKEND, **kw)
    got = cams.triangulate_detections(det, out_dir=tmp_path, backend=BACKEND, **kw)
    assert np.array_equal(got, want)
    for name in ("line_segments.npz", "edge_weights.json", "communities.npz"):
        assert (tmp_path / name).is_file()

    class Never:   # a stage whose file exists is not computed again: neither the detector nor the backend is asked
        def __getattr__(self, name):
            raise AssertionError(f"{name} was used although the stage file exists")

    (tmp_path / "communities.npz").unlink()
    assert np.array_equal(cams.triangulate_detections(Never(), out_dir=tmp_path, backend=Never(), **kw), want)
    (tmp_path / "communities.npz").unlink()
    (tmp_path / "edge_weights.json").unlink()
    assert np.array_equal(cams.triangulate_detections(Never(), out_dir=tmp_path, backend=BACKEND, **kw), want)
    assert np.array_equal(cams.triangulate_detections(Never(), out_dir=tmp_path, backend=Never(), **kw), want)
    # metres -> local units: a set whose local frame is half scale sees half the threshold and ray length
    half = PhotogrammetryCameraSet(cams.cameras, local_to_epsg_4978_transform=np.diag([2.0, 2.0, 2.0, 1.0]))
    asked = {}

    class Spy(StandInBackend):
        def ray_pair_edges(self, starts, ends, ray_ids, threshold):
            asked["threshold"] = threshold
            return super().ray_pair_edges(starts, ends, ray_ids, threshold)

    half.triangulate_detections(det, backend=Spy(), similarity_threshold_meters=0.5, seed=1)
    assert asked["threshold"] == pytest.approx(0.25, rel=1e-12)   # 0.5 / cbrt(det): the cube root rounds


def test_tile_decode_is_exact():
    """The kernel's own decode of its 1-D grid (gr_ray_pairs_tile), every tile for small grids, the ends of every row for the
    largest."""
    from geograypher_amd import _hip

    lib = _hip.load_library()
    r, c = ctypes.c_int64(), ctypes.c_int64()
    for T in (1, 2, 3, 7, 64, 201):
        k = 0
        for row in range(T):
            for col in range(row, T):
                assert lib.gr_ray_pairs_tile(k, T, ctypes.byref(r), ctypes.byref(c)) == 0
                assert (r.value, c.value) == (row, col)
                k += 1
        assert lib.gr_ray_pairs_tile(k, T, ctypes.byref(r), ctypes.byref(c)) == -1
    T = 32768
    for row in list(range(0, T, 97)) + [T - 2, T - 1]:
        off = row * T - row * (row - 1) // 2
        for k, col in ((off, row), (off + T - row - 1, T - 1)):
            assert lib.gr_ray_pairs_tile(k, T, ctypes.byref(r), ctypes.byref(c)) == 0
            assert (r.value, c.value) == (row, col)
    assert lib.gr_ray_pairs_tile(0, T + 1, ctypes.byref(r), ctypes.byref(c)) == -1


