"""tests/context_steps.py -- a catalogue of small calls ("steps") on one raster context and a runner that holds a context to
"any history, same answer".  A helper module (not a conftest); it works with any backend that has the `HipRaster` interface.

A step is a named callable `step(backend) -> dict[str, np.ndarray]`.  It sets EVERY option it depends on, uploads its own mesh,
makes its calls and returns its outputs as host arrays: options persist by contract, so a step never relies on one's current
value.  What a step must return is computed once, on the host, from the project's oracles (oracle_c.raster for ids and depth
bits, oracle_c.project_labels and oracle_np for votes, counts, sums and pairs, the stand-ins for the two stage calls) -- never
from the library under test.  Every output is compared exactly (ids, depth bits, votes, counts, pair tables, status words) or as
its own test compares it: the float sums and the argmax like tests/test_hip_parity.py (`_same`: the same NaNs, equal values),
the reprojected rows like tests/test_reproject_gpu.py (4 x the stand-in's measured error).  No tolerance is set here.

`Step.status` names the words of `last_stats` that do not depend on the context's history (every step sets the slots per tile,
which forgets what the context had learned): the value a FRESH context reports is the expectation (`expected[name]["status"]`,
filled in by the GPU test).  `last_retries` and `rebinned_groups` are history by design: tests/test_learned_table_gpu.py.

The scenes are those of tests/test_context_buffers_gpu.py::_scene: mesh A 15 x 15 quads (450 faces), mesh B 31 x 31 quads
(1922 faces), images of 32 x 32, 96 x 64 and 130 x 70 (width x height), at most 5 views per step.  A2 is A with other vertices:
a mesh the face count alone cannot tell from A.
"""
import functools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import crs_standin as cs  # noqa: E402
import outline_standin as osn  # noqa: E402
from covering_standin import points_bounds_np  # noqa: E402

from geograypher_amd import _hip  # noqa: E402
from geograypher_amd.utils import synthetic  # noqa: E402
from geograypher_amd.utils.geospatial import crs_tuple  # noqa: E402
from oracle import oracle_c, oracle_np  # noqa: E402

STATUS_WORDS = ("max_entries", "overflow", "views_done", "overflow_causes")
UTM, GEO = "EPSG:32610", "EPSG:4326"


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _mesh(n, shift=0.0):
    verts_q, faces, _ = osn.grid_mesh(n, n)
    xy = verts_q / 1e6
    z = np.zeros(len(xy)) if not shift else 0.4 * np.sin(xy[:, 0] * 0.9) * np.cos(xy[:, 1] * 0.7)
    points = np.column_stack([xy[:, 0] + shift, xy[:, 1], z])
    return points.astype(np.float32), faces.astype(np.int32)


def _views(mesh, poses, h, w, order="r1", depth=False):
    points, faces = mesh
    recs = synthetic.camera_set_from_poses(poses, 30.0 * w / 32, w, h).get_raster_records(1.0, near=0.05)
    out = [oracle_c.raster(points, faces, recs[v], h, w, want_depth=depth, vertex_order=order) for v in range(len(poses))]
    s = dict(points=points, faces=faces, recs=recs, h=h, w=w, F=faces.shape[0])
    if depth:
        s["ids"], s["depth"] = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    else:
        s["ids"] = np.stack(out)
    return s


POSES_A = [synthetic.nadir_pose(7.5, 7.5, 20.0), synthetic.nadir_pose(6.0, 8.0, 16.0, yaw_deg=30.0),
           synthetic.nadir_pose(8.5, 6.5, 18.0, yaw_deg=-50.0), synthetic.nadir_pose(7.0, 7.0, 24.0, yaw_deg=75.0, tilt_x_deg=4.0),
           synthetic.nadir_pose(9.0, 8.0, 15.0, yaw_deg=-15.0, tilt_y_deg=-3.0)]
POSES_B = [synthetic.nadir_pose(15.5, 15.5, 40.0), synthetic.nadir_pose(12.0, 17.0, 33.0, yaw_deg=30.0),
           synthetic.nadir_pose(17.0, 14.0, 36.0, yaw_deg=-50.0), synthetic.nadir_pose(14.0, 14.0, 45.0, yaw_deg=75.0, tilt_x_deg=4.0),
           synthetic.nadir_pose(18.0, 16.0, 30.0, yaw_deg=-15.0, tilt_y_deg=-3.0)]
POSES_FAR = [synthetic.nadir_pose(30.0, 24.0, 150.0, yaw_deg=10.0)]   # the whole of B in one 64 x 32 tile of the 96 x 64 image


@functools.lru_cache(maxsize=None)
def scene(name):
    a, a2, b = _mesh(15), _mesh(15, shift=0.375), _mesh(31)
    if name == "A32":
        return _views(a, POSES_A, 32, 32)
    if name == "A130gl":   # (the two vertex orders differ in two pixels of view 1 here; at 32 x 32 and 96 x 64 in none)
        return _views(a, POSES_A[:3], 70, 130, order="gl")
    if name == "A96":
        return _views(a, POSES_A[:2], 64, 96, depth=True)
    if name == "A2_32":
        return _views(a2, POSES_A[:3], 32, 32)
    if name == "B32":
        return _views(b, POSES_B[:2], 32, 32)
    if name == "B96":
        return _views(b, POSES_B[:2], 64, 96)
    if name == "B130":
        return _views(b, POSES_B, 70, 130)
    if name == "Bfar":
        return _views(b, POSES_FAR, 64, 96)
    raise KeyError(name)


def _labels(s, C, views):
    return np.stack([synthetic.synthetic_labels(s["ids"][v], v, C) for v in views])


def _votes(s, C, views):
    want_v, want_c = np.zeros((s["F"], C), dtype=np.uint32), np.zeros(s["F"], dtype=np.uint32)
    labels = _labels(s, C, views)
    for k, v in enumerate(views):
        oracle_c.project_labels(s["ids"][v], labels[k], s["F"], C, want_v, want_c, neg1_is_last_face=True)
    return want_v, want_c


# ---- options ---------------------------------------------------------------------------------------------------------------------
def set_options(backend, thl=5, cap=512, var=0, batch=64, order="r1"):
    """Every option a raster call depends on, explicitly (a backend without options -- the host oracle -- has the order alone)."""
    if hasattr(backend, "set_option"):
        backend.set_option(_hip.GR_OPT_TILE_H_LOG2, thl)
        backend.set_option(_hip.GR_OPT_VARIANT, var)
        backend.set_option(_hip.GR_OPT_BATCH, batch)
        backend.set_option(_hip.GR_OPT_DIRECT_BUDGET_MB, 24 << 10)
        backend.set_option(_hip.GR_OPT_DEBUG, 0)
        backend.set_option(_hip.GR_OPT_DIRECT_CAP, cap)   # (forgets what the context has learned)
    backend.set_vertex_order(order)


def _upload(backend, s):
    backend.upload_mesh(s["points"], s["faces"])


# ---- the steps -------------------------------------------------------------------------------------------------------------------
class Step:
    """name; run(backend) -> outputs; want() -> the oracle's outputs; same: the outputs compared like test_hip_parity's `_same`;
    close: output -> a check(got, want) of its own; status: the history-free words of `last_stats`.  (A step that is about an
    option gives the same outputs on a backend without options, the host oracle: `set_options`.)"""

    def __init__(self, name, run, want, same=(), close=None, status=()):
        self.name, self.run, self._want, self.same, self.close = name, run, want, tuple(same), dict(close or {})
        self.status = tuple(status)

    @functools.lru_cache(maxsize=None)
    def want(self):
        return {k: np.asarray(v) for k, v in self._want().items()}


def _ids_step(name, scene_name, views, depth=False, **opts):
    def run(b):
        s = scene(scene_name)
        set_options(b, **opts)
        _upload(b, s)
        try:
            got = b.raster_face_ids(s["recs"][views], s["h"], s["w"], want_depth=depth)
        finally:
            if opts.get("order", "r1") != "r1":
                b.set_vertex_order("r1")
        if depth:
            return {"ids": _np(got[0]), "depth_bits": _np(got[1]).view(np.int32)}
        return {"ids": _np(got)}

    def want():
        s = scene(scene_name)
        out = {"ids": s["ids"][views]}
        if depth:
            out["depth_bits"] = s["depth"][views].view(np.int32)
        return out

    return Step(name, run, want, status=STATUS_WORDS)


def _fused_step(name, scene_name, views, C, **opts):
    def run(b):
        s = scene(scene_name)
        set_options(b, **opts)
        _upload(b, s)
        votes, counts = b.new_vote_buffers(C)
        b.raster_project_labels(s["recs"][views], _labels(s, C, views), C, votes, counts)
        return {"votes": _np(votes).view(np.uint32), "counts": _np(counts).view(np.uint32)}

    def want():
        v, c = _votes(scene(scene_name), C, views)
        return {"votes": v, "counts": c}

    return Step(name, run, want, status=STATUS_WORDS)


def _float_images():
    s = scene("A32")
    rng = np.random.default_rng(31)
    img = rng.normal(0.0, 1.0, (3, 32, 32, 2))
    img[rng.random(img.shape) < 0.1] = np.nan
    return s, img


def _run_values(b):
    import torch

    s, img = _float_images()
    set_options(b)
    _upload(b, s)
    sums = torch.zeros((s["F"], 2), dtype=torch.float64, device=b.device)
    counts = torch.zeros((s["F"],), dtype=torch.int32, device=b.device)
    b.project_values(s["ids"][:3], img, sums, counts)
    avg, summed, cnt = b.finalize_sums(sums, counts)
    return {"avg": _np(avg), "summed": _np(summed), "counts": _np(cnt)}


def _want_values():
    s, img = _float_images()
    projs = [oracle_np.project_image(s["ids"][v].astype(np.int64), img[v], s["F"], neg1_is_last_face=True) for v in range(3)]
    with np.errstate(invalid="ignore"):
        avg, rest = oracle_np.aggregate(projs, s["F"])
    return {"avg": avg, "summed": rest["summed_projections"], "counts": rest["projection_counts"]}


NC = 5


def _class_images():
    s = scene("A32")
    cls = np.random.default_rng(9).integers(0, NC, (3, 32, 32)).astype(np.float64)
    cls[np.random.default_rng(10).random(cls.shape) < 0.2] = np.nan
    return s, cls


def _index_pairs(ids, cls, F):
    """derived_meshes.py:470-520 as sorted (face * NC + class) keys with multiplicities, and the per-face counts."""
    counts, keys = np.zeros(F, dtype=np.int64), []
    for v in range(ids.shape[0]):
        p = oracle_np.project_image(ids[v].astype(np.int64), cls[v][..., None], F, neg1_is_last_face=True)
        inds = np.nonzero(np.isfinite(p[:, 0]))[0]
        counts[inds] += 1
        keys.append(inds.astype(np.int64) * NC + p[inds, 0].astype(np.int64))
    uniq, mult = np.unique(np.concatenate(keys), return_counts=True)
    return {"keys": uniq, "mult": mult.astype(np.int64), "counts": counts}


def _run_pairs(b):
    import torch

    s, cls = _class_images()
    set_options(b)
    _upload(b, s)
    counts = torch.zeros((s["F"],), dtype=torch.int32, device=b.device)
    keys, mult = b.project_index_pairs(s["ids"][:3], cls, NC, counts)
    return {"keys": keys, "mult": mult, "counts": _np(counts)}


RECTS = np.array([[2, 3, 20, 18, 1], [10, 10, 30, 31, 3], [0, 0, 32, 32, 0], [5, 20, 16, 32, 4], [12, 0, 13, 9, 2],
                  [25, 25, 32, 32, 1]], dtype=np.int32)
RECT_OFFSETS = np.array([0, 2, 2, 6])   # view 1 has no rectangle, view 2 is painted all over first


def _painted():
    img = np.full((3, 32, 32), np.nan)
    for v in range(3):
        for i0, j0, i1, j1, c in RECTS[RECT_OFFSETS[v]:RECT_OFFSETS[v + 1]].tolist():
            img[v, i0:i1, j0:j1] = c
    return img


def _run_rects(b):
    import torch

    s = scene("A32")
    set_options(b)
    _upload(b, s)
    counts = torch.zeros((s["F"],), dtype=torch.int32, device=b.device)
    acc = b.new_pair_accumulator(NC, counts)
    acc.add_rects(s["ids"][:2], RECTS[:2], RECT_OFFSETS[:3])
    acc.add_rects(s["ids"][2], RECTS[2:], np.array([0, 4]))
    keys, mult = acc.finish()
    return {"keys": keys, "mult": mult, "counts": _np(counts)}


def _argmax_input():
    rng = np.random.default_rng(17)
    arr = rng.integers(0, 4, (450, 7)).astype(np.float64)
    arr[rng.random(arr.shape) < 0.3] = 0.0
    arr[::13] = 0.0
    arr[5, 2] = np.nan
    return arr


def _utm_rows():
    rng = np.random.default_rng(65)
    return np.column_stack([552000.0 + rng.uniform(0, 4000, 65), 4182000.0 + rng.uniform(0, 4000, 65), rng.uniform(0, 300, 65)])


def _run_stage(b):
    s = scene("B32")
    set_options(b)
    bounds, bad = b.points_bounds(s["points"].astype(np.float64))
    out, stats = b.reproject_points(_utm_rows(), UTM, GEO)
    return {"bounds": _np(bounds), "nonfinite": _np(bad).reshape(-1), "geo": _np(out), "crs_stats": _np(stats)}


def _want_stage():
    s = scene("B32")
    bounds, bad = points_bounds_np(s["points"].astype(np.float64), 1)
    geo, st = cs.reproject(_utm_rows(), crs_tuple(UTM), crs_tuple(GEO))
    return {"bounds": bounds, "nonfinite": np.array([bad]), "geo": geo, "crs_stats": cs.stats_of(st)}


def _geo_close(got, want):
    """tests/test_reproject_gpu.py: NaN on the flagged rows alone, the rest within 4 x the stand-in's own measured error"""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    worst, bound = cs.worst_errors(got, want, "geo"), cs.bounds(cs.load_golden(), 4.0)
    assert (worst <= bound).all(), (worst, bound)


def _run_refused(b):
    s = scene("A32")
    set_options(b)
    _upload(b, s)
    votes, counts = b.new_vote_buffers(3)
    try:
        b.raster_project_labels(s["recs"][:3], _labels(s, 3, [0, 1]), 3, votes, counts)   # three cameras, two label planes
    except ValueError:
        return {"refused": np.array([1]), "votes": _np(votes).view(np.uint32)}
    return {"refused": np.array([0]), "votes": _np(votes).view(np.uint32)}


V3, V5 = [0, 1, 2], [0, 1, 2, 3, 4]
CATALOGUE = [
    _ids_step("ids A 32x32", "A32", V3),
    _ids_step("ids+depth A 96x64", "A96", [0, 1], depth=True),
    _ids_step("ids B 32x32", "B32", [0, 1]),
    _ids_step("ids B 130x70 batch 2", "B130", V5, batch=2),                       # three launch groups
    _fused_step("fused A 1 view C=3", "A32", [0], 3),
    _fused_step("fused A 5 views batch 2 C=17", "A32", V5, 17, batch=2),           # side stream, two winner buffers
    _fused_step("fused B 96x64 votes inline", "B96", [0, 1], 3, batch=1, var=_hip.GR_VAR_VOTES_INLINE),
    _ids_step("dense B cap 64", "Bfar", [0], cap=64),                                # looked at, binned again
    _ids_step("dense B cap 64 no look", "Bfar", [0], cap=64, var=_hip.GR_VAR_NO_LOOK),  # GR_EOVERFLOW, status, retry
    _ids_step("ids B chains micro", "B32", [0, 1], var=_hip.GR_VAR_CHAINS | _hip.GR_VAR_MICRO_ALWAYS),
    _ids_step("ids A2 exact binning", "A2_32", V3, cap=0),
    _ids_step("ids A 96x64 tile height 6", "A96", [0, 1], thl=6,
              var=_hip.GR_VAR_ONE_TILE | _hip.GR_VAR_ENT48 | _hip.GR_VAR_GENERAL_IDS),
    _ids_step("ids A 130x70 gl order", "A130gl", V3, order="gl"),
    Step("project_values A", _run_values, _want_values, same=("avg", "summed", "counts")),
    Step("project_index_pairs A", _run_pairs, lambda: _index_pairs(scene("A32")["ids"][:3], _class_images()[1], 450)),
    Step("rect pairs A", _run_rects, lambda: _index_pairs(scene("A32")["ids"][:3], _painted(), 450)),
    Step("argmax_nonzero", lambda b: {"argmax": _np(b.argmax_nonzero(_argmax_input()))},
         lambda: {"argmax": oracle_np.find_argmax_nonzero_value(_argmax_input())}, same=("argmax",)),
    Step("bounds then reproject 65", _run_stage, _want_stage, close={"geo": _geo_close}),
    Step("refused fused A", _run_refused, lambda: {"refused": np.array([1]), "votes": np.zeros((450, 3), dtype=np.uint32)}),
]
STEPS = {s.name: s for s in CATALOGUE}
NAMES = [s.name for s in CATALOGUE]
assert len(STEPS) == len(CATALOGUE)


def expected(names=NAMES):
    """{step: {output: array}} from the oracles (cached: computed once per process and shared, arrays read-only)."""
    out = {}
    for n in names:
        out[n] = dict(STEPS[n].want())
        for a in out[n].values():
            a.setflags(write=False)
    return out


def _same(a, b):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0))


def check(step, got, want, status=None):
    """One step's outputs (and, where `status` holds a backend's `last_stats`, its history-free words) against `want`."""
    outputs = {k: v for k, v in want.items() if k != "status"}
    assert set(got) == set(outputs), (sorted(got), sorted(outputs))
    for key, w in outputs.items():
        g = np.asarray(got[key])
        assert g.shape == w.shape, (key, g.shape, w.shape)
        if key in step.close:
            step.close[key](g, w)
        elif key in step.same:
            _same(g.astype(np.float64), w.astype(np.float64))
        else:
            bad = np.argwhere(g != w)
            assert bad.size == 0, f"{key}: {len(bad)} values differ, first at {bad[0].tolist()}"
    if status is not None and "status" in want:
        got_words = {k: status.get(k) for k in step.status}
        assert got_words == want["status"], (got_words, want["status"])


def run(backend, names, expected, history=None):
    """Run the named steps in order on `backend` and check each one.  `history` (a list, extended in place) holds what ran on the
    context before; a mismatch names the whole list of steps so far, so that `run(fresh_backend, <that list>, expected)` replays it."""
    history = [] if history is None else history
    for name in names:
        step = STEPS[name]
        history.append(name)
        try:
            got = step.run(backend)
            check(step, got, expected[name], getattr(backend, "last_stats", None) if step.status else None)
        except AssertionError as e:
            raise AssertionError(f"step {name!r} differs after {len(history) - 1} earlier steps; replay: {history!r}\n{e}") from None
    return history


SEEDS = (11, 12, 13, 14, 15, 16, 17, 18)
SEQUENCE_LENGTH = 60


def pair_sequence(first):
    """X, Y for every Y of the catalogue, on one context: every ordered pair that starts with X is adjacent once."""
    return [name for y in NAMES for name in (first, y)]


def seeded_sequence(seed, n=SEQUENCE_LENGTH):
    return [NAMES[k] for k in np.random.default_rng(seed).integers(0, len(NAMES), n)]
