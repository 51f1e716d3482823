"""The two picture calls under the stream contract of include/geograster.h (tests/stream_probe.py).  gr_shade_view and
gr_composite_labels take their stream as a field of a descriptor, so they are not among the functions whose last parameter is
`void *stream` and the table of tests/test_stream_contract_gpu.py does not list them; they are held to the same contract here, with
the legs of that table's rows: (a) alone on a side stream, (b) with the default stream held, (c) with their inputs zeroed until a delay
on their own stream has passed, (d) both; outputs fenced and poisoned, compared with the numpy stand-in byte for byte.  Neither
call synchronises: leg A must count for every one of their calls."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import vis_standin as vs  # noqa: E402
from geograypher_amd.utils import colormaps  # noqa: E402
from tests import stream_probe as sp  # noqa: E402
from tests.test_vis_gpu import random_composite_case, shade_planes  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    backend = sp.StreamProbeHipRaster(0)
    yield backend
    backend.close()


@pytest.fixture(scope="module")
def side(probe):
    sp.cycles_per_second(probe.device)
    return sp.pick_side_stream(probe.device)


@pytest.fixture(scope="module")
def scenes():
    """Inputs and the stand-in's answers: computed once, outside every hold, never written to.  Zeroed inputs give other bytes:
    zero ids are face 0 everywhere, a zero photo is black."""
    rng = np.random.default_rng(41)
    s = {}
    ids, depth, rgb, light = shade_planes(rng, 17, 65, 2)
    s["shade"] = dict(args=(ids, depth, rgb, light, 2, 2, 0.75), want=vs.shade_view(ids, depth, rgb, light, 2, 2, 0.75))
    verts = (rng.normal(size=(90, 3)) * 5.0).astype(np.float32)
    faces = rng.integers(0, 90, (257, 3)).astype(np.int32)
    d = np.array([0.0, 0.6, -0.8])
    s["light"] = dict(args=(verts, faces, d, 0.3), want=vs.face_light(verts, faces, d, 0.3))
    assert len(np.unique(s["light"]["want"])) > 8
    s["composite"] = []
    for kind in (0, 2):
        case = random_composite_case(rng, 17, 257, kind)
        s["composite"].append(dict(args=case, want=vs.composite(*case)))
    photo = s["composite"][0]["args"][0]
    assert photo.dtype == np.uint8 and photo.any() and colormaps.table("tab10").shape == (10, 3)
    return s


def row_shade_view(p, s):
    got = p.shade_view(*s["shade"]["args"]).cpu().numpy()
    assert np.array_equal(got, s["shade"]["want"])
    light = p.face_light(*s["light"]["args"]).cpu().numpy()
    assert np.array_equal(light, s["light"]["want"])


def row_composite_labels(p, s):
    for case in s["composite"]:
        got = p.composite_labels(*case["args"]).cpu().numpy()
        assert np.array_equal(got, case["want"])


ROWS = {"shade_view": ("gr_shade_view", row_shade_view, 2), "composite_labels": ("gr_composite_labels", row_composite_labels, 2)}


@pytest.mark.parametrize("name", list(ROWS))
def test_row(probe, side, scenes, name):
    function, body, n_calls = ROWS[name]
    record = sp.run_row(probe, side, name, lambda p: body(p, scenes))
    assert record["held"] is True
    assert record["calls"] == [function] * n_calls
    assert len(record["leg_a"]) == 2 * n_calls
    waited = {call.waited for call in record["leg_a"]}
    assert waited == {False}, f"{function} waited for its stream: the header says it only enqueues"
