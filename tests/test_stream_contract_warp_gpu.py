"""The raster -> raster call under the stream contract of include/geograster.h (tests/stream_probe.py).  gr_warp_raster takes its
stream as a field of a descriptor, so it is not among the functions whose last parameter is `void *stream` and the table of
tests/test_stream_contract_gpu.py does not list it; it is held to the same contract here, with the legs of that table's rows: (a) alone
on a side stream, (b) with the default stream held, (c) with its inputs zeroed until a delay on its own stream has passed, (d) both;
outputs fenced and poisoned, compared with the numpy stand-in.  The call does not synchronise: leg A must count for every call."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import warp_raster_standin as ws  # noqa: E402
from geograypher_amd.utils.geospatial import default_warp_grid  # noqa: E402
from geograypher_amd.utils.raster import invert_affine  # noqa: E402
from tests import stream_probe as sp  # noqa: E402

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
    """Inputs and the stand-in's answers: computed once, outside every hold, never written to.  A zeroed source gives other bytes:
    every sample is 0, and the sources hold no 0."""
    rng = np.random.default_rng(43)
    s = {}
    data = rng.integers(1, 256, (4, 29, 37), dtype=np.uint8)
    t = (0.31, 0.02, -2.0, -0.015, 0.33, -1.5)
    inv = invert_affine((1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    s["same"] = []
    for name, kind in (("nearest", ws.NEAREST), ("bilinear", ws.BILINEAR)):
        want, stats, _, _ = ws.warp(data, inv, None, t, (0, 0, 129, 99), resampling=kind, dst_nodata=0.0)
        s["same"].append(dict(args=(data, inv, None, t, (0, 0, 129, 99)), kw=dict(resampling=name, dst_nodata=0.0), want=want, stats=stats))
        assert (want != 0).any()
    standin = ws.WarpStandinBackend()
    name, src, sinv, src_crs, dt, (h, w), dst_crs, _ = ws.cross_scenes(
        lambda d, tr, a, b: default_warp_grid(((d.shape[1], d.shape[2]), tr), a, b, standin))[0]
    want, stats, und, _ = ws.warp(src, sinv, None, dt, (0, 0, w, h), ws._crs(src_crs), ws._crs(dst_crs), ws.NEAREST, -1.0)
    assert not und.any() and (src != 0).all()
    s["cross"] = dict(args=(src, sinv, None, dt, (0, 0, w, h)), kw=dict(src_crs=src_crs, dst_crs=dst_crs, dst_nodata=-1.0), want=want, stats=stats)
    return s


def row_warp_raster(p, s):
    for case in s["same"] + [s["cross"]]:
        out, stats = p.warp_raster(*case["args"], **case["kw"])
        assert out.cpu().numpy().tobytes() == case["want"].tobytes()
        assert stats.cpu().numpy().tolist() == case["stats"].tolist()


ROWS = {"warp_raster": ("gr_warp_raster", row_warp_raster, 3)}


@pytest.mark.parametrize("name", list(ROWS))
def test_row(probe, side, scenes, name):
    function, body, n_calls = ROWS[name]
    record = sp.run_row(probe, side, name, lambda p: body(p, scenes))
    assert record["held"] is True
    assert record["calls"] == [function] * n_calls
    assert len(record["leg_a"]) == 2 * n_calls
    waited = {call.waited for call in record["leg_a"]}
    assert waited == {False}, f"{function} waited for its stream: the header says it only enqueues"
