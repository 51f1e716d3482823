"""The nearest-point call under the stream contract of include/geograster.h (tests/stream_probe.py).  gr_nearest_points takes its
stream as a field of a descriptor, so it is not among the functions whose last parameter is `void *stream` and the table of
tests/test_stream_contract_gpu.py does not list it; it is held to the same contract here (rule K9), with the legs of that table's
rows: (a) alone on a side stream, (b) with the default stream held, (c) with its inputs zeroed until a delay on its own stream has
passed, (d) both; outputs fenced and poisoned, compared with the numpy stand-in.  A call with refs and queries synchronises its own
stream, for the bounds and once per level, as its header says: leg A records it as one that waited -- with the default stream
still held, so it waited for nothing else.  Without refs or without queries it only enqueues: leg A counts for it."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import nearest_points_scenes as sc  # noqa: E402
import nearest_points_standin as nn  # noqa: E402
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
    """Inputs and the stand-in's answers: computed once, outside every hold, never written to.  Zeroed inputs give other bytes:
    all refs at the origin, row 0 for every query, other distances."""
    cases = []
    for s in (sc.duplicates_scene(), sc.two_clusters_scene(), sc.sizes_scene(0, 65), sc.sizes_scene(65, 0)):
        index, dist2, _, counts = nn.nearest(s["ref"], s["query"], s["max_distance"])
        cases.append(dict(s, want=(index, dist2), counts=counts))
    assert (cases[0]["want"][0] != 0).any() and (cases[1]["want"][0] != 0).any()
    return cases


def body(p, cases):
    for s in cases:
        index, dist2, stats = p.nearest_points(s["ref"], s["query"], max_distance=s["max_distance"], cell=s["cell"], max_rings=s["max_rings"],
                                               return_dist2=True)
        for g, w in zip((index, dist2), s["want"]):
            assert g.cpu().numpy().tobytes() == w.tobytes(), s["name"]
        assert tuple(stats.cpu().numpy()[:3].tolist()) == s["counts"], s["name"]


def test_the_search_waits_for_its_own_stream_only(probe, side, scenes):
    record = sp.run_row(probe, side, "nearest_points", lambda p: body(p, scenes[:2]))
    assert record["held"] is True, "the call waited, and the default stream was still held: it waited for its own stream alone"
    assert record["calls"] == ["gr_nearest_points"] * 2
    assert len(record["leg_a"]) == 4
    assert {call.waited for call in record["leg_a"]} == {True}, "gr_nearest_points reads the bounds and a word per level back: the header says so"


def test_without_refs_or_queries_it_only_enqueues(probe, side, scenes):
    record = sp.run_row(probe, side, "nearest_points_empty", lambda p: body(p, scenes[2:]))
    assert record["held"] is True
    assert record["calls"] == ["gr_nearest_points"] * 2
    assert len(record["leg_a"]) == 4
    assert {call.waited for call in record["leg_a"]} == {False}, "R == 0 or Q == 0: no read-back"
