"""The face-sieve call under the stream contract of include/geograster.h (tests/stream_probe.py).  gr_face_sieve takes its stream
as a field of a descriptor, so it is not among the functions whose last parameter is `void *stream` and the table of
tests/test_stream_contract_gpu.py does not list it; it is held to the same contract here, with the legs of that table's rows: (a) alone
on a side stream, (b) with the default stream held, (c) with its inputs zeroed until a delay on its own stream has passed, (d) both;
outputs fenced and poisoned, compared with the numpy stand-in.  A call with rounds synchronises its own stream, as its header
says: leg A records it as one that waited -- with the default stream still held, so it waited for nothing else.  The labelling
alone (min_measure = 0) only enqueues: leg A counts for it."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import face_sieve_scenes as sc  # noqa: E402
import face_sieve_standin as fs  # noqa: E402
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
    faces of three equal corners are all degenerate, comp is -1 throughout."""
    cases = []
    for s in (sc.random_scene(0, 5, True), sc.border_scene(257), dict(sc.random_scene(1, 0, False), name="labelling_alone")):
        class_out, comp, stats, _ = fs.sieve(s["faces"], s["classes"], s["weights"], s["min_measure"], s["fill"], n_vertices=s["V"])
        assert (comp >= 0).all() and (stats[fs.ROUNDS] >= 1) == (s["min_measure"] > 0)
        cases.append(dict(s, want=(class_out, comp, stats)))
    return cases


def body(p, cases):
    for s in cases:
        got = p.face_sieve(s["faces"], s["classes"], s["weights"], s["min_measure"], s["fill"], n_vertices=s["V"])
        for g, w in zip(got, s["want"]):
            assert g.cpu().numpy().tobytes() == w.tobytes(), s["name"]


def test_rounds_wait_for_their_own_stream_only(probe, side, scenes):
    record = sp.run_row(probe, side, "face_sieve", lambda p: body(p, scenes[:2]))
    assert record["held"] is True, "the call waited, and the default stream was still held: it waited for its own stream alone"
    assert record["calls"] == ["gr_face_sieve"] * 2
    assert len(record["leg_a"]) == 4
    assert {call.waited for call in record["leg_a"]} == {True}, "gr_face_sieve with rounds synchronises its stream: the header says so"


def test_the_labelling_alone_only_enqueues(probe, side, scenes):
    record = sp.run_row(probe, side, "face_components", lambda p: body(p, scenes[2:]))
    assert record["held"] is True
    assert record["calls"] == ["gr_face_sieve"]
    assert len(record["leg_a"]) == 2
    assert {call.waited for call in record["leg_a"]} == {False}, "min_measure = 0 has no round and no read-back"
