"""The harness of tests/context_steps.py checks itself (as tests/test_fuzz_tools.py checks the fuzz tools): with the host oracle
in the library's place every step passes in any order, and a backend that leaks state from one call to the next in ONE stated way
makes the pair sequences and the seeded sequences raise.  The three leaks are the kinds a context could have: it keeps the
previous mesh where the face count did not change, it leaves its stand-in for `winner` set after a refused call, it hands back
the previous vertex order."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import context_steps as steps  # noqa: E402
from covering_standin import points_bounds_np  # noqa: E402
from crs_standin import CrsStandinBackend  # noqa: E402

from oracle import oracle_c
from tests.oracle_backend import OracleBackend


class HostBackend(OracleBackend):
    """`OracleBackend` with what the catalogue calls beyond it: depth, the two stage calls, rectangle pairs, and the binding's
    refusal of a fused call with one label plane too few.  It has no options: `set_options` sets the vertex order alone."""

    def raster_face_ids(self, cams, h, w, out=None, want_depth=False, check=True):
        if not want_depth:
            return super().raster_face_ids(cams, h, w)
        cams = np.asarray(cams, dtype=np.float32).reshape(-1, 16)
        res = [oracle_c.raster(self.verts, self.faces, c, h, w, want_depth=True, vertex_order=self.vertex_order) for c in cams]
        return torch.from_numpy(np.stack([r[0] for r in res])), torch.from_numpy(np.stack([r[1] for r in res]))

    def raster_project_labels(self, cams, labels, C, votes, counts, **kw):
        if np.asarray(cams).shape[0] != np.asarray(labels).shape[0]:
            raise ValueError("camera records and label images differ in number")
        return super().raster_project_labels(cams, labels, C, votes, counts, **kw)

    def points_bounds(self, points, stride=1):
        bounds, bad = points_bounds_np(points, stride)
        return torch.from_numpy(bounds), torch.tensor([bad], dtype=torch.int64)

    def reproject_points(self, *args, **kw):
        return CrsStandinBackend().reproject_points(*args, **kw)

    def new_pair_accumulator(self, n_classes, counts, neg1_is_last_face=True):
        acc = super().new_pair_accumulator(n_classes, counts, neg1_is_last_face)

        def add_rects(ids, rects, offsets):
            ids = np.asarray(ids)
            ids = ids[None] if ids.ndim == 2 else ids
            img = np.full(ids.shape, np.nan)
            for v in range(ids.shape[0]):
                for i0, j0, i1, j1, c in np.asarray(rects)[offsets[v]:offsets[v + 1]].tolist():
                    img[v, i0:i1, j0:j1] = c
            acc.add(ids, img[..., None])

        acc.add_rects = add_rects
        return acc


class KeepsTheMesh(HostBackend):
    """leak 1: an upload with as many faces as the last one is taken for the same mesh"""

    def upload_mesh(self, verts, faces):
        if self.verts is not None and np.asarray(faces).shape[0] == self.n_faces:
            return
        super().upload_mesh(verts, faces)


class KeepsTheWinners(HostBackend):
    """leak 2: the fused call finds its winners before it looks at the label planes, and a refused call leaves them set: the next
    fused call folds them in with its own"""

    def __init__(self):
        super().__init__()
        self.winner = []

    def raster_project_labels(self, cams, labels, C, votes, counts, **kw):
        labels = np.asarray(labels)
        self.winner += list(self.raster_face_ids(cams, labels.shape[1], labels.shape[2]).numpy())
        if np.asarray(cams).shape[0] != labels.shape[0]:
            raise ValueError("camera records and label images differ in number")
        for v, ids in enumerate(self.winner):
            if ids.shape == labels.shape[1:]:
                self.project_labels(ids, labels[min(v, labels.shape[0] - 1)], C, votes, counts)
        self.winner = []


class HandsBackThePreviousOrder(HostBackend):
    """leak 3: a call runs in the vertex order that was set before the last one"""

    def __init__(self):
        super().__init__()
        self.requested = "r1"

    def set_vertex_order(self, name):
        super().set_vertex_order(self.requested)
        self.requested = name


LEAKS = [KeepsTheMesh, KeepsTheWinners, HandsBackThePreviousOrder]


@pytest.fixture(scope="module")
def expected():
    return steps.expected()


def _pairs(make, expected):
    for first in steps.NAMES:
        steps.run(make(), steps.pair_sequence(first), expected)


def _seeded(make, expected):
    for seed in steps.SEEDS:
        steps.run(make(), steps.seeded_sequence(seed), expected)


def test_the_catalogue_is_what_the_suite_says(expected):
    assert len(steps.NAMES) >= 18 and set(expected) == set(steps.NAMES)
    assert all(len(steps.seeded_sequence(s)) == 60 for s in steps.SEEDS) and len(set(steps.SEEDS)) == 8
    seen = {(a, b) for first in steps.NAMES for a, b in zip(steps.pair_sequence(first)[::2], steps.pair_sequence(first)[1::2])}
    assert seen == {(a, b) for a in steps.NAMES for b in steps.NAMES}
    # what makes a leak visible is in the catalogue: two meshes of one face count with other ids, views the two vertex orders
    # tell apart, votes to fold twice
    assert (steps.scene("A32")["ids"][:3] != steps.scene("A2_32")["ids"]).sum() > 100
    assert steps.scene("A32")["F"] == steps.scene("A2_32")["F"] == 450 and steps.scene("B32")["F"] == 1922
    r1 = steps._views(steps._mesh(15), steps.POSES_A[:3], 70, 130)
    assert (r1["ids"] != steps.scene("A130gl")["ids"]).sum() > 0
    assert expected["fused A 1 view C=3"]["counts"].max() >= 1


def test_every_step_alone_and_every_ordered_pair(expected):
    _pairs(HostBackend, expected)


def test_seeded_sequences(expected):
    _seeded(HostBackend, expected)


@pytest.mark.parametrize("leak", LEAKS)
def test_the_pair_sequences_see_a_leak(expected, leak):
    with pytest.raises(AssertionError, match="replay: "):
        _pairs(leak, expected)


@pytest.mark.parametrize("leak", LEAKS)
def test_the_seeded_sequences_see_a_leak(expected, leak):
    with pytest.raises(AssertionError, match="replay: "):
        _seeded(leak, expected)


def test_a_failure_names_the_steps_to_replay(expected):
    history = []
    with pytest.raises(AssertionError) as e:
        steps.run(KeepsTheMesh(), ["argmax_nonzero", "ids A 32x32", "ids A2 exact binning"], expected, history)
    assert history == ["argmax_nonzero", "ids A 32x32", "ids A2 exact binning"] and repr(history) in str(e.value)
    with pytest.raises(AssertionError):
        steps.run(KeepsTheMesh(), history, expected)        # the replay line reproduces it on a new backend
    steps.run(HostBackend(), history, expected)
