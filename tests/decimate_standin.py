"""Checker of gr_cluster_count / gr_cluster_decimate (rules D1-D9), on the host and by another method than the
device's: Python integers and plain loops -- a dict of cells, `min` over (d2, index) tuples, a set of frozensets for the duplicate
faces -- where the library sorts keys and scans flags.  `StandInBackend` offers the two calls with the binding's signatures, so the
host code (`utils.geometric.cluster_cell_size`, `TexturedPhotogrammetryMesh.decimate`) runs against it without a GPU.

The statistics words are the binding's (GR_DECIM_STAT_*): kept faces, kept vertices, bad faces, occupied cells, collapsed faces,
duplicate faces, vertices outside the key range, 0."""
import numpy as np

CELL_LIMIT = 1 << 21
STAT_WORDS = 8


def cell_of(q, s):
    """D2: the cell (cx, cy, cz) of a snapped vertex, or None outside the key range."""
    if min(q) < 0:
        return None
    c = tuple(v // s for v in q)
    return None if max(c) >= CELL_LIMIT else c


def centre_distance(q, c, s):
    """D3: d2 of a vertex to the centre of its cell, in doubled grid steps."""
    return sum((2 * (v - k * s) - s) ** 2 for v, k in zip(q, c))


def representatives(verts_q, s):
    """D2, D3 -> (rep: a list of V ints, -1 outside the key range; the dict cell -> [(d2, index) of its members])."""
    s = int(s)
    cells = {}
    for i, row in enumerate(np.asarray(verts_q).tolist()):
        c = cell_of(row, s)
        if c is not None:
            cells.setdefault(c, []).append((centre_distance(row, c, s), i))
    rep = [-1] * len(verts_q)
    for members in cells.values():
        best = min(members)[1]
        for _, i in members:
            rep[i] = best
    return rep, cells


def cluster_count_py(verts_q, s) -> int:
    return len(representatives(verts_q, s)[1])


def cluster_decimate_py(verts_q, faces, s):
    """D2-D8 -> (rep (V,) int32, face_ids int64, point_ids int64, new_faces (n, 3) int32, stats (STAT_WORDS,) int64)."""
    V = len(verts_q)
    rep, cells = representatives(verts_q, s)
    outside = sum(1 for r in rep if r < 0)
    bad = collapsed = duplicates = 0
    seen, kept = set(), []
    for f, (a, b, c) in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if not all(0 <= v < V for v in (a, b, c)) or min(rep[a], rep[b], rep[c]) < 0:
            bad += 1
            continue
        triple = (rep[a], rep[b], rep[c])
        if len(set(triple)) < 3:                       # D5
            collapsed += 1
            continue
        if frozenset(triple) in seen:                  # D6: an earlier face has these three cells
            duplicates += 1
            continue
        seen.add(frozenset(triple))
        kept.append((f, triple))
    used = sorted({r for _, triple in kept for r in triple})      # D8
    position = {r: k for k, r in enumerate(used)}
    new_faces = np.array([[position[r] for r in triple] for _, triple in kept], dtype=np.int32).reshape(-1, 3)
    stats = np.array([len(kept), len(used), bad, len(cells), collapsed, duplicates, outside, 0], dtype=np.int64)
    return (np.array(rep, dtype=np.int32), np.array([f for f, _ in kept], dtype=np.int64), np.array(used, dtype=np.int64), new_faces,
            stats)


class StandInBackend:
    """`HipRaster.cluster_count` and `HipRaster.cluster_decimate` on the CPU; counts the probes.  (No constructor: the class is
    mixed into other stand-ins.)"""

    probes = 0

    def cluster_count(self, verts_q, s):
        self.probes += 1
        return cluster_count_py(verts_q, s)

    def cluster_decimate(self, verts_q, faces, s, check=True):
        out = cluster_decimate_py(verts_q, faces, s)
        if check and out[4][2]:
            raise ValueError(f"gr_cluster_decimate: {int(out[4][2])} faces name a vertex outside [0, {len(verts_q)})")
        return out


# -- the hand-worked scene: 2 x 2 x 1 cells of side 1 000 000 ---------------------------------------------------------------------------
HAND_S = 1_000_000


def hand_scene():
    """(verts_q, faces, s, vertex fates, face fates).  Cells A = (0, 0, 0), B = (1, 0, 0), C = (0, 1, 0), D = (1, 1, 0); a cell's centre
    is 500 000 behind its corner on every axis.  A vertex fate is (q, cell, representative, why); a face fate is (corners, fate, why)
    with fate "kept", "collapsed", "duplicate" or "bad"."""
    vertices = [
        ((500_000, 500_000, 500_000), "A", 0, "the centre of A: d2 = 0"),
        ((100_000, 100_000, 500_000), "A", 0, "a corner region of A"),
        ((900_000, 200_000, 500_000), "A", 0, "A, 100 000 before the face x = 1 000 000"),
        ((1_000_000, 400_000, 500_000), "B", 4, "exactly ON the face x = 1 000 000: the upper cell, B (floor division)"),
        ((1_400_000, 500_000, 500_000), "B", 4, "200 000 left of B's centre: d2 = 4e10; the mirror image of vertex 5, the lower index wins"),
        ((1_600_000, 500_000, 500_000), "B", 4, "200 000 right of B's centre: d2 = 4e10, the same as vertex 4"),
        ((500_000, 1_500_000, 400_000), "C", 6, "100 000 under C's centre; coincident with vertex 7, the lower index wins"),
        ((500_000, 1_500_000, 400_000), "C", 6, "the same position as vertex 6"),
        ((1_500_000, 1_500_000, 500_000), "D", 8, "the centre of D; no kept face uses D, so 8 is not among the kept vertices"),
        ((1_900_000, 1_900_000, 100_000), "D", 8, "a corner region of D"),
    ]
    V = len(vertices)
    faces = [
        ((1, 2, 0), "collapsed", "all three corners in A"),
        ((7, 3, 1), "kept", "representatives (6, 4, 0): the first face over the cells {A, B, C}, kept with ITS winding"),
        ((2, 5, 7), "duplicate", "representatives (0, 4, 6): the same three cells as face 1, opposite winding"),
        ((0, 3, 4), "collapsed", "two corners in B"),
        ((8, 9, 6), "collapsed", "two corners in D: the only face that names D's vertices"),
        ((0, 4, V), "bad", f"names vertex {V}, one past the last"),
        ((6, 0, 5), "duplicate", "representatives (6, 0, 4): the cells {A, B, C} once more, the winding of face 1"),
    ]
    verts_q = np.array([q for q, _, _, _ in vertices], dtype=np.int64)
    return verts_q, np.array([c for c, _, _ in faces], dtype=np.int32), HAND_S, vertices, faces


HAND_EXPECTED = {
    "rep": [0, 0, 0, 4, 4, 4, 6, 6, 8, 8],
    "face_ids": [1],
    "point_ids": [0, 4, 6],
    "new_faces": [[2, 1, 0]],
    "stats": [1, 3, 1, 4, 3, 2, 0, 0],
}


# -- the random scene -----------------------------------------------------------------------------------------------------------------
RANDOM_S = 1_000_000
RANDOM_SEED = 11


def random_scene(seed=RANDOM_SEED):
    """(verts_q (4000, 3) int64 >= 0, faces (8000, 3) int32): vertices on a lattice of step s / 4 over a box of 6 x 6 x 3 cells (both
    ends included, so a quarter of the lattice planes ARE cell faces and many vertices coincide), 200 of them nudged by up to +-3
    grid steps (never below 0); 50 vertices are named by no face and lie four cells higher, in cells that hold nothing else; a face
    is a vertex and two vertices within 40 places of it in (x, y, z)-sorted
    order; the first 300 faces are reversed copies of the next 300."""
    rng = np.random.default_rng(seed)
    V, F, step = 4000, 8000, RANDOM_S // 4
    lattice = np.column_stack([rng.integers(0, 25, V), rng.integers(0, 25, V), rng.integers(0, 13, V)]).astype(np.int64)
    verts_q = lattice * step
    nudged = rng.choice(V, 200, replace=False)
    verts_q[nudged] += rng.integers(-3, 4, (200, 3))
    verts_q = np.maximum(verts_q, 0)                                          # D1: q >= 0, and the lattice stays on the cell faces
    unnamed = rng.choice(V, 50, replace=False)
    verts_q[unnamed, 2] += 4 * RANDOM_S                                       # a layer of cells of their own: representatives no face uses
    order = np.lexsort((verts_q[:, 2], verts_q[:, 1], verts_q[:, 0]))
    order = order[~np.isin(order, unnamed)]                                   # the vertices faces may name, sorted by (x, y, z)
    n = len(order)
    first = rng.integers(0, n, F)
    second = np.clip(first + rng.integers(-40, 41, F), 0, n - 1)
    third = np.clip(first + rng.integers(-40, 41, F), 0, n - 1)
    faces = np.column_stack([order[first], order[second], order[third]]).astype(np.int32)
    faces[:300] = faces[300:600, ::-1]
    return np.ascontiguousarray(verts_q), np.ascontiguousarray(faces)


def hard_cases(verts_q, faces, s):
    """What makes the random scene hard, counted: vertices on a cell boundary, cells with a tie for the smallest d2 (and those ties
    between distinct positions), vertices that share their position with another, collapsed and duplicate faces, representatives
    that no kept face uses, vertices that no face names."""
    rows = np.asarray(verts_q).tolist()
    rep, cells = representatives(verts_q, s)
    ties = ties_apart = 0
    for members in cells.values():
        best = min(members)[0]
        at_best = [i for d, i in members if d == best]
        if len(at_best) > 1:
            ties += 1
            ties_apart += len({tuple(rows[i]) for i in at_best}) > 1
    positions = {}
    for row in rows:
        positions[tuple(row)] = positions.get(tuple(row), 0) + 1
    out = cluster_decimate_py(verts_q, faces, s)
    return {
        "cells": len(cells),
        "boundary": sum(1 for row in rows if any(v % s == 0 for v in row)),
        "tie_cells": ties, "tie_cells_apart": ties_apart,
        "coincident": sum(1 for row in rows if positions[tuple(row)] > 1),
        "collapsed": int(out[4][4]), "duplicates": int(out[4][5]),
        "unused_representatives": len(set(r for r in rep if r >= 0) - set(out[2].tolist())),
        "unnamed_vertices": len(rows) - len(set(np.asarray(faces).reshape(-1).tolist())),
    }
