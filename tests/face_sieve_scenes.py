"""The scenes of the face-sieve tests, shared by tests/test_face_sieve_host.py and
tests/test_face_sieve_gpu.py: a helper module, not a conftest.  The hand scenes carry their answers, written out by hand; the
border, spiral and random scenes are compared with tests/face_sieve_standin.py.

A statistics block reads [rounds, components before, components after, faces changed, small left, degenerate, fan edges, round
cap, bad faces]."""
import numpy as np


def strip_faces(n):
    """A triangle strip: face i = (i, i + 1, i + 2).  Face i shares an edge with i - 1 and i + 1 and only a vertex with i + 2."""
    i = np.arange(n, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], axis=1).reshape(-1, 3)


def grid_faces(nx, ny):
    """nx x ny quads, each split along the diagonal v00-v11: quad q = j nx + i gives the faces 2q = (v00, v10, v11) and 2q + 1 =
    (v00, v11, v01).  -> (faces (2 nx ny, 3) int32, the number of vertices)."""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    v00 = (j * (nx + 1) + i).reshape(-1)
    v10, v01, v11 = v00 + 1, v00 + nx + 1, v00 + nx + 2
    faces = np.stack([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)], axis=1).reshape(-1, 3)
    return faces.astype(np.int32), (nx + 1) * (ny + 1)


def scene(name, faces, classes, want_class, want_comp, want_stats, min_measure=0, fill=False, weights=None, canon=None, V=None):
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    if V is None:
        V = len(canon) if canon is not None else (int(faces.max()) + 1 if len(faces) else 0)
    return dict(name=name, faces=faces, classes=np.asarray(classes, dtype=np.int32), min_measure=min_measure, fill=fill,
                weights=None if weights is None else np.asarray(weights, dtype=np.int64),
                canon=None if canon is None else np.asarray(canon, dtype=np.int32), V=V,
                want_class=np.asarray(want_class, dtype=np.int32), want_comp=np.asarray(want_comp, dtype=np.int32),
                want_stats=list(want_stats))


FAN = [[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5]]
P60 = 1 << 60

HAND = [
    scene("no_face", np.zeros((0, 3)), [], [], [], [0, 0, 0, 0, 0, 0, 0, 0, 0], min_measure=2),
    # one face: small, no neighbour, a root
    scene("one_face", [[0, 1, 2]], [3], [3], [0], [0, 1, 1, 0, 1, 0, 0, 0, 0], min_measure=2),
    # equal measures tie: the lower id is greater, face 1 takes face 0's class; the merged component measures 2, not < 2
    scene("two_faces_tie", strip_faces(2), [1, 2], [1, 1], [0, 0], [1, 2, 1, 1, 0, 0, 0, 0, 0], min_measure=2),
    # measures 1 < 2 < 3 under threshold 3: {0} -> {1, 2} -> {3, 4, 5}, the chain resolves in ONE changing round
    scene("chain_1_2_3", strip_faces(6), [1, 2, 2, 3, 3, 3], [3] * 6, [0] * 6, [1, 3, 1, 3, 0, 0, 0, 0, 0], min_measure=3),
    # {1, 2} is small (2 < 3) but greater than both neighbours: a root; {0} and {3} join it
    scene("small_local_maximum", strip_faces(4), [1, 2, 2, 3], [2] * 4, [0] * 4, [1, 3, 1, 2, 0, 0, 0, 0, 0], min_measure=3),
    # a second, disconnected piece of one face: small, nothing to join, it stays
    scene("isolated_island", np.r_[strip_faces(3), [[5, 6, 7]]], [1, 1, 1, 2], [1, 1, 1, 2], [0, 0, 0, 3], [0, 2, 2, 0, 1, 0, 0, 0, 0],
          min_measure=2),
    # fans on the edge (0, 1): the equal classes join although they are not consecutive among the edge's faces
    scene("fan_of_3", FAN[:3], [1, 2, 1], [1, 2, 1], [0, 1, 0], [0, 2, 2, 0, 0, 0, 1, 0, 0]),
    scene("fan_of_4", FAN, [1, 2, 1, 2], [1, 2, 1, 2], [0, 1, 0, 1], [0, 2, 2, 0, 0, 0, 1, 0, 0]),
    # face 1 = (1, 2, 2) is degenerate: in no component, it keeps class 2 and adds nothing to the edge (1, 2), which faces 0 and 2
    # share; face 2 ties with face 0 and takes its class; the merged component (measure 2 < 5) has no neighbour left
    scene("degenerate_between", [[0, 1, 2], [1, 2, 2], [2, 1, 3]], [1, 2, 3], [1, 2, 1], [0, -1, 0], [1, 2, 1, 1, 1, 1, 0, 0, 0],
          min_measure=5),
    # one common vertex is not adjacency
    scene("vertex_touch", [[0, 1, 2], [2, 3, 4]], [1, 2], [1, 2], [0, 1], [0, 2, 2, 0, 2, 0, 0, 0, 0], min_measure=2),
    # unlabelled (any negative value) is a barrier: {0} has no labelled neighbour and stays, the unlabelled face is never small
    scene("unlabelled_barrier", strip_faces(5), [1, -7, 2, 2, 2], [1, -1, 2, 2, 2], [0, 1, 2, 2, 2], [0, 3, 3, 0, 1, 0, 0, 0, 0],
          min_measure=2),
    # ... with filling: round 1 the unlabelled face joins {2, 3, 4} (measure 3 beats 1), round 2 {0} joins the lot
    scene("unlabelled_filled", strip_faces(5), [1, -7, 2, 2, 2], [2] * 5, [0] * 5, [2, 3, 1, 2, 0, 0, 0, 0, 0], min_measure=2, fill=True),
    # an unlabelled island (measure 2) whose labelled neighbours measure 1: it fills all the same, from the lower id of the tie;
    # round 2: {3} (1 < 3) joins {0, 1, 2}
    scene("unlabelled_island_fills", strip_faces(4), [1, -1, -1, 2], [1] * 4, [0] * 4, [2, 3, 1, 3, 0, 0, 0, 0, 0], min_measure=3, fill=True),
    # a labelled small island whose only neighbour is unlabelled stays
    scene("only_unlabelled_neighbour", strip_faces(2), [1, -1], [1, -1], [0, 1], [0, 2, 2, 0, 1, 0, 0, 0, 0], min_measure=2),
    # a measure equal to the threshold is not small
    scene("measure_equals_threshold", strip_faces(4), [1, 1, 2, 2], [1, 1, 2, 2], [0, 0, 2, 2], [0, 2, 2, 0, 0, 0, 0, 0, 0], min_measure=2),
    # sums of 2^61 and 2^61 - 1 (equal as float64): the second is small under 2^61 and joins the first, which is not
    scene("weights_reach_2_61", strip_faces(4), [1, 1, 2, 2], [1] * 4, [0] * 4, [1, 2, 1, 2, 0, 0, 0, 0, 0], min_measure=1 << 61,
          weights=[P60, P60, P60, P60 - 1]),
    # a seam: vertices 3, 4 duplicate 1, 2.  Two components as it is, one when welded
    scene("seam_open", [[0, 1, 2], [4, 3, 5]], [1, 1], [1, 1], [0, 1], [0, 2, 2, 0, 0, 0, 0, 0, 0], V=6),
    scene("seam_welded", [[0, 1, 2], [4, 3, 5]], [1, 1], [1, 1], [0, 0], [0, 1, 1, 0, 0, 0, 0, 0, 0], canon=[0, 1, 2, 1, 2, 5]),
]

BORDER_SIZES = (63, 64, 65, 255, 256, 257, 1025)


def border_scene(n):
    """A strip of n faces with alternating classes, min_measure 2."""
    return dict(name=f"strip_{n}", faces=strip_faces(n), classes=(1 + np.arange(n) % 2).astype(np.int32), min_measure=2, fill=False,
                weights=None, canon=None, V=n + 2)


def spiral_scene(side=45):
    """side x side quads (4050 faces at 45): the quads of a square spiral arm, one quad wide, are class 1, the rest class 2 -- two
    components of a long diameter each."""
    arm = np.zeros((side, side), bool)
    inside = lambda r, c: 0 <= r < side and 0 <= c < side
    r, c, dr, dc = 0, 0, 0, 1
    arm[0, 0] = True
    moved = True
    while moved:
        moved = False
        for _ in range(2):          # straight on, else one turn to the right; the walk keeps one free quad between its windings
            nr, nc = r + dr, c + dc
            if inside(nr, nc) and not arm[nr, nc] and not (inside(nr + dr, nc + dc) and arm[nr + dr, nc + dc]):
                r, c, moved = nr, nc, True
                arm[r, c] = True
                break
            dr, dc = dc, -dr
    faces, V = grid_faces(side, side)
    classes = np.repeat(np.where(arm.reshape(-1), 1, 2), 2).astype(np.int32)
    return dict(name="spiral", faces=faces, classes=classes, min_measure=0, fill=False, weights=None, canon=None, V=V)


RANDOM_SEEDS = (0, 1, 2, 3)
RANDOM_THRESHOLDS = (2, 5, 50)


def random_scene(seed, min_measure, fill):
    """40 x 40 quads, 3 classes drawn iid with 5 % unlabelled, weights 1..7 (many ties)."""
    rng = np.random.default_rng(seed)
    faces, V = grid_faces(40, 40)
    F = len(faces)
    classes = rng.integers(0, 3, F).astype(np.int32)
    classes[rng.random(F) < 0.05] = -1
    weights = rng.integers(1, 8, F).astype(np.int64)
    return dict(name=f"random_{seed}_{min_measure}_{int(fill)}", faces=faces, classes=classes, min_measure=min_measure, fill=fill,
                weights=weights, canon=None, V=V)


def random_scenes():
    return [random_scene(seed, t, fill) for seed in RANDOM_SEEDS for t in RANDOM_THRESHOLDS for fill in (False, True)]


def merged(scenes, min_measure, fill):
    """The scenes as disconnected pieces of ONE call: vertices and faces offset piece by piece, unit weights.  -> (the merged scene,
    [(first face, the piece)])."""
    faces, classes, canon, at, v0, f0 = [], [], [], [], 0, 0
    for s in scenes:
        at.append((f0, s))
        faces.append(s["faces"] + v0)
        classes.append(s["classes"])
        canon.append((np.arange(s["V"]) if s["canon"] is None else s["canon"]) + v0)
        v0 += s["V"]
        f0 += len(s["faces"])
    return dict(name=f"merged_{min_measure}_{int(fill)}", faces=np.concatenate(faces).astype(np.int32),
                classes=np.concatenate(classes).astype(np.int32), min_measure=min_measure, fill=fill, weights=None,
                canon=np.concatenate(canon).astype(np.int32), V=v0), at
