"""The face sieve restated in numpy, for the tests: a helper module, not a conftest.  Vectorised
numpy and `scipy.sparse.csgraph.connected_components` for I4; it shares no code with the device path or with
`geograypher_amd.utils.geometric`.  Everything is int64 arithmetic: measures stay below 2^62.

`sieve(...)` -> (class_out (F,) int32, comp (F,) int32, stats (STAT_WORDS,) int64, info) where `info` holds what the tests ask
beyond the call's outputs: the face pairs of I3 and the measures of the final components."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

ROUNDS, BEFORE, AFTER, CHANGED, SMALL_LEFT, DEGENERATE, FAN_EDGES, ROUND_CAP, BAD_FACES, STAT_WORDS = range(10)


def face_pairs(faces, vertex_canon, V):
    """I1, I3 -> (pairs (n, 2) of edge-neighbours, each unordered pair once per shared edge; live (F,) bool; degenerate (F,) bool;
    bad (F,) bool; the number of edges shared by more than two faces)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = len(faces)
    bad = ((faces < 0) | (faces >= V)).any(axis=1)
    v = np.where(bad[:, None], 0, faces)
    if vertex_canon is not None:
        canon = np.asarray(vertex_canon, dtype=np.int64)
        v = canon[v] if V else v
        bad |= ((v < 0) | (v >= V)).any(axis=1)
    degenerate = ~bad & ((v[:, 0] == v[:, 1]) | (v[:, 1] == v[:, 2]) | (v[:, 0] == v[:, 2]))
    live = ~bad & ~degenerate
    ids = np.nonzero(live)[0]
    a = v[ids][:, [0, 1, 2]].reshape(-1)
    b = v[ids][:, [1, 2, 0]].reshape(-1)
    key = np.minimum(a, b) * max(V, 1) + np.maximum(a, b)
    owner = np.repeat(ids, 3)
    order = np.argsort(key, kind="stable")
    key, owner = key[order], owner[order]
    start = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0] if len(key) else np.zeros(0, np.int64)
    length = np.diff(np.r_[start, len(key)])
    pairs = []
    for k in np.unique(length[length > 1]):
        group = owner[start[length == k][:, None] + np.arange(k)[None, :]]           # (runs of k faces, k)
        i, j = np.triu_indices(int(k), 1)
        pairs.append(np.stack([group[:, i].reshape(-1), group[:, j].reshape(-1)], axis=1))
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    return pairs, live, degenerate, bad, int((length > 2).sum())


def components(pairs, cls, live):
    """I4 -> comp (F,) int64: the smallest face of the face's component, -1 where not live."""
    F = len(cls)
    if F == 0:
        return np.zeros(0, np.int64)
    same = pairs[cls[pairs[:, 0]] == cls[pairs[:, 1]]]
    graph = coo_matrix((np.ones(len(same), np.int8), (same[:, 0], same[:, 1])), shape=(F, F))
    _, label = connected_components(graph, directed=False)
    first = np.full(label.max() + 1 if F else 0, F, np.int64)
    np.minimum.at(first, label, np.arange(F))
    return np.where(live, first[label], -1) if F else np.zeros(0, np.int64)


def measures(comp, weights):
    """I5 -> m (F,) int64, at the component's id."""
    m = np.zeros(len(comp), np.int64)
    w = np.ones(len(comp), np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    np.add.at(m, comp[comp >= 0], w[comp >= 0])
    return m


def small_components(comp, cls, m, min_measure, fill_unlabelled):
    """I7 -> (F,) bool, set at the ids of the small components."""
    is_id = comp == np.arange(len(comp))
    return is_id & (m < min_measure) & ((cls >= 0) | bool(fill_unlabelled))


def pointers(pairs, comp, cls, m, small):
    """I6, I8 -> ptr (F,) int64 over component ids (identity: a root), the roots of the chains resolved."""
    F = len(comp)
    both = np.concatenate([pairs, pairs[:, ::-1]])
    A, g = comp[both[:, 0]], both[:, 1]
    B = comp[g]
    take = (A != B) & small[A] & (cls[g] >= 0)
    A, B = A[take], B[take]
    order = np.lexsort((B, -m[B], A))          # by A, then the greatest B first: the largest measure, the lowest id
    A, B = A[order], B[order]
    head = np.r_[True, A[1:] != A[:-1]] if len(A) else np.zeros(0, bool)
    A, T = A[head], B[head]
    greater = (m[T] > m[A]) | ((m[T] == m[A]) & (T < A))
    points = (cls[A] < 0) | greater
    ptr = np.arange(F)
    ptr[A[points]] = T[points]
    for _ in range(F + 1):
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            return ptr
        ptr = nxt
    raise AssertionError("the pointers of I8 have a cycle")


def sieve(faces, classes, weights=None, min_measure=0, fill_unlabelled=False, vertex_canon=None, max_rounds=64, n_vertices=None):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = len(faces)
    if vertex_canon is not None:
        V = len(vertex_canon)
    elif n_vertices is not None:
        V = int(n_vertices)
    else:
        V = int(faces.max()) + 1 if F else 0
    cls = np.maximum(np.asarray(classes, dtype=np.int64).reshape(-1), -1)
    assert len(cls) == F
    pairs, live, degenerate, bad, fans = face_pairs(faces, vertex_canon, V)
    stats = np.zeros(STAT_WORDS, np.int64)
    stats[DEGENERATE], stats[FAN_EDGES], stats[BAD_FACES] = degenerate.sum(), fans, bad.sum()
    rounds = 0
    while True:
        comp = components(pairs, cls, live)
        m = measures(comp, weights)
        small = small_components(comp, cls, m, min_measure, fill_unlabelled)
        n_comp = int((comp == np.arange(F)).sum())
        if rounds == 0:
            stats[BEFORE] = n_comp
        if min_measure == 0 or rounds == max_rounds:
            break
        ptr = pointers(pairs, comp, cls, m, small)
        root = np.where(live, ptr[np.maximum(comp, 0)], -1)
        new = np.where(live & (root != comp), cls[np.maximum(root, 0)], cls)
        changed = int((new != cls).sum())
        if changed == 0:
            break
        cls = new
        rounds += 1
        stats[CHANGED] += changed
        if rounds == max_rounds:
            stats[ROUND_CAP] = 1
    stats[ROUNDS], stats[AFTER], stats[SMALL_LEFT] = rounds, n_comp, small.sum()
    info = dict(pairs=pairs, measures=m, small=small, live=live)
    return cls.astype(np.int32), comp.astype(np.int32), stats, info


def small_left_have_no_labelled_neighbour(class_out, comp, info):
    """The termination property of I9: no small component that remains is edge-adjacent to a labelled face of another component."""
    pairs, small = info["pairs"], info["small"]
    both = np.concatenate([pairs, pairs[:, ::-1]])
    A, B = comp[both[:, 0]], comp[both[:, 1]]
    return not bool(((A != B) & small[A] & (class_out[both[:, 1]] >= 0)).any())
