"""The image-selection rule-set restated in plain numpy / scipy: the yardstick of gr_set_cover.

Written for reading, not for speed, and without a line of the library.  Also: the brute-force optimum for small instances, the
two properties a selection must have (`covers`, `irreducible`) and two instance generators."""
import itertools
import math

import numpy as np
from scipy import sparse


def incidence(A):
    """(F, N) bool CSR of "view v sees face f": values are ignored, explicit zeros are no entries (M1)."""
    A = sparse.csr_matrix(A)
    A = sparse.csr_matrix((A.data != 0, A.indices.copy(), A.indptr.copy()), shape=A.shape)   # (the caller's arrays stay as they are)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def required_faces(A, min_observations=1):
    """M1, M2: (F,) bool."""
    A = incidence(A)
    obs = np.diff(A.indptr)
    return obs >= max(min_observations, 1)


def set_cover(A, min_observations=1, prune=True):
    """M1-M7 -> {"selected" (N,) bool, "order" (k,) int32, "gains" (k,) int64, "pruned" (p,) int32, "n_required", "n_covered"}."""
    A = incidence(A)
    F, N = A.shape
    rows = [A.indices[A.indptr[f]:A.indptr[f + 1]] for f in range(F)] if F * N < 10_000 else None
    by_view = A.tocsc()
    required = required_faces(A, min_observations)
    covered = np.zeros(F, dtype=bool)
    order, gains = [], []

    def faces_of(v):
        return by_view.indices[by_view.indptr[v]:by_view.indptr[v + 1]]

    # M3: the number of required, uncovered faces each view sees -- kept up to date as faces get covered
    gain = np.asarray(A[required].sum(axis=0)).reshape(-1).astype(np.int64) if F and N else np.zeros(N, dtype=np.int64)
    while N and gain.max() > 0:                     # M4, M5
        v = int(np.argmax(gain))                    # the first maximum: ties to the lowest view
        order.append(v)
        gains.append(int(gain[v]))
        mine = faces_of(v)
        new = mine[required[mine] & ~covered[mine]]
        assert len(new) == gain[v]
        covered[new] = True
        if rows is not None:                        # small: literally "every view of the face's row loses one"
            for f in new:
                gain[rows[f]] -= 1
        else:
            gain -= np.asarray(A[new].sum(axis=0)).reshape(-1).astype(np.int64)
    selected = np.zeros(N, dtype=bool)
    selected[order] = True

    pruned = []
    if prune:                                       # M6
        m = np.asarray(A[:, np.flatnonzero(selected)].sum(axis=1)).reshape(-1).astype(np.int64) if len(order) else np.zeros(F, np.int64)
        for v in reversed(order):
            mine = faces_of(v)
            if np.all(m[mine[required[mine]]] >= 2):
                selected[v] = False
                m[mine] -= 1
                pruned.append(v)
    return {"selected": selected, "order": np.array(order, dtype=np.int32), "gains": np.array(gains, dtype=np.int64),
            "pruned": np.array(pruned, dtype=np.int32), "n_required": int(required.sum()),
            "n_covered": int((covered & required).sum())}


def covers(A, required, mask) -> bool:
    """Every required face is seen by a view of the mask."""
    A = incidence(A)
    mask = np.asarray(mask, dtype=bool)
    seen = np.asarray(A[:, np.flatnonzero(mask)].sum(axis=1)).reshape(-1) > 0
    return bool(np.all(seen[np.asarray(required, dtype=bool)]))


def irreducible(A, required, mask) -> bool:
    """No view of the mask can be taken out without uncovering a required face."""
    mask = np.asarray(mask, dtype=bool)
    for v in np.flatnonzero(mask):
        smaller = mask.copy()
        smaller[v] = False
        if covers(A, required, smaller):
            return False
    return True


def brute_force_optimum(A, required) -> int:
    """The size of a smallest covering subset, over all subsets (N <= 12)."""
    A = incidence(A).toarray()
    N = A.shape[1]
    assert N <= 12
    need = A[np.asarray(required, dtype=bool)]
    for size in range(N + 1):
        for subset in itertools.combinations(range(N), size):
            if np.all(need[:, list(subset)].any(axis=1)):
                return size
    raise AssertionError("a required face is seen by some view: all views together cover")


def greedy_bound(optimum: int, A, required) -> int:
    """ceil(optimum * H(d)), d the largest number of required faces one view sees: the textbook guarantee of greedy set cover."""
    A = incidence(A)
    d = int(np.asarray(A[np.asarray(required, dtype=bool)].sum(axis=0)).max()) if A.shape[1] and np.any(required) else 0
    harmonic = sum(1.0 / i for i in range(1, d + 1))
    return int(math.ceil(optimum * harmonic - 1e-9))


def random_incidence(F, N, density, seed):
    """(F, N) bool CSR with about density * F * N entries."""
    rng = np.random.default_rng(seed)
    return sparse.csr_matrix(sparse.random(F, N, density=density, format="csr", random_state=rng, dtype=np.float64) != 0)


def footprint_incidence(F, N, seed, views_per_face=12.0):
    """Views as rectangles over a grid of about F faces (exactly rows * cols of them), centred on a jittered flight-line pattern:
    the overlapping structure of a real survey.  Returns (rows * cols, N) bool CSR."""
    rng = np.random.default_rng(seed)
    rows = int(math.sqrt(F))
    cols = F // rows
    lines = max(int(math.sqrt(N)), 1)
    per_line = int(math.ceil(N / lines))
    half_h = max(int(rows * math.sqrt(views_per_face) / (2 * lines)), 1)
    half_w = max(int(cols * math.sqrt(views_per_face) / (2 * per_line)), 1)
    ii, jj = [], []
    for v in range(N):
        ci = (v // per_line + 0.5) / lines * rows + rng.normal(0, rows / (8 * lines))
        cj = (v % per_line + 0.5) / per_line * cols + rng.normal(0, cols / (8 * per_line))
        r0, r1 = max(int(ci) - half_h, 0), min(int(ci) + half_h, rows)
        c0, c1 = max(int(cj) - half_w, 0), min(int(cj) + half_w, cols)
        if r1 <= r0 or c1 <= c0:
            continue
        faces = (np.arange(r0, r1)[:, None] * cols + np.arange(c0, c1)[None, :]).reshape(-1)
        ii.append(faces)
        jj.append(np.full(faces.shape, v))
    ii = np.concatenate(ii) if ii else np.zeros(0, dtype=np.int64)
    jj = np.concatenate(jj) if jj else np.zeros(0, dtype=np.int64)
    return sparse.csr_matrix((np.ones(len(ii), dtype=bool), (ii, jj)), shape=(rows * cols, N))
