"""The stand-in of gr_nearest_points (a helper module for the tests): brute force in numpy, in chunks of
queries, with K2's expression exactly -- ((dx dx + dy dy) + dz dz) in float64, numpy rounds every operation on its own -- and
`argmin`, whose first minimum is the lowest row.  Beside the answer it returns the gap to the second-best d2 of every query
(0: a tie; +inf: fewer than two participating refs), which says where another exact method may name another row."""
import numpy as np

REF_NONFINITE, QUERY_NONFINITE, NO_ANSWER, LEVELS, CARRIED, CELLS_PROBED, CANDIDATES, CELL_BITS, RING_CAP = range(9)
STAT_WORDS = 9
CHUNK_BYTES = 1 << 26


def as_points(p):
    p = np.asarray(p, dtype=np.float64)
    if p.ndim == 2 and p.shape[1] == 2:
        p = np.concatenate([p, np.zeros((len(p), 1))], axis=1)
    assert p.ndim == 2 and p.shape[1] == 3, p.shape
    return p


def nearest(ref, query, max_distance=None):
    """-> (index (Q,) int32, dist2 (Q,) float64, gap (Q,) float64, counts: the three words of the statistics that depend on the
    inputs alone: non-finite refs, non-finite queries, queries without an answer)."""
    ref, query = as_points(ref), as_points(query)
    Q = len(query)
    part = np.nonzero(np.isfinite(ref).all(axis=1))[0]
    r = ref[part]
    finite_q = np.isfinite(query).all(axis=1)
    index = np.full(Q, -1, dtype=np.int32)
    dist2 = np.full(Q, np.nan)
    gap = np.full(Q, np.inf)
    md2 = np.inf if max_distance is None else np.float64(max_distance) * np.float64(max_distance)
    if len(r):
        rows = np.nonzero(finite_q)[0]
        step = max(1, CHUNK_BYTES // (8 * len(r)))
        with np.errstate(over="ignore"):
            for at in range(0, len(rows), step):
                q = query[rows[at:at + step]]
                dx, dy, dz = (q[:, None, k] - r[None, :, k] for k in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                best = np.argmin(d2, axis=1)
                took = d2[np.arange(len(q)), best]
                if len(r) > 1:
                    d2[np.arange(len(q)), best] = np.inf
                    with np.errstate(invalid="ignore"):
                        second = d2.min(axis=1) - took
                    gap[rows[at:at + step]] = np.where(np.isnan(second), 0.0, second)
                keep = took <= md2
                index[rows[at:at + step]] = np.where(keep, part[best], -1)
                dist2[rows[at:at + step]] = np.where(keep, took, np.nan)
    counts = (int(len(ref) - len(part)), int((~finite_q).sum()), int((index < 0).sum()))
    return index, dist2, gap, counts


def gather(values, index, fill):
    """values[index] where index >= 0, fill elsewhere."""
    values = np.asarray(values)
    out = np.full((len(index),) + values.shape[1:], fill, dtype=values.dtype)
    out[index >= 0] = values[index[index >= 0]]
    return out


class StandinNearestBackend:
    """`HipRaster.nearest_points` by the stand-in, on the host; it records its calls.  (Mixed into other stand-ins: `calls` is made on
    first use.)"""
    vertex_order = "r1"

    def nearest_points(self, ref, query, *, max_distance=None, cell=0.0, max_rings=2, return_dist2=False):
        from geograypher_amd import _hip

        ref, query = np.asarray(ref), np.asarray(query)
        if ref.ndim != 2 or ref.shape[1] != 3 or query.ndim != 2 or query.shape[1] != 3:
            raise ValueError(f"ref must be (R, 3) and query (Q, 3), got {ref.shape} and {query.shape}")
        _hip.check_nearest_arguments(len(ref), len(query), max_distance, cell, max_rings)
        self.__dict__.setdefault("nearest_calls", []).append(dict(R=len(ref), Q=len(query), max_distance=max_distance, cell=cell,
                                                                  max_rings=max_rings))
        index, dist2, _, counts = nearest(ref, query, max_distance)
        stats = np.zeros(STAT_WORDS, dtype=np.int64)
        stats[:3] = counts
        stats[LEVELS] = 1 if len(ref) > counts[0] and len(query) else 0
        return (index, dist2, stats) if return_dist2 else (index, stats)
