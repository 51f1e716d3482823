"""Numeric stage of the multiview-detection workflow (reference: geograypher/utils/numeric.py:39-236, 330-619).

The quadratic part -- the clamped segment-to-segment distance of every pair of rays -- runs on the device
(`HipRaster.ray_pair_edges`, gr_ray_pairs); what is left on the host works on the kept edges only: the `min_dist` floor, the
optional transform, the 1 / d weight, the reference's edge order, and the Louvain communities: networkx as in the reference
(the default), or `method="device"`: a deterministic Louvain and the community points on the device (`ray_communities`,
gr_louvain_communities, gr_community_points).  There is no CPU
fallback for the distance stage: `backend` is a `HipRaster` (default: the shared one of the current device) or any object with
the same `ray_pair_edges(starts, ends, ray_ids, threshold)` method.

`select_covering_views` is the set-cover stage of the annotation_image_selection workflow: a face x view visibility matrix ->
a small set of views that together see every required face, chosen on the device (`HipRaster.set_cover`, gr_set_cover).
"""
from __future__ import annotations

import json
import typing
from pathlib import Path

import numpy as np

from geograypher_amd.constants import PATH_TYPE


def _host(x) -> np.ndarray:
    """device tensor or array -> numpy"""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _clip0(x, hi):
    return np.minimum(np.maximum(x, 0.0), hi)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def segment_closest_points(a0: np.ndarray, a1: np.ndarray, b0: np.ndarray, b1: np.ndarray):
    """Closest points between every segment a0 -> a1 (N of them, axis 0) and every segment b0 -> b1 (M, axis 1), clamped to
    the segments: (pA (N, M, 3), pB (N, M, 3), dist (N, M)).  The host form of what gr_ray_pairs evaluates per pair
    (compute_approximate_ray_intersections(clamp=True), numeric.py:39-236); used on the few rays of one community.

    Skew lines meet closest at t0 = det(t, uB, n) / |n|^2 along A and t1 = det(t, uA, n) / |n|^2 along B (n = uA x uB,
    t = b0 - a0).  A parameter outside its segment is clamped and the other point re-projected: B from the clamped A first,
    then A from the updated B.  Exactly parallel segments (|n|^2 == 0) are placed by the projections d0, d1 of B's ends on A's
    axis: B wholly before a0 or behind a1 pairs that end of A with B's nearer end, otherwise A's point is d0 clamped and B's
    point the foot of the perpendicular.  A zero-length segment has NaN directions and NaN results."""
    a0, a1, b0, b1 = (np.asarray(x, dtype=np.float64) for x in (a0, a1, b0, b1))
    with np.errstate(invalid="ignore", divide="ignore"):
        A, B = a1 - a0, b1 - b0
        magA = np.sqrt((A[:, 0] ** 2 + A[:, 1] ** 2) + A[:, 2] ** 2)[:, None]
        magB = np.sqrt((B[:, 0] ** 2 + B[:, 1] ** 2) + B[:, 2] ** 2)[None, :]
        uA = (A / magA)[:, None, :]
        uB = (B / magB.T)[None, :, :]
        sA, sB = a0[:, None, :], b0[None, :, :]
        n = _cross(uA, uB)
        denom = np.sqrt(_dot(n, n)) ** 2
        parallel = denom == 0
        denom = np.where(parallel, 1.0, denom)
        t = sB - sA
        t0 = _dot(_cross(t, uB), n) / denom
        t1 = _dot(_cross(t, uA), n) / denom
        pA = sA + _clip0(t0, magA)[..., None] * uA
        pB = sB + _clip0(t1, magB)[..., None] * uB
        oobA = (t0 < 0) | (t0 > magA)
        oobB = (t1 < 0) | (t1 > magB)
        pB = np.where(oobA[..., None], sB + _clip0(_dot(pA - sB, uB), magB)[..., None] * uB, pB)
        pA = np.where(oobB[..., None], sA + _clip0(_dot(pB - sA, uA), magA)[..., None] * uA, pA)
        if parallel.any():
            base = _dot(uA, sA)
            d0 = _dot(uA, sB) - base
            d1 = _dot(uA, b1[None, :, :]) - base
            before = (d0 <= 0) & (d1 <= 0)
            after = (d0 >= magA) & (d1 >= magA)
            nearer = np.where((np.abs(d0) < np.abs(d1))[..., None], sB, b1[None, :, :])
            mA = sA + _clip0(d0, magA)[..., None] * uA
            g = sB - mA
            mB = mA + (g - _dot(g, uA)[..., None] * uA)
            qA = np.where(after[..., None], a1[:, None, :], np.where(before[..., None], sA, mA))
            qB = np.where((before | after)[..., None], nearer, mB)
            pA = np.where(parallel[..., None], qA, pA)
            pB = np.where(parallel[..., None], qB, pB)
        e = pA - pB
        dist = np.sqrt((e[..., 0] ** 2 + e[..., 1] ** 2) + e[..., 2] ** 2)
    return pA, pB, dist


def intersection_average(starts: np.ndarray, ends: np.ndarray) -> np.ndarray:
    """Mean of the closest points between all pairs of distinct segments (numeric.py:330-347): (3,)."""
    starts, ends = np.asarray(starts, dtype=np.float64), np.asarray(ends, dtype=np.float64)
    pA, pB, _ = segment_closest_points(starts, ends, starts, ends)
    mask = ~np.eye(starts.shape[0], dtype=bool)
    return np.mean(np.vstack([pA[mask], pB[mask]]), axis=0)


def ray_pair_edges(starts, ends, ray_IDs, similarity_threshold: float, min_dist: float = 1e-6, step: int = 5000,
                   transform: typing.Optional[typing.Callable[[np.ndarray], np.ndarray]] = None, backend=None):
    """`calc_graph_weights` as arrays: (i, j, weight) -- int64, int64, float64 -- of every graph edge, in the reference's order
    for `step`.  A Python list of millions of tuples costs more than the kernel; use this form for large surveys.

    After the device call, on the kept distances and in this order (numeric.py:488-498, 410-425): d < min_dist -> min_dist;
    `transform` (it is given the 1-D array of kept distances where the reference hands it a whole block matrix: elementwise
    callables only); non-finite values dropped; weight = 1 / d in float64.  Order: the reference visits the (step, step)
    blocks of the upper triangle row by row (its `chunk_slices`) and each block row-major, and networkx takes its node order
    from the edge list, so the order is part of the result."""
    if step <= 0:
        raise ValueError(f"step must be positive, got {step}")
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    starts, ends = np.asarray(starts, dtype=np.float64).reshape(-1, 3), np.asarray(ends, dtype=np.float64).reshape(-1, 3)
    ids = np.asarray(ray_IDs).reshape(-1)
    if not np.array_equal(ids, ids.astype(np.int32)):
        raise ValueError("ray_IDs must be integers within the int32 range")
    i, j, d = (_host(x) for x in backend.ray_pair_edges(starts, ends, ids.astype(np.int32), float(similarity_threshold)))
    i, j, d = i.astype(np.int64), j.astype(np.int64), d.astype(np.float64)
    d = np.where(d < min_dist, min_dist, d)
    if transform is not None:
        d = np.asarray(transform(d), dtype=np.float64)
        if d.shape != i.shape:
            raise ValueError("transform must be elementwise: it changed the shape of the distances")
    keep = np.isfinite(d)
    i, j, d = i[keep], j[keep], d[keep]
    with np.errstate(divide="ignore"):
        w = 1 / d
    order = np.lexsort((j, i, j // step, i // step))
    return i[order], j[order], w[order]


def calc_graph_weights(starts, ends, ray_IDs, similarity_threshold: float, out_dir: typing.Optional[PATH_TYPE] = None,
                       min_dist: float = 1e-6, step: int = 5000,
                       transform: typing.Optional[typing.Callable[[np.ndarray], np.ndarray]] = None, backend=None):
    """Graph edges between rays of different images that pass within `similarity_threshold` of each other, weighted by the
    inverse distance (numeric.py:428-506): a list of (i, j, {"weight": w}) or, with `out_dir`, the path of the
    `edge_weights.json` written there.  `step` only decides the ORDER of the list (see `ray_pair_edges`); the device kernel has
    its own tiling.  `transform`: elementwise callables only."""
    i, j, w = ray_pair_edges(starts, ends, ray_IDs, similarity_threshold, min_dist=min_dist, step=step, transform=transform,
                             backend=backend)
    edge_weights = [(a, b, {"weight": c}) for a, b, c in zip(i.tolist(), j.tolist(), w.tolist())]
    if out_dir is None:
        return edge_weights
    path = Path(out_dir) / "edge_weights.json"
    with path.open("w") as file:
        json.dump(edge_weights, file)
    return path


COMMUNITY_WEIGHT_SCALE = 1024   # L1 of DESIGN.md section 8p: the device sees q = max(1, rint(w * 1024))


def quantise_weights(w) -> np.ndarray:
    """L1: float edge weights -> the int64 weights the device works on, q = max(1, rint(w * COMMUNITY_WEIGHT_SCALE)).  ValueError:
    a weight that is not finite or not positive, a q above 2^31 - 1, or twice the sum of the q at or above 2^53 (below it every
    sum of the rule-set is exact in int64 and converts to float64 exactly)."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(w) & (w > 0)):
        raise ValueError("edge weights must be finite and positive")
    scaled = np.rint(w * COMMUNITY_WEIGHT_SCALE)
    if scaled.size and float(scaled.max()) > 2**31 - 1:
        raise ValueError(f"an edge weight of {float(w.max())} exceeds 2^31 - 1 after quantisation (x {COMMUNITY_WEIGHT_SCALE})")
    q = np.maximum(scaled.astype(np.int64), 1)
    if 2 * int(q.sum(dtype=np.int64)) >= 2**53:   # (q <= 2^31 - 1 each: the int64 sum itself cannot overflow)
        raise ValueError("twice the sum of the quantised edge weights reaches 2^53")
    return q


def community_modularity(record: dict, resolution: float = 1.0) -> float:
    """L13: Q = sum over the communities of in_c / M2 - resolution (tot_c / M2)^2, from the record of `louvain_communities`."""
    M2 = float(record["M2"])
    if M2 == 0:
        return 0.0
    c_in, c_tot = np.asarray(record["in"], dtype=np.float64), np.asarray(record["tot"], dtype=np.float64)
    return float(np.sum(c_in / M2 - float(resolution) * (c_tot / M2) ** 2))


def ray_communities(i, j, w, n_rays: int, resolution: float = 1.0, backend=None, max_sweeps: int = 32) -> dict:
    """Communities of the ray graph on the device (gr_louvain_communities): the edges as arrays -- i, j
    (E,) int, w (E,) float weights, as `ray_pair_edges` returns them -- of a graph of `n_rays` vertices.  The weights are
    quantised (`quantise_weights`, L1); the indices are checked on the device.  Returns the record of
    `HipRaster.louvain_communities` plus "modularity".  Deterministic: the same edges give the same record in every run."""
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    q = quantise_weights(_host(w))
    record = dict(backend.louvain_communities(i, j, q, int(n_rays), resolution=float(resolution), max_sweeps=int(max_sweeps)))
    record["modularity"] = community_modularity(record, resolution)
    return record


def _edge_arrays(edge_weights):
    """The tuple list of `calc_graph_weights` (or what json made of it), or an (i, j, w) triple of arrays -> (i, j, w) arrays."""
    if isinstance(edge_weights, tuple) and len(edge_weights) == 3 and all(hasattr(x, "shape") for x in edge_weights):
        return edge_weights
    i = np.fromiter((int(e[0]) for e in edge_weights), dtype=np.int64, count=len(edge_weights))
    j = np.fromiter((int(e[1]) for e in edge_weights), dtype=np.int64, count=len(edge_weights))
    w = np.fromiter((float(e[2]["weight"]) for e in edge_weights), dtype=np.float64, count=len(edge_weights))
    return i, j, w


def _device_communities(starts, ends, edge_weights, resolution, backend):
    """("ray_IDs", "community_points") of calc_communities(method="device"); None where the graph has no edge."""
    i, j, w = _edge_arrays(edge_weights)
    if int(np.shape(i)[0]) == 0:
        return None
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    record = ray_communities(i, j, w, starts.shape[0], resolution=resolution, backend=backend)
    community = np.asarray(record["community"])
    ray_IDs = np.where(community < 0, np.nan, community.astype(np.float64))
    points = _host(backend.community_points(starts, ends, community, int(record["n_communities"])))
    return ray_IDs, np.asarray(points, dtype=np.float64).reshape(-1, 3)


def _finish_communities(found, transform_to_epsg_4978, out_dir):
    """The result of calc_communities(method="device") from ("ray_IDs", "community_points") or None: the keys, the optional
    transform and the file of the networkx path, restated here so that that path stays as it is."""
    ecef = None
    if found is not None:
        ray_IDs, community_points = found
        result = {"ray_IDs": ray_IDs, "community_points": community_points}
        if transform_to_epsg_4978 is not None:
            homogenous = np.concatenate([community_points, np.ones_like(community_points[:, 0:1])], axis=1)
            ecef = (np.asarray(transform_to_epsg_4978) @ homogenous.T).T
    else:
        result = {"ray_IDs": np.zeros((0,), dtype=int), "community_points": np.zeros((0, 3))}
        if transform_to_epsg_4978 is not None:
            ecef = np.zeros((0, 4))
    if ecef is not None:
        try:
            import pyproj
        except ImportError:
            result["community_points_epsg_4978"] = ecef[:, :3]
        else:
            tr = pyproj.Transformer.from_crs(pyproj.CRS.from_epsg(4978), pyproj.CRS.from_epsg(4326))
            lat, lon, alt = tr.transform(ecef[:, 0], ecef[:, 1], ecef[:, 2])
            result["community_points_latlon"] = np.vstack([lat, lon, alt]).T
    if out_dir is not None:
        path = Path(out_dir) / "communities.npz"
        np.savez(path, **result)
        return path
    return result


def calc_communities(starts, ends, edge_weights, louvain_resolution: float = 1.0, out_dir: typing.Optional[PATH_TYPE] = None,
                     transform_to_epsg_4978: typing.Optional[np.ndarray] = None, seed=None, method: str = "networkx", backend=None):
    """Louvain communities of the ray graph and one 3D point per community (numeric.py:509-619).  Returns, or with `out_dir`
    saves as `communities.npz`, a dict with "ray_IDs" ((N,) float: community of every ray, NaN for a ray without an edge) and
    "community_points" ((M, 3): `intersection_average` of the community's rays), communities ordered by falling size.

    `seed` goes to networkx.community.louvain_communities (the reference is unseeded).  With `transform_to_epsg_4978` the
    reference adds "community_points_latlon" through pyproj.  Where pyproj is missing the transformed points are returned as
    "community_points_epsg_4978" instead and no lat/lon key is written: the conversion is not approximated.

    `method="device"` computes both on the device instead (`ray_communities`, `HipRaster.community_points`; DESIGN.md section
    8p): a deterministic rule-set, so `seed` is ignored and the partition is not the one networkx would draw; `edge_weights`
    may then also be an (i, j, w) triple of arrays; `backend` as for `ray_pair_edges`.  The keys, shapes and dtypes are the same."""
    if method not in ("networkx", "device"):
        raise ValueError(f"method must be 'networkx' or 'device', got {method!r}")
    starts, ends = np.asarray(starts, dtype=np.float64), np.asarray(ends, dtype=np.float64)
    if method == "device":
        found = _device_communities(starts, ends, edge_weights, louvain_resolution, backend)
        return _finish_communities(found, transform_to_epsg_4978, out_dir)
    import networkx

    graph = networkx.Graph([(int(e[0]), int(e[1]), dict(e[2])) for e in edge_weights])
    ecef = None
    if len(graph) > 0:
        communities = networkx.community.louvain_communities(graph, weight="weight", resolution=louvain_resolution, seed=seed)
        communities = sorted(communities, key=len, reverse=True)
        ray_IDs = np.full(starts.shape[0], fill_value=np.nan)
        community_points = []
        for community_ID, community in enumerate(communities):
            inds = np.array(list(community))
            ray_IDs[inds] = community_ID
            community_points.append(intersection_average(starts[inds], ends[inds]))
        community_points = np.vstack(community_points)
        result = {"ray_IDs": ray_IDs, "community_points": community_points}
        if transform_to_epsg_4978 is not None:
            homogenous = np.concatenate([community_points, np.ones_like(community_points[:, 0:1])], axis=1)
            ecef = (np.asarray(transform_to_epsg_4978) @ homogenous.T).T
    else:
        result = {"ray_IDs": np.zeros((0,), dtype=int), "community_points": np.zeros((0, 3))}
        if transform_to_epsg_4978 is not None:
            ecef = np.zeros((0, 4))
    if ecef is not None:
        try:
            import pyproj
        except ImportError:
            result["community_points_epsg_4978"] = ecef[:, :3]
        else:
            tr = pyproj.Transformer.from_crs(pyproj.CRS.from_epsg(4978), pyproj.CRS.from_epsg(4326))
            lat, lon, alt = tr.transform(ecef[:, 0], ecef[:, 1], ecef[:, 2])
            result["community_points_latlon"] = np.vstack([lat, lon, alt]).T
    if out_dir is not None:
        path = Path(out_dir) / "communities.npz"
        np.savez(path, **result)
        return path
    return result


SET_COVER_MAX_VIEWS = 65536      # GR_SETCOVER_MAX_VIEWS of include/geograster.h
SET_COVER_MAX_FACES = 2**31 - 1  # F < 2^31


def select_covering_views(visibility, min_observations_to_be_included=1, prune: bool = True, backend=None) -> dict:
    """A small set of views that together see every required face -- the set-cover stage of annotation_image_selection
    (reference: entrypoints/annotation_image_selection.py:142-174, there SetCoverPy on a dense matrix; the rule-set here is
    DESIGN.md section 8j, M1-M8, solved on the device by gr_set_cover).

    `visibility`: (F, N) scipy sparse matrix or array of any format, or a dense 2-D array; a non-zero entry means "view v sees
    face f".  It is brought to canonical CSR (duplicates summed, explicit zeros dropped, sorted indices, int64 pointers, int32
    indices), uploaded and handed to `backend.set_cover` (default: the shared `HipRaster` of the current device).  A face is
    required iff at least max(min_observations_to_be_included, 1) views see it -- a face that no view sees is never required,
    where the reference's solver would be infeasible.  Returns the record of `HipRaster.set_cover`: "selected" (N,) bool is the
    mask the workflow saves.  ValueError: `visibility` is not 2-D, or F or N exceed SET_COVER_MAX_FACES / SET_COVER_MAX_VIEWS."""
    from scipy import sparse

    is_sparse = sparse.issparse(visibility)
    if not is_sparse:
        visibility = np.asarray(visibility)
    if visibility.ndim != 2:
        raise ValueError(f"visibility must be (faces, views), got shape {tuple(visibility.shape)}")
    n_faces, n_views = (int(x) for x in visibility.shape)
    if n_faces > SET_COVER_MAX_FACES or n_views > SET_COVER_MAX_VIEWS:   # before a CSR of that many rows is built
        raise ValueError(f"visibility of shape {(n_faces, n_views)} exceeds the limits of the selection: {SET_COVER_MAX_FACES} "
                         f"faces, {SET_COVER_MAX_VIEWS} views")
    csr = sparse.csr_matrix(visibility, copy=True) if is_sparse else sparse.csr_matrix(visibility != 0)   # (a CSR input shares its arrays otherwise)
    if np.isnan(float(min_observations_to_be_included)):
        raise ValueError("min_observations_to_be_included is not a number")
    csr.sum_duplicates()
    csr.eliminate_zeros()
    csr.sort_indices()
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    return backend.set_cover(csr.indptr.astype(np.int64), csr.indices.astype(np.int32), n_faces, n_views,
                             min_observations=float(min_observations_to_be_included), prune=prune)


def create_ramped_weighting(rectangle_shape: typing.Tuple[int, int], ramp_dist_frac: float) -> np.ndarray:
    """The weight of every pixel of a (rows, columns) tile, float64 in [0, 1] (reference: utils/numeric.py:14-36; rule O2 of
    DESIGN.md 8m): along each axis a ramp of n evenly spaced values from 0 to 1 / ramp_dist_frac, cut off at 1, and the same ramp
    from the far edge; a pixel takes the smallest of its four ramp values.  Pixels further than `ramp_dist_frac` of the side from
    every edge weigh 1, and the outermost ring weighs 0."""
    ramps = []
    for n in rectangle_shape[:2]:
        ramp = np.clip(np.linspace(0, 1 / ramp_dist_frac, num=n), 0, 1)
        ramps.append(np.minimum(ramp, ramp[::-1]))
    return np.minimum(ramps[0][:, None], ramps[1][None, :])
