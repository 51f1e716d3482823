"""Geometric helpers of the multiview-detection workflow (reference: geograypher/utils/geometric.py:97-106, 144-254).

This package has no pyvista: a boundary surface is a `(points (V, 3) float, faces (F, 3) int)` pair, and the ray / surface
intersection runs on the device (`HipRaster.clip_rays`, gr_rays_clip: brute force over a coarse covering mesh).
"""
from __future__ import annotations

import typing

import numpy as np


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def get_scale_from_transform(transform: typing.Union[np.ndarray, None]):
    """Isotropic scale of a 4x4 transform: the cube root of the determinant of its 3x3 block; 1 for None
    (geometric.py:97-106)."""
    if transform is None:
        return 1
    if transform.shape != (4, 4):
        raise ValueError(f"Transform shape was {transform.shape}")
    return np.cbrt(np.linalg.det(transform[:3, :3]))


def clip_line_segments(boundaries, origins: np.ndarray, directions: np.ndarray,
                       image_indices: typing.Union[typing.List[int], np.ndarray],
                       ray_limit: typing.Optional[float] = None, backend=None):
    """Clip rays between two boundary surfaces, keeping the rays that hit both (geometric.py:144-254).

    boundaries: two (points, faces) pairs, e.g. (ceiling, floor).  Returns (starts, ends, directions, image indices) of the
    kept rays: start = the nearest hit on boundaries[0], end = the nearest hit on boundaries[1] (along the infinite ray from
    the origin, t >= 0), direction re-normalised from the two hits.  `ray_limit` drops a ray whose |origin - end| exceeds it.
    The kept rays come in ascending ray index (the reference iterates a Python set of ray indices: its order is whatever the
    set yields).  `backend`: a `HipRaster` (default: the shared one) or an object with its `clip_rays` method."""
    if len(boundaries) != 2:
        raise ValueError(f"2 boundaries required, not {len(boundaries)}")
    if any(not (isinstance(b, (tuple, list)) and len(b) == 2) for b in boundaries):
        raise ValueError(f"(points, faces) pairs required, found {[type(b) for b in boundaries]}")
    origins, directions = np.asarray(origins), np.asarray(directions)
    if origins.shape != directions.shape:
        raise ValueError(f"origins and directions mismatched ({origins.shape} != {directions.shape})")
    if origins.ndim != 2 or origins.shape[1] != 3:
        raise ValueError(f"(N, 3) input arrays required, found {origins.shape}")
    if len(origins) != len(image_indices):
        raise ValueError(f"origins and image indices mismatched ({len(origins)} != {len(image_indices)})")
    if len(origins) == 0:
        return origins.copy(), origins.copy(), directions.copy(), np.array(image_indices)
    if backend is None:
        from geograypher_amd._hip import default_backend

        backend = default_backend()
    origins = origins.astype(np.float64)
    hits = []
    for points, faces in boundaries:
        hit, _t, pts = (_host(x) for x in backend.clip_rays(origins, directions.astype(np.float64), np.asarray(points),
                                                            np.asarray(faces)))
        hits.append((hit.astype(bool), pts))
    keep = hits[0][0] & hits[1][0]
    pt0, pt1 = hits[0][1], hits[1][1]
    if ray_limit is not None:
        with np.errstate(invalid="ignore"):
            keep &= ~(np.linalg.norm(origins - pt1, axis=1) > ray_limit)
    pt0, pt1 = pt0[keep], pt1[keep]
    with np.errstate(invalid="ignore", divide="ignore"):
        new_directions = (pt1 - pt0) / np.linalg.norm(pt1 - pt0, axis=1, keepdims=True)
    return pt0, pt1, new_directions, np.asarray(image_indices)[keep]
