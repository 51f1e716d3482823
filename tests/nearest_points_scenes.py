"""The scenes of the nearest-point tests (a helper module for the tests): the smallest at which each part of
gr_nearest_points can go wrong.  A scene is a dict: name, ref, query, and the arguments max_distance, cell, max_rings of the call
(the defaults of `HipRaster.nearest_points` where a scene does not care).  Everything is seeded; nothing here needs a GPU."""
import numpy as np

DEFAULTS = dict(max_distance=None, cell=0.0, max_rings=2)
SIZES_R = (0, 1, 63, 64, 65)
SIZES_Q = (0, 1, 63, 64, 65, 257)


def scene(name, ref, query, **kw):
    ref, query = np.ascontiguousarray(ref, dtype=np.float64), np.ascontiguousarray(query, dtype=np.float64)
    ref.setflags(write=False)
    query.setflags(write=False)
    return dict(DEFAULTS, name=name, ref=ref, query=query, **kw)


def lattice_scene():
    """Integer points: the arithmetic of K2 is exact, and many queries have two refs at one distance (the lowest row wins)."""
    rng = np.random.default_rng(11)
    ref = np.unique(rng.integers(-40, 40, (3000, 3)), axis=0).astype(np.float64)
    rng.shuffle(ref, axis=0)
    return scene("lattice", ref, rng.integers(-45, 45, (2000, 3)))


def terrain_scene():
    """A 120 x 120 height field far from the origin, as a mesh in EPSG:4978 is: a random quarter of the vertices against all."""
    rng = np.random.default_rng(12)
    i, j = np.meshgrid(np.arange(120), np.arange(120), indexing="ij")
    x, y = 0.37 * i, 0.41 * j
    z = 3.0 * np.sin(x / 7.0) * np.cos(y / 5.0) + rng.normal(0.0, 0.05, x.shape)
    points = np.stack([x, y, z], axis=-1).reshape(-1, 3) + np.array([-2.6e6, -4.3e6, 3.9e6])
    return scene("terrain", points[rng.permutation(len(points))[:len(points) // 4]], points)


def duplicates_scene():
    """Every ref row occurs three times: the lowest of the three rows is the answer."""
    rng = np.random.default_rng(13)
    base = rng.normal(0.0, 10.0, (200, 3))
    ref = np.concatenate([base, base, base])[rng.permutation(600)]
    return scene("duplicates", ref, np.concatenate([rng.normal(0.0, 12.0, (300, 3)), base[:40]]))


def two_clusters_scene():
    """Two clusters 1 km apart, queries inside them, midway and far outside the box; cells of 1 cm and one ring force several
    levels."""
    rng = np.random.default_rng(14)
    ref = np.concatenate([rng.normal(0.0, 1.0, (300, 3)), rng.normal(0.0, 1.0, (300, 3)) + (1000.0, 0.0, 0.0)])
    query = np.concatenate([rng.normal(0.0, 1.5, (100, 3)), rng.normal(0.0, 1.5, (100, 3)) + (1000.0, 0.0, 0.0),
                            rng.normal(0.0, 20.0, (60, 3)) + (500.0, 0.0, 0.0), rng.normal(0.0, 100.0, (60, 3)) + (-9000.0, 7000.0, 3000.0),
                            [[500.0, 0.0, 0.0], [1e12, -1e12, 1e9], [-1e300, 0.0, 0.0]]])
    return scene("two_clusters", ref[rng.permutation(600)], query, cell=0.01, max_rings=1)


def nonfinite_scene():
    rng = np.random.default_rng(15)
    ref, query = rng.normal(0.0, 5.0, (150, 3)), rng.normal(0.0, 6.0, (130, 3))
    ref[[0, 17, 64, 149], [0, 1, 2, 0]] = (np.nan, np.inf, -np.inf, np.nan)
    ref[90] = np.nan
    query[[3, 63, 64, 129], [2, 0, 1, 1]] = (np.nan, -np.inf, np.inf, np.nan)
    return scene("nonfinite", ref, query)


def no_finite_ref_scene():
    ref = np.full((5, 3), 1.0)
    ref[:, 1] = (np.nan, np.inf, np.nan, -np.inf, np.nan)
    return scene("no_finite_ref", ref, np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [1.0, 2.0, 3.0]]))


def sizes_scene(R, Q):
    rng = np.random.default_rng(1000 * R + Q)
    return scene(f"sizes_R{R}_Q{Q}", rng.normal(0.0, 3.0, (R, 3)), rng.normal(0.0, 4.0, (Q, 3)))


def one_point_scene():
    """All refs at one point: the extent is 0 on every axis."""
    rng = np.random.default_rng(16)
    return scene("one_point", np.tile([[7.5, -2.25, 1e6]], (70, 1)), np.concatenate([rng.normal(0.0, 3.0, (66, 3)), [[7.5, -2.25, 1e6]]]))


def collinear_scene():
    """Refs on a line along x: two extents are 0."""
    rng = np.random.default_rng(17)
    ref = np.zeros((500, 3))
    ref[:, 0] = rng.uniform(-50.0, 50.0, 500)
    query = rng.normal(0.0, 30.0, (300, 3))
    return scene("collinear", ref + (3.0, 4.0, 5.0), query)


def corner_scene():
    """Refs on the maximum corner of the box with the smallest cell there is, e1 / 2^21: floor((hi - lo) / cell) is 2^21, one past
    the last cell, and has to be clipped."""
    rng = np.random.default_rng(18)
    ref = np.concatenate([rng.uniform(0.0, 64.0, (200, 3)), np.tile([[64.0, 64.0, 64.0]], (3, 1)), [[0.0, 0.0, 0.0]],
                          [[64.0, 0.0, 64.0]], [[64.0, 64.0, 0.0]]])
    query = np.concatenate([rng.uniform(60.0, 70.0, (100, 3)), [[64.0, 64.0, 64.0]], [[100.0, 100.0, 100.0]], [[64.0, 63.99999, 64.0]]])
    return scene("corner", ref, query, cell=64.0 / 2 ** 21, max_rings=1)


def planar_scene():
    """(n, 2) inputs: z = 0."""
    rng = np.random.default_rng(19)
    return scene("planar", rng.uniform(0.0, 100.0, (400, 2)), rng.uniform(-5.0, 105.0, (257, 2)))


def threshold_scenes():
    """The ref is exactly 5 from the query -- (3, 4, 0): 9 + 16 = 25 without rounding --: max_distance = 5 keeps it, the float64
    below 5 does not."""
    ref, query = np.array([[13.0, 24.0, 7.0], [500.0, 0.0, 0.0]]), np.array([[10.0, 20.0, 7.0], [13.0, 24.0, 7.0]])
    return [scene("threshold_kept", ref, query, max_distance=5.0),
            scene("threshold_dropped", ref, query, max_distance=float(np.nextafter(5.0, 0.0)))]


def main_scenes():
    return [lattice_scene(), terrain_scene(), duplicates_scene(), two_clusters_scene()]


def degenerate_scenes():
    return ([nonfinite_scene(), no_finite_ref_scene(), one_point_scene(), collinear_scene(), corner_scene(), planar_scene()] + threshold_scenes()
            + [sizes_scene(R, Q) for R in SIZES_R for Q in SIZES_Q])


def all_scenes():
    return main_scenes() + degenerate_scenes()


def sweep_arguments(s):
    """The (cell, max_rings) pairs of the parameter sweep: K3 says none of them reaches the answer."""
    part = s["ref"][np.isfinite(s["ref"]).all(axis=1)]
    e1 = float(np.max(part.max(axis=0) - part.min(axis=0))) if len(part) else 0.0
    e1 = e1 if e1 > 0 else 1.0
    return [(cell, rings) for cell in (0.0, 1e-3 * e1, e1 / 3.0, 10.0 * e1) for rings in (1, 2, 5)]
