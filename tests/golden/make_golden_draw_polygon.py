"""Writes tests/golden/reference_draw_polygon.npz: masks of the REAL `skimage.draw.polygon(rows, cols, shape=...)` for the
rings `RegionDetectionSegmentor` must fill identically (tests/test_region_segmentor_host.py).  Run with an interpreter that
has scikit-image (made with 0.18.3); the package itself never imports it.

Arrays: `shapes` (n, 2) int, `offsets` (n + 1,) int, `verts` (N, 2) float64 (row, col), `names` (n,) str, and `masks`, the
n bool masks flattened one behind the other (mask k is shapes[k][0] x shapes[k][1])."""
from pathlib import Path

import numpy as np
from skimage import draw


def rings():
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, shape, pts):
        out.append((name, shape, np.asarray(pts, dtype=np.float64).reshape(-1, 2)))

    for k in range(6):  # convex: points on an ellipse, sorted by angle
        n = int(rng.integers(3, 12))
        t = np.sort(rng.uniform(0, 2 * np.pi, n))
        c, rad = rng.uniform(15, 50, 2), rng.uniform(4, 25, 2)
        add(f"convex{k}", (64, 80), np.stack([c[0] + rad[0] * np.sin(t), c[1] + rad[1] * np.cos(t)], axis=1))
    for k in range(6):  # concave: a star with random radii
        n = int(rng.integers(5, 24))
        t = np.linspace(0, 2 * np.pi, n, endpoint=False)
        rad = rng.uniform(3, 28, n)
        add(f"concave{k}", (64, 80), np.stack([32 + rad * np.sin(t), 40 + rad * np.cos(t)], axis=1))
    for k in range(6):  # self-intersecting: random points in random order
        n = int(rng.integers(4, 10))
        add(f"selfx{k}", (48, 37), rng.uniform(-5, 50, (n, 2)))
    for k in range(4):  # partly off-image
        n = int(rng.integers(3, 9))
        add(f"partly_off{k}", (40, 50), rng.uniform(-30, 80, (n, 2)))
    add("off_above", (40, 50), [(-20, 5), (-3, 5), (-3, 30), (-20, 30)])
    add("off_right", (40, 50), [(5, 60.5), (30, 60.5), (30, 90), (5, 90)])
    add("off_below_left", (40, 50), [(45, -20), (60, -20), (60, -2)])
    # integer vertices: pixel centres on vertices, on horizontal, vertical and diagonal edges
    add("int_rect", (40, 40), [(20, 20), (20, 30), (30, 30), (30, 20), (20, 20)])
    add("int_rect_ccw", (40, 40), [(20, 20), (30, 20), (30, 30), (20, 30)])
    add("int_rect_at_origin", (40, 40), [(0, 0), (0, 10), (10, 10), (10, 0), (0, 0)])
    add("int_rect_over_edge", (30, 30), [(25, 25), (25, 35), (35, 35), (35, 25)])
    add("int_rect_thin", (20, 20), [(5, 3), (5, 15), (6, 15), (6, 3)])
    add("int_tri", (40, 40), [(0, 0), (0, 10), (10, 0)])
    add("int_tri_ccw", (40, 40), [(5, 5), (25, 5), (5, 25)])
    add("int_tri_apex", (32, 32), [(2, 16), (30, 2), (30, 30)])
    add("int_diamond", (33, 33), [(16, 2), (30, 16), (16, 30), (2, 16)])
    add("int_bowtie", (30, 30), [(5, 5), (25, 25), (5, 25), (25, 5)])
    add("int_L", (30, 30), [(2, 2), (2, 20), (10, 20), (10, 10), (20, 10), (20, 2)])
    add("half_tri", (40, 40), [(0.5, 0.5), (0.5, 10.5), (10.5, 0.5)])
    add("collinear3", (30, 30), [(3, 3), (10, 10), (20, 20)])
    add("collinear3_flat", (30, 30), [(7, 2), (7, 12), (7, 25)])
    add("repeated_close", (40, 40), [(4, 4), (4, 19.5), (22.25, 19.5), (22.25, 4), (4, 4), (4, 4)])
    add("single_pixel", (10, 10), [(3, 3), (3, 4), (4, 4), (4, 3)])
    add("sub_pixel", (10, 10), [(3.2, 3.2), (3.2, 3.7), (3.7, 3.7), (3.7, 3.2)])
    add("two_points", (12, 12), [(2, 2), (8, 8)])
    return out


def main():
    names, shapes, offsets, verts, masks = [], [], [0], [], []
    for name, shape, pts in rings():
        rr, cc = draw.polygon(pts[:, 0], pts[:, 1], shape=shape)
        mask = np.zeros(shape, dtype=bool)
        mask[rr, cc] = True
        names.append(name)
        shapes.append(shape)
        verts.append(pts)
        offsets.append(offsets[-1] + pts.shape[0])
        masks.append(mask.reshape(-1))
    out = Path(__file__).resolve().parent / "reference_draw_polygon.npz"
    np.savez_compressed(out, names=np.array(names), shapes=np.array(shapes, dtype=np.int64),
                        offsets=np.array(offsets, dtype=np.int64), verts=np.concatenate(verts),
                        masks=np.concatenate(masks))
    print(out, len(names), "rings", int(np.concatenate(masks).sum()), "pixels")


if __name__ == "__main__":
    main()
