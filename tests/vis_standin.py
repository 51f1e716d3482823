"""numpy stand-ins of the picture calls (include/geograster_vis.h): the same operations in the same order,
each rounded on its own, so the device must give every byte.  `composite` is also held against the reference's own answers
(tests/golden/composites.npz) by tests/test_vis_host.py."""
import numpy as np

NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))   # V5: (row, column) offsets in units of r


def face_light(verts, faces, view_dir, ambient):
    """V3 -> (F,) uint8."""
    verts = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    d = np.asarray(view_dir, dtype=np.float64)
    ambient = np.float64(ambient)
    shade = np.ones(len(faces))
    good = ((faces >= 0) & (faces < len(verts))).all(axis=1)
    a, b, c = (verts[faces[good][:, k]] for k in range(3))
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    length = np.sqrt((nx * nx + ny * ny) + nz * nz)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.abs((nx * d[0] + ny * d[1]) + nz * d[2]) / length
    shade[good] = np.where(length != 0.0, s, 1.0)
    with np.errstate(invalid="ignore"):
        v = np.floor((ambient + (np.float64(1.0) - ambient) * shade) * 255.0 + 0.5)
        v = np.where(v >= 255.0, 255.0, np.where(v >= 0.0, v, 0.0))
    return v.astype(np.uint8)


def shade_view(ids, depth, face_rgb, face_light_, supersample, radius, strength, background=(255, 255, 255)):
    """V4-V7 in float32 -> (H, W, 3) uint8."""
    f32 = np.float32
    ids = np.asarray(ids, dtype=np.int32)
    depth = np.asarray(depth, dtype=f32)
    rgb = np.asarray(face_rgb, dtype=np.uint8).reshape(-1, 3)
    light = np.asarray(face_light_, dtype=np.uint8).reshape(-1)
    s, r, k = int(supersample), int(radius), f32(strength)
    Hs, Ws = ids.shape
    H, W, F = Hs // s, Ws // s, len(rgb)
    face = (ids >= 0) & (ids < F)
    safe = np.where(face, ids, 0)
    occl = np.ones((Hs, Ws), dtype=f32)
    with np.errstate(all="ignore"):
        if k != 0:
            padded = np.full((Hs + 2 * r, Ws + 2 * r), np.inf, dtype=f32)
            padded[r:r + Hs, r:r + Ws] = depth
            total = np.zeros((Hs, Ws), dtype=f32)
            for dy, dx in NEIGHBOURS:
                zq = padded[r + dy * r:r + dy * r + Hs, r + dx * r:r + dx * r + Ws]
                t = (depth - zq) / depth
                total = total + np.where(t > 0, t, f32(0))
            occl = f32(1) / (f32(1) + k * total)
        if F:
            lit = light[safe].astype(f32) / f32(255)
            colour = (rgb[safe].astype(f32) * lit[..., None]) * occl[..., None]
        else:
            colour = np.zeros((Hs, Ws, 3), dtype=f32)
        colour = np.where(face[..., None], colour, np.asarray(background, dtype=f32))
        acc = np.zeros((H, W, 3), dtype=f32)
        for sy in range(s):          # row-major over the samples of a pixel
            for sx in range(s):
                acc = acc + colour[sy::s, sx::s]
        v = np.floor(acc / f32(s * s) + f32(0.5))
        v = np.where(v >= 255, f32(255), np.where(v >= 0, v, f32(0)))
    assert v.dtype == f32
    return v.astype(np.uint8)


def composite_scalars(label, discrete):
    """(shift, scale) of a continuous one-channel label as the reference takes them (V11): nanmin of the values (a uint8 label
    divided by 255), and the maximum of the shifted values over the pixels that are not null, 1.0 where there is none."""
    label = np.asarray(label)
    if discrete or label.ndim == 3:
        return 0.0, 1.0
    x = label / 255 if label.dtype == np.uint8 else label.astype(np.float64)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            shift = np.nanmin(x)
        valid = (x - shift)[~((x == 0) | ~np.isfinite(x))]
    return float(shift), float(valid.max()) if valid.size else 1.0


def _byte(v):
    """V12"""
    with np.errstate(all="ignore"):
        x = v * 255.0
        ok = (x > -2147483649.0) & (x < 2147483648.0)
        return np.where(ok, x, 0.0).astype(np.int32).astype(np.uint8)


def composite(photo, label, table, discrete, shift, scale, weight, grey):
    """V8-V12 in float64 -> (h, 3 w, 3) uint8."""
    photo, label = np.asarray(photo), np.asarray(label)
    c = photo / 255 if photo.dtype == np.uint8 else photo.astype(np.float64)
    with np.errstate(all="ignore"):
        if label.ndim == 3:
            assert not (label.dtype == np.uint8 and discrete)
            lab = label / 255 if label.dtype == np.uint8 else label.astype(np.float64)
        elif label.dtype == np.uint8 and discrete:
            table = np.asarray(table, dtype=np.float64)
            lab = table[np.minimum(label.astype(np.int64), len(table) - 1)]
            lab[label == 0] = 0.0
        else:
            table = np.asarray(table, dtype=np.float64)
            N = len(table)
            x = label / 255 if label.dtype == np.uint8 else label.astype(np.float64)
            null = (x == 0) | ~np.isfinite(x)
            if not discrete:
                x = (x - np.float64(shift)) / np.float64(scale)
            t = x * np.float64(N)
            t = np.where(t == N, np.float64(N - 1), t)
            idx = np.where(t < 0, 0, np.where(t >= N, N - 1, np.where(np.isnan(t), 0, t))).astype(np.int64)
            lab = table[idx]
            lab[np.isnan(t) | null] = 0.0
        base = np.repeat((((c[..., 0] + c[..., 1]) + c[..., 2]) / 3.0)[..., None], 3, axis=2) if grey else c
        overlay = (np.float64(1.0) - np.float64(weight)) * base + np.float64(weight) * lab
        return _byte(np.concatenate((lab, c, overlay), axis=1))
