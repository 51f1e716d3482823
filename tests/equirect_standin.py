"""numpy stand-in for the device resampling of equirectangular photos into perspective views (gr_equirect_view), written for
the tests: the sample order and the value round trip of DESIGN.md "Equirectangular resampling", per sample, with the
pre-truncation values and the sampling coordinates exposed.  tests/test_equirect_host.py pins it to the reference's own output
in tests/golden/reference_equirect.npz and to live scipy.ndimage.map_coordinates; the GPU tests then use it where no golden
exists.

Keep this copy: geograypher_amd/utils/image.py prepares the same host inputs (the x / y vectors and the rotation matrix), and
this module must not be "simplified" to import them -- the tests would then compare the package with itself.  Both are pinned
to the reference's goldens separately."""
import numpy as np

FILL = 0.0   # the fill value of the reference's flexible_inputs_warp call (utils/image.py:241-243 leaves the default)


def rotation_matrix(roll_deg, pitch_deg, yaw_deg):
    """utils/image.py:29-55: roll about the camera's Z, pitch about X, yaw about Y."""
    from scipy.spatial.transform import Rotation

    yaw, pitch, roll = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg), np.deg2rad(roll_deg)
    perm = np.array([[0, 0, 1], [1, 0, 0], [0, -1, 0]])
    rot = Rotation.from_euler("ZYX", [yaw, pitch, roll]).as_matrix()
    return perm.T @ rot @ perm


def view_axes(fov_deg, output_size, oversample_factor):
    """utils/image.py:174-196: the ray coordinates of the oversampled view's columns and rows."""
    out_h, out_w = output_size
    out_w = int(out_w * oversample_factor)
    out_h = int(out_h * oversample_factor)
    fov = np.deg2rad(fov_deg)
    aspect_ratio = out_h / out_w
    x_dist = np.tan(fov / 2)
    y_dist = x_dist * aspect_ratio
    pixel_width = (2 * x_dist) / out_w
    x = np.arange(-x_dist + pixel_width / 2, x_dist, pixel_width)
    y = np.arange(-y_dist + pixel_width / 2, y_dist, pixel_width)
    assert len(x) == out_w and len(y) == out_h
    return x, y


def sample_coordinates(x, y, rot, H, W):
    """(i, j), each (len(y), len(x)) f64: utils/image.py:199-235."""
    xv, yv = np.meshgrid(x, -y)
    d = np.stack((xv, yv, np.ones_like(xv)), axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d @ rot.T
    horizontal = np.arctan2(d[..., 0], d[..., 2])
    altitude = np.arcsin(np.clip(d[..., 1], -1.0, 1.0))
    i = (0.5 - altitude / np.pi) * H
    j = (horizontal / (2 * np.pi) + 0.5) * W
    return np.clip(i, 0, H - 1), np.clip(j, 0, W)


def value_range(img):
    """vmin, vrange of utils/image.py:89-92 with fill 0."""
    vmin = min(float(np.min(img)), FILL)
    vmax = max(float(np.max(img)), FILL)
    return vmin, vmax - vmin


def channel_bounds(img3, vmin, vrange):
    """(C, 2): the normalised [min, max] of every channel, widened to hold the normalised fill (skimage's clip)."""
    norm = (img3.astype(float) - vmin) / vrange
    nfill = (FILL - vmin) / vrange
    lo = np.minimum(norm.min(axis=(0, 1)), nfill)
    hi = np.maximum(norm.max(axis=(0, 1)), nfill)
    return np.stack([lo, hi], axis=1)


def _taps(norm, rows, cols, nfill):
    """norm[rows, cols] of the image with column W = column 0 appended; everything outside that reads the fill."""
    H, W = norm.shape[:2]
    inside = (rows >= 0) & (rows < H) & (cols >= 0) & (cols <= W)
    r = np.where(inside, rows, 0).astype(np.int64)
    c = np.where(inside, cols, 0).astype(np.int64)
    c = np.where(c == W, 0, c)
    v = norm[r, c]
    return np.where(inside[..., None], v, nfill)


def interpolate(norm, i, j, order, nfill):
    """The normalised, unclipped sample of every channel at (i, j): (..., C)."""
    if order == 0:
        return _taps(norm, np.floor(i + 0.5), np.floor(j + 0.5), nfill)
    if order != 1:
        raise NotImplementedError(f"interpolation order {order}")
    r0, c0 = np.floor(i), np.floor(j)
    tr, tc = i - r0, j - c0
    wr0, wr1 = (1.0 - tr)[..., None], tr[..., None]
    wc0, wc1 = (1.0 - tc)[..., None], tc[..., None]
    t = _taps(norm, r0, c0, nfill) * wr0 * wc0
    t = t + _taps(norm, r0, c0 + 1, nfill) * wr0 * wc1
    t = t + _taps(norm, r0 + 1, c0, nfill) * wr1 * wc0
    t = t + _taps(norm, r0 + 1, c0 + 1, nfill) * wr1 * wc1
    return t


def sample_values(img, i, j, order=1):
    """Per-sample values BEFORE the truncation to the source dtype: (ny, nx, C) f64, or None for a source without variation."""
    img3 = np.atleast_3d(img)
    vmin, vrange = value_range(img3)
    if vrange == 0:
        return None
    norm = (img3.astype(float) - vmin) / vrange
    nfill = (FILL - vmin) / vrange
    t = interpolate(norm, i, j, order, nfill)
    if order != 0:
        b = channel_bounds(img3, vmin, vrange)
        t = np.minimum(np.maximum(t, b[:, 0]), b[:, 1])
    return t * vrange + vmin


def sampling_mask(i, j, H, W):
    """utils/image.py:255-265."""
    mask = np.zeros((H, W + 1), dtype=bool)
    mask[np.round(i).astype(int), np.round(j).astype(int)] = True
    mask[:, 0] |= mask[:, -1]
    return mask[:, :-1]


def perspective_np(equi_img, x, y, rot, oversample_factor=1, order=1, return_mask=False, return_debug=False):
    """What the device computes from the same host inputs.  return_debug adds {"pre": per-sample values before truncation
    (ny, nx, C) or None, "ij": (2, ny, nx)}."""
    img = np.asarray(equi_img)
    H, W = img.shape[:2]
    os_ = int(oversample_factor)
    ny, nx = len(y), len(x)
    i, j = sample_coordinates(x, y, rot, H, W)
    pre = sample_values(img, i, j, order)
    img3 = np.atleast_3d(img)
    if pre is None:
        samples = np.full((ny, nx, img3.shape[2]), FILL, dtype=img.dtype)
    else:
        samples = pre.astype(img.dtype)   # truncation toward zero for integers
    if os_ > 1:
        C = samples.shape[2]
        blocks = samples.astype(float).reshape(ny // os_, os_, nx // os_, os_, C)
        # row-major over the block: the order in which the device adds its samples
        acc = np.zeros((ny // os_, nx // os_, C))
        for a in range(os_):
            for b in range(os_):
                acc = acc + blocks[:, a, :, b, :]
        out = acc / (os_ * os_)
    else:
        out = samples
    out = np.squeeze(out)
    res = [out]
    if return_mask:
        res.append(sampling_mask(i, j, H, W))
    if return_debug:
        res.append({"pre": pre, "ij": np.stack([i, j])})
    return res[0] if len(res) == 1 else tuple(res)


def perspective_from_equirectangular_np(equi_img, fov_deg, output_size=(1440, 1440), yaw_deg=0, pitch_deg=0, roll_deg=0,
                                        warp_order=1, oversample_factor=1, return_mask=False, return_debug=False):
    """The reference's signature (utils/image.py:129-139)."""
    x, y = view_axes(fov_deg, output_size, oversample_factor)
    rot = rotation_matrix(roll_deg, pitch_deg, yaw_deg)
    return perspective_np(equi_img, x, y, rot, oversample_factor, warp_order, return_mask, return_debug)


class StandInBackend:
    """The device call of HipRaster behind geograypher_amd.utils.image, on the host."""

    def __init__(self):
        self.equirect_uploads = 0

    def equirect_upload(self, equi_img):
        self.equirect_uploads += 1
        return np.asarray(equi_img)

    def equirect_view(self, source, x, y, rot, output_size, oversample_factor=1, order=1, return_mask=False,
                      return_debug=False):
        return perspective_np(source, x, y, rot, oversample_factor, order, return_mask, return_debug)
