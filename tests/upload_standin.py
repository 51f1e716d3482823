"""TEST INFRASTRUCTURE ONLY: gr_mesh_upload (csrc/mesh_upload.hip) and k_cull_blocks (csrc/binning.hip) restated in numpy,
operation for operation in float32.  The library is compiled with -ffp-contract=off and correctly rounded divide / sqrt, so
every operation rounds on its own there as it does here: the products are compared bit for bit.  Anchored by
tests/test_mesh_upload_host.py (hand-worked cases, containment in exact arithmetic, the cull against float64), which never
runs the library."""
import numpy as np

F32 = np.float32
GR_BLOCK = 64
GR_BLOCK_VERTS = 192
_INF = F32(np.inf)
THIRD = F32(1.0) / F32(3.0)   # the 1.0f / 3.0f of k_face_codes
M64 = (1 << 64) - 1


# ---- float <-> ordered uint32 (atomicMin / atomicMax on floats) ----------------------------------------------------------
def float_ordered(x) -> np.ndarray:
    b = np.asarray(x, dtype=F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def ordered_float(u) -> np.ndarray:
    u = np.asarray(u, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(F32)


def fmin_all(x, axis=None) -> np.ndarray:
    """fminf over `x` started at +inf: NaN is dropped, -0 lies below +0 (v_min_f32)."""
    key = np.where(np.isnan(x), float_ordered(_INF), float_ordered(x))
    return ordered_float(np.minimum(key.min(axis=axis, initial=float_ordered(_INF)), float_ordered(_INF)))


def fmax_all(x, axis=None) -> np.ndarray:
    """fmaxf over `x` started at -inf: NaN is dropped, +0 lies above -0 (v_max_f32)."""
    key = np.where(np.isnan(x), float_ordered(-_INF), float_ordered(x))
    return ordered_float(np.maximum(key.max(axis=axis, initial=float_ordered(-_INF)), float_ordered(-_INF)))


# ---- k_mesh_bounds and the host code behind it ----------------------------------------------------------------------------
def mesh_bounds_words(verts) -> np.ndarray:
    """The six words the upload reads back: ordered min x3, ordered max x3 of the FINITE coordinates of all vertices."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    fin = np.isfinite(v)
    lo = fmin_all(np.where(fin, v, _INF), axis=0)
    hi = fmax_all(np.where(fin, v, -_INF), axis=0)
    return np.concatenate([float_ordered(lo), float_ordered(hi)])


def mesh_sig(F: int, V: int, words) -> int:
    """splitmix64 steps over F, V and the six bounds words; 0 is never answered."""
    h = 0x9E3779B97F4A7C15 ^ int(F)

    def mix(h, v):
        h = (h + int(v) + 0x9E3779B97F4A7C15) & M64
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & M64
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & M64
        return h ^ (h >> 31)

    h = mix(h, V)
    for w in words:
        h = mix(h, w)
    return h if h else 1


def extents(words):
    """(lo [3], ext [3]): ext = hi - lo, 0 without a finite coordinate on the axis or where hi - lo overflows."""
    with np.errstate(all="ignore"):
        lo, hi = ordered_float(words[:3]), ordered_float(words[3:])
        ext = np.where(hi >= lo, hi - lo, F32(0)).astype(F32)
        ext = np.where(~(ext >= 0) | np.isinf(ext), F32(0), ext).astype(F32)
    return lo, ext


def morton_axes(ext):
    """ax0, ax1 as the two swaps of gr_mesh_upload leave them (ties keep the earlier choice)."""
    ax0, ax1, axs = 0, 1, 2
    if ext[axs] > ext[ax0]:
        axs, ax0 = ax0, axs
    if ext[axs] > ext[ax1]:
        axs, ax1 = ax1, axs
    return ax0, ax1


def spread16(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint32) & np.uint32(0xFFFF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x00FF00FF)
    x = (x | (x << np.uint32(4))) & np.uint32(0x0F0F0F0F)
    x = (x | (x << np.uint32(2))) & np.uint32(0x33333333)
    x = (x | (x << np.uint32(1))) & np.uint32(0x55555555)
    return x


def _code16(c, lo, inv) -> np.ndarray:
    """(uint32_t) fminf(fmaxf((c - lo) * inv, 0), 65535): NaN -> 0, then truncation"""
    with np.errstate(all="ignore"):
        q = ((c - lo).astype(F32) * inv).astype(F32)
    q = np.where(np.isnan(q), F32(0), q)
    q = np.minimum(np.maximum(q, F32(0)), F32(65535))
    return np.trunc(q).astype(np.uint32)


def face_codes(verts, faces) -> np.ndarray:
    """k_face_codes with the arguments gr_mesh_upload hands it: the 32-bit Morton code of every face."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lo, ext = extents(mesh_bounds_words(v))
    ax0, ax1 = morton_axes(ext)
    out = []
    for ax in (ax0, ax1):
        with np.errstate(all="ignore"):
            inv = F32(65535) / ext[ax] if ext[ax] > 0 else F32(0)
            p0, p1, p2 = v[f[:, 0], ax], v[f[:, 1], ax], v[f[:, 2], ax]
            c = (((p0 + p1).astype(F32) + p2).astype(F32) * THIRD).astype(F32)
        out.append(spread16(_code16(c, lo[ax], F32(inv))))
    return (out[0] | (out[1] << np.uint32(1))).astype(np.uint32)


# ---- k_block_bounds, k_block_vertices ------------------------------------------------------------------------------------
def block_sphere(lo, hi, centre_slack: bool = True) -> np.ndarray:
    """centre and radius from a block's box, in the order of k_block_bounds -> float32 [4].  `centre_slack=False`: the radius
    without the term for the centre's rounding, as it was before that term (the host tests show what it misses)."""
    with np.errstate(all="ignore"):
        c = (F32(0.5) * (lo + hi).astype(F32)).astype(F32)
        r2 = F32(0)
        for d in range(3):
            e = F32(0.5) * F32(hi[d] - lo[d])
            r2 = F32(r2 + F32(e * e))
        # the centre's own rounding: see k_block_bounds
        slack = F32(F32(F32(np.abs(c[0]) + np.abs(c[1])) + np.abs(c[2])) * F32(2.0 ** -23))
        r = F32(F32(F32(np.sqrt(r2)) * F32(1.0001)) + F32(1e-6))
        if centre_slack:
            r = F32(r + slack)
    return np.array([c[0], c[1], c[2], r], dtype=F32)


def upload_np(verts, faces, centre_slack: bool = True) -> dict:
    """What gr_mesh_upload leaves behind: orig (F,) int32, blk (B, 4) float32, bvert (B, 192, 3) float32 (NaN behind a
    block's count: unspecified in the library), bidx (F,) uint32, counts (B,), mesh_sig, and codes / axes / words for the
    anchoring tests."""
    v = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    F, V = f.shape[0], v.shape[0]
    words = mesh_bounds_words(v)
    codes = face_codes(v, f)
    orig = np.argsort(codes, kind="stable").astype(np.int32)
    B = (F + GR_BLOCK - 1) // GR_BLOCK
    blk = np.empty((B, 4), dtype=F32)
    bvert = np.full((B, GR_BLOCK_VERTS, 3), np.nan, dtype=F32)
    bidx = np.empty(F, dtype=np.uint32)
    counts = np.empty(B, dtype=np.int64)
    for b in range(B):
        members = orig[b * GR_BLOCK:(b + 1) * GR_BLOCK]
        corners = f[members].reshape(-1)                   # corner order: face by face, corner by corner
        soup = v[corners]
        blk[b] = block_sphere(fmin_all(soup, axis=0), fmax_all(soup, axis=0), centre_slack)
        number = {}
        local = np.empty(corners.shape[0], dtype=np.uint32)
        for k, g in enumerate(corners.tolist()):
            if g not in number:
                number[g] = len(number)
                bvert[b, number[g]] = v[g]
            local[k] = number[g]
        counts[b] = len(number)
        local = local.reshape(-1, 3)
        bidx[b * GR_BLOCK:b * GR_BLOCK + members.shape[0]] = (local[:, 0] | (local[:, 1] << np.uint32(8)) | (local[:, 2] << np.uint32(16))
                                                             | np.uint32((len(number) - 1) << 24))
    lo, ext = extents(words)
    return {"orig": orig, "blk": blk, "bvert": bvert, "bidx": bidx, "counts": counts, "mesh_sig": mesh_sig(F, V, words),
            "codes": codes, "axes": morton_axes(ext), "words": words}


# ---- k_cull_blocks ---------------------------------------------------------------------------------------------------
def cull_np(blk, cam16, h: int, w: int) -> np.ndarray:
    """keep (B,) bool: the five tests of k_cull_blocks term by term; any NaN keeps the block."""
    blk = np.asarray(blk, dtype=F32).reshape(-1, 4)
    cam = np.asarray(cam16, dtype=F32).reshape(16)
    with np.errstate(all="ignore"):
        dx, dy, dz = blk[:, 0] - cam[9], blk[:, 1] - cam[10], blk[:, 2] - cam[11]
        qx = (cam[0] * dx + cam[3] * dy) + cam[6] * dz
        qy = (cam[1] * dx + cam[4] * dy) + cam[7] * dz
        qz = (cam[2] * dx + cam[5] * dy) + cam[8] * dz
        fe, r = np.abs(cam[12]), blk[:, 3] * F32(1.001)
        mxl, mxr = cam[13] + F32(2), (F32(w) - cam[13]) + F32(2)
        myt, myb = cam[14] + F32(2), (F32(h) - cam[14]) + F32(2)
        out = qz + r < cam[15]
        out = out | (cam[12] * qx + mxl * qz < -r * (fe + np.abs(mxl)))
        out = out | (-cam[12] * qx + mxr * qz < -r * (fe + np.abs(mxr)))
        out = out | (cam[12] * qy + myt * qz < -r * (fe + np.abs(myt)))
        out = out | (-cam[12] * qy + myb * qz < -r * (fe + np.abs(myb)))
    for t in (qx, qy, qz, r):
        assert t.dtype == F32
    return ~out
