"""The kernels behind the rasterizer (project.hip) at the edges where kernels go wrong, against the numpy restatement of the
reference (oracle/oracle_np.py): id images and value arrays are the caller's, so they are drawn here -- fuzz-style id
images (piecewise-constant patches + noise, -1 background) over a mesh of F degenerate faces, no rasterizer involved.

Covered: k_winner's scalar load path (ids at a misaligned address) and widths around its 1024-column block; the 8-view
stride of the vote kernels and the 64-view launch groups (GR_MAX_BATCH) of the host loops; float sums that turn NaN at a
group's or a call's last view; byte-packed label votes filled to 64 per group and class counts up to 255; the uint8 cast of
the save_renders epilogue at its boundaries; class indices that do not fit an integer; the radix-sort pair count over all
64 key bits; and the argmax row sum in numpy's pairwise order, float32 included.  Every comparison is exact, NaN positions
and the sign of zero included."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_np

pytestmark = pytest.mark.gpu


# ---- helpers ------------------------------------------------------------------------------------------------------------
def _mesh(hip, F):
    hip.upload_mesh(np.zeros((3, 3), dtype=np.float32), np.zeros((F, 3), dtype=np.int32))


def _ids(rng, n, h, w, F):
    ids = np.empty((n, h, w), dtype=np.int32)
    for v in range(n):
        ph, pw = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        coarse = rng.integers(-1, F, size=((h + ph - 1) // ph, (w + pw - 1) // pw))
        img = np.kron(coarse, np.ones((ph, pw), dtype=np.int64))[:h, :w]
        noise = rng.random((h, w)) < 0.1
        img = np.where(noise, rng.integers(-1, F, size=(h, w)), img)
        img[rng.random((h, w)) < 0.2] = -1
        ids[v] = img
    return ids


def _same(got, want):
    """Bit for bit: the same NaN positions and the same bits everywhere else (-0.0 is not 0.0)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    bad = np.nonzero(got[keep].view(np.uint64) != want[keep].view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size} values differ, first: got {got[keep][bad[0]]!r}, want {want[keep][bad[0]]!r}"


def _misaligned(ids, device):
    """The same ids as a view at storage offset 1 of a larger tensor: 4 bytes past a 16-byte boundary."""
    big = torch.empty(ids.size + 4, dtype=torch.int32, device=device)
    t = big[1:1 + ids.size].view(ids.shape)
    t.copy_(torch.from_numpy(ids))
    assert t.data_ptr() % 16 == 4
    return t


def _one_hot(labels, C):
    return oracle_np.inds_to_one_hot(labels, C).astype(np.float64)


def _want_sums(projs, F):
    """aggregate (meshes.py:2044-2084) as the kernels implement it: the nansum of two or more views (one view: the
    projection with NaN channels of a seen face as 0, like the host mirror of a single view)."""
    if len(projs) > 1:
        with np.errstate(invalid="ignore", over="ignore"):
            avg, info = oracle_np.aggregate(projs, F)
        return avg, info["summed_projections"], info["projection_counts"].reshape(F)
    s = np.where(np.isnan(projs[0]), 0.0, projs[0])
    c = np.any(np.isfinite(projs[0]), axis=1).astype(np.float64)
    s[c == 0] = np.nan
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / c[:, None], s, c


def _index_oracle(ids, cls, F, nc, compat):
    """derived_meshes.py:470-520 as sorted (face * nc + class) keys with multiplicities, and the per-face counts."""
    counts = np.zeros(F, dtype=np.int64)
    keys = []
    for v in range(ids.shape[0]):
        p = oracle_np.project_image(ids[v].astype(np.int64), cls[v][..., None], F, neg1_is_last_face=compat)
        inds = np.nonzero(np.isfinite(p[:, 0]))[0]
        counts[inds] += 1
        c = p[inds, 0].astype(np.int64)
        assert c.size == 0 or (c.min() >= 0 and c.max() < nc)
        keys.append(inds.astype(np.int64) * nc + c)
    uniq, mult = np.unique(np.concatenate(keys), return_counts=True)
    if nc * F <= 10_000_000 and F > 1:  # the dense restatement agrees (a one-face mesh is an error in the reference)
        projs = [oracle_np.project_image(ids[v].astype(np.int64), cls[v][..., None], F, neg1_is_last_face=compat)
                 for v in range(ids.shape[0])]
        _, dc, ds = oracle_np.aggregate_index_sparse(projs, F, nc)
        dense = np.zeros(F * nc, dtype=np.int64)
        dense[uniq] = mult
        assert np.array_equal(dense.reshape(F, nc), ds) and np.array_equal(dc[:, 0], counts)
    return counts, uniq, mult


# ---- winners: shapes, face counts, alignment, compat --------------------------------------------------------------------
SHAPES = [(1, 1), (1, 5), (17, 1), (15, 1023), (16, 1024), (33, 1025), (3, 4099)]


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("F", [1, 2, 255, 256, 257, 4097])
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_winners_at_edge_shapes(hip, hw, F, compat):
    h, w = hw
    rng = np.random.default_rng(h * 100003 + w * 31 + F * 7 + compat)
    n = 2
    _mesh(hip, F)
    ids = _ids(rng, n, h, w, F)
    # a face whose only pixel is pixel 0 (key 1), and one whose last pixel is (h-1, w-1) (key = P) in every view
    a, b = 0, F // 2
    for v in range(n):
        if F > 1:
            ids[v][ids[v] == a] = b
        ids[v, 0, 0] = a
        ids[v, -1, -1] = b
    C = 3
    img = rng.normal(0, 1, (n, h, w, C)) * 10.0 ** rng.integers(-3, 4, (n, h, w, C))
    img[rng.random((n, h, w, C)) < 0.05] = np.nan
    img[rng.random((n, h, w, C)) < 0.02] = -0.0
    projs = [oracle_np.project_image(ids[v].astype(np.int64), img[v], F, neg1_is_last_face=compat) for v in range(n)]
    if F > 1 and h * w > 1:
        assert np.array_equal(projs[0][a], img[0, 0, 0], equal_nan=True)
    assert np.array_equal(projs[0][b], img[0, -1, -1], equal_nan=True)
    labels = rng.integers(0, 6, (n, h, w)).astype(np.uint8)
    labels[rng.random((n, h, w)) < 0.05] = 255
    cls = rng.integers(0, 7, (n, h, w)).astype(np.float64)
    cls[rng.random((n, h, w)) < 0.3] = np.nan
    want_avg, want_sum, want_cnt = _want_sums(projs, F)
    lab_projs = [oracle_np.project_image(ids[v].astype(np.int64), _one_hot(labels[v], 4), F, neg1_is_last_face=compat)
                 for v in range(n)]
    want_lavg, want_lsum, want_lcnt = _want_sums(lab_projs, F)
    want_pc, want_keys, want_mult = _index_oracle(ids, cls, F, 7, compat)
    results = []
    for ids_in in (torch.from_numpy(ids).to(hip.device), _misaligned(ids, hip.device)):
        for v in range(n):
            _same(hip.project_view(ids_in[v], img[v], neg1_is_last_face=compat).cpu().numpy(), projs[v])
        sums = torch.zeros((F, C), dtype=torch.float64, device=hip.device)
        cnt = torch.zeros((F,), dtype=torch.int32, device=hip.device)
        hip.project_values(ids_in, img, sums, cnt, neg1_is_last_face=compat)
        avg, summed, counts = (t.cpu().numpy() for t in hip.finalize_sums(sums, cnt))
        _same(summed, want_sum)
        _same(avg, want_avg)
        _same(counts, want_cnt)
        votes, vc = hip.new_vote_buffers(4)
        hip.project_labels(ids_in, labels, 4, votes, vc, neg1_is_last_face=compat)
        lavg, lsum, lcnt = (t.cpu().numpy() for t in hip.finalize_votes(votes, vc))
        _same(lsum, want_lsum)
        _same(lavg, want_lavg)
        _same(lcnt, want_lcnt)
        pc = torch.zeros((F,), dtype=torch.int32, device=hip.device)
        keys, mult = hip.project_index_pairs(ids_in, cls, 7, pc, neg1_is_last_face=compat)
        assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult)
        assert np.array_equal(pc.cpu().numpy(), want_pc)
        results.append((summed, lsum, keys))
    # aligned (16-byte id loads) and misaligned (scalar loads) agree with each other as well
    for x, y in zip(*results):
        assert np.array_equal(x, y, equal_nan=True)


# ---- views per call: the 8-view stride and the 64-view launch groups ----------------------------------------------------
VIEWS = [1, 7, 8, 9, 63, 64, 65, 130]


@pytest.mark.parametrize("n", VIEWS)
def test_views_per_call(hip, n):
    rng = np.random.default_rng(5000 + n)
    F, h, w, C = 300, 9, 13, 2
    _mesh(hip, F)
    ids = _ids(rng, n, h, w, F)
    ids[:, 0, 0] = 0  # face 0: seen in every view, at pixel 0
    ids[:, 1:][ids[:, 1:] == 0] = 1
    ids[:, 0, 1:][ids[:, 0, 1:] == 0] = 1
    img = rng.normal(0, 1, (n, h, w, C))
    img[rng.random((n, h, w, C)) < 0.1] = np.nan
    projs = [oracle_np.project_image(ids[v].astype(np.int64), img[v], F) for v in range(n)]
    want_avg, want_sum, want_cnt = _want_sums(projs, F)
    sums = torch.zeros((F, C), dtype=torch.float64, device=hip.device)
    cnt = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    hip.project_values(ids, img, sums, cnt)
    avg, summed, counts = (t.cpu().numpy() for t in hip.finalize_sums(sums, cnt))
    _same(summed, want_sum)
    _same(avg, want_avg)
    _same(counts, want_cnt)
    labels = rng.integers(0, 5, (n, h, w)).astype(np.uint8)
    lab_projs = [oracle_np.project_image(ids[v].astype(np.int64), _one_hot(labels[v], 4), F) for v in range(n)]
    want_lavg, want_lsum, want_lcnt = _want_sums(lab_projs, F)
    votes, vc = hip.new_vote_buffers(4)
    hip.project_labels(ids, labels, 4, votes, vc)
    lavg, lsum, lcnt = (t.cpu().numpy() for t in hip.finalize_votes(votes, vc))
    _same(lsum, want_lsum)
    _same(lavg, want_lavg)
    _same(lcnt, want_lcnt)
    assert lcnt[0] == n
    cls = rng.integers(0, 5, (n, h, w)).astype(np.float64)
    cls[rng.random((n, h, w)) < 0.2] = np.nan
    want_pc, want_keys, want_mult = _index_oracle(ids, cls, F, 5, True)
    pc = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    keys, mult = hip.project_index_pairs(ids, cls, 5, pc)
    assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult)
    assert np.array_equal(pc.cpu().numpy(), want_pc)


# ---- float sums: NaN, infinities, -0.0, subnormals, overflow; NaN made at group and call boundaries ---------------------
NAN_AT = [7, 63, 64, 127, 128, 129]  # 63: last view of the first launch group, 129: last view of the call


@pytest.mark.parametrize("calls", [1, 2, 3])
@pytest.mark.parametrize("C", [1, 2, 7, 33])
def test_float_sums_special_values(hip, C, calls):
    rng = np.random.default_rng(100 * C + calls)
    n, F, h, w = 130, 64, 6, 20
    S = 3 * len(NAN_AT)  # scripted faces 0..S-1: pixel (0, j) of a view shows face j when the script says so
    _mesh(hip, F)
    ids = rng.integers(S, F, (n, h, w)).astype(np.int32)
    ids[rng.random((n, h, w)) < 0.2] = -1
    ids[:, 0, :S] = -1  # background aliases face F - 1 (not scripted)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, 2.2250738585072014e-308 / 3, 1e308, -1e308])
    img = rng.normal(0, 1, (n, h, w, C))
    pick = rng.random((n, h, w, C)) < 0.15
    img[pick] = rng.choice(specials, int(pick.sum()))
    ids[0, 1, :S] = np.arange(S)  # every scripted face has a finite observation: it counts, its sum is not reset to NaN
    img[0, 1, :S] = 1.0
    for k, t in enumerate(NAN_AT):
        j = 3 * k
        # face j: +inf at view t - 1, -inf at view t -> the running sum turns NaN at view t
        ids[t - 1, 0, j] = ids[t, 0, j] = j
        img[t - 1, 0, j] = np.inf
        img[t, 0, j] = -np.inf
        # face j + 1: 1e308 + 1e308 overflows to +inf (views t - 2, t - 1), -inf at view t
        ids[t - 2, 0, j + 1] = ids[t - 1, 0, j + 1] = ids[t, 0, j + 1] = j + 1
        img[t - 2, 0, j + 1] = img[t - 1, 0, j + 1] = 1e308
        img[t, 0, j + 1] = -np.inf
        # face j + 2: NaN at view t, seen again later (if there is a later view) with a subnormal
        ids[t, 0, j + 2] = j + 2
        img[t, 0, j + 2] = np.nan
        if t + 1 < n:
            ids[t + 1, 0, j + 2] = j + 2
            img[t + 1, 0, j + 2] = 5e-324
    projs = [oracle_np.project_image(ids[v].astype(np.int64), img[v], F) for v in range(n)]
    want_avg, want_sum, want_cnt = _want_sums(projs, F)
    assert np.isnan(want_sum[3 * NAN_AT.index(129), 0]) and np.isnan(want_sum[3 * NAN_AT.index(129) + 1, 0])
    assert not np.isnan(want_sum[3 * NAN_AT.index(63), 0])
    sums = torch.zeros((F, C), dtype=torch.float64, device=hip.device)
    cnt = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    bounds = np.linspace(0, n, calls + 1).astype(int)
    for v0, v1 in zip(bounds[:-1], bounds[1:]):
        hip.project_values(ids[v0:v1], img[v0:v1], sums, cnt)
    avg, summed, counts = (t.cpu().numpy() for t in hip.finalize_sums(sums, cnt))
    _same(summed, want_sum)
    _same(avg, want_avg)
    _same(counts, want_cnt)


# ---- label votes: class counts up to 255, labels >= C, the byte-packed accumulator filled to 64 -------------------------
@pytest.mark.parametrize("C", [1, 2, 15, 16, 17, 254, 255])
def test_label_votes_class_counts(hip, C):
    rng = np.random.default_rng(700 + C)
    n, F, h, w = 130, 50, 5, 8
    _mesh(hip, F)
    ids = _ids(rng, n, h, w, F)
    ids[:, 0, 0] = 0  # face 0 wins pixel 0 of every view with the same label: 64 votes per launch group in one byte
    ids[:, 1:][ids[:, 1:] == 0] = 1
    ids[:, 0, 1:][ids[:, 0, 1:] == 0] = 1
    labels = rng.integers(0, min(C + 3, 256), (n, h, w)).astype(np.uint8)
    labels[rng.random((n, h, w)) < 0.1] = 255
    labels[:, 0, 0] = C - 1
    lab_projs = (oracle_np.project_image(ids[v].astype(np.int64), _one_hot(labels[v], C), F) for v in range(n))
    with np.errstate(invalid="ignore"):
        want_avg, info = oracle_np.aggregate(lab_projs, F)
    votes, vc = hip.new_vote_buffers(C)
    hip.project_labels(ids, labels, C, votes, vc)
    avg, summed, cnt = (t.cpu().numpy() for t in hip.finalize_votes(votes, vc))
    _same(summed, info["summed_projections"])
    _same(avg, want_avg)
    _same(cnt, info["projection_counts"])
    assert summed[0, C - 1] == n


# ---- gathers: the uint8 cast at its boundaries ---------------------------------------------------------------------------
TEX_VALUES = [0.0, -0.0, 5e-324, -5e-324, 254.99999999999997, 255.0, np.nextafter(255.0, np.inf), 255.5, 256.0, -1.0,
              np.nan, np.inf, -np.inf, 1e300]


@pytest.mark.parametrize("null_value", [0, 7, 255])
@pytest.mark.parametrize("C", [1, 3, 5])
def test_gathers_at_uint8_boundaries(hip, C, null_value):
    rng = np.random.default_rng(C * 10 + null_value)
    F = 3 * len(TEX_VALUES)
    tex = np.array(TEX_VALUES * ((F * C) // len(TEX_VALUES) + 1))[:F * C]
    tex = tex[rng.permutation(F * C)].reshape(F, C)
    tex[0] = TEX_VALUES[:C]
    ids = rng.integers(-1, F, (7, 37)).astype(np.int32)  # 259 pixels: not a multiple of the 256-thread block
    ids.reshape(-1)[:F] = np.arange(F)
    want = oracle_np.render_flat_gather(ids.astype(np.int64), tex)
    _same(hip.gather_texture(ids, tex).cpu().numpy(), want)
    want_u8 = oracle_np.render_postprocess_uint8(want, null_value=null_value)
    got_u8 = hip.gather_texture_u8(ids, tex, null_value=null_value).cpu().numpy()
    assert got_u8.dtype == np.uint8
    np.testing.assert_array_equal(got_u8, want_u8.reshape(got_u8.shape))


# ---- index pairs: class values at and beyond the integer range -----------------------------------------------------------
NCLASSES = [1, 7, 2 ** 33 + 1]


def _valid_values(nc):
    return [-0.999, -0.0, 0.0, float(nc - 1), float(nc - 1) + 0.999]


def _invalid_values(nc):
    return [-1.0, float(nc), 2.0 ** 53, 2.0 ** 63, 1e300, -1e300, -(2.0 ** 63)]


def _pair_scene(rng, F, nc, values):
    n, h, w = 2, 6, 11
    ids = _ids(rng, n, h, w, F)
    cls = rng.integers(0, min(nc, 1000), (n, h, w)).astype(np.float64)
    cls[rng.random((n, h, w)) < 0.2] = np.nan
    # the given values at the winning (last) pixels of faces 1..len(values) in view 1
    for k, x in enumerate(values):
        ids[1][ids[1] == k + 1] = -1
        ids[1, -1, -1 - k] = k + 1
        cls[1, -1, -1 - k] = x
    return ids, cls


@pytest.mark.parametrize("nc", NCLASSES)
def test_index_pairs_valid_edges(hip, nc):
    rng = np.random.default_rng(nc % 1000)
    F = 40
    _mesh(hip, F)
    ids, cls = _pair_scene(rng, F, nc, _valid_values(nc))
    # an invalid value at a pixel that does NOT win its face is no observation: no error
    ids[1, 0, 0] = ids[1, 0, 1] = F - 2
    cls[1, 0, 0] = 1e300
    for compat in (True, False):
        want_pc, want_keys, want_mult = _index_oracle(ids, cls, F, nc, compat)
        pc = torch.zeros((F,), dtype=torch.int32, device=hip.device)
        keys, mult = hip.project_index_pairs(ids, cls, nc, pc, neg1_is_last_face=compat)
        assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult)
        assert np.array_equal(pc.cpu().numpy(), want_pc)
        acc_pc = torch.zeros((F,), dtype=torch.int32, device=hip.device)
        acc = hip.new_pair_accumulator(nc, acc_pc, neg1_is_last_face=compat)
        acc.add(ids[:1], cls[:1])
        acc.add(ids[1:], cls[1:])
        keys, mult = acc.finish()
        assert np.array_equal(keys, want_keys) and np.array_equal(mult, want_mult)
        assert np.array_equal(acc_pc.cpu().numpy(), want_pc)


@pytest.mark.parametrize("nc", NCLASSES)
@pytest.mark.parametrize("k", range(7))
def test_index_pairs_invalid_value_raises(hip, nc, k):
    x = _invalid_values(nc)[k]
    rng = np.random.default_rng(k)
    F = 40
    _mesh(hip, F)
    ids, cls = _pair_scene(rng, F, nc, [x])
    pc = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    with pytest.raises(IndexError):
        hip.project_index_pairs(ids, cls, nc, pc)
    acc = hip.new_pair_accumulator(nc, torch.zeros((F,), dtype=torch.int32, device=hip.device))
    acc.add(ids, cls)
    with pytest.raises(IndexError):
        acc.finish()


def test_index_pairs_class_count_limit(hip):
    """n_classes up to 2^53 compares exactly in double (2^53 - 1 is a class, 2^53 is not); above it is refused."""
    F = 5
    _mesh(hip, F)
    ids = np.array([[[0, 1, 2, -1]]], dtype=np.int32)
    nc = 2 ** 53
    pc = torch.zeros((F,), dtype=torch.int32, device=hip.device)
    keys, mult = hip.project_index_pairs(ids, np.array([[[nc - 1.0, 0.0, np.nan, np.nan]]]), nc, pc,
                                         neg1_is_last_face=False)
    assert keys.tolist() == [nc - 1, nc] and mult.tolist() == [1, 1]
    with pytest.raises(IndexError):
        hip.project_index_pairs(ids, np.array([[[float(nc), 0.0, np.nan, np.nan]]]), nc, pc, neg1_is_last_face=False)
    with pytest.raises(ValueError):
        hip.project_index_pairs(ids, np.zeros((1, 1, 4)), nc + 1, pc)


# ---- gr_count_pairs: keys over all 64 bits ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65537, 2 ** 21 + 3])
def test_count_pairs_full_key_range(hip, n):
    rng = np.random.default_rng(n)
    pool = np.concatenate([np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64),
                           rng.integers(0, 2 ** 64 - 1, max(1, n // 16), dtype=np.uint64, endpoint=True)])
    keys = pool[rng.integers(0, pool.size, n)]
    keys[: min(n, 5)] = pool[: min(n, 5)]
    keys_t = torch.from_numpy(keys.view(np.int64).copy()).to(hip.device)
    uniq = torch.empty((n,), dtype=torch.int64, device=hip.device)
    mult = torch.empty((n,), dtype=torch.int32, device=hip.device)
    n_unique = ctypes.c_int64(-1)
    with torch.cuda.device(hip.device):  # as PairAccumulator._compact calls it
        rc = hip.lib.gr_count_pairs(hip._ctx, keys_t.data_ptr(), n, uniq.data_ptr(), mult.data_ptr(), ctypes.byref(n_unique),
                                    hip._stream())
    hip._check(rc, "gr_count_pairs")
    want_keys, want_mult = np.unique(keys, return_counts=True)
    k = int(n_unique.value)
    assert k == want_keys.size
    assert np.array_equal(uniq[:k].cpu().numpy().view(np.uint64), want_keys)
    assert np.array_equal(mult[:k].cpu().numpy().view(np.uint32), want_mult)
    assert np.array_equal(keys_t.cpu().numpy().view(np.uint64), keys)  # the caller's keys are left as they were


# ---- argmax: numpy's row sum, first maximum, first NaN ------------------------------------------------------------------
ARGMAX_C = [1, 2, 7, 8, 9, 16, 17, 127, 128, 129, 136, 255, 256, 257, 1000]
ROW_ZERO_IN_NUMPY = [0.2, 0.3, -0.1, -0.3, 0.3, -0.3, -0.3, 0.2]     # numpy: 0 -> NaN (left to right: 5.55e-17 -> 1)
ROW_NONZERO_IN_NUMPY = [-0.2, -0.1, -0.2, 0.3, 1.0, -0.3, -0.3, -0.2]  # numpy: -1.1e-16 -> 4 (left to right: 0 -> NaN)


def _argmax_rows(rng, C, F):
    a = rng.integers(-3, 4, (F, C)) * 0.1  # mixed signs that cancel
    k = 0

    def put(row):
        nonlocal k
        a[k] = row
        k += 1

    put(np.zeros(C))
    put(np.full(C, -0.0))
    for pos in (0, C // 2, C - 1):
        r = a[k].copy(); r[pos] = np.nan; put(r)
        r = a[k].copy(); r[pos] = np.inf; put(r)
        r = a[k].copy(); r[pos] = -np.inf; put(r)
    r = np.full(C, 2.0); r[C // 3] = 5.0; r[C - 1] = 5.0; put(r)  # ties: the first maximum
    r = -np.arange(1.0, C + 1); put(r)
    r = np.zeros(C); r[C - 1] = 1e-300; put(r)
    if C > 1:
        r = np.zeros(C); r[0] = np.nan; r[1] = np.inf; put(r)      # NaN first
        r = np.ones(C); r[-1] = np.nan; r[0] = 9.0; put(r)         # NaN later
    if C >= 8:
        r = np.zeros(C); r[:8] = ROW_ZERO_IN_NUMPY; put(r)
        r = np.zeros(C); r[:8] = ROW_NONZERO_IN_NUMPY; put(r)
        r = np.zeros(C); r[C - 8:] = ROW_ZERO_IN_NUMPY; put(r)
    return a


def _argmax_check(hip, a):
    a_np = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    want = np.asarray(oracle_np.find_argmax_nonzero_value(a_np)).reshape(a.shape[0])
    got = hip.argmax_nonzero(a)
    assert got.dtype == torch.float64
    _same(got.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("C", ARGMAX_C)
def test_argmax_float64(hip, C):
    rng = np.random.default_rng(C)
    a = _argmax_rows(rng, C, 300)  # 300 rows: not a multiple of the 256-thread block
    _argmax_check(hip, a)
    _argmax_check(hip, np.empty((0, C)))  # F = 0: an empty result, as numpy gives


def test_argmax_named_rows(hip):
    a = np.array([ROW_ZERO_IN_NUMPY, ROW_NONZERO_IN_NUMPY])
    got = hip.argmax_nonzero(a).cpu().numpy()
    assert np.isnan(got[0]) and got[1] == 4.0


@pytest.mark.parametrize("C", ARGMAX_C)
def test_argmax_float32(hip, C):
    rng = np.random.default_rng(10_000 + C)
    a = _argmax_rows(rng, C, 300).astype(np.float32)
    f = rng.normal(0, 1, (200, C)).astype(np.float32) * np.float32(10.0) ** rng.integers(-4, 9, (200, 1)).astype(np.float32)
    a = np.concatenate([a, f, -f[:, ::-1]])
    if C >= 3:
        r = np.zeros(C, dtype=np.float32); r[:3] = (1e8, 1.0, -1e8)  # float32: 0 -> NaN (float64: 1 -> 0)
        a = np.concatenate([a, r[None]])
    _argmax_check(hip, a)
    _argmax_check(hip, torch.from_numpy(a).to(hip.device))
    if C >= 3:
        assert np.isnan(hip.argmax_nonzero(a[-1:]).cpu().numpy()[0])


@pytest.mark.parametrize("dtype", [np.int32, np.uint32])
@pytest.mark.parametrize("C", [1, 8, 9, 129, 1000])
def test_argmax_integer_votes(hip, C, dtype):
    rng = np.random.default_rng(C + (dtype == np.uint32))
    if dtype == np.int32:
        a = rng.integers(-3, 4, (300, C)).astype(np.int32)
        a[:, 0] = np.int32(2 ** 31 - 1)
        a[:150, -1] = np.int32(-(2 ** 31))
    else:
        a = rng.integers(0, 4, (300, C)).astype(np.uint32)
        a[rng.random(300) < 0.3] = 0
        a[::7, C // 2] = np.uint32(2 ** 32 - 1)
    a[-1] = 0
    _argmax_check(hip, a)
