"""-m gpu: the learned binning table (csrc/geograster.hip: a ring of 8 entries per context, a ring of 64 per process, a cache file
that several processes rewrite).  Lessons are counted as tests/test_overflow_protocol.py::_lessons counts them; the ids of every
call are compared with the oracle's.  Every test starts from gr_learned_cache_clear() and ends as
test_second_context_and_new_process_start_sized ends: no cache file, an empty table.

The scenes: mesh B of tests/context_steps.py (1922 faces) moved by m / 8 along x -- another mesh signature per m, as the existing
test moves a mesh --, images of 64 k x 32, k = 1 .. 11 (k tiles), one far view each that puts the whole mesh into one or two
tiles: more than the 64 (or the default 512) slots a tile has."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))   # the stand-ins import one another by their plain names

import context_steps as steps  # noqa: E402

from geograypher_amd import _hip
from geograypher_amd._hip import HipRaster, load_library
from geograypher_amd.utils import synthetic
from oracle import oracle_c

pytestmark = pytest.mark.gpu

FAR = synthetic.nadir_pose(15.5, 15.5, 40.0, yaw_deg=10.0)      # f = 30: the mesh is 23 pixels wide
STRIP = synthetic.nadir_pose(15.5, 15.5, 110.0, yaw_deg=10.0)   # f = 600: a strip of the mesh over four of the ten tiles
EXACT = -1                                                        # a learned cap of -1: this (mesh, image size) bins exactly


def mesh(m):
    points, faces = steps._mesh(31)
    points = points.copy()
    points[:, 0] += 0.125 * m
    return points, faces


def view(m, k, pose=FAR, f=30.0):
    """(camera records (1, 16), h, w, the oracle's ids) of the view of mesh m at 64 k x 32"""
    w, h = 64 * k, 32
    recs = synthetic.camera_set_from_poses([pose], f, w, h).get_raster_records(1.0, near=0.05)
    points, faces = mesh(m)
    return recs, h, w, oracle_c.raster(points, faces, recs[0], h, w)


def lessons(ctx):
    return ctx.last_retries + ctx.last_stats["rebinned_groups"]


def raster(ctx, m, k, **kw):
    """One checked call; -> the lessons it took."""
    recs, h, w, want = view(m, k, **kw)
    ids = ctx.raster_face_ids(recs, h, w).cpu().numpy()
    assert np.array_equal(ids[0], want), (m, k)
    return lessons(ctx)


def context(m, cap=None, share=True):
    ctx = HipRaster(0)
    if cap is not None:
        ctx.set_option(_hip.GR_OPT_DIRECT_CAP, cap)      # (switches sharing off)
    ctx.set_option(_hip.GR_OPT_SHARE_LEARNED, 1 if share else 0)
    ctx.upload_mesh(*mesh(m))
    return ctx


def lessons_of_a_new_context(m, k, cap=None, **kw):
    ctx = context(m, cap=cap)
    try:
        return raster(ctx, m, k, **kw), dict(ctx.last_stats)
    finally:
        ctx.close()


def signature(m):
    ctx = context(m)
    try:
        return ctx.debug_upload()["mesh_sig"]
    finally:
        ctx.close()


def data_lines(path):
    return [line.split() for line in Path(path).read_text().splitlines() if line.strip() and not line.startswith("#")]


def keys_of(path):
    out = set()
    for fields in data_lines(path):
        assert len(fields) == 5, fields
        sig, (T, cap, full, micro) = int(fields[0], 16), (int(x) for x in fields[1:])
        assert T > 0 and (cap == EXACT or 0 < cap <= 65536) and full in (0, 1) and micro in (0, 1), fields
        out.add((sig, T))
    return out


@pytest.fixture()
def table(tmp_path):
    """An empty process-wide table and no cache file; `table(path)` points the library at one.  Left the same way."""
    lib = load_library()
    assert lib.gr_learned_cache_file(None) == 0 and lib.gr_learned_cache_clear() == 0

    def point_at(path):
        assert lib.gr_learned_cache_file(str(path).encode()) == 0

    point_at.clear = lambda: lib.gr_learned_cache_clear()
    try:
        yield point_at
    finally:
        lib.gr_learned_cache_file(None)
        lib.gr_learned_cache_clear()


def test_the_ring_of_8_of_a_context(table):
    """Sharing off, 64 slots per tile, ten image sizes (ten tile counts).  Ascending: a lesson each.  Descending: sizes 10 .. 3 are
    remembered; sizes 9 and 10 took the slots of sizes 1 and 2 ([n_learned % 8] is replaced next), which learn once more."""
    ctx = context(0, cap=64, share=False)
    try:
        assert [raster(ctx, 0, k) for k in range(1, 11)] == [1] * 10
        assert ctx.last_stats["max_entries"] > 64
        assert [raster(ctx, 0, k) for k in range(10, 0, -1)] == [0] * 8 + [1, 1]
    finally:
        ctx.close()


def test_the_ring_of_64_of_the_process_with_a_file(table, tmp_path):
    """66 (mesh, tile count) pairs, six meshes of eleven sizes, into a table of 64 with a cache file: a lesson survives its own save.
    (Before the fix of save_learned_locked the re-read of the file put the entry the 65th lesson had replaced back, which replaced
    the next one, whose line put it back in turn ... and the last line landed on the 65th lesson itself.)"""
    cache = tmp_path / "learned.txt"
    table(cache)
    pairs = [(m, k) for m in range(6) for k in range(1, 12)]
    assert len(pairs) == 66
    sigs = {}
    for m in range(6):
        ctx = context(m)
        try:
            sigs[m] = ctx.debug_upload()["mesh_sig"]
            for k in range(1, 12):
                assert raster(ctx, m, k) == 1, (m, k)
                n = 11 * m + k
                keys = keys_of(cache)
                assert len(data_lines(cache)) == min(n, 64), (m, k)
                assert (sigs[m], k) in keys, f"lesson {n} is not in the file it was saved to"
        finally:
            ctx.close()
    assert len(set(sigs.values())) == 6
    assert lessons_of_a_new_context(5, 11)[0] == 0                 # the 66th pair, from the table in memory
    assert lessons_of_a_new_context(5, 10)[0] == 0                 # the 65th
    assert lessons_of_a_new_context(0, 1)[0] == 1                  # the first: its slot was taken (and it takes the third's now)
    table.clear()
    table(cache)
    assert lessons_of_a_new_context(5, 11)[0] == 0                 # ... and from the file alone
    assert len(data_lines(cache)) <= 64


def test_the_file_as_input(table, tmp_path):
    """A hand-written file: what parse_learned_line takes and refuses, merge_cap for a key that comes twice, and the ring's rule for
    more lines than the table holds (the last 64 keys stay).  The contexts have 64 slots per tile of their own and share: what
    they use is the larger of 64 and the table's word.  Exact binning shows in `max_entries`, which is then a view's total and
    not a tile's: the far view at 512 x 32 has the mesh across the border of two tiles."""
    s0, s1 = signature(0), signature(1)
    big = 2048                                                     # slots enough for all 1922 faces in one tile
    strip = dict(pose=STRIP, f=600.0)
    probe = context(1, cap=4096, share=False)
    try:
        assert raster(probe, 1, 10, **strip) == 0
        need = probe.last_stats["max_entries"]                     # what the strip view needs
        raster(probe, 1, 8)                                        # (the far view's faces are micro faces: a lesson of its own)
        direct_far = probe.last_stats["max_entries"]
        probe.set_option(_hip.GR_OPT_DIRECT_CAP, 128)
        assert raster(probe, 1, 10, **strip) == 1                  # 128 slots alone are too few
        probe.set_option(_hip.GR_OPT_DIRECT_CAP, 0)
        assert raster(probe, 1, 10, **strip) == 0
        exact_strip = probe.last_stats["max_entries"]
        exact_far = {}
        for m in (1, 0):
            probe.upload_mesh(*mesh(m))
            raster(probe, m, 8)
            exact_far[m] = probe.last_stats["max_entries"]
    finally:
        probe.close()
    assert 128 < need <= 256 and exact_strip > need and min(exact_far.values()) > direct_far, (need, exact_strip, direct_far, exact_far)
    filler = [f"{0x1000 + i:016x} {1 + i % 7} 192 0 0" for i in range(70)]
    filler[0] = f"{s0:016x} 1 {big} 0 0"                           # the first of 75 keys: replaced while the file is read
    filler[69] = f"{s0:016x} 2 {big} 0 0"
    lines = ["# a comment"] + filler + [
        f"{s0:016x} 3 {big} 0",                                    # four fields: the format before 0.2.2
        f"{s0:016x} 4 {big} 0 0",
        "slots per tile: see the manual",
        f"{s0:016x} 0 {big} 0 0",                                  # T = 0
        f"{s0:016x} 5 65537 0 0",
        f"{s0:016x} 6 -2 0 0",
        f"{s0:016x} 8 -1 0 0",                                     # exact binning
        f"{s1:016x} 10 128 0 0", f"{s1:016x} 10 256 0 0",          # merge_cap: 256
        f"{s1:016x} 8 256 0 0", f"{s1:016x} 8 -1 0 0",             # merge_cap: exact
    ]
    cache = tmp_path / "written_by_hand.txt"
    cache.write_text("\n".join(lines) + "\n")
    table(cache)
    for k in (2, 3, 4):
        took, stats = lessons_of_a_new_context(0, k, cap=64)
        assert took == 0 and 64 < stats["max_entries"] <= big, k
    took, stats = lessons_of_a_new_context(1, 10, cap=64, **strip)
    assert took == 0 and stats["max_entries"] == need              # 256 slots: single-pass binning, nothing to learn
    for m in (0, 1):
        took, stats = lessons_of_a_new_context(m, 8, cap=64)
        assert took == 0 and stats["max_entries"] == exact_far[m], m
    for k in (1, 5, 6):                                            # replaced at the read, cap 65537, cap -2
        assert lessons_of_a_new_context(0, k, cap=64)[0] == 1, k
    assert keys_of(cache) >= {(s0, k) for k in (1, 2, 3, 4, 5, 6, 8)} | {(s1, 8), (s1, 10)}   # rewritten by the three lessons
    assert len(data_lines(cache)) == 64


def test_two_processes_one_file(table, tmp_path):
    """The parent learns pair 2, a fresh child process pair 1 into the same file, the parent pair 3: the file holds all three."""
    cache = tmp_path / "geograster_learned.txt"                    # where GEOGRAYPHER_AMD_CACHE=<dir> puts it
    table(cache)
    s0 = signature(0)
    ctx = context(0)
    try:
        assert raster(ctx, 0, 2) == 1
        assert keys_of(cache) == {(s0, 2)}
        child = (
            "import sys\n"
            f"sys.path.insert(0, {str(Path(__file__).resolve().parents[1])!r})\n"
            "from tests.test_learned_table_gpu import context, raster\n"
            "ctx = context(0)\n"
            "print('LESSONS', raster(ctx, 0, 1), raster(ctx, 0, 2))\n"
            "ctx.close()\n"
        )
        env = dict(os.environ, GEOGRAYPHER_AMD_CACHE=str(tmp_path))
        res = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        assert "LESSONS 1 0" in res.stdout, res.stdout               # pair 1 learned, pair 2 read from the file
        assert keys_of(cache) == {(s0, 1), (s0, 2)}
        assert raster(ctx, 0, 3) == 1
        assert keys_of(cache) == {(s0, 1), (s0, 2), (s0, 3)}
    finally:
        ctx.close()
    assert lessons_of_a_new_context(0, 1)[0] == 0                  # merged in from the file at the parent's save
