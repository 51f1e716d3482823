"""bench.run's DISTRIBUTED control flow, end to end, before the first real multi-GPU run: two gloo ranks on the CPU drive
the very function the driver launches -- every `all_reduce` call site (ranks_seen, the MAX-over-ranks reductions of the
timed windows, the packed vote reduce of the aggregate / c4 / c5 legs), the barriers, the rank-0-only JSON line, the exit
code of a line that would claim more GPUs than answered -- with a stand-in for the HIP backend (the CPU oracle dressed as
`HipRaster`, tests/oracle_backend.py) and a toy workload.  What it cannot cover is RCCL itself.  The legs run with
`--full`; the plain run (headline window only, `--dump-outputs`) is checked on its own."""
import io
import json
import os
import socket
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.oracle_backend import OracleBackend


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _BenchStub(OracleBackend):
    """OracleBackend + the bookkeeping surface bench.py reads: profiling spans, status, retry counters."""

    def __init__(self):
        super().__init__()
        self.unchecked_calls = 0   # steps: raster calls with check=False
        self.last_retries = 0
        self.last_stats = {}
        self._prof = None

    def set_profiling(self, enabled):
        self._prof = dict(setup_ms=0.0, scan_ms=0.0, fill_ms=0.0, raster_ms=0.0, project_ms=0.0, vote_ms=0.0, gather_ms=0.0,
                          raster_launches=0, views=0) if enabled else None

    def stage_times(self):
        out = dict(self._prof)
        self.set_profiling(True)
        return out

    def _note(self, n_views, seconds, fused=False):
        self.last_stats = {"records": 10 * n_views, "entries": 20 * n_views, "max_entries": 5, "entry_cap": 512, "overflow": 0,
                           "views_done": n_views}
        if self._prof is not None:
            self._prof["setup_ms"] += 250.0 * seconds
            self._prof["raster_ms"] += 700.0 * seconds
            self._prof["vote_ms"] += 50.0 * seconds if fused else 0.0
            self._prof["raster_launches"] += 1
            self._prof["views"] += n_views

    def raster_face_ids(self, cams, h, w, out=None, want_depth=False, check=True):
        t0 = time.perf_counter()
        ids = super().raster_face_ids(np.asarray(cams), h, w)
        if out is not None:
            out.copy_(ids)
        self._note(ids.shape[0], time.perf_counter() - t0)
        if not check:
            self.unchecked_calls += 1
            self.last_stats = {"unchecked": True}
        return out if out is not None else ids

    def raster_project_labels(self, cams, labels, C, votes, counts, ids_out=None, neg1_is_last_face=True, check=True):
        t0 = time.perf_counter()
        super().raster_project_labels(np.asarray(cams), np.asarray(labels), C, votes, counts, neg1_is_last_face=neg1_is_last_face)
        self._note(int(np.asarray(cams).shape[0]), time.perf_counter() - t0, fused=True)

    def raster_status(self):
        return {"records": 10, "entries": 20, "max_entries": 5, "entry_cap": 512, "overflow": 0, "views_done": 1}


class _StubRig:
    dist_backend = "gloo"
    overrides = {}
    backends = []

    def __init__(self):
        import bench

        kw = dict(n_side=24, extent=400.0, H=48, W=64, f=48.0, views_per_rank=3, c3_views=6, c4_views_per_rank=4, n_classes=4,
                  c5_n_side=30, c5_extent=800.0, c5_H=40, c5_W=60, c5_f=45.0, c5_views_total=8, c5_views_per_rank=4,
                  c5_classes=10, c5_raster_views=2, min_leg_s=0.0, precondition_s=0.0)
        kw.update(self.overrides)
        self.workload = bench.Workload(**kw)

    def device(self, local_rank):
        return torch.device("cpu")

    def init_process_group(self, dev):
        dist.init_process_group(self.dist_backend)

    def synchronize(self, dev):
        pass

    def make_raster(self, local_rank):
        self.backends.append(_BenchStub())
        return self.backends[-1]

    def checker(self):
        from oracle import oracle_c

        return oracle_c

    def side_legs(self):
        return False


FULL = ["--steps", "2", "--warmup", "1", "--windows", "2", "--min-timed-s", "0", "--full"]


def _rank(rank, world, port, out_dir, gpus_flag, overrides=None, flags=FULL):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    sys.modules.pop("bench", None)
    import bench

    _StubRig.overrides = dict(overrides or {})

    args = bench.parse_args(["--gpus", str(gpus_flag), *flags])
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = bench.run(args, _StubRig())
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as fh:
        json.dump({"rc": rc, "stdout": buf.getvalue(), "unchecked_calls": [b.unchecked_calls for b in _StubRig.backends]}, fh)


def _run(tmp_path, world, gpus_flag, overrides=None, flags=FULL):
    mp.spawn(_rank, args=(world, _free_port(), str(tmp_path), gpus_flag, overrides, flags), nprocs=world, join=True)
    return [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]


@pytest.mark.timeout(600)
def test_two_ranks_run_the_whole_bench_and_rank0_prints_one_line(tmp_path):
    res = _run(tmp_path, 2, 2)
    assert [r["rc"] for r in res] == [0, 0]
    assert res[1]["stdout"].strip() == ""                      # only rank 0 speaks
    lines = [l for l in res[0]["stdout"].splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["scaling"] == "weak" and line["steps"] == 2
    assert line["ms_per_step_windows"]["n"] == 2 and line["timed_gpu_s"] > 0 and line["value"] > 0
    assert line["config"]["parallelism"].endswith("dp2") and line["config"]["views_per_gpu_per_step"] == 3
    # whole-job aggregate: both ranks' views in the numerator
    assert abs(line["views_per_s"] - 2 * 3 * 2 / (line["ms_per_step"] * 2e-3)) / line["views_per_s"] < 1e-3
    for key in ("roofline", "rooflines", "aggregate", "c4", "c5"):
        assert line[key] is not None, key
    assert line["cpu_baseline"] is None and line["workload_2"] is None and line["api"] is None  # N == 1 legs
    F = line["config"]["faces"]
    assert line["c4"]["all_reduce_bytes"] == F * 5 * 4 and line["c4"]["views_per_gpu"] == 4
    ring = line["c4"]["all_reduce_algorithmic_ms"]
    assert ring["bytes_on_the_wire_per_gpu"] == F * 5 * 4  # 2 (N - 1) / N = 1 at N = 2
    assert line["c4"]["face_observations_after_reduce"] > 0 and line["aggregate"]["faces_observed"] > 0
    assert line["c5"]["views_per_gpu"] == 4 and line["c5"]["all_reduce_bytes"] > 0
    assert set(line["rooflines"]) == {"k_setup_cull", "k_raster_tile_fused", "k_vote_labels"}
    for r in [line["roofline"], *line["rooflines"].values()]:
        assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["frac"] == pytest.approx(r["achieved"] / r["peak"], abs=1e-4)


@pytest.mark.timeout(600)
def test_one_rank_equals_the_sum_of_its_views(tmp_path):
    """World size 1 through the same entry point: the all-reduce sites are no-ops, the observation counts of the sharded run
    above can only be larger (twice the views)."""
    res = _run(tmp_path, 1, 1)
    assert res[0]["rc"] == 0
    line = json.loads(res[0]["stdout"].strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["ranks_seen"] == 1 and line["c4"]["all_reduce_algorithmic_ms"]["bytes_on_the_wire_per_gpu"] == 0
    assert line["cpu_baseline"] is not None and line["cpu_baseline"]["kind"] == "port"   # the CPU leg runs at N == 1
    assert "equal the CPU oracle's: True" in line["aggregate"]["oracle_check"]


@pytest.mark.timeout(600)
def test_a_line_that_claims_more_gpus_than_answered_is_refused(tmp_path):
    res = _run(tmp_path, 2, 3)
    assert [r["rc"] for r in res] == [3, 3] and all(r["stdout"].strip() == "" for r in res)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [2, 3])
def test_a_rank_without_views_still_joins_every_collective(tmp_path, world):
    """Fewer views than ranks in the c4 and c5 legs (one view each): the ranks whose shard is empty must still walk through
    every barrier, every MAX reduction and the packed vote reduce -- a rank that skipped one would hang the job (here: the
    test would time out) -- and the reduced votes are those of the one view."""
    res = _run(tmp_path, world, world, overrides=dict(c4_views_total=1, c5_views_total=1))
    assert [r["rc"] for r in res] == [0] * world
    line = json.loads(res[0]["stdout"].strip().splitlines()[-1])
    assert line["n_gpus"] == world and line["ranks_seen"] == world
    assert [r["rank"] for r in line["ranks"]] == list(range(world))        # the rank -> device map of the line
    assert line["c4"]["views_per_gpu"] == 1 and line["c5"]["views_per_gpu"] == 1      # rank 0 holds the one view
    assert line["c4"]["face_observations_after_reduce"] > 0 and line["c5"]["face_observations_after_reduce"] > 0
    assert line["c4"]["reps"] >= 3 and line["c5"]["aggregate_reps"] >= 2


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [1, 2])
def test_a_plain_run_times_exactly_its_steps_and_nothing_else(tmp_path, world):
    """Without --full: set-up, warm-up, ONE window of exactly --steps steps and the headline line -- no profiled windows, no
    roofline, no side leg, no CPU baseline."""
    import bench

    res = _run(tmp_path, world, world, flags=["--steps", "5", "--warmup", "2"])
    assert [r["rc"] for r in res] == [0] * world
    assert all(r["unchecked_calls"] == [bench.PRECONDITION_STEPS + 2 + 5] for r in res)
    assert all(r["stdout"].strip() == "" for r in res[1:])
    lines = [l for l in res[0]["stdout"].splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
    assert line["steps"] == 5 and line["warmup"] == 2 and line["n_gpus"] == world and line["value"] > 0
    assert line["unit"] == "Mpix/s" and line["higher_is_better"] is True
    for key in ("ms_per_step_windows", "timed_gpu_s", "roofline", "rooflines", "cpu_baseline", "aggregate", "c4", "c5",
                "workload_2", "workload_3", "quarter_scale", "api", "io"):
        assert key not in line, key
    assert abs(line["views_per_s"] - world * 3 * 5 / (line["ms_per_step"] * 5e-3)) / line["views_per_s"] < 1e-3


@pytest.mark.timeout(600)
def test_dump_outputs_holds_the_last_step_and_repeats_from_run_to_run(tmp_path):
    """--dump-outputs DIR: the ids of the last timed step (small enough here to be written whole) as float32, the same in two
    runs with the same arguments, and equal to the CPU oracle's ids of the same views."""
    from geograypher_amd.utils import synthetic
    from oracle import oracle_c

    dumps = []
    for k in range(2):
        out = tmp_path / f"out{k}"
        res = _run(tmp_path, 1, 1, flags=["--steps", "3", "--warmup", "0", "--dump-outputs", str(out)])
        assert res[0]["rc"] == 0
        assert sorted(p.name for p in out.iterdir()) == ["face_ids.npy"]
        dumps.append(np.load(out / "face_ids.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (3, 48, 64)
    assert np.array_equal(dumps[0], dumps[1])
    points, faces = synthetic.terrain_mesh(24, 400.0)
    recs = synthetic.survey_cameras(10, 5, 40.0, 60.0, seed=3, f=48.0, width=64, height=48).get_raster_records(1.0, near=1.0)[:3]
    want, _ = oracle_c.raster_views(points, faces, recs, 48, 64, n_threads=1)
    assert np.array_equal(dumps[0], want.astype(np.float32)) and (want >= 0).any()


def test_dump_outputs_samples_a_large_output_at_fixed_positions(tmp_path, monkeypatch):
    """Above DUMP_SAMPLES elements the ids are sampled at seeded, distinct, ascending positions whose flat indices are
    written beside them; at the default sample size both files together stay within 64 MB."""
    sys.modules.pop("bench", None)
    import bench

    assert bench.DUMP_SAMPLES * (4 + 8) <= 64 << 20
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 1000)
    ids = torch.arange(-1, 5 * 40 * 30 - 1, dtype=torch.int32).reshape(5, 40, 30)
    bench.dump_outputs(tmp_path / "a", ids, 6000, 0, 1)
    bench.dump_outputs(tmp_path / "b", ids, 6000, 1, 2)
    got, idx = np.load(tmp_path / "a" / "face_ids.npy"), np.load(tmp_path / "a" / "face_ids_index.npy")
    assert got.dtype == np.float32 and idx.dtype == np.float64 and got.shape == idx.shape == (1000,)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < ids.numel()
    assert np.array_equal(got, ids.reshape(-1).numpy()[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "b" / "face_ids_rank1.npy"), got)
    assert np.array_equal(np.load(tmp_path / "b" / "face_ids_index_rank1.npy"), idx)
