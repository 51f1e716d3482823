"""csrc/device_buffer.hpp on its own: how a context owns device memory (Buf, reserve, reserve_group, release, release_all).
tests/device_buffer_main.cpp instantiates the header with a policy of its own (malloc / free, a counting quiesce hook, a k-th
allocation that fails), is compiled with the host C++ compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run as a
program of its own with the leak detector on.  No GPU, no HIP header, nothing loaded into Python.  The source test pins what the
header is for: one allocation and one free in the whole library, none of the old capacity fields."""
import subprocess
from pathlib import Path

import pytest

from tests.test_scratch_layout_host import SANITIZE, host_compiler

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "geograypher_amd" / "csrc"
REMOVED = ("ctrl_have", "comp_have", "nrow_have", "work_have", "clip_have", "rec_have", "touched_have", "visits_have", "blk_cap",
           "soup_cap", "winner_bytes")


def test_buffer_header_is_the_only_owner_of_device_memory():
    from geograypher_amd import build

    text = (CSRC / "device_buffer.hpp").read_text()
    assert "#include <hip" not in text and '#include "gr_internal.hpp"' not in text
    assert CSRC / "device_buffer.hpp" in build.HEADERS
    units = "".join(p.read_text() for p in build.SOURCES + build.HEADERS)
    assert units.count("hipMalloc(") == 1 and units.count("hipFree(") == 1
    internal = (CSRC / "gr_internal.hpp").read_text()
    assert '#include "device_buffer.hpp"' in internal and internal.count("hipMalloc(") == 1 and internal.count("hipFree(") == 1
    assert not [name for name in REMOVED if name in internal]


def test_buffer_program_runs_clean_under_asan_and_ubsan(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++ or $CXX)")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([cxx, SANITIZE, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip(f"{cxx} cannot link {SANITIZE} (no sanitizer runtime): {linked.stderr.strip()[-200:]}")
    exe = tmp_path / "device_buffer"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", SANITIZE, "-fno-sanitize-recover=undefined",
                            f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(ROOT / "tests" / "device_buffer_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok: device buffer" and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    assert "LeakSanitizer" not in run.stderr
