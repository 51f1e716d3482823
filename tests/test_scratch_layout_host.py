"""csrc/scratch_layout.hpp on its own: the bump-pointer layout every stage call carves its scratch with (Carve, up256,
bit_length).  tests/scratch_layout_main.cpp is compiled with the host C++ compiler under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program of its own: every offset a multiple of 256, arrays disjoint, rewind puts the
next array at the mark, total() the maximum over both overlay branches, arrays of no elements take no space.  No GPU, no HIP
header, nothing loaded into Python."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "geograypher_amd" / "csrc"
SANITIZE = "-fsanitize=address,undefined"


def host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def test_layout_header_includes_no_hip_and_is_a_build_header():
    from geograypher_amd import build

    text = (CSRC / "scratch_layout.hpp").read_text()
    assert "#include <hip" not in text and '#include "gr_internal.hpp"' not in text
    assert CSRC / "scratch_layout.hpp" in build.HEADERS
    units = "".join(p.read_text() for p in build.SOURCES) + (CSRC / "gr_internal.hpp").read_text()
    assert units.count("size_t up256(") == 0 and text.count("size_t up256(") == 1 and text.count("int bit_length(") == 1
    # the sorts and scans that run in a layout are stated in one header: no size-query macro, no hipcub call anywhere else
    assert CSRC / "cub_steps.hpp" in build.HEADERS
    steps = code_lines(CSRC / "cub_steps.hpp")
    assert "hipcub::DeviceRadixSort::SortPairs(" in steps and "hipcub::DeviceScan::ExclusiveSum(" in steps
    for path in list(build.SOURCES) + [h for h in build.HEADERS if h.name != "cub_steps.hpp"]:
        code = code_lines(path)
        assert "GR_CUB_MAX" not in code and "hipcub::" not in code and "<hipcub/" not in code, path.name


def code_lines(path):
    """The file without its // comments."""
    return "\n".join(line.split("//")[0] for line in path.read_text().splitlines())


def test_layout_program_runs_clean_under_asan_and_ubsan(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++ or $CXX)")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([cxx, SANITIZE, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip(f"{cxx} cannot link {SANITIZE} (no sanitizer runtime): {linked.stderr.strip()[-200:]}")
    exe = tmp_path / "scratch_layout"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", SANITIZE, "-fno-sanitize-recover=undefined",
                            f"-I{CSRC}", "-o", str(exe), str(ROOT / "tests" / "scratch_layout_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok: scratch layout" and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
