"""The fenced, poisoned allocator of tests/fenced_backend.py on CPU tensors (no GPU): its layout, that it sees a stray write on
either side of a payload and names it, and that every entry point of the binding that allocates an output has a fenced case
in tests/test_output_fences_gpu.py."""
import ast
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.fenced_backend import FENCE, POISON, FencedAllocator, fenced

DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64]
SHAPES = [(1,), (3,), (7, 37), (2, 3, 5), (513,), (4096,), 5]


def _buffer(alloc, k=-1):
    return alloc.live[k][0]


def test_poison_reads_as_the_documented_values():
    raw = np.full(8, POISON, dtype=np.uint8)
    assert POISON not in (0x00, 0xFF)
    assert raw[0] == 127
    assert raw[:4].view(np.int32)[0] == 2_139_062_143
    assert raw.view(np.int64)[0] == 9_187_201_950_435_737_471
    f32, f64 = float(raw[:4].view(np.float32)[0]), float(raw.view(np.float64)[0])
    assert np.isfinite(f32) and 3.396e38 < f32 < 3.397e38 and f32 < float(np.finfo(np.float32).max)
    assert np.isfinite(f64) and 1.382e306 < f64 < 1.383e306
    assert FENCE % 512 == 0 and FENCE >= 4096


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_layout_alignment_and_poison(shape, dtype):
    alloc = FencedAllocator("cpu")
    t = alloc.empty(shape, dtype)
    want_shape = (shape,) if isinstance(shape, int) else shape
    assert tuple(t.shape) == want_shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
    n = t.numel() * t.element_size()
    buf = _buffer(alloc)
    assert buf.dtype == torch.uint8 and buf.numel() >= FENCE + n + FENCE and buf.numel() % 512 == 0
    # the payload starts FENCE bytes (a multiple of 512) into the buffer and the tail fence at byte n exactly
    assert t.data_ptr() - buf.data_ptr() == FENCE and (t.data_ptr() - buf.data_ptr()) % 512 == 0
    assert bool((buf == POISON).all())
    assert np.array_equal(t.reshape(-1).view(torch.uint8).numpy(), np.full(n, POISON, dtype=np.uint8))
    # zeros / full write the payload only
    z = alloc.zeros(shape, dtype)
    assert not z.any() and bool((_buffer(alloc)[:FENCE] == POISON).all()) and bool((_buffer(alloc)[FENCE + n:] == POISON).all())
    f = alloc.full(shape, 3, dtype)
    assert bool((f == 3).all()) and bool((_buffer(alloc)[:FENCE] == POISON).all()) and bool((_buffer(alloc)[FENCE + n:] == POISON).all())
    assert alloc.check_fences() == 3 and alloc.live == []


@pytest.mark.parametrize("shape", [(0,), (0, 3), (4, 0)], ids=str)
def test_zero_size_requests_pass_through(shape):
    alloc = FencedAllocator("cpu")
    for make in (alloc.empty, alloc.zeros, lambda s, d: alloc.full(s, 1.0, d)):
        t = make(shape, torch.float64)
        plain = torch.empty(shape, dtype=torch.float64)
        assert tuple(t.shape) == shape and t.dtype == torch.float64 and t.numel() == 0
        assert t.data_ptr() == plain.data_ptr() == 0   # what `_ptr` and the binding's null checks see
    assert alloc.live == [] and alloc.check_fences() == 0


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.float64], ids=lambda d: str(d).split(".")[-1])
def test_stray_writes_are_caught_and_named(dtype):
    alloc = FencedAllocator("cpu")
    shape = (3, 7)
    size = torch.empty((), dtype=dtype).element_size()
    n = 21 * size
    # inside the payload, first and last byte included: no failure
    t = alloc.empty(shape, dtype)
    raw = _buffer(alloc)
    raw[FENCE] = 0
    raw[FENCE + n - 1] = 0xFF
    t.fill_(1)
    assert alloc.check_fences() == 1
    # one byte before the payload
    alloc.empty(shape, dtype)
    _buffer(alloc)[FENCE - 1] = 0
    with pytest.raises(AssertionError, match=re.escape(f"front fence of the {shape} {dtype} allocation") + r".*offset -1 from") as err:
        alloc.check_fences()
    assert "0x00" in str(err.value) and alloc.live == []
    # one byte after it: the tail fence starts at byte n, not at a rounded-up offset
    assert n % 512 != 0
    alloc.empty(shape, dtype)
    _buffer(alloc)[FENCE + n] = 0xFF
    with pytest.raises(AssertionError, match=re.escape(f"tail fence of the {shape} {dtype} allocation") + rf".*offset {n} from") as err:
        alloc.check_fences()
    assert "0xFF" in str(err.value)
    # the far ends of both fences, and an earlier allocation among later clean ones
    alloc.empty(shape, dtype)
    _buffer(alloc)[0] = 1
    alloc.empty((5,), torch.int64)
    with pytest.raises(AssertionError, match=rf"front fence of the {re.escape(str(shape))}.*offset -{FENCE} from"):
        alloc.check_fences()
    alloc.empty(shape, dtype)
    _buffer(alloc)[-1] = 1
    total = _buffer(alloc).numel()
    with pytest.raises(AssertionError, match=rf"tail fence.*offset {total - FENCE - 1} from"):
        alloc.check_fences()
    # a write of the poison value itself changes nothing and cannot be seen
    alloc.empty(shape, dtype)
    _buffer(alloc)[FENCE - 1] = POISON
    assert alloc.check_fences() == 1


def test_context_manager_checks_on_exit_and_keeps_the_bodys_error():
    alloc = FencedAllocator("cpu")
    with fenced(alloc):
        alloc.empty((4,), torch.int32).zero_()
    assert alloc.live == []
    with pytest.raises(AssertionError, match="tail fence"):
        with fenced(alloc):
            alloc.empty((4,), torch.int32)
            _buffer(alloc)[FENCE + 16] = 0
    with pytest.raises(KeyError):
        with fenced(alloc):
            alloc.empty((4,), torch.int32)
            _buffer(alloc)[FENCE + 16] = 0
            raise KeyError("the body's own error")
    assert alloc.live == []


# ---- coverage: every entry point that allocates an output has a fenced case ------------------------------------------------
ALLOCATORS = {"_empty", "_zeros", "_full", "_stats"}
CLASSES = ("HipRaster", "PairAccumulator")


def _called_attributes(func):
    return {node.func.attr for node in ast.walk(func) if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)}


def allocating_entry_points():
    """{"method" or "PairAccumulator.method"} of the public methods of `HipRaster` and `PairAccumulator` whose body calls
    `_empty`, `_zeros`, `_full` or `_stats`, directly (nested functions included) or through private methods of the two
    classes that do (`_gather`, `_count_pairs`, `_make_room`, `_compact`, ...)."""
    source = Path(__file__).resolve().parents[1] / "geograypher_amd" / "_hip.py"
    tree = ast.parse(source.read_text())
    methods = {}
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef) and cls.name in CLASSES:
            for f in cls.body:
                if isinstance(f, ast.FunctionDef):
                    methods[(cls.name, f.name)] = _called_attributes(f)
    assert {c for c, _ in methods} == set(CLASSES)
    allocating = set(ALLOCATORS)          # private method names that allocate, grown to a fixed point
    while True:
        more = {name for (_, name), calls in methods.items() if name.startswith("_") and not name.startswith("__")
                and calls & allocating} - allocating
        if not more:
            break
        allocating |= more
    assert {"_gather", "_count_pairs"} <= allocating
    return {name if cls == "HipRaster" else f"{cls}.{name}" for (cls, name), calls in methods.items()
            if not name.startswith("_") and calls & allocating}


def test_every_allocating_entry_point_has_a_fenced_case():
    from tests import test_output_fences_gpu as gpu

    found = allocating_entry_points()
    assert {"raster_face_ids", "gather_texture", "set_cover", "sample_raster", "PairAccumulator.add",
            "PairAccumulator.finish"} <= found, "the walk over _hip.py no longer finds what it must"
    assert not set(gpu.COVERED) & set(gpu.EXEMPT)
    missing = sorted(found - set(gpu.COVERED) - set(gpu.EXEMPT))
    assert not missing, f"entry points that allocate an output but have no fenced case in test_output_fences_gpu.py: {missing}"
    for name, tests in gpu.COVERED.items():
        assert tests, name
        for test in tests:
            assert callable(getattr(gpu, test, None)), f"COVERED[{name!r}] names {test}, which the module does not define"
    for name, reason in gpu.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) > 20 and "\n" not in reason, f"EXEMPT[{name!r}] needs a one-line reason"
