"""The table checks of `PairAccumulator.add_rects` / `add_polygons` (`_hip._host_array`, `_check_offsets`, `_check_int32`):
functions of host arrays, run here without a device or the library.  Every message is the literal text callers have seen
since the rectangle and polygon paths were added."""
import numpy as np
import pytest
import torch

from geograypher_amd import _hip


def _fails(message, fn, *args, **kwargs):
    with pytest.raises(ValueError) as err:
        fn(*args, **kwargs)
    assert str(err.value) == message


def _rect(offsets, n, total):
    _hip._check_offsets(np.asarray(offsets), n, total, "views", "rectangle", "rectangles")


def _poly(offsets, n, total):
    _hip._check_offsets(np.asarray(offsets), n, total, "views", "polygon", "rings")


def _vert(offsets, n, total):
    _hip._check_offsets(np.asarray(offsets), n, total, "rings", "vertex", "vertices", at_least_one="vertex per ring")


def test_wrong_length():
    _fails("3 views need 4 rectangle offsets, got 3", _rect, [0, 2, 5], 3, 5)
    _fails("3 views need 4 polygon offsets, got 5", _poly, [0, 1, 2, 3, 5], 3, 5)
    _fails("2 rings need 3 vertex offsets, got 2", _vert, [0, 7], 2, 7)
    _fails("0 views need 1 rectangle offsets, got 0", _rect, np.zeros(0, dtype=np.int64), 0, 0)


def test_first_offset_not_zero():
    _fails("rectangle offsets must rise from 0 to 5 (the number of rectangles)", _rect, [1, 2, 5], 2, 5)
    _fails("polygon offsets must rise from 0 to 5 (the number of rings)", _poly, [-1, 2, 5], 2, 5)
    _fails("vertex offsets must rise from 0 to 7 (the number of vertices), at least one vertex per ring", _vert, [1, 3, 7], 2, 7)


def test_last_offset_not_the_row_total():
    _fails("rectangle offsets must rise from 0 to 6 (the number of rectangles)", _rect, [0, 2, 5], 2, 6)
    _fails("polygon offsets must rise from 0 to 4 (the number of rings)", _poly, [0, 2, 5], 2, 4)
    _fails("vertex offsets must rise from 0 to 8 (the number of vertices), at least one vertex per ring", _vert, [0, 3, 7], 2, 8)
    _fails("rectangle offsets must rise from 0 to 1 (the number of rectangles)", _rect, [0], 0, 1)


def test_a_falling_step():
    _fails("rectangle offsets must rise from 0 to 5 (the number of rectangles)", _rect, [0, 4, 3, 5], 3, 5)
    _fails("polygon offsets must rise from 0 to 5 (the number of rings)", _poly, [0, 6, 5], 2, 5)
    _fails("vertex offsets must rise from 0 to 7 (the number of vertices), at least one vertex per ring", _vert, [0, 5, 4, 7], 3, 7)


def test_a_ring_with_zero_vertices():
    _fails("vertex offsets must rise from 0 to 7 (the number of vertices), at least one vertex per ring", _vert, [0, 3, 3, 7], 3, 7)
    _rect([0, 3, 3, 7], 3, 7)   # ... which a view of rectangles or of rings may be
    _poly([0, 3, 3, 7], 3, 7)


def test_a_value_beyond_int32():
    rects = np.array([[0, 0, 4, 4, 1], [0, 0, 4, 4, 2**31]], dtype=np.int64)
    _fails("rectangle corners and classes must fit in int32", _hip._check_int32, rects, "rectangle corners and classes")
    rects[1, 4] = -2**31 - 1
    _fails("box corners and classes must fit in int32", _hip._check_int32, rects, "box corners and classes")
    _fails("vertex offsets must fit in int32", _hip._check_int32, np.array([0, 3, 2**31]), "vertex offsets")
    rects[1, 4] = -2**31      # the extremes of int32 fit
    rects[0, 4] = 2**31 - 1
    _hip._check_int32(rects, "rectangle corners and classes")
    _hip._check_int32(np.zeros((0, 5), dtype=np.int64), "rectangle corners and classes")   # an empty table has no extremes


def test_tables_that_pass():
    _rect([0], 0, 0)                      # zero views
    _poly([0], 0, 0)
    _vert([0], 0, 0)                      # ... and so zero rings
    _rect([0, 3, 3, 8], 3, 8)             # an empty view between full ones
    _poly([0, 512, 512, 513], 3, 513)
    _vert([0, 1, 4, 9], 3, 9)             # a ring of one vertex is a ring
    _rect(np.array([0, 2, 5], dtype=np.int32), 2, 5)


def test_host_array_takes_tensors_and_arrays():
    a = np.arange(10, dtype=np.int64).reshape(2, 5)
    assert _hip._host_array(a) is a
    for got in (_hip._host_array(torch.from_numpy(a)), _hip._host_array(a.tolist())):
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, a)
