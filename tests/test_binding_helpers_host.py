"""The binding's module-level helpers, without a device: the count-then-fill protocol over a fake attempt, the null pointer,
and the "float32 stays, everything else becomes float64" rule."""
import numpy as np
import pytest
import torch

from geograypher_amd import _hip
from geograypher_amd._hip import GR_EINVAL, GR_EOVERFLOW, GR_OK


class Library:
    """A fake count-then-fill entry point holding `total` items: overflows when offered less (unless `codes` says otherwise)."""

    def __init__(self, total, codes=None):
        self.total, self.codes, self.caps, self.checked = total, list(codes or []), [], []

    def attempt(self, cap):
        self.caps.append(cap)
        rc = self.codes.pop(0) if self.codes else (GR_EOVERFLOW if self.total > cap > 0 else GR_OK)
        return rc, self.total, ("filled", min(cap, self.total))

    def check(self, rc, name):
        self.checked.append((rc, name))
        if rc != GR_OK:
            raise ValueError(f"{name}: code {rc}") if rc == GR_EINVAL else RuntimeError(f"{name} failed (code {rc})")

    def run(self, cap, something_to_fill=lambda total: total > 0, check=None):
        return _hip._count_then_fill("gr_fake", self.attempt, cap, something_to_fill, check or self.check)


def test_a_call_that_fits_is_made_once():
    lib = Library(total=5)
    assert lib.run(8) == (("filled", 5), 1)
    assert lib.caps == [8] and lib.checked == [(GR_OK, "gr_fake")]


def test_an_overflow_is_repeated_once_at_exactly_the_reported_total():
    lib = Library(total=37)
    assert lib.run(8) == (("filled", 37), 2)
    assert lib.caps == [8, 37] and lib.checked == [(GR_OK, "gr_fake")]


def test_no_room_offered_and_something_to_fill_is_repeated_at_the_total():
    lib = Library(total=3)
    assert lib.run(0) == (("filled", 3), 2)
    assert lib.caps == [0, 3]


def test_no_room_offered_and_a_caller_that_needs_room_for_a_zero_total_is_repeated_at_one():
    lib = Library(total=0)
    assert lib.run(0, something_to_fill=lambda total: True) == (("filled", 0), 2)
    assert lib.caps == [0, 1]


def test_no_room_offered_and_nothing_to_fill_is_made_once():
    lib = Library(total=0)
    assert lib.run(0) == (("filled", 0), 1)
    assert lib.caps == [0] and lib.checked == [(GR_OK, "gr_fake")]


def test_two_overflows_raise():
    lib = Library(total=9, codes=[GR_EOVERFLOW, GR_EOVERFLOW])
    with pytest.raises(RuntimeError, match=r"gr_fake failed \(code -6\)"):   # the backend's check: what the caller sees today
        lib.run(4)
    assert lib.caps == [4, 9]
    lib = Library(total=9, codes=[GR_EOVERFLOW, GR_EOVERFLOW])
    with pytest.raises(RuntimeError, match="gr_fake reported two different totals for the same input"):
        lib.run(4, check=lambda rc, name: None)   # ... and under a check that lets the code pass
    assert lib.caps == [4, 9]


def test_another_code_goes_to_the_check_at_once():
    lib = Library(total=9, codes=[GR_EINVAL])
    with pytest.raises(ValueError, match="gr_fake: code -1"):
        lib.run(4)
    assert lib.caps == [4] and lib.checked == [(GR_EINVAL, "gr_fake")]
    lib = Library(total=9, codes=[GR_EINVAL])
    seen = []
    assert lib.run(0, check=lambda rc, name: seen.append(rc)) == (("filled", 0), 1)   # not even at cap 0 with a total
    assert lib.caps == [0] and seen == [GR_EINVAL]


def test_ptr_of_none_is_the_null_pointer():
    assert _hip._ptr(None) is None
    t = torch.zeros(3)
    assert _hip._ptr(t) == t.data_ptr()


@pytest.mark.parametrize("name,stays", [("uint8", False), ("int32", False), ("float32", True), ("float64", False)])
def test_float32_stays_and_everything_else_becomes_float64(name, stays):
    want = ("float32", _hip.GR_DTYPE_F32) if stays else ("float64", _hip.GR_DTYPE_F64)
    values = np.array([[0, 1, 200], [3, 2, 1]])
    a = values.astype(name)
    out, *kind = _hip._float_kind(a)
    assert tuple(kind) == want and out.dtype == np.dtype(want[0]) and np.array_equal(out, values)
    assert (out is a) == (name in ("float32", "float64"))   # converted on the host only where it has to be
    t = torch.as_tensor(a)
    out, *kind = _hip._float_kind(t)
    assert tuple(kind) == want and out is t   # a tensor is converted by the backend, on the device
    out, *kind = _hip._float_kind(values.tolist())
    assert tuple(kind) == ("float64", _hip.GR_DTYPE_F64) and out.dtype == np.float64
