"""A `HipRaster` whose output allocations are fenced and poisoned (a helper module for the tests, not a conftest).

The binding allocates every output through `HipRaster._empty`, `_zeros`, `_full` and `_stats` (`_stats` goes through the first
two).  `FencedHipRaster` overrides the three: a request of n payload bytes becomes ONE uint8 buffer of FENCE + n + FENCE + pad
bytes, filled with `POISON` from end to end, and the caller gets `buf[FENCE:FENCE + n]` viewed as its dtype and shape.

  * FENCE is a multiple of 512 bytes, so the payload keeps the alignment torch gives an allocation of its own (kernels may
    rely on it).  The tail fence starts at byte n exactly -- not at a rounded-up offset --, so a store ONE element past the end
    is seen; `pad` (< 512 bytes) only rounds the buffer's size up and belongs to the tail fence.
  * A missing store leaves the poison in the payload, whatever an earlier call left in the block the caching allocator hands
    back: the comparison with the stand-in then fails.
  * A stray store within FENCE bytes of either side changes a fence byte: `check_fences()` fails and names it.

`POISON` = 0x7F, neither 0x00 nor 0xFF, reads as a value no stage produces at the shapes of the tests:

    uint8    127                         (the one type with no impossible value: the tests use fewer than 127 classes and
                                          nodata 255 for uint8 outputs, and assert that on the stand-in's answer)
    int32    2 139 062 143               (0x7F7F7F7F: no face, vertex, ring or pair index; as a count, more than any input holds)
    int64    9 187 201 950 435 737 471   (0x7F7F7F7F7F7F7F7F)
    float32  ~ 3.3961775e+38             (finite, a hair under FLT_MAX: no depth)
    float64  ~ 1.3824172e+306            (finite: no coordinate, weight, height or average; not NaN, which IS a legal result)

A zero-size request is passed through as a plain `torch.empty`: its `data_ptr()` stays what the binding's null checks expect.

The allocator part needs no GPU: `FencedAllocator(device)` works for any torch device (the host tests run it on the CPU).
"""
import contextlib
import math

import torch

from geograypher_amd._hip import HipRaster

POISON = 0x7F
FENCE = 4096          # bytes on either side of the payload: a multiple of 512, at least 4096
_ALIGN = 512

assert POISON not in (0x00, 0xFF) and FENCE % _ALIGN == 0 and FENCE >= 4096


class FencedAllocator:
    """The fenced, poisoned allocations of one torch device, and the record of those not yet checked."""

    def __init__(self, device, fence: int = FENCE):
        assert fence % _ALIGN == 0 and fence >= 4096, "the fence is a multiple of 512 bytes, at least 4096"
        self.device = torch.device(device)
        self.fence = int(fence)
        self.live = []        # (buffer, payload bytes, shape, dtype) of every allocation since the last check

    def empty(self, shape, dtype):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(k) for k in shape)
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        if n == 0:
            return torch.empty(shape, dtype=dtype, device=self.device)
        G = self.fence
        total = -(-(G + n + G) // _ALIGN) * _ALIGN
        buf = torch.full((total,), POISON, dtype=torch.uint8, device=self.device)
        self.live.append((buf, n, shape, dtype))
        return buf[G:G + n].view(dtype).reshape(shape)

    def zeros(self, shape, dtype):
        return self.empty(shape, dtype).zero_()

    def full(self, shape, value, dtype):
        return self.empty(shape, dtype).fill_(value)

    def forget(self):
        self.live = []

    def payloads(self, dtype):
        """The payloads of the recorded allocations of one dtype, as the kernels left them (uint8 flags are read here before the
        binding turns them into bool, where the poison would pass for True)."""
        G = self.fence
        return [buf[G:G + n].view(dt).reshape(shape) for buf, n, shape, dt in self.live if dt == dtype]

    def check_fences(self):
        """Both fences of every recorded allocation still hold POISON, or AssertionError naming the allocation's shape and
        dtype, the side and the first changed byte's offset from the payload's first byte (front: negative; tail: from the
        payload's size n upwards).  The allocations are forgotten either way."""
        live, self.live = self.live, []
        G = self.fence
        for buf, n, shape, dtype in live:
            for side, part, origin in (("front", buf[:G], -G), ("tail", buf[G + n:], n)):
                changed = part != POISON
                if bool(changed.any()):
                    k = int(changed.nonzero()[0, 0])
                    raise AssertionError(
                        f"{side} fence of the {shape} {dtype} allocation ({n} payload bytes) was written: first changed byte at "
                        f"offset {origin + k} from the payload's start, now 0x{int(part[k]):02X}, "
                        f"{int(changed.sum())} fence bytes changed in all")
        return len(live)


class FencedHipRaster(HipRaster):
    """`HipRaster` whose outputs all come from a `FencedAllocator` on its device."""

    def __init__(self, device=None, fence: int = FENCE):
        super().__init__(device)
        self.fences = FencedAllocator(self.device, fence)

    def _empty(self, shape, dtype):
        return self.fences.empty(shape, dtype)

    def _zeros(self, shape, dtype):
        return self.fences.zeros(shape, dtype)

    def _full(self, shape, value, dtype):
        return self.fences.full(shape, value, dtype)

    def check_fences(self):
        return self.fences.check_fences()


@contextlib.contextmanager
def fenced(backend):
    """The calls of the body run on fresh records; on exit the device is waited for (a backend with a `wait_before_fence_check`
    of its own waits that way instead) and every fence checked.  A body that raises keeps its own error (the records are dropped)."""
    fences = getattr(backend, "fences", backend)
    fences.forget()
    try:
        yield backend
    except BaseException:
        fences.forget()
        raise
    wait = getattr(backend, "wait_before_fence_check", None)   # tests/stream_probe.py: the stream of the body, the device may be held
    if wait is not None:
        wait()
    elif fences.device.type == "cuda":
        torch.cuda.synchronize(fences.device)
    fences.check_fences()
