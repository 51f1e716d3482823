"""A `FencedHipRaster` that shows work issued at the wrong TIME (a helper module for the tests, not a conftest).

include/geograster.h promises that all work of a call is enqueued on the `stream` it is given and that nothing waits behind the
caller's back.  On torch's default stream neither can be seen: everything serialises with everything else.  The probe runs a call
on a side stream (`pick_side_stream`) and puts two things in its way; outputs stay fenced and poisoned with 0x7F.

Leg B, the default stream is held (`held_default_stream`): a long `torch.cuda._sleep` is enqueued on the device's default stream and
an event `released` recorded behind it.  The body runs under `torch.cuda.stream(side)` and reads its results on `side`.

  * what the call handed to the null stream has not run when the results are read: poison or stale words are compared;
  * a wait for the whole device or for the null stream outlasts the hold: `released` is signalled when the body ends, and the
    hold fails with `HOLD_ENDED`.  A hold that is too short fails the same way: it never passes vacuously.

Leg A, the producer is delayed: `_dev` hands on a private copy of every input and keeps it in a registry (`InputRegistry`; the
caller's tensors are never touched).  `_rc`, through which the binding makes every library call, first enqueues ON THE CURRENT
STREAM: zero every registered input, a delay, restore every input from its clean clone, record an event `ready`.  Then it calls.

  * an operation of the call on ANY other stream (the library's own side stream without its event wait, the null stream, a host
    read that comes too early) reads zeros.  Zero is an index, an offset and a count in range for every array of every scene of
    the tests, so a misrouted kernel computes a wrong answer and reads nothing out of bounds;
  * if `ready` is still unsignalled when the library returns, the whole call was enqueued while its inputs were zeros: the leg
    COUNTS for that call.  If it is signalled, the call itself waited for its stream; the leg proves nothing there and the call
    is recorded as one that waits (`CallRecord.waited`), to be compared with the header's "Synchronises `stream`" notes.

The lengths are conditions, not tolerances: `released` and `ready` are what keeps a length that is too short from hiding anything.

The registry and the zero / restore sequence work on CPU tensors (tests/test_stream_probe_host.py)."""
import contextlib
import time
from collections import namedtuple

import torch

from tests.fenced_backend import FENCE, FencedHipRaster, fenced

HOLD_ENDED = "the hold ended before the results were read: the hold is too short, or the call waited for the default stream"
NO_SIDE_STREAM = "none of 8 candidate streams runs while the default stream is held"
MIN_HOLD_S = 0.25
HOLD_FACTOR = 20
MIN_DELAY_S = 0.020
DELAY_FACTOR = 10

CallRecord = namedtuple("CallRecord", "name host_seconds waited")   # waited: None without leg A


class InputRegistry:
    """Private copies of the inputs of a row and a clean clone of each."""

    def __init__(self):
        self.entries = []     # (the copy the library reads, its clean clone)

    def private(self, tensor):
        copy = tensor.clone()
        self.entries.append((copy, copy.clone()))
        return copy

    def zero(self):
        for copy, _ in self.entries:
            copy.zero_()

    def restore(self):
        for copy, clean in self.entries:
            copy.copy_(clean)

    def clear(self):
        self.entries = []

    def __len__(self):
        return len(self.entries)


# ---- delays -------------------------------------------------------------------------------------------------------------------
_cycles_per_second = {}


def cycles_per_second(device):
    """What `torch.cuda._sleep` counts in a second on this device: one short sleep timed with two events, once per module, before
    any hold.  The sleep is lengthened until it lasts a millisecond, so that the launch does not weigh."""
    device = torch.device(device)
    if device not in _cycles_per_second:
        stream = torch.cuda.default_stream(device)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(1000)          # loads the kernel
            stream.synchronize()
            cycles = 1_000_000
            for _ in range(6):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                torch.cuda._sleep(cycles)
                b.record(stream)
                b.synchronize()
                seconds = a.elapsed_time(b) / 1000.0
                if seconds >= 1e-3:
                    break
                cycles *= 10
        assert seconds > 0, "a sleep of torch.cuda._sleep took no time"
        _cycles_per_second[device] = cycles / seconds
    return _cycles_per_second[device]


def enqueue_delay(device, seconds):
    """A delay of `seconds` on the current stream of the device."""
    torch.cuda._sleep(max(int(seconds * cycles_per_second(device)), 1))


@contextlib.contextmanager
def held_stream(stream, seconds):
    """`stream` is busy for `seconds` from here; -> the event `released` recorded behind the delay.  When the body ends, `released`
    must still be unsignalled (AssertionError `HOLD_ENDED` otherwise); then the stream is waited for, so that what follows starts
    clean.  A body that raises keeps its own error."""
    device = stream.device
    cycles_per_second(device)
    released = torch.cuda.Event()
    with torch.cuda.stream(stream):
        enqueue_delay(device, seconds)
        released.record(stream)
    try:
        yield released
    except BaseException:
        stream.synchronize()
        raise
    still_held = not released.query()
    stream.synchronize()
    assert still_held, HOLD_ENDED


def held_default_stream(device, seconds):
    """`held_stream` on the default stream of `device`: torch's default stream is the null stream of the HIP runtime."""
    default = torch.cuda.default_stream(torch.device(device))
    assert default.cuda_stream == 0, "the default stream of torch is the null stream"
    return held_stream(default, seconds)


PICKED = []      # (the index of the candidate taken, the candidates that waited behind a hold) of every pick, in order


def pick_side_stream(device, beside=(), short_hold=0.05):
    """A stream of torch's pool that runs while the default stream -- and each stream of `beside` in turn -- is held.  A process
    has few hardware queues here, and a stream that shares one with a held stream waits behind every hold.  At most 8 candidates,
    one short hold each per held stream: a small `fill_` on the candidate must complete while `released` is unsignalled.  Which
    candidate was taken is written to `PICKED`."""
    device = torch.device(device)
    behind = []
    for k in range(8):
        candidate = torch.cuda.Stream(device)
        assert candidate.cuda_stream != 0, "a side stream must not be the null stream"
        if not runs_beside(candidate, (torch.cuda.default_stream(device),) + tuple(beside), short_hold):
            behind.append(k)
            continue
        PICKED.append((k, behind))
        print(f"\nstream probe | candidate {k} of torch's pool runs while {1 + len(beside)} other stream(s) are held; "
              f"candidates that waited behind a hold: {behind or 'none'}")
        return candidate
    raise AssertionError(NO_SIDE_STREAM)


def runs_beside(candidate, held, short_hold=0.05):
    """Does a small `fill_` on `candidate` complete while each stream of `held`, in turn, is busy for `short_hold` seconds?"""
    device = candidate.device
    word = torch.zeros((64,), dtype=torch.int32, device=device)
    torch.cuda.synchronize(device)
    try:
        for k, busy in enumerate(held):
            with held_stream(busy, short_hold):
                with torch.cuda.stream(candidate):
                    word.fill_(k + 1)
                candidate.synchronize()
    except AssertionError:
        return False
    assert word.cpu().tolist() == [len(held)] * 64
    return True


_pool = {}


def pool_placement(device, short_hold=0.03):
    """(the handles of torch's pool streams of `device` in the order `torch.cuda.Stream(device)` hands them out, {handle: does it
    run while the default stream is held}): one short hold per stream, once per process.  A stream keeps the hardware queue it got
    at its first use, so the answer stays.  Measured on the MI355X with 4 hardware queues a process: of the 32 streams of the pool,
    every fourth in the order of first use waits behind a held null stream, always the same ones."""
    device = torch.device(device)
    if device not in _pool:
        order, runs = [], {}
        for _ in range(256):
            stream = torch.cuda.Stream(device)
            if stream.cuda_stream in runs:
                break
            order.append(stream.cuda_stream)
            runs[stream.cuda_stream] = runs_beside(stream, (torch.cuda.default_stream(device),), short_hold)
        assert any(runs.values()), NO_SIDE_STREAM
        _pool[device] = (order, runs)
        waits = [k for k, h in enumerate(order) if not runs[h]]
        print(f"\nstream probe | torch's pool has {len(order)} streams; those that wait behind a held default stream, in the order "
              f"they are handed out: {waits or 'none'}")
    return _pool[device]


def advance_pool(device, n):
    """Takes streams from torch's pool until the next `n` it will hand out all run while the default stream is held (the pool goes
    round: `pool_placement`); -> their handles."""
    order, runs = pool_placement(device)
    for _ in range(len(order) + 1):
        at = order.index(torch.cuda.Stream(device).cuda_stream)
        coming = [order[(at + 1 + j) % len(order)] for j in range(n)]
        if all(runs[h] for h in coming):
            return coming
    raise AssertionError(f"torch's pool has no {n} streams in a row that run while the default stream is held")


# ---- the backend --------------------------------------------------------------------------------------------------------------
class StreamProbeHipRaster(FencedHipRaster):
    """`FencedHipRaster` whose inputs are private, registered copies and whose library calls can be put behind a delayed producer
    (`delay_seconds` > 0).  `calls` records every library call since `begin`."""

    def __init__(self, device=None, fence: int = FENCE):
        super().__init__(device, fence)
        self.registry = InputRegistry()
        self.delay_seconds = 0.0
        self.calls = []

    def begin(self, delay_seconds=0.0):
        self.registry.clear()
        self.calls = []
        self.delay_seconds = float(delay_seconds)

    def _dev(self, array, dtype):
        return self.registry.private(super()._dev(array, dtype))

    def around_call(self, name, call):
        """Leg A round one call on the current stream: zero the inputs, delay, restore, record `ready`; `call()`; was `ready` still
        unsignalled when it returned?"""
        ready = None
        if self.delay_seconds > 0:
            self.registry.zero()
            enqueue_delay(self.device, self.delay_seconds)
            self.registry.restore()
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
        t0 = time.perf_counter()
        result = call()
        seconds = time.perf_counter() - t0
        self.calls.append(CallRecord(name, seconds, None if ready is None else bool(ready.query())))
        return result

    def _rc(self, name, *args):
        return self.around_call(name, lambda: FencedHipRaster._rc(self, name, *args))

    def wait_before_fence_check(self):
        """`fenced` waits for the stream the body ran on, not for the device: the device may be held."""
        torch.cuda.current_stream(self.device).synchronize()


# ---- a row --------------------------------------------------------------------------------------------------------------------
def run_body(probe, side, body, delay_seconds=0.0):
    """`body(probe)` under `torch.cuda.stream(side)` inside `fenced(probe)`; the body copies every result to the host on `side`.
    -> (wall seconds, the library calls made)."""
    probe.begin(delay_seconds)
    t0 = time.perf_counter()
    try:
        with torch.cuda.stream(side):
            with fenced(probe):
                body(probe)
            side.synchronize()
    finally:
        probe.delay_seconds = 0.0
    return time.perf_counter() - t0, list(probe.calls)


def _summary(calls):
    seen = {}      # "function:counted" or "function:waited" -> how often, in the order of the first call
    for c in calls:
        key = c.name if c.waited is None else f"{c.name}:{'waited' if c.waited else 'counted'}"
        seen[key] = seen.get(key, 0) + 1
    return " ".join(f"{key} x{n}" for key, n in seen.items()) or "-"


REPORT = []      # one record per row run: what the `-s` output shows


def run_row(probe, side, name, body, legs="abcd", own_stream_may_queue=False):
    """The steps of a row: (a) on the side stream alone -- measured, and also the warm-up that sizes the arena, loads the kernels
    and lets a raster call look at an unknown image size: scratch growth is a documented synchronisation --, (b) leg B, (c) leg A,
    (d) both.  Fences are checked after each (`run_body`).
    The hold is HOLD_FACTOR times the wall time of (a), at least MIN_HOLD_S; the delay MIN_DELAY_S or DELAY_FACTOR times the host
    time of the slowest binding call of (a).  Under (d) the host also waits for one delay per library call whenever it reads a
    result, so the hold is longer there by twice the sum of the delays.  -> the record appended to `REPORT`.
    `own_stream_may_queue` is for a row whose call uses a stream the LIBRARY creates: the runtime may give that stream the hardware
    queue of the null stream, and its work then waits behind the hold although nothing was issued to the null stream.  For such a
    row the end of a hold is recorded (`held` False) instead of raised; everything else holds as for every row."""
    device = probe.device
    t_row = time.perf_counter()
    wall, calls = run_body(probe, side, body)
    slowest = max((c.host_seconds for c in calls), default=0.0)
    hold = max(MIN_HOLD_S, HOLD_FACTOR * wall)
    delay = max(MIN_DELAY_S, DELAY_FACTOR * slowest)
    record = dict(row=name, wall=wall, hold=hold, delay=delay, calls=[c.name for c in calls], held=None, leg_a=[])

    def under_hold(seconds, delay_seconds):
        """-> the library calls of the step.  `own_stream_may_queue`: the end of the hold is recorded, not raised -- the
        comparisons of the body have passed by then, and a result computed too early would have failed them first."""
        made = []
        try:
            with held_default_stream(device, seconds):
                made = run_body(probe, side, body, delay_seconds)[1]
        except AssertionError as error:
            if not own_stream_may_queue or str(error) != HOLD_ENDED:
                raise
            record["held"] = False
            return list(probe.calls)
        record["held"] = record["held"] is not False
        return made

    if "b" in legs:
        under_hold(hold, 0.0)
    if "c" in legs:
        record["leg_a"] = run_body(probe, side, body, delay)[1]
    if "d" in legs:
        record["leg_a"] = record["leg_a"] + under_hold(hold + 2 * delay * max(len(calls), 1), delay)
    record["row_seconds"] = time.perf_counter() - t_row
    REPORT.append(record)
    print(f"\nstream probe | {name} | wall {wall * 1e3:.1f} ms | hold {hold:.2f} s | delay {delay * 1e3:.0f} ms | "
          f"row {record['row_seconds']:.1f} s | "
          f"default stream still held when the results were read: {record['held']} | leg A: {_summary(record['leg_a'])}")
    return record
