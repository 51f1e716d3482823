"""The stream probe of tests/stream_probe.py without a GPU: every function of the headers under include/ that takes a stream has a
row in tests/test_stream_contract_gpu.py, the "Synchronises" notes of the headers are the table the GPU module holds leg A against,
and the input registry with its zero / restore sequence works on CPU tensors and never touches a caller's tensor."""
import re
from pathlib import Path

import numpy as np
import torch

from tests.stream_probe import InputRegistry

ROOT = Path(__file__).resolve().parents[1]
N_STREAM_CALLS = 48


def _stream_declarations():
    """{function: (header, the comment in front of it)} of every function of every header under include/ whose last parameter is
    `void *stream`.  The arguments are read from the text without its comments, as tests/test_cabi.py::_declarations reads them;
    the comment of a function is the last one in front of it with nothing but declarations and the call's own `enum { ... };` in
    between (gr_argmax_nonzero_f64 and gr_polygon_box_pairs_fill are described with the declaration above them)."""
    found = {}
    for header in sorted((ROOT / "include").glob("*.h")):
        text = header.read_text()
        stripped = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
        takes_stream = set()
        for name, args in re.findall(r"\b(gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", stripped):
            args = [a.strip() for a in " ".join(args.split()).split(",")]
            if args[-1] == "void *stream":
                takes_stream.add(name)
        comment = ""
        tokens = r"(enum\s*\{.*?\}\s*;)|(/\*.*?\*/)|\b(gr_[a-z0-9_]+)\s*\([^()]*\)\s*;|([^\s/]+|/)"
        for enum, block, name, other in re.findall(tokens, text, flags=re.S):
            if enum:
                continue          # the enumerators of the call stand between its comment and its declaration
            if block:
                comment = block
            elif name:
                if name in takes_stream:
                    assert name not in found, name
                    found[name] = (header.name, comment)
            elif other not in ("int", "const", "char", "*"):
                comment = ""      # code between the comment and the declaration: an enum, a typedef, a #define
        assert takes_stream <= set(found), header.name
    return found


def test_every_stream_taking_function_has_a_row_or_a_reason():
    from tests import test_stream_contract_gpu as gpu

    declared = _stream_declarations()
    assert len(declared) == N_STREAM_CALLS, sorted(declared)
    assert {"gr_mesh_upload", "gr_raster_face_ids", "gr_nadir_raster", "gr_polygon_box_pairs_fill", "gr_argmax_nonzero_f64"} <= set(declared)
    assert not set(gpu.COVERED) & set(gpu.EXEMPT)
    missing = sorted(set(declared) - set(gpu.COVERED) - set(gpu.EXEMPT))
    assert not missing, f"stream-taking functions without a row in test_stream_contract_gpu.py: {missing}"
    unknown = sorted((set(gpu.COVERED) | set(gpu.EXEMPT)) - set(declared))
    assert not unknown, f"rows for functions no header declares with a stream: {unknown}"
    for name, rows in gpu.COVERED.items():
        assert rows and all(row in gpu.ROWS for row in rows), name
    for name, reason in gpu.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) > 20 and "\n" not in reason, f"EXEMPT[{name!r}] needs a one-line reason"
    for name, note in gpu.NOTES.items():
        assert (name in gpu.ROWS or callable(getattr(gpu, name, None))) and isinstance(note, str) and len(note.strip()) > 20, name


def test_the_synchronises_table_is_what_the_headers_say():
    """A stream-taking function is in `SYNCHRONISES` exactly when the comment in front of its declaration says that the call
    synchronises (or is synchronous)."""
    from tests import test_stream_contract_gpu as gpu

    marked = {name for name, (_, comment) in _stream_declarations().items() if re.search(r"synchron(is|ous)", comment, re.I)}
    assert {"gr_mesh_upload", "gr_count_pairs", "gr_louvain_communities"} <= marked
    assert "gr_rays_clip" not in marked and "gr_argmax_nonzero_f64" not in marked
    assert marked == gpu.SYNCHRONISES, (sorted(marked - gpu.SYNCHRONISES), sorted(gpu.SYNCHRONISES - marked))


def test_registry_zeroes_and_restores_private_copies_only():
    rng = np.random.default_rng(0)
    caller = [torch.from_numpy(rng.integers(1, 100, (257,)).astype(np.int32)), torch.from_numpy(rng.normal(size=(3, 5))),
              torch.from_numpy(rng.integers(1, 255, (7, 3)).astype(np.uint8))]
    kept = [t.clone() for t in caller]
    registry = InputRegistry()
    private = [registry.private(t) for t in caller]
    assert len(registry) == 3
    for p, t in zip(private, caller):
        assert p.data_ptr() != t.data_ptr() and torch.equal(p, t) and p.dtype == t.dtype and p.shape == t.shape
    registry.zero()
    assert all(not bool(p.any()) for p in private), "every registered input reads as zeros while the producer is delayed"
    assert all(torch.equal(t, k) for t, k in zip(caller, kept)), "a caller's tensor was modified"
    registry.restore()
    assert all(torch.equal(p, k) for p, k in zip(private, kept))
    # a copy the "library" scribbled on comes back from the clean clone, the clone itself is never handed out
    private[0].fill_(7)
    registry.zero()
    registry.restore()
    assert torch.equal(private[0], kept[0])
    assert all(torch.equal(t, k) for t, k in zip(caller, kept)), "a caller's tensor was modified"
    registry.clear()
    assert len(registry) == 0
    registry.zero()
    registry.restore()
    assert all(torch.equal(p, k) for p, k in zip(private, kept)), "a cleared registry touches nothing"


def test_the_probes_dev_hands_on_private_copies_on_the_cpu():
    """`StreamProbeHipRaster._dev` on a stand-in for the backend (no library, no GPU): numpy arrays and tensors alike become
    registered private copies of the asked dtype, and the caller's data stays as it was."""
    from tests import stream_probe as sp

    class OnCpu(sp.StreamProbeHipRaster):
        def __init__(self):          # no context: the device is the host
            self.device = torch.device("cpu")
            self.registry = sp.InputRegistry()
            self.delay_seconds = 0.0
            self.calls = []

    probe = OnCpu()
    array = np.arange(1, 13, dtype=np.int64).reshape(3, 4)
    tensor = torch.arange(1.0, 6.0, dtype=torch.float64)
    a = probe._dev(array, torch.int32)
    t = probe._dev(tensor, torch.float64)
    assert a.dtype == torch.int32 and a.tolist() == array.tolist() and t.data_ptr() != tensor.data_ptr() and len(probe.registry) == 2
    probe.registry.zero()
    assert not a.any() and not t.any() and array[0, 0] == 1 and tensor[0] == 1.0
    probe.registry.restore()
    assert a.tolist() == array.tolist() and torch.equal(t, tensor)
    # without a delay `around_call` only records the call
    assert probe.around_call("nothing", lambda: 5) == 5
    assert [(c.name, c.waited) for c in probe.calls] == [("nothing", None)]
    probe.begin()
    assert len(probe.registry) == 0 and probe.calls == []
