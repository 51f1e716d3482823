"""The C-ABI library loads and exports every symbol include/geograster.h declares (no compute without a GPU)."""
import ctypes
import re
from pathlib import Path

import pytest

from geograypher_amd import _hip

ROOT = Path(__file__).resolve().parents[1]


def _declared_symbols():
    text = (ROOT / "include" / "geograster.h").read_text()
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(_hip.EXPORTED_SYMBOLS)


def _declarations():
    """{symbol: [the C text of every argument]} of every function include/geograster.h declares, comments stripped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", (ROOT / "include" / "geograster.h").read_text(), flags=re.S)
    found = {}
    for name, args in re.findall(r"\b(gr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        args = " ".join(args.split())
        found[name] = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
    return found


def _kind(c_argument=None, ctype=None):
    """The kind of a header argument, or of a ctypes argument type: pointer, int64, int, double."""
    if ctype is not None:
        if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
            return "pointer"
        return {ctypes.c_int64: "int64", ctypes.c_int: "int", ctypes.c_int32: "int", ctypes.c_double: "double"}[ctype]
    if "*" in c_argument:
        return "pointer"
    words = [w for w in re.findall(r"\w+", c_argument) if w != "const"]
    return {"int64_t": "int64", "int": "int", "int32_t": "int", "double": "double"}[words[0]]


def test_every_signature_agrees_with_the_header_in_count_and_kind():
    """All symbols at once: the binding hands the library as many arguments as the header declares, and each is of the declared
    kind (a pointer, a 64-bit integer, an int, a double).  A short `argtypes` list, or an int where the library reads an
    int64_t, is a bad pointer or a bad size in a kernel's arguments."""
    declared = _declarations()
    assert sorted(declared) == sorted(_hip._SIGNATURES) and len(declared) == 47
    for name, arguments in declared.items():
        argtypes = _hip._SIGNATURES[name]
        assert len(arguments) == len(argtypes), f"{name}: the header declares {len(arguments)} arguments, the binding {len(argtypes)}"
        for k, (argument, ctype) in enumerate(zip(arguments, argtypes)):
            assert _kind(argument) == _kind(ctype=ctype), f"{name}, argument {k} ({argument!r}) is bound as {ctype.__name__}"


def test_library_exports_every_declared_symbol_at_header_version_126():
    """Every declared symbol is exported, and the library reports the version the header declares (126: gr_warp_f64 reads
    `fill` at infinite coordinates) -- a stale build or a header bumped without the library fails here."""
    lib = ctypes.CDLL(str(_hip.library_path()))
    for name in _declared_symbols():
        assert hasattr(lib, name), f"libgeograster.so does not export {name}"
    header = int(re.search(r"#define GR_VERSION (\d+)", (ROOT / "include" / "geograster.h").read_text()).group(1))
    lib.gr_version.restype = ctypes.c_int
    assert lib.gr_version() == header == 126


def _header_enumerators():
    """{name: value} of every enumerator of every `enum { ... }` in include/geograster.h."""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "geograster.h").read_text(), flags=re.S)
    found = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, re.S):
        for item in filter(None, (x.strip() for x in body.split(","))):
            name, value = re.fullmatch(r"(GR_\w+)\s*=\s*(-?\d+)", item).groups()
            assert name not in found, name
            found[name] = int(value)
    return found


def test_binding_constants_are_the_header_enumerators():
    """Every enumerator of the header is a module constant of the binding with the same value, and the binding has no GR_*
    integer the header does not define (GR_CAM_FLOATS is the header's one #define among them): a name missing on either side
    fails, so does a value that moved on one side only."""
    header = _header_enumerators()
    assert len(header) >= 35 and header["GR_EOVERFLOW"] == -6 and header["GR_VAR_NO_LOOK"] == 16384
    text = (ROOT / "include" / "geograster.h").read_text()
    header["GR_CAM_FLOATS"] = int(re.search(r"#define GR_CAM_FLOATS (\d+)", text).group(1))
    binding = {k: v for k, v in vars(_hip).items() if k.startswith("GR_") and isinstance(v, int)}
    assert sorted(binding) == sorted(header)
    assert binding == header


def _header_struct(name):
    """[(field, C type)] of `typedef struct <name> { ... }` in include/geograster.h."""
    text = (ROOT / "include" / "geograster.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(m.group(2), m.group(1)) for m in re.finditer(r"\b(int64_t|int32_t|float|double)\s+(\w+)\s*;", body)]


C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}


@pytest.mark.parametrize("struct,mirror", [("gr_raster_stats", _hip.RasterStats), ("gr_stage_times", _hip.StageTimes)])
def test_binding_structures_mirror_the_header(struct, mirror):
    """The library WRITES these structures through the caller's pointer: a binding with a shorter mirror is a buffer overrun."""
    want = [(n, C_TYPES[t]) for n, t in _header_struct(struct)]
    assert len(want) >= 8
    assert [(n, t) for n, t in mirror._fields_] == want


def test_integration_stub_structure_mirrors_the_header():
    """... and so is the reference-side stub of INTEGRATION.md (executed as written by tests/test_integration_stub.py on the GPU)."""
    text = (ROOT / "INTEGRATION.md").read_text()
    block = re.search(r"class Stats\(ctypes.Structure\):.*?_fields_ = (.*?)\n\s*stats, v0", text, re.S).group(1)
    fields = eval(block.replace("\\\n", " "), {"ctypes": ctypes})
    assert fields == [(n, C_TYPES[t]) for n, t in _header_struct("gr_raster_stats")]


def test_no_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _hip.HipRaster()
    from geograypher_amd.meshes import TexturedPhotogrammetryMesh
    from geograypher_amd.utils import synthetic

    (mesh, _colors) = synthetic.make_simple_mesh([], None)
    tm = TexturedPhotogrammetryMesh(mesh, log_level="ERROR")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.pix2face(synthetic.make_simple_camera_set(), apply_distortion=False)


def test_product_never_imports_the_oracle():
    for path in (ROOT / "geograypher_amd").rglob("*.py"):
        text = path.read_text()
        assert "import oracle" not in text and "from oracle" not in text, path


def test_overflow_causes_is_bound_and_answers_without_a_device():
    """gr_raster_overflow_causes (header <-> export <-> binding): bound with the declared signature; it only reads the context
    on the host, so a null context answers 0 without a GPU."""
    text = (ROOT / "include" / "geograster.h").read_text()
    assert re.search(r"\bint gr_raster_overflow_causes\(const gr_ctx \*ctx\);", text)
    assert "gr_raster_overflow_causes" in _hip.EXPORTED_SYMBOLS
    lib = _hip.load_library()
    assert lib.gr_raster_overflow_causes.restype is ctypes.c_int
    assert lib.gr_raster_overflow_causes.argtypes == [ctypes.c_void_p]
    assert lib.gr_raster_overflow_causes(None) == 0
