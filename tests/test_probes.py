"""CPU test of the device probes' entry points (csrc/probes.hpp): the argument check comes before anything touches HIP."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

DMT_ERR_INVALID = 1


def probe_declarations():
    """{name: [parameter text, ...]} of every dmt_test_* function include/dmt_hip.h declares"""
    text = (ROOT / "include" / "dmt_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: [p.strip() for p in params.split(",")] for name, params in re.findall(r"\bint\s+(dmt_test_[a-z0-9_]+)\s*\(([^)]*)\)", text)}


def null_argument(param):
    if "*" in param:
        return C.c_void_p(None)
    ctype = {"int": C.c_int, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "float": C.c_float}[param.split()[0]]
    return ctype(0)


def test_error_code_matches_header():
    text = (ROOT / "include" / "dmt_hip.h").read_text()
    assert int(re.search(r"\bDMT_ERR_INVALID\s*=\s*(\d+)", text).group(1)) == DMT_ERR_INVALID


def test_every_probe_rejects_a_null_context(pkg):
    """Each dmt_test_* entry point, called with a null context and every other argument null or zero, returns
    DMT_ERR_INVALID: no device is selected, nothing is allocated and nothing is dereferenced before the check."""
    from cuda_optix_pathtracing_amd import binding
    lib = pkg.load_library()
    decls = probe_declarations()
    assert sorted(decls) == sorted(s for s in binding.EXPORTED_SYMBOLS if s.startswith("dmt_test_"))
    for name, params in sorted(decls.items()):
        assert params[0] == "dmt_ctx* ctx", (name, params[0])
        fn = getattr(lib, name)
        fn.restype = C.c_int
        assert fn(*[null_argument(p) for p in params]) == DMT_ERR_INVALID, name
