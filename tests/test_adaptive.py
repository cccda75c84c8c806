"""Adaptive sampling without a GPU (dmt_render_adaptive): the C ABI declares and exports it, the binding
wraps it, and the CLI rejects bad --adaptive / --min-spp values before it creates a context."""
import subprocess
from pathlib import Path

import pytest

from test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"


def test_header_declares_render_adaptive():
    assert "dmt_render_adaptive" in declared_symbols()
    text = (ROOT / "include" / "dmt_hip.h").read_text()
    decl = text[text.index("int dmt_render_adaptive("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int dmt_render_adaptive(dmt_ctx* ctx, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, float threshold, "
                    "int x0, int y0, int x1, int y1, uint32_t* rounds, uint64_t* samples)")


def test_library_exports_render_adaptive(pkg):
    assert hasattr(pkg.load_library(), "dmt_render_adaptive")
    from cuda_optix_pathtracing_amd import binding
    assert "dmt_render_adaptive" in binding.EXPORTED_SYMBOLS
    assert callable(getattr(binding.Renderer, "render_adaptive", None))


def test_null_context_is_invalid(pkg):
    import ctypes as C
    lib = pkg.load_library()
    rounds, samples = C.c_uint32(7), C.c_uint64(7)
    rc = lib.dmt_render_adaptive(None, C.c_uint32(0), C.c_uint32(16), C.c_uint32(4), C.c_float(0.1), 0, 0, 8, 8,
                                 C.byref(rounds), C.byref(samples))
    assert rc == 1  # DMT_ERR_INVALID


def _run(*args):
    assert EXE.exists(), "run __graft_entry__.build()"
    return subprocess.run([str(EXE), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, message", [
    (("--adaptive",), "missing value"),
    (("--adaptive", "-1"), "invalid --adaptive"),
    (("--adaptive", "nan"), "invalid --adaptive"),
    (("--adaptive", "inf"), "invalid --adaptive"),
    (("--adaptive", "0.05x"), "invalid --adaptive"),
    (("--adaptive", "0.05", "--spp", "32", "--kspp", "8", "--min-spp", "64"), "invalid --min-spp"),
    (("--adaptive", "0.05", "--min-spp", "-1"), "invalid --min-spp"),
    (("--min-spp", "8"), "--min-spp needs --adaptive"),
    (("--adaptive", "0.05", "--save-partial"), "--save-partial"),
])
def test_cli_rejects_bad_adaptive_values_before_any_gpu_call(args, message):
    r = _run(*args)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "dmt_ctx_create" not in r.stderr and "Running HIP Kernel" not in r.stdout


def test_cli_help_lists_adaptive_flags():
    h = _run("--help")
    assert h.returncode == 0
    for flag in ("--adaptive <T>", "--min-spp <N>", "_spp.png"):
        assert flag in h.stdout, flag
