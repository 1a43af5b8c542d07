"""scpr_decompress_streams at the C boundary, without a GPU: include/scpr_amd.h compiles from a C and a C++ caller that fill a
scpr_decode_call array, the library exports the entry point, and the whole-call refusals that need no device answer SCPR_E_PARAM."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "screenpressor_amd", "libscpr_amd.so")

# one source, compiled as C and as C++: the refusals that come before any device is touched, and the struct's layout
CALLER = r"""
#include <stdio.h>
#include <string.h>
#include "scpr_amd.h"

int main(void) {
    scpr_decode_call calls[2];
    uint32_t sizes[1] = {0};
    int ftypes[1] = {0};
    memset(calls, 0, sizeof(calls));
    calls[0].codec = NULL;
    calls[0].d_packets = sizes;
    calls[0].sizes = sizes;
    calls[0].ftypes = ftypes;
    calls[0].nframes = 1;
    calls[0].d_frames_out = ftypes;
    calls[0].pitch = 4;
    calls[0].result = 7;
    calls[1] = calls[0];
    int a = scpr_decompress_streams(NULL, 1);
    int b = scpr_decompress_streams(calls, -1);
    int c = scpr_decompress_streams(calls, 0);
    int d = scpr_decompress_streams(calls, 2); /* NULL codecs */
    printf("%d %d %d %d %d %d\n", a, b, c, d, calls[0].result, (int)sizeof(scpr_decode_call));
    return 0;
}
"""


def _compile(tmp_path, cxx):
    src = tmp_path / ("caller.cpp" if cxx else "caller.c")
    src.write_text(CALLER)
    exe = str(tmp_path / ("caller_cxx" if cxx else "caller_c"))
    cc = ["g++", "-std=c++14"] if cxx else ["gcc", "-std=c99"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", os.path.dirname(LIB), "-lscpr_amd",
                                "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,--allow-shlib-undefined"])
    return exe


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "scpr_amd.h")).read()
    assert "scpr_decode_call" in text and "int scpr_decompress_streams(scpr_decode_call* calls, int ncalls);" in text


@pytest.mark.skipif(not os.path.exists(LIB), reason="HIP library not built (run python __graft_entry__.py)")
def test_library_exports_the_call():
    import torch  # noqa: F401  (one HIP runtime per process: see screenpressor_amd/codec.py)
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "scpr_decompress_streams")
    from screenpressor_amd import codec
    assert "scpr_decompress_streams" in codec.EXPORTS


@pytest.mark.skipif(not os.path.exists(LIB), reason="HIP library not built (run python __graft_entry__.py)")
@pytest.mark.parametrize("cxx", [False, True], ids=["c", "cxx"])
def test_c_and_cxx_callers_compile_link_and_are_refused_without_a_device(tmp_path, cxx):
    exe = _compile(tmp_path, cxx)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    a, b, c, d, result, size = (int(x) for x in out.stdout.split())
    # SCPR_E_PARAM for NULL / ncalls < 0 / NULL codecs, SCPR_OK for none; a refused call leaves `result` alone
    assert (a, b, c, d, result) == (-2, -2, 0, -2, 7)
    assert size == 8 + 8 + 8 + 8 + 4 + 4 + 8 + 4 + 4  # (the layout ScprDecodeCall mirrors)


@pytest.mark.skipif(not os.path.exists(LIB), reason="HIP library not built (run python __graft_entry__.py)")
def test_python_struct_matches_the_header():
    from screenpressor_amd.codec import ScprDecodeCall, load_library
    assert ctypes.sizeof(ScprDecodeCall) == 56
    L = load_library()
    assert L.scpr_decompress_streams(None, 1) == -2
    arr = (ScprDecodeCall * 1)()
    assert L.scpr_decompress_streams(arr, -1) == -2
    assert L.scpr_decompress_streams(arr, 0) == 0
    assert L.scpr_decompress_streams(arr, 1) == -2  # (a NULL codec)
