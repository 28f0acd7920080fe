"""The C-ABI of the admission forecast, without a GPU: the three entry points exist in the built library with the signatures
include/kt_engine.h declares, the Python binding declares the same argument lists, and the header constant is Python's."""
import ctypes as C
import os
import re
import subprocess

from kube_throttler_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kube_throttler_amd", "csrc")

# A C compiler holds the header's declarations against these function-pointer types: an assignment of a function with another
# signature is an error under -Werror.
PROGRAM = r'''
#include "kt_engine.h"
typedef int32_t (*launch_fn)(kt_engine*, int64_t, const int64_t*, int64_t, const int64_t*, const int32_t*, int32_t, void*);
typedef int32_t (*fetch_fn)(kt_engine*, int64_t, int64_t*, uint8_t*);
typedef int32_t (*instants_fn)(kt_engine*, int64_t, int32_t, int64_t, int32_t, int64_t, int64_t*, int32_t*, int64_t*);
int main(void) {
  launch_fn a = kt_forecast_launch;
  fetch_fn b = kt_forecast_fetch;
  instants_fn c = kt_override_instants;
  /* a NULL engine is refused before anything else is looked at */
  if (a(0, 0, 0, 1, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 2;
  if (b(0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 3;
  if (c(0, 0, 0, 0, 0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 4;
  return KT_FORECAST_NONE == -1 ? 0 : 1;
}
'''


def test_symbols_signatures_and_constant(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    for name in ("kt_forecast_launch", "kt_forecast_fetch", "kt_override_instants"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in E.EXPORTS
    src = tmp_path / "forecast_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "forecast_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_header_constant_and_binding_match():
    with open(os.path.join(ROOT, "include", "kt_engine.h")) as fh:
        text = fh.read()
    m = re.search(r"#define\s+KT_FORECAST_NONE\s+\((-?\d+)\)", text)
    assert m and int(m.group(1)) == E.FORECAST_NONE == -1
    L = E.lib()
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert L.kt_forecast_launch.argtypes == [p, i64, p, i64, p, p, i32, p]
    assert L.kt_forecast_fetch.argtypes == [p, i64, p, p]
    assert L.kt_override_instants.argtypes == [p, i64, i32, i64, i32, i64, p, p, C.POINTER(i64)]
    for name in ("forecast_launch", "forecast_fetch", "forecast", "override_instants"):
        assert callable(getattr(E.Engine, name))
