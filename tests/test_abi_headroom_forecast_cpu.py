"""The C-ABI of the headroom forecast, without a GPU: both entry points exist in the built library with the signatures
include/kt_engine.h declares, and the Python binding declares the same argument lists."""
import ctypes as C
import os
import subprocess

from kube_throttler_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kube_throttler_amd", "csrc")

# A C compiler holds the header's declarations against these function-pointer types: an assignment of a function with another
# signature is an error under -Werror.
PROGRAM = r'''
#include "kt_engine.h"
typedef int32_t (*launch_fn)(kt_engine*, int64_t, const int64_t*, int64_t, const int64_t*, const int32_t*, int32_t, int64_t, int64_t, void*);
typedef int32_t (*fetch_fn)(kt_engine*, int64_t, int64_t*, int64_t*, int32_t*);
int main(void) {
  launch_fn a = kt_headroom_forecast_launch;
  fetch_fn b = kt_headroom_forecast_fetch;
  /* a NULL engine is refused before anything else is looked at */
  if (a(0, 0, 0, 1, 0, 0, 0, 1, 1, 0) != KT_ERR_INVALID_ARGUMENT) return 2;
  if (b(0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 3;
  return KT_FORECAST_NONE == -1 && KT_HEADROOM_MAX_CAP == 0x7FFFFFFF ? 0 : 1;
}
'''


def test_symbols_and_signatures(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    for name in ("kt_headroom_forecast_launch", "kt_headroom_forecast_fetch"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in E.EXPORTS
    src = tmp_path / "headroom_forecast_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "headroom_forecast_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_binding_matches():
    L = E.lib()
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert L.kt_headroom_forecast_launch.argtypes == [p, i64, p, i64, p, p, i32, i64, i64, p]
    assert L.kt_headroom_forecast_fetch.argtypes == [p, i64, p, p, p]
    for name in ("headroom_forecast_launch", "headroom_forecast_fetch", "headroom_forecast"):
        assert callable(getattr(E.Engine, name))
