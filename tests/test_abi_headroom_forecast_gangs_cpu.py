"""The C-ABI of the gang headroom forecast, without a GPU: the two entry points exist in the built library with the signatures
include/kt_engine.h declares, a NULL engine is refused, and the Python binding declares the same argument lists."""
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
typedef int32_t (*launch_fn)(kt_engine*, int64_t, const int64_t*, int64_t, const int64_t*, int64_t, const int64_t*, const int32_t*, int32_t,
                             int64_t, int64_t, void*);
typedef int32_t (*fetch_fn)(kt_engine*, int64_t, int64_t*, int64_t*, int32_t*, int64_t*);
int main(void) {
  launch_fn a = kt_headroom_forecast_gangs_launch;
  fetch_fn b = kt_headroom_forecast_gangs_fetch;
  /* a NULL engine is refused before anything else is looked at: the instants, the cap, the offsets */
  if (a(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0) != KT_ERR_INVALID_ARGUMENT) return 2;
  if (a(0, 3, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 3;
  if (b(0, 0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 4;
  return KT_HEADROOM_MAX_CAP == 0x7FFFFFFF && KT_FORECAST_NONE == -1 ? 0 : 1;
}
'''


def test_symbols_and_signatures(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    for name in ("kt_headroom_forecast_gangs_launch", "kt_headroom_forecast_gangs_fetch"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in E.EXPORTS
    src = tmp_path / "headroom_forecast_gangs_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "headroom_forecast_gangs_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_null_engine_is_refused_through_the_binding():
    L = E.lib()
    assert L.kt_headroom_forecast_gangs_launch(None, 0, None, 0, None, 0, None, None, 0, 1, 1, None) == -1
    assert L.kt_headroom_forecast_gangs_launch(None, -1, None, -1, None, 1, None, None, 0, 0, 0, None) == -1
    assert L.kt_headroom_forecast_gangs_fetch(None, 0, None, None, None, None) == -1


def test_binding_matches_the_header():
    L = E.lib()
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert L.kt_headroom_forecast_gangs_launch.argtypes == [p, i64, p, i64, p, i64, p, p, i32, i64, i64, p]
    assert L.kt_headroom_forecast_gangs_fetch.argtypes == [p, i64, p, p, p, p]
    for name in ("headroom_forecast_gangs_launch", "headroom_forecast_gangs_fetch", "headroom_forecast_gangs"):
        assert callable(getattr(E.Engine, name))
