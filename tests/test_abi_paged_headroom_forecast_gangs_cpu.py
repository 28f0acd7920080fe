"""The C-ABI of the gang headroom forecast over pages, without a GPU: kt_paged_headroom_forecast_gangs exists in the built library
with the signature include/kt_engine.h declares, a missing page array / no pages / a negative count / a NULL page is refused
before any page is looked at, and the Python binding declares the same argument list."""
import ctypes as C
import os
import subprocess

from kube_throttler_amd import engine as E, paging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kube_throttler_amd", "csrc")

# A C compiler holds the header's declaration against this function-pointer type: an assignment of a function with another
# signature is an error under -Werror.
PROGRAM = r'''
#include "kt_engine.h"
typedef int32_t (*paged_fn)(kt_engine* const*, int32_t, int64_t, const int64_t*, int64_t, const int64_t*, int64_t, const int64_t*,
                            const int32_t*, int32_t, int64_t, int64_t, int64_t*, int64_t*, int32_t*, int64_t*);
int main(void) {
  paged_fn f = kt_paged_headroom_forecast_gangs;
  kt_engine* none[1] = {0};
  int64_t s[1] = {0}, off[1] = {0};
  int32_t ns[1] = {0};
  /* refused before a page is looked at: the array is missing, there is no page, a count is negative */
  if (f(0, 1, 0, 0, 0, off, 1, s, ns, 0, 1, 1, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 2;
  if (f(none, 0, 0, 0, 0, off, 1, s, ns, 0, 1, 1, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 3;
  if (f(none, -1, 0, 0, 0, off, 1, s, ns, 0, 1, 1, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 4;
  if (f(none, 1, -1, 0, 0, off, 1, s, ns, 0, 1, 1, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 5;
  if (f(none, 1, 0, 0, -1, off, 1, s, ns, 0, 1, 1, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 6;
  /* ... and a page that is NULL */
  if (f(none, 1, 0, 0, 0, off, 1, s, ns, 0, 1, 1, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 7;
  return KT_HEADROOM_MAX_CAP == 0x7FFFFFFF && KT_FORECAST_NONE == -1 ? 0 : 1;
}
'''


def test_symbol_and_signature(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    assert hasattr(lib, "kt_paged_headroom_forecast_gangs"), "kt_paged_headroom_forecast_gangs is not exported"
    assert "kt_paged_headroom_forecast_gangs" in E.EXPORTS
    src = tmp_path / "paged_headroom_forecast_gangs_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "paged_headroom_forecast_gangs_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_bad_page_sets_are_refused_through_the_binding():
    L = E.lib()
    none = (C.c_void_p * 1)(None)
    s, ns, off = (C.c_int64 * 1)(0), (C.c_int32 * 1)(0), (C.c_int64 * 1)(0)
    sp, nsp, op = C.cast(s, C.c_void_p), C.cast(ns, C.c_void_p), C.cast(off, C.c_void_p)
    f = L.kt_paged_headroom_forecast_gangs
    assert f(None, 1, 0, None, 0, op, 1, sp, nsp, 0, 1, 1, None, None, None, None) == -1
    assert f(none, 0, 0, None, 0, op, 1, sp, nsp, 0, 1, 1, None, None, None, None) == -1
    assert f(none, 1, -1, None, 0, op, 1, sp, nsp, 0, 1, 1, None, None, None, None) == -1
    assert f(none, 1, 0, None, -1, op, 1, sp, nsp, 0, 1, 1, None, None, None, None) == -1
    assert f(none, 1, 0, None, 0, op, 1, sp, nsp, 0, 1, 1, None, None, None, None) == -1


def test_binding_matches_the_header():
    L = E.lib()
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert L.kt_paged_headroom_forecast_gangs.argtypes == [C.POINTER(p), i32, i64, p, i64, p, i64, p, p, i32, i64, i64, p, p, p, p]
    assert callable(E.paged_headroom_forecast_gangs) and callable(paging.PagedEngine.headroom_forecast_gangs)
    assert callable(paging.paged_headroom_forecast_gangs_of)
