"""The C-ABI of the elastic gang preemption query, without a GPU: the two entry points exist in the built library with the
signatures include/kt_engine.h declares — the rule arrays between the offsets and the candidates, the flags word before the stream,
the members between the victims and the blocker —, a NULL engine is refused, and the Python binding declares the same argument
lists."""
import ctypes as C
import inspect
import os
import subprocess

from kube_throttler_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kube_throttler_amd", "csrc")

# A C compiler holds the header's declarations against these function-pointer types: an assignment of a function with another
# signature is an error under -Werror.
PROGRAM = r'''
#include "kt_engine.h"
typedef int32_t (*launch_fn)(kt_engine*, int64_t, const int64_t*, int64_t, const int64_t*, const int64_t*, const uint8_t*, int64_t, const int64_t*,
                             int64_t, int32_t, int32_t, uint32_t, void*);
typedef int32_t (*fetch_fn)(kt_engine*, int64_t, int64_t*, uint8_t*, int64_t*, int64_t*);
int main(void) {
  launch_fn a = kt_preempt_gangs_elastic_launch;
  fetch_fn b = kt_preempt_gangs_elastic_fetch;
  /* a NULL engine is refused before anything else is looked at: the offsets, the rule, the flags */
  if (a(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 2;
  if (a(0, 3, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0x2u, 0) != KT_ERR_INVALID_ARGUMENT) return 3;
  if (b(0, 0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 4;
  return KT_GANG_MEMBER_REQUIRED == 0x1u && KT_PREEMPT_REPRIEVE == 0x1u && KT_PREEMPT_NONE == -1 ? 0 : 1;
}
'''


def test_symbols_and_signatures(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    for name in ("kt_preempt_gangs_elastic_launch", "kt_preempt_gangs_elastic_fetch"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in E.EXPORTS
    src = tmp_path / "preempt_gangs_elastic_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "preempt_gangs_elastic_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_null_engine_is_refused_through_the_binding():
    L = E.lib()
    assert L.kt_preempt_gangs_elastic_launch(None, 0, None, 0, None, None, None, 0, None, 0, 0, 0, 0, None) == -1
    assert L.kt_preempt_gangs_elastic_launch(None, -1, None, -1, None, None, None, 1, None, 0, 0, 1, 2, None) == -1
    assert L.kt_preempt_gangs_elastic_fetch(None, 0, None, None, None, None) == -1


def test_binding_matches_the_header():
    L = E.lib()
    p, i64, i32, u32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
    assert L.kt_preempt_gangs_elastic_launch.argtypes == [p, i64, p, i64, p, p, p, i64, p, i64, i32, i32, u32, p]
    assert L.kt_preempt_gangs_elastic_fetch.argtypes == [p, i64, p, p, p, p]
    for name in ("preempt_gangs_elastic_launch", "preempt_gangs_elastic_fetch", "preempt_gangs_elastic"):
        assert callable(getattr(E.Engine, name))
    assert list(inspect.signature(E.Engine.preempt_gangs_elastic).parameters) == [
        "self", "pod_rows", "gang_off", "min_members", "cand_rows", "now", "required", "on_equal", "reprieve", "want_victims"]
