"""The C-ABI of the gang reprieve pass, without a GPU: the entry point exists in the built library with the signature
include/kt_engine.h declares — that of kt_preempt_gangs_launch —, a NULL engine and negative counts are refused, and the Python
binding declares the same argument list."""
import ctypes as C
import inspect
import os
import subprocess

from kube_throttler_amd import engine as E
from kube_throttler_amd import paging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kube_throttler_amd", "csrc")

# A C compiler holds the header's declarations against this function-pointer type: an assignment of a function with another
# signature is an error under -Werror.
PROGRAM = r'''
#include "kt_engine.h"
typedef int32_t (*launch_fn)(kt_engine*, int64_t, const int64_t*, int64_t, const int64_t*, int64_t, const int64_t*, int64_t, int32_t, int32_t,
                             void*);
int main(void) {
  launch_fn a = kt_preempt_gangs_reprieve_launch;
  launch_fn plain = kt_preempt_gangs_launch;
  /* a NULL engine is refused before anything else is looked at, exactly as the plain gang launch refuses it */
  if (a(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 2;
  if (plain(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != KT_ERR_INVALID_ARGUMENT) return 3;
  return KT_PREEMPT_NONE == -1 ? 0 : 1;
}
'''


def test_symbol_and_signature(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    assert hasattr(lib, "kt_preempt_gangs_reprieve_launch"), "kt_preempt_gangs_reprieve_launch is not exported"
    assert "kt_preempt_gangs_reprieve_launch" in E.EXPORTS
    src = tmp_path / "preempt_gangs_reprieve_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "preempt_gangs_reprieve_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_the_header_states_the_definition():
    text = open(os.path.join(ROOT, "include", "kt_engine.h")).read()
    assert "int32_t kt_preempt_gangs_reprieve_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off" in text
    assert "Out of scope: a reprieve pass for gangs" not in text


def test_binding_matches():
    L = E.lib()
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert L.kt_preempt_gangs_reprieve_launch.argtypes == [p, i64, p, i64, p, i64, p, i64, i32, i32, p]
    assert L.kt_preempt_gangs_reprieve_launch.argtypes == L.kt_preempt_gangs_launch.argtypes
    assert callable(E.Engine.preempt_gangs_reprieve_launch)
    # the walk is opt-in on both sides: the default keeps what the calls answered before
    assert inspect.signature(E.Engine.preempt_gangs).parameters["reprieve"].default is False
    assert inspect.signature(paging.preempt_gangs_of).parameters["reprieve"].default is False
