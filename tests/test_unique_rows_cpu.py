"""kt::unique_rows (kube_throttler_amd/csrc/kt_rows.h), which makes the row list of kt_delete_pods unique before an incremental
engine's delta scan gathers through it: tests/cpp/unique_rows_test.cpp compares it with std::set — empty, one entry, ascending lists
(returned in place, nothing allocated), descending, all equal, 8193 entries over 300 rows, row 0 and the last row of the capacity."""
import os
import subprocess

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kube_throttler_amd", "host")


def test_unique_rows_against_std_set():
    subprocess.check_call(["make", "-C", HOST, "unique_rows_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "unique_rows_test")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout.splitlines()[-1]
