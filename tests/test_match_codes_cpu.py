"""The match-code record (kube_throttler_amd/csrc/kt_match_codes.h: 16 bytes per pod row, a count and up to 15 codes k << 6 | bit,
0xFF for "more than 15"): tests/cpp/match_codes_test.cpp round-trips every count 0..15, checks the overflow header from 16 codes on,
ascending order, and the run rule on hand-made and random masks against a bit-by-bit restatement.  The program is the header alone
with a main of its own, built and run under -fsanitize=address,undefined."""
import os
import subprocess

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kube_throttler_amd", "host")


def test_match_codes_helpers_under_sanitizers():
    subprocess.check_call(["make", "-C", HOST, "match_codes_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "match_codes_test")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.splitlines()[-1] == "match_codes_test: ok"
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
