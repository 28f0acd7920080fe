"""make_pack_plan with 9 bits of headroom (the two-per-CU aggregate scan's up to 512 slabs): tests/cpp/pack_plan_headroom_test.cpp
sums worst-case slabs class by class, as the slab reductions do, and compares with exact sums."""
import os
import subprocess

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kube_throttler_amd", "host")


def test_pack_plans_with_nine_bits_of_headroom():
    from kube_throttler_amd import engine
    engine.build()
    subprocess.check_call(["make", "-C", HOST, "pack_plan_headroom_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "pack_plan_headroom_test")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout.splitlines()[-1]
