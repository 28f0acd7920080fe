"""Runs tests/cpp/host_plugin_namespace_test.cpp: the C++ plugin mirror lives through Namespace events — a Throttle and pods
before their Namespace object, the object afterwards, an update of its labels, its delete, the delete of an unknown name, its
return — and is held at every checkpoint to a twin built in one go from the state it has reached; on one page and on two."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kube_throttler_amd", "host")


def test_host_plugin_namespace_events():
    subprocess.check_call(["make", "-C", HOST, "host_plugin_namespace_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "host_plugin_namespace_test")], capture_output=True, text=True, timeout=180)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
