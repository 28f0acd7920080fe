"""Runs tests/cpp/host_plugin_pages_test.cpp: the C++ plugin mirror with more than 16 resource names — pages created as
names arrive (one after a ReconcileAll), held to a twin that registered every name up front."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kube_throttler_amd", "host")


def test_host_plugin_pages():
    subprocess.check_call(["make", "-C", HOST, "host_plugin_pages_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "host_plugin_pages_test")], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
