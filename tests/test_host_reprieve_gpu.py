"""Runs the C++ plugin mirror's reprieve driver (tests/cpp/host_plugin_reprieve_test.cpp): KubeThrottler::Preempt(reprieve) against
the walk by delete + ReconcileAll + PreFilter on a twin plugin, and — here — the victim NAMES it prints against the manifest
model (``paging.preempt_of(reprieve=True)`` on the snapshot of the same 20-pod scenario written as manifests)."""
import os
import re
import subprocess

import pytest

import preempt_reference as PR
from kube_throttler_amd import paging
from test_host_preempt_gpu import scenario

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")


def model_answers(cs, reprieve=True):
    names = [p["metadata"]["name"] for p in cs.pods]
    assert len(names) == 20
    snap = cs.build_pages()[0].snapshot
    ctx = paging.preempt_context(snap, PR.NOW)
    up = [f"r{i:02d}" for i in range(16)]
    lists = {"up": up, "down": up[::-1], "web": ["r03", "r07", "r11"], "empty": []}

    def answer(pod, lst):
        cands = [names.index(c) for c in lists[lst]]
        prefix, victims = paging.preempt_of(snap, names.index(pod), cands, PR.NOW, False, ctx=ctx, reprieve=reprieve)
        if prefix <= 0:
            return "none" if prefix < 0 else "pass"
        return ",".join(c for c, v in zip(lists[lst], victims) if v)

    return answer


def test_host_plugin_reprieve():
    exe = os.path.join(HOST, "host_plugin_reprieve_test")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", HOST, "host_plugin_reprieve_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    lines = re.findall(r"^REPRIEVE (\S+) (\S+) -> (\S+)$", r.stdout, re.M)
    answer, whole = model_answers(scenario()), model_answers(scenario(), reprieve=False)
    assert {(p, lst) for p, lst, _ in lines} == {("cpu2", "up"), ("cpu2", "down"), ("gpu2", "up"), ("gpu2", "down"), ("huge", "up"),
                                                 ("free", "up"), ("cpu2", "web"), ("gpu2", "empty")}
    for pod, lst, got in lines:
        assert got == answer(pod, lst), f"{pod} over {lst}: the mirror says {got}, the manifest model {answer(pod, lst)}"
    # the scenario asks something: the walk takes somebody out of the prefix mask, and both kinds of "nothing to delete" occur
    by = {(p, lst): got for p, lst, got in lines}
    assert by[("cpu2", "up")].count(",") < whole("cpu2", "up").count(",")
    assert by[("huge", "up")] == "none" and by[("free", "up")] == "pass"
