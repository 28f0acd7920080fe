"""Runs the C++ plugin mirror's preemption driver (tests/cpp/host_plugin_preempt_test.cpp): KubeThrottler::Preempt against
delete + ReconcileAll + PreFilter on a twin plugin, and — here — the victim NAMES it prints against the manifest model
(``paging.preempt_of`` on the snapshot of the same 20-pod scenario written as manifests)."""
import os
import re
import subprocess

import pytest

import preempt_reference as PR
from kube_throttler_amd import paging
from kube_throttler_amd.objects import ClusterState

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")


def scenario() -> ClusterState:
    """The driver's scenario: 16 pods on a node (r03, r07, r11, r15 are web pods, the even ones of the batch tier, every fourth
    holds a gpu, r05 has finished, r10 belongs to another scheduler), 4 pending pods, a Throttle on the job label (12 pods, 6 cpu)
    and a ClusterThrottle on the batch tier (4 gpus)."""
    cs = ClusterState()
    cs.add_namespace("ns1", {})

    def pod(name, labels, requests, running, phase=None, scheduler="my-scheduler"):
        spec = {"schedulerName": scheduler, "containers": [{"name": "c", "resources": {"requests": requests}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns1", "labels": labels}, "spec": spec,
                "status": {"phase": phase or ("Running" if running else "Pending")}})

    for i in range(16):
        labels = {"app": "web" if i % 4 == 3 else "job"}
        if i % 2 == 0:
            labels["tier"] = "batch"
        requests = {"cpu": f"{(i % 3 + 1) * 500}m"}
        if i % 4 == 0:
            requests["amd.com/gpu"] = "1"
        pod(f"r{i:02d}", labels, requests, True, "Succeeded" if i == 5 else None, "default-scheduler" if i == 10 else "my-scheduler")
    pod("cpu2", {"app": "job"}, {"cpu": "2"}, False)
    pod("gpu2", {"app": "job", "tier": "batch"}, {"cpu": "500m", "amd.com/gpu": "2"}, False)
    pod("huge", {"app": "job"}, {"cpu": "8"}, False)
    pod("free", {"app": "web"}, {"cpu": "1"}, False)
    cs.add({"kind": "Throttle", "metadata": {"name": "jobs", "namespace": "ns1"},
            "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "job"}}}]},
                     "threshold": {"resourceCounts": {"pod": 12}, "resourceRequests": {"cpu": "6"}}}})
    cs.add({"kind": "ClusterThrottle", "metadata": {"name": "gpus"},
            "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"tier": "batch"}}}]},
                     "threshold": {"resourceRequests": {"amd.com/gpu": "4"}}}})
    return cs


def model_answers(cs):
    names = [p["metadata"]["name"] for p in cs.pods]
    assert len(names) == 20
    snap = cs.build_pages()[0].snapshot
    ctx = paging.preempt_context(snap, PR.NOW)
    up = [f"r{i:02d}" for i in range(16)]
    lists = {"up": up, "down": up[::-1], "web": ["r03", "r07", "r11"], "empty": []}

    def answer(pod, lst):
        cands = [names.index(c) for c in lists[lst]]
        prefix, victims = paging.preempt_of(snap, names.index(pod), cands, PR.NOW, False, ctx=ctx)
        if prefix <= 0:
            return "none" if prefix < 0 else "pass"
        return ",".join(c for c, v in zip(lists[lst], victims) if v)

    return answer


def test_host_plugin_preempt():
    exe = os.path.join(HOST, "host_plugin_preempt_test")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", HOST, "host_plugin_preempt_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    lines = re.findall(r"^PREEMPT (\S+) (\S+) -> (\S+)$", r.stdout, re.M)
    answer = model_answers(scenario())
    assert {(p, lst) for p, lst, _ in lines} == {("cpu2", "up"), ("cpu2", "down"), ("gpu2", "up"), ("gpu2", "down"), ("huge", "up"),
                                                 ("free", "up"), ("cpu2", "web"), ("gpu2", "empty")}
    for pod, lst, got in lines:
        assert got == answer(pod, lst), f"{pod} over {lst}: the mirror says {got}, the manifest model {answer(pod, lst)}"
    # the scenario asks something: several victims, a different set per order, and both kinds of "nothing to delete"
    by = {(p, lst): got for p, lst, got in lines}
    assert by[("cpu2", "up")].count(",") >= 1 and by[("cpu2", "up")] != by[("cpu2", "down")]
    assert by[("huge", "up")] == "none" and by[("free", "up")] == "pass"
