"""Runs the C++ plugin mirror's gang headroom driver (tests/cpp/host_plugin_headroom_gang_test.cpp): KubeThrottler::HeadroomGang
against counting AdmitGangs of fresh same-shape replicas on a twin plugin, and — here — the copies, limiting throttles and
blockers it prints against ``paging.headroom_gangs_of`` on the same scenario written as manifests (status written back by a
reconcile, as the driver's ReconcileAll does)."""
import os
import re
import subprocess

import pytest

from kube_throttler_amd import paging
from kube_throttler_amd.objects import ClusterState
from test_paged_admit_cpu import write_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")


def scenario() -> ClusterState:
    """The driver's scenario: a Throttle on the job label (cpu 4) with three running job pods of 500m each, a Throttle on the
    worker role (7 pods); a launcher (250m), two workers (300m each), a pod that exceeds the threshold, one no throttle affects
    and one in a namespace without a Namespace object."""
    cs = ClusterState()
    cs.add_namespace("ns1", {})

    def pod(name, labels, requests, running, ns="ns1"):
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": requests}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": ns, "labels": labels}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})

    for i in range(3):
        pod(f"r{i}", {"app": "job"}, {"cpu": "500m"}, True)
    pod("launcher", {"app": "job"}, {"cpu": "250m"}, False)
    pod("w1", {"app": "job", "role": "worker"}, {"cpu": "300m"}, False)
    pod("w2", {"app": "job", "role": "worker"}, {"cpu": "300m"}, False)
    pod("huge", {"app": "job"}, {"cpu": "20"}, False)
    pod("free", {"app": "web"}, {"cpu": "1"}, False)
    pod("ghost", {"app": "job"}, {"cpu": "100m"}, False, ns="ghost")
    for name, label, threshold in (("jobs", {"app": "job"}, {"resourceRequests": {"cpu": "4"}}),
                                   ("few", {"role": "worker"}, {"resourceCounts": {"pod": 7}})):
        cs.add({"kind": "Throttle", "metadata": {"name": name, "namespace": "ns1"},
                "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": label}}]},
                         "threshold": threshold}})
    return cs


def test_host_plugin_headroom_gang(oracle_mod):
    exe = os.path.join(HOST, "host_plugin_headroom_gang_test")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", HOST, "host_plugin_headroom_gang_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout  # ... the "pages" error of a mirror on two pages among them
    lines = re.findall(r"^HEADROOMGANG (\S+) (\d+) -> (\d+) (\S+) (\S+)$", r.stdout, re.M)
    assert {(m, int(c)) for m, c, _, _, _ in lines} == {
        ("launcher+w1+w2", 10), ("w2+w1+launcher", 10), ("w1+w2", 10), ("launcher+w1+w2", 2), ("launcher", 50), ("launcher+free", 50),
        ("launcher+huge+w1", 10), ("launcher+ghost+huge", 10), ("huge+ghost", 10)}
    cs = scenario()
    write_status(cs, oracle_mod)
    page = cs.build_pages()[0]
    names = [p["metadata"]["name"] for p in cs.pods]
    for members, cap, copies, limiting, blocker in lines:
        members = members.split("+")
        want = paging.headroom_gangs_of(page.snapshot, [names.index(m) for m in members], int(cap))
        got = (int(copies), -1 if limiting == "-" else page.thr_names.index(limiting), -1 if blocker == "-" else members.index(blocker))
        assert got == want, f"{members} cap {cap}: the mirror says {got}, the manifest model {want}"
    # the scenario asks something: the order decides the blocker, the pod count decides for the workers alone, the cap, an Error
    by = {(m, int(c)): (int(copies), limiting, blocker) for m, c, copies, limiting, blocker in lines}
    assert by[("launcher+w1+w2", 10)] == (2, "ns1/jobs", "w2") and by[("w2+w1+launcher", 10)] == (2, "ns1/jobs", "launcher")
    assert by[("w1+w2", 10)] == (3, "ns1/few", "w2") and by[("launcher+w1+w2", 2)] == (2, "-", "-")
    assert by[("launcher+ghost+huge", 10)] == (0, "-", "ghost") and by[("huge+ghost", 10)] == (0, "ns1/jobs", "huge")
