"""Runs the C++ plugin mirror's forecast driver (tests/cpp/host_plugin_forecast_test.cpp): KubeThrottler::RetryAfter against a
fresh twin plugin per judged instant (ReconcileAll at the instant + PreFilter), and — here — the instants and verdicts it prints
against the manifest model (``paging.override_instants_of`` and ``paging.forecast_of`` on the same scenario written as manifests)."""
import os
import re
import subprocess

import pytest

from kube_throttler_amd import paging
from kube_throttler_amd.objects import ClusterState
from kube_throttler_amd.quantity import parse_rfc3339

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")
NOW_TEXT = "2026-01-01T12:00:00Z"


def scenario() -> ClusterState:
    """The driver's scenario: a Throttle on the job label (cpu 2) with a freeze hour (cpu 500m) and a night window (cpu 10), three
    running job pods of 500m each and four pending pods."""
    cs = ClusterState()
    cs.add_namespace("ns1", {})

    def pod(name, labels, requests, running):
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": requests}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns1", "labels": labels}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})

    for i in range(3):
        pod(f"r{i}", {"app": "job"}, {"cpu": "500m"}, True)
    pod("job", {"app": "job"}, {"cpu": "1"}, False)
    pod("small", {"app": "job"}, {"cpu": "250m"}, False)
    pod("huge", {"app": "job"}, {"cpu": "20"}, False)
    pod("free", {"app": "web"}, {"cpu": "1"}, False)
    cs.add({"kind": "Throttle", "metadata": {"name": "jobs", "namespace": "ns1"},
            "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "job"}}}]},
                     "threshold": {"resourceRequests": {"cpu": "2"}},
                     "temporaryThresholdOverrides": [
                         {"begin": "2026-01-01T14:00:00Z", "end": "2026-01-01T15:00:00Z", "threshold": {"resourceRequests": {"cpu": "500m"}}},
                         {"begin": "2026-01-01T22:00:00Z", "end": "2026-01-02T06:00:00Z", "threshold": {"resourceRequests": {"cpu": "10"}}}]}})
    return cs


def model_answer(cs, pod, horizon):
    """-> (first instant as (seconds, nanoseconds) or None, verdict digits) by the manifest model."""
    names = [p["metadata"]["name"] for p in cs.pods]
    snap = cs.build_pages()[0].snapshot
    now = parse_rfc3339(NOW_TEXT)
    instants = [now] + paging.override_instants_of(snap, now, (now[0] + horizon, now[1]))
    first, verdicts = paging.forecast_of(snap, names.index(pod), instants)
    return (instants[first] if first >= 0 else None), "".join(str(v) for v in verdicts)


def test_host_plugin_retry_after():
    exe = os.path.join(HOST, "host_plugin_forecast_test")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", HOST, "host_plugin_forecast_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    lines = re.findall(r"^RETRY (\S+) (\d+) -> (\S+) (\d+)$", r.stdout, re.M)
    assert {(p, int(h)) for p, h, _, _ in lines} == {("job", 86400), ("job", 3600), ("job", 36000), ("job", 35999), ("small", 86400),
                                                     ("huge", 7 * 86400), ("free", 86400)}
    cs = scenario()
    for pod, horizon, got, digits in lines:
        want, want_digits = model_answer(cs, pod, int(horizon))
        assert digits == want_digits, f"{pod} over {horizon} s: the mirror says {digits}, the manifest model {want_digits}"
        assert (None if got == "never" else parse_rfc3339(got)) == want, f"{pod} over {horizon} s: {got}, the manifest model {want}"
    # the scenario asks something: the night window's begin, a pod that never passes, a window that just misses the begin
    by = {(p, int(h)): (got, digits) for p, h, got, digits in lines}
    assert by[("job", 86400)] == ("2026-01-01T22:00:00Z", "11101")
    assert by[("huge", 7 * 86400)][0] == "never" and by[("job", 35999)][0] == "never"
    assert by[("small", 86400)] == (NOW_TEXT, "01000") and by[("free", 86400)] == (NOW_TEXT, "00000")
