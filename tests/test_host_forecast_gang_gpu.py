"""Runs the C++ plugin mirror's gang forecast driver (tests/cpp/host_plugin_forecast_gang_test.cpp): KubeThrottler::RetryAfterGang
against a fresh twin plugin per judged instant (ReconcileAll at the instant + AdmitGangs of the one gang), and — here — the
instants, verdicts and blockers it prints against the manifest model (``paging.override_instants_of`` and
``paging.forecast_gangs_of`` on the same scenario written as manifests)."""
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
NIGHT = "2026-01-01T22:00:00Z"


def scenario() -> ClusterState:
    """The driver's scenario: a Throttle on the job label (cpu 2) with a freeze hour (cpu 500m) and a night window (cpu 10), three
    running job pods of 500m each and five pending pods, two of them small job pods that only fit together at night."""
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
    pod("small2", {"app": "job"}, {"cpu": "300m"}, False)
    pod("huge", {"app": "job"}, {"cpu": "20"}, False)
    pod("free", {"app": "web"}, {"cpu": "1"}, False)
    cs.add({"kind": "Throttle", "metadata": {"name": "jobs", "namespace": "ns1"},
            "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "job"}}}]},
                     "threshold": {"resourceRequests": {"cpu": "2"}},
                     "temporaryThresholdOverrides": [
                         {"begin": "2026-01-01T14:00:00Z", "end": "2026-01-01T15:00:00Z", "threshold": {"resourceRequests": {"cpu": "500m"}}},
                         {"begin": "2026-01-01T22:00:00Z", "end": "2026-01-02T06:00:00Z", "threshold": {"resourceRequests": {"cpu": "10"}}}]}})
    return cs


def model_answer(cs, members, horizon):
    """-> (first instant as (seconds, nanoseconds) or None, verdict digits, blocker names) by the manifest model."""
    names = [p["metadata"]["name"] for p in cs.pods]
    snap = cs.build_pages()[0].snapshot
    now = parse_rfc3339(NOW_TEXT)
    instants = [now] + paging.override_instants_of(snap, now, (now[0] + horizon, now[1]))
    first, verdicts, blockers = paging.forecast_gangs_of(snap, [names.index(m) for m in members], instants)
    return (instants[first] if first >= 0 else None), "".join(str(v) for v in verdicts), ",".join("-" if b < 0 else members[b] for b in blockers)


def test_host_plugin_retry_after_gang():
    exe = os.path.join(HOST, "host_plugin_forecast_gang_test")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", HOST, "host_plugin_forecast_gang_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    lines = re.findall(r"^RETRYGANG (\S+) (\d+) -> (\S+) (\d+) (\S+)$", r.stdout, re.M)
    assert {(m, int(h)) for m, h, _, _, _ in lines} == {
        ("small+small2", 86400), ("small2+small", 86400), ("small+small2", 3600), ("small+small2", 36000), ("small+small2", 35999),
        ("small", 86400), ("small+free", 86400), ("small+huge+small2", 7 * 86400), ("job+small+small2", 86400)}
    cs = scenario()
    for members, horizon, got, digits, blockers in lines:
        want, want_digits, want_blockers = model_answer(cs, members.split("+"), int(horizon))
        assert digits == want_digits, f"{members} over {horizon} s: the mirror says {digits}, the manifest model {want_digits}"
        assert blockers == want_blockers, f"{members} over {horizon} s: the mirror says {blockers}, the manifest model {want_blockers}"
        assert (None if got == "never" else parse_rfc3339(got)) == want, f"{members} over {horizon} s: {got}, the manifest model {want}"
    # the scenario asks something: the job passes only from the night window's begin while each member alone passes now, the
    # blocker depends on the order and on the instant, a window that just misses the begin
    by = {(m, int(h)): (got, digits, blockers) for m, h, got, digits, blockers in lines}
    assert by[("small+small2", 86400)] == (NIGHT, "11101", "small2,small,small2,-,small2")
    assert by[("small2+small", 86400)] == (NIGHT, "11101", "small,small2,small,-,small")
    assert by[("small", 86400)] == (NOW_TEXT, "01000", "-,small,-,-,-")
    assert by[("small+small2", 35999)][0] == "never" and by[("small+huge+small2", 7 * 86400)][0] == "never"
    names = [p["metadata"]["name"] for p in cs.pods]
    snap = cs.build_pages()[0].snapshot
    now = parse_rfc3339(NOW_TEXT)
    for m in ("small", "small2"):
        assert paging.forecast_of(snap, names.index(m), [now])[0] == 0
