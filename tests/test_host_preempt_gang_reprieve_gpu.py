"""Runs the C++ plugin mirror's gang reprieve driver (tests/cpp/host_plugin_preempt_gang_reprieve_test.cpp):
KubeThrottler::PreemptGang(reprieve) against the walk by delete + ReconcileAll + AdmitGangs on a twin plugin, and — here — the
victim NAMES it prints against the directed table of tests/preempt_gangs_reprieve_reference.py and the model
(``paging.preempt_gangs_of(reprieve=True)`` on the snapshots of the same two scenarios)."""
import os
import re
import subprocess

import pytest

import preempt_gangs_reprieve_reference as GRR
import preempt_reference as PR
from kube_throttler_amd import paging

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")
SCENARIOS = ("gang-one-one-six", "reserved-prefix-keeps-victims")


def _names(cands, prefix, victims):
    if prefix <= 0:
        return "none" if prefix < 0 else "pass"
    return ",".join(f"p{c}" for c, v in zip(cands, victims) if v)


def test_host_plugin_preempt_gang_reprieve():
    exe = os.path.join(HOST, "host_plugin_preempt_gang_reprieve_test")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", HOST, "host_plugin_preempt_gang_reprieve_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    by = {(s, kind): got for s, kind, got in re.findall(r"^GANGREPRIEVE (\S+) (\S+) -> (\S+)$", r.stdout, re.M)}
    assert {s for s, _ in by} == set(SCENARIOS)
    for name in SCENARIOS:
        build, prefixes, victims = GRR.DIRECTED[name]
        snap, ms, cands = build()
        # PreFilter's isThrottledOnEqual is false: the table's first column
        assert by[(name, "walk")] == _names(cands, prefixes[0], victims[0]), name
        k, v, _ = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, False, reprieve=True)
        assert by[(name, "walk")] == _names(cands, k, v), name
        k, v, _ = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, False)
        assert by[(name, "plain")] == _names(cands, k, v), name  # the default call is unchanged
    # the scenarios ask something: somebody is reprieved, and the members' own sets do not make up the gang's
    assert by[("gang-one-one-six", "walk")] == "p5" and by[("gang-one-one-six", "plain")] == "p3,p4,p5"
    assert by[("reserved-prefix-keeps-victims", "walk")] == "p2,p3"
    assert by[("reserved-prefix-keeps-victims", "alone-p0")] == by[("reserved-prefix-keeps-victims", "alone-p1")] == "p2"
