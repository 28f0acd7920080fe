"""Runs the C++ plugin mirror's gang preemption driver (tests/cpp/host_plugin_preempt_gang_test.cpp): KubeThrottler::PreemptGang
against delete + ReconcileAll + AdmitGangs per prefix on a twin plugin, and — here — the victim NAMES and the blocking member it
prints against the manifest model (``paging.preempt_gangs_of`` on the snapshot of the same 20-pod scenario written as manifests)."""
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
GANGS = ["cpu2+gpu2", "gpu2+cpu2", "cpu2+free", "cpu2+huge"]


def model_answers(cs):
    names = [p["metadata"]["name"] for p in cs.pods]
    assert len(names) == 20
    snap = cs.build_pages()[0].snapshot
    ctx = paging.preempt_context(snap, PR.NOW)
    up = [f"r{i:02d}" for i in range(16)]
    lists = {"up": up, "down": up[::-1]}

    def answer(gang, lst):
        members = gang.split("+")
        cands = [names.index(c) for c in lists[lst]]
        prefix, victims, blocker = paging.preempt_gangs_of(snap, [names.index(p) for p in members], cands, PR.NOW, False, ctx=ctx)
        who = members[blocker] if blocker >= 0 else "-"
        if prefix <= 0:
            return ("none" if prefix < 0 else "pass"), who
        return ",".join(c for c, v in zip(lists[lst], victims) if v), who

    def alone(pod, lst):
        cands = [names.index(c) for c in lists[lst]]
        return sum(paging.preempt_of(snap, names.index(pod), cands, PR.NOW, False, ctx=ctx)[1])

    return answer, alone


def test_host_plugin_preempt_gang():
    exe = os.path.join(HOST, "host_plugin_preempt_gang_test")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", HOST, "host_plugin_preempt_gang_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    lines = re.findall(r"^PREEMPTGANG (\S+) (\S+) -> (\S+) (\S+)$", r.stdout, re.M)
    answer, alone = model_answers(scenario())
    assert {(g, lst) for g, lst, _, _ in lines} == {(g, lst) for g in GANGS for lst in ("up", "down")}
    for gang, lst, got, who in lines:
        assert (got, who) == answer(gang, lst), f"{gang} over {lst}: the mirror says {(got, who)}, the manifest model {answer(gang, lst)}"
    # the scenario asks something: a gang that needs more victims than either member alone, an order of the list that matters, a
    # gang without a prefix, and a blocker that follows the order of the members
    by = {(g, lst): (got, who) for g, lst, got, who in lines}
    assert by[("cpu2+gpu2", "down")][0].count(",") + 1 > max(alone("cpu2", "down"), alone("gpu2", "down"))
    assert by[("cpu2+gpu2", "up")][0] != by[("cpu2+gpu2", "down")][0]
    assert by[("cpu2+huge", "up")] == ("none", "cpu2") and by[("gpu2+cpu2", "up")][1] == "gpu2"
