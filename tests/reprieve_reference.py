"""The reference of the reprieve pass (kt_preempt_reprieve_launch), shared by tests/test_reprieve_cpu.py, tests/test_reprieve_gpu.py
and tests/test_host_reprieve_gpu.py.

The walk of the issue, step by step, on ``preempt_reference.passes_without`` (delete, oracle reconcile, oracle check) and nothing
else: for j = k-1 .. 0 the candidate c_j is put back when the preemptor still passes in the cluster without the remaining
victims.  Nothing here shares code with ``paging.preempt_of`` or the kernel.  The directed cases of the reprieve pass are built
by hand on ``preempt_reference.tiny`` and from a few manifests; ``big_last`` and ``wide`` build the shapes of the GPU suite."""
import numpy as np

import preempt_reference as PR
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState

NOW = PR.NOW
PENDING, COUNTED, tiny = PR.PENDING, PR.COUNTED, PR.tiny


def reference_reprieve(snap, oracle_mod, p, cands, prefix, now=NOW, on_equal=False):
    """-> the reprieved victim bytes [len(cands)] behind the prefix ``prefix`` (what the prefix query's own reference answers).
    The walk starts from the WHOLE prefix deleted and visits every position: a candidate outside the prefix mask — not counted,
    or matched by no throttle that affects p — changes nothing the preemptor's PreFilter reads, comes back at its turn and is
    not a victim, so the walk over the mask and the walk over the prefix end in the same set; this one needs no mask."""
    if prefix <= 0:
        return [0] * len(cands)
    victims = [int(j < prefix) for j in range(len(cands))]
    for j in range(prefix - 1, -1, -1):
        rest = [c for q, c in enumerate(cands) if victims[q] and q != j]
        if PR.passes_without(snap, oracle_mod, p, rest, now, on_equal):
            victims[j] = 0
    return victims


def reference(snap, oracle_mod, p, cands, now=NOW, on_equal=False):
    """-> (prefix, reprieved victims), all by delete + reconcile + check."""
    k = PR.reference_prefix(snap, oracle_mod, p, cands, now, on_equal)
    return k, reference_reprieve(snap, oracle_mod, p, cands, k, now, on_equal)


def has_negative_requests(snap, rows):
    return any(int(snap.ctr_req[int(snap.pod_ctr_off[r]):int(snap.pod_ctr_off[r + 1])].min(initial=0)) < 0 for r in rows)


# ---- directed cases: (snapshot, preemptor, candidates) ----
def two_throttles(shared_victim=False):
    """Throttle thr-a (label a, cpu 10) and throttle thr-b (label b, cpu 10) both select the pending pod, which carries both
    labels and asks 3.  Each throttle is at 9 through a small and a big pod of its own: each needs ITS big pod gone, and nothing
    is reprieved across them.  ``shared_victim``: both are at 9 through a small pod, a rest and one pod that carries both labels
    — the one victim that both affecting throttles match."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})

    def pod(name, labels, cpu, running=True):
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": cpu}}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": labels}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})

    pod("pending", {"a": "1", "b": "1"}, "3", running=False)
    if shared_victim:
        # both throttles are at 9 of 10: the pod that both match (5) frees both, the small ones (1 each) free neither
        pod("small-a", {"a": "1"}, "1")
        pod("small-b", {"b": "1"}, "1")
        pod("both", {"a": "1", "b": "1"}, "5")
        pod("rest-a", {"a": "1"}, "3")
        pod("rest-b", {"b": "1"}, "3")
        cands = [1, 2, 3]
    else:
        # A needs its big pod gone, B needs its big pod gone; the small ones come back
        pod("small-a", {"a": "1"}, "1")
        pod("big-a", {"a": "1"}, "8")
        pod("small-b", {"b": "1"}, "1")
        pod("big-b", {"b": "1"}, "8")
        cands = [1, 3, 2, 4]
    for key in ("a", "b"):
        cs.add({"kind": "Throttle", "metadata": {"name": "thr-" + key, "namespace": "ns0"},
                "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "10"}},
                         "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {key: "1"}}}]}}})
    return cs.build_pages()[0].snapshot, 0, cands


def error_throttle_beside_a_reconciled_one():
    """Two Throttles select the pending pod (app=a, cpu 3) and every candidate.  "err" has a second term that does not convert
    and pod "other" (app=b) reaches it: its reconcile is an error and it keeps its stored status — no calculatedAt, so the check
    reads spec (cpu 100) against an empty `used`, and it passes whoever is deleted.  Its override (cpu 5, active at `now`) and the
    fresh sums must NOT be what it is judged on: with keeper 4 still running, 4 + 1 + 3 > 5 would refuse every reprieve.  "real"
    (cpu 10) is reconciled: 4 + 1 + 1 + 6 = 12 has to come down to 7, the prefix is 3, and the walk keeps only the 6."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    for name, app, cpu, running in (("pending", "a", "3", False), ("keeper", "a", "4", True), ("s1", "a", "1", True), ("s2", "a", "1", True),
                                    ("big", "a", "6", True), ("other", "b", "4", True)):
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": cpu}}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": app}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "err", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "100"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}},
                                                    {"podSelector": {"matchExpressions": [{"key": "app", "operator": "Bogus"}]}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": "2026-02-01T00:00:00Z",
                                                      "threshold": {"resourceRequests": {"cpu": "5"}}}]}})
    cs.add({"kind": "Throttle", "metadata": {"name": "real", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "10"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}}]}}})
    return cs.build_pages()[0].snapshot, 0, [2, 3, 4]


DIRECTED = {
    # the issue's example: threshold 10, the preemptor asks 3, others use 4, the candidates 1, 1, 6 -> only the last has to go
    "one-one-six": lambda: (tiny([{0: 3}, {0: 4}, {0: 1}, {0: 1}, {0: 6}], {0: 10}, flags=[PENDING] + [COUNTED] * 4), 0, [2, 3, 4]),
    "two-throttles-two-victims": two_throttles,
    "victim-of-two-throttles": lambda: two_throttles(shared_victim=True),
    # cpu threshold 0 on a Throttle; pod 1 carries cpu with the value 0: back in `used` it makes step 3 (0 >= 0) stop the
    # preemptor, whose negative request passes steps 1 and 4 — the sums cannot tell, only the contributor count
    "zero-valued-name-comes-back": lambda: (tiny([{0: -1}, {0: 0}, {1: 1}], {0: 0}, flags=[PENDING, COUNTED, COUNTED]), 0, [2, 1]),
    # cpu is far from its threshold, the pod count is what blocks: 4 counted, threshold 3 -> two must go, none comes back
    "pod-count-alone": lambda: (tiny([{0: 1}] * 5, {0: 100}, count=3, flags=[PENDING] + [COUNTED] * 4), 0, [1, 2, 3, 4]),
    # candidate 1 asks -4: deleting it RAISES `used` (8 -> 12), the prefix has to reach candidate 2 (6 + 3 <= 10), and the walk
    # puts candidate 1 back (2 + 3) after it has refused candidate 2 (12 + 3)
    "negative-request-candidate": lambda: (tiny([{0: 3}, {0: -4}, {0: 6}, {0: 6}], {0: 10}, flags=[PENDING] + [COUNTED] * 3), 0, [1, 2, 3]),
    # prefix 0, nothing is walked ...
    "error-throttle-override-active": PR.DIRECTED["error-throttle-override-active"],
    # ... and with a positive prefix: the error throttle matches every masked victim and stays out of the walk
    "error-throttle-beside-a-reconciled-one": error_throttle_beside_a_reconciled_one,
    # the error candidate (3) cuts the list to [1]: one victim is not enough, nothing is walked
    "error-candidate-cuts": PR.DIRECTED["error-candidate-cuts"],
    # ... and behind an answerable prefix: [1, 2 | 3 (error) ...]
    "error-candidate-behind-the-prefix": lambda: (tiny([{0: 3}, {0: 1}, {0: 6}, {0: 4}, {0: 3}], {0: 10}, flags=[PENDING] + [COUNTED] * 4,
                                                       pod_ns=[0, 0, 0, 1, 0], cluster=True), 0, [1, 2, 3, 4]),
    # used 2 + 4 + 4 against 10, the preemptor asks 2: at exact equality the two on_equal values keep different victims
    "equality-throttle": lambda: (tiny([{0: 2}, {0: 2}, {0: 4}, {0: 4}], {0: 10}, flags=[PENDING] + [COUNTED] * 3), 0, [1, 2, 3]),
    "equality-clusterthrottle": lambda: (tiny([{0: 2}, {0: 2}, {0: 4}, {0: 4}], {0: 10}, cluster=True, flags=[PENDING] + [COUNTED] * 3), 0,
                                         [1, 2, 3]),
    "equality-step3-clusterthrottle": PR.DIRECTED["equality-step3-clusterthrottle"],
}


def big_last(m, T=1, row=0, D=2, dim=0, **kw):
    """Pod 0 pending asking 1 of ``dim``; candidates 1 .. m running with 1 of ``dim`` each, except the last but one in list order,
    which uses m; threshold m.  `used` is 2 m - 1 and has to come down to m - 1: only with the big pod gone, so the prefix is
    m - 1 and its mask m - 1 ones; the walk keeps the big pod out and puts the m - 2 small ones before it back (all but one of
    them with on_equal) — the masked positions straddle the blocks of 64 candidates."""
    other = {d: 2 for d in range(D) if d != dim}
    small, big = dict(other), dict(other)
    small[dim], big[dim] = 1, m
    reqs = [small] * m
    reqs[m - 2] = big
    snap = tiny([{dim: 1}] + reqs, {dim: m}, flags=[PENDING] + [COUNTED] * m, D=D, T=T, row=row, **kw)
    return snap, 0, list(range(1, m + 1))


def wide(L, m, D=3, T=None, seed=0, n_pre=1):
    """``L`` Throttles of namespace 0 that select every pod (rows T - L .. T - 1 of ``T``; the rows before them belong to the
    empty namespace 2 and affect nobody, row 0 excepted: it selects everyone under a threshold nothing reaches — with T = 1030
    it lies in the first chunk of the matrix row and the L rows in the second).  Pods 0 .. n_pre - 1 are pending and ask 1 .. 2 of every name; candidates follow, running, with random
    small amounts of random names.  Throttle row T - 1 - d binds name d at about 0.55 of what is used (the other affecting rows
    name it with thresholds nothing reaches): the binding entries are the LAST of the list, and every name asks for its own
    victims -> (snapshot, preemptor rows, candidate rows)."""
    import random
    r = random.Random(1009 * seed + L + 31 * m + D)
    T = L if T is None else T
    assert D <= L <= T
    reqs = [{d: 1 + (i + d) % 2 for d in range(D)} for i in range(n_pre)]
    for _ in range(m):
        reqs.append({d: r.randint(0, 3) for d in range(D) if r.random() < 0.6} or {0: 1})
    used = [sum(q.get(d, 0) for q in reqs[n_pre:]) for d in range(D)]
    s = tiny(reqs, {}, flags=[PENDING] * n_pre + [COUNTED] * m, D=D, T=T)
    s.thr_spec.set_row(0, {d: 1 << 40 for d in range(D)}, 1 << 40)
    for t in range(T - L, T):
        s.thr_ns[t] = 0
        s.thr_spec.set_row(t, {d: (1 << 40) + t for d in range(D)}, None)
    for d in range(D):
        s.thr_spec.set_row(T - 1 - d, {d: max(3, (used[d] * 11) // 20)}, None)
    return s, list(range(n_pre)), list(range(n_pre, n_pre + m))
