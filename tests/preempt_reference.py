"""The reference of the preemption query (kt_preempt_launch), shared by tests/test_preempt_cpu.py and tests/test_preempt_gpu.py.

For k = 0 .. m_eff: a copy of the snapshot in which the candidates c_0 .. c_{k-1} are deleted (pod_flags = 0, as the tests of the
pod event path model a deleted row), the oracle's reconcile at ``now`` written into the copy's stored status for the rows
without error, then the oracle's check of the preemptor.  The first k with Success is the answer.  Nothing here shares code
with ``paging.preempt_of`` or the kernel."""
import copy
import random

import numpy as np

import test_manifest_model as TM
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState
from kube_throttler_amd.quantity import parse_rfc3339

NOW = parse_rfc3339(TM.NOW_TEXT)
COUNTED = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED


def copy_snapshot(snap):
    snap._keep = None  # (the ctypes view of the arrays: rebuilt on demand)
    return copy.deepcopy(snap)


def responsible_rows(snap):
    need = S.THR_VALID | S.THR_RESPONSIBLE
    return np.nonzero((snap.thr_flags[:snap.n_thr] & need) == need)[0].astype(np.int32)


def passes_without(snap, oracle_mod, p, deleted, now, on_equal) -> bool:
    """PreFilter(p) is Success in the cluster without the pod rows ``deleted``, every responsible throttle reconciled at now."""
    s = copy_snapshot(snap)
    for c in deleted:
        s.pod_flags[int(c)] = 0
    rows = responsible_rows(s)
    if len(rows):
        r = oracle_mod.Oracle(s).reconcile(now, rows=rows)
        s.apply_status(r.used, r.calc, r.calc_updated, r.thrl_flag, r.thrl_has, r.thrl_pod, r.error, rows=rows)
    _, summary = oracle_mod.Oracle(s).check(rows=np.array([p], np.int64), on_equal=on_equal, want_status=False)
    return (int(summary[0]) & 3) == S.VERDICT_ALLOW


def effective_length(snap, oracle_mod, cands) -> int:
    """m_eff: the list ends before the first candidate whose own PreFilter is an error or whose row is invalid."""
    if not len(cands):
        return 0
    _, summary = oracle_mod.Oracle(snap).check(rows=np.asarray(cands, np.int64), want_status=False)
    for j, c in enumerate(cands):
        if not int(snap.pod_flags[c]) & S.POD_VALID or (int(summary[j]) & 3) == S.VERDICT_ERROR:
            return j
    return len(cands)


def reference_prefix(snap, oracle_mod, p, cands, now=NOW, on_equal=False) -> int:
    if not int(snap.pod_flags[p]) & S.POD_VALID:
        return -1
    _, summary = oracle_mod.Oracle(snap).check(rows=np.array([p], np.int64), want_status=False)
    if (int(summary[0]) & 3) == S.VERDICT_ERROR:
        return -1
    for k in range(effective_length(snap, oracle_mod, cands) + 1):
        if passes_without(snap, oracle_mod, p, cands[:k], now, on_equal):
            return k
    return -1


def check_victims(snap, oracle_mod, p, cands, prefix, victims, now=NOW, on_equal=False):
    """The victim-mask property: all zero without a positive prefix, nothing at or beyond the prefix, only counted pods, and
    deleting exactly the masked pods lets the preemptor through."""
    victims = [int(v) for v in victims]
    assert len(victims) == len(cands)
    if prefix <= 0:
        assert not any(victims)
        return
    assert not any(victims[prefix:])
    masked = [c for c, v in zip(cands, victims) if v]
    for c in masked:
        assert (int(snap.pod_flags[c]) & (COUNTED | S.POD_FINISHED)) == COUNTED, f"victim {c} is not counted"
    assert passes_without(snap, oracle_mod, p, masked, now, on_equal), f"pod {p}: deleting the masked pods {masked} does not let it through"


# ---- random manifest clusters: up to 60 pods x 12 throttles, most pods running under the throttler's scheduler ----
def preempt_cluster(seed) -> ClusterState:
    r = random.Random(7919 * seed + 13)
    cs = ClusterState()
    namespaces = ["ns0", "ns1", "ns2"]
    for n in namespaces:
        cs.add_namespace(n, {"zone": r.choice(["a", "b"]), "kubernetes.io/metadata.name": n})
    pod_namespaces = namespaces + (["ghost"] if seed % 4 == 0 else [])  # "ghost" has no Namespace object
    for i in range(r.randint(30, 60)):
        spec = {"schedulerName": r.choice(["my-scheduler"] * 6 + ["default-scheduler"]),
                "containers": [{"name": f"c{k}", "resources": {"requests": TM._requests(r)}} for k in range(r.randint(1, 2))]}
        if r.random() < 0.15:
            spec["initContainers"] = [{"name": "i", "resources": {"requests": TM._requests(r, 0.5)}}]
        phase = "Pending"
        if r.random() < 0.7:
            spec["nodeName"] = "node-1"
            phase = r.choice(["Running"] * 8 + ["Succeeded", "Failed"])
        cs.add({"kind": "Pod", "metadata": {"name": f"pod{i}", "namespace": r.choice(pod_namespaces), "labels": TM._labels(r)},
                "spec": spec, "status": {"phase": phase}})
    for i in range(r.randint(6, 12)):
        cluster = r.random() < 0.5
        terms = []
        for _ in range(r.randint(1, 2)):
            t = {"podSelector": TM._selector(r, allow_bad=seed % 5 == 0)}
            if cluster and r.random() < 0.5:
                t["namespaceSelector"] = {"matchLabels": {"zone": r.choice(["a", "b"])}}
            terms.append(t)
        threshold = {}
        if r.random() < 0.6:
            threshold["resourceCounts"] = {"pod": r.randint(3, 12)}
        rr = {name: r.choice(vs) for name, vs in (("cpu", ["3", "4", "6"]), ("memory", ["2Gi", "3Gi", "4Gi"]), ("amd.com/gpu", ["4", "6", "8"]))
              if r.random() < 0.45}
        if rr or not threshold:
            threshold["resourceRequests"] = rr
        spec = {"throttlerName": r.choice(["kube-throttler"] * 7 + ["someone-else"]), "selector": {"selectorTerms": terms}, "threshold": threshold}
        if r.random() < 0.2:
            spec["temporaryThresholdOverrides"] = [
                {"begin": r.choice(TM.TIMES), "end": r.choice(TM.TIMES), "threshold": TM._amount(r, 3)} for _ in range(r.randint(1, 2))]
        md = {"name": f"thr{i}"}
        if not cluster:
            md["namespace"] = r.choice(namespaces)
        cs.add({"kind": "ClusterThrottle" if cluster else "Throttle", "metadata": md, "spec": spec})
        if r.random() < 0.25:
            nn = (md.get("namespace", "") if not cluster else "") + "/" + md["name"]
            cs.reserved[("ClusterThrottle" if cluster else "Throttle", nn)] = {
                "resourceCounts": {"pod": 1}, "resourceRequests": {"cpu": r.choice(["100m", "500m"])}}
    return cs


def preempt_cases(seed, snap, n_cases=6):
    """[(preemptor row, candidate rows)]: preemptors are pods outside their list; the lists are random orders of random
    subsets of the other pods — counted, pending, finished and foreign-scheduler pods alike."""
    r = random.Random(104729 * seed + 1)
    out = []
    for _ in range(n_cases):
        p = r.randrange(snap.n_pods)
        others = [c for c in range(snap.n_pods) if c != p]
        r.shuffle(others)
        out.append((p, others[:r.choice([0, 3, len(others) // 2, len(others), len(others), len(others)])]))
    return out


# ---- snapshots built by hand: pods of namespace 0 that one Throttle / ClusterThrottle row selects ----
PENDING = S.POD_VALID | S.POD_SCHED_MATCH


def tiny(pod_requests, threshold, count=None, cluster=False, flags=None, D=2, T=1, row=0, pod_ns=None, reserved=None, override=None,
         stale=False):
    """Pods with one container each ({dim: value}); namespace 0 holds the pods (``pod_ns`` overrides: namespace 1 has no
    Namespace object, namespace 2 is empty).  Throttle row ``row`` selects every pod of namespace 0 (one empty term) under
    ``threshold`` / ``count``; with ``row`` > 0 row 0 selects them too under a threshold nothing reaches, and the other rows are
    Throttles of namespace 2 with a pod-count threshold of 0 (they would block whoever they matched).  ``reserved``:
    ({dim: value}, count) on row ``row``; ``override``: ({dim: value}, count) active at every instant; ``stale``: a stored
    status that says "throttled" with a large `used`, which a fresh reconcile replaces."""
    n = len(pod_requests)
    s = S.Snapshot(D, 1)
    s.alloc_namespaces(3, 0)
    s.ns_valid[1] = 0
    s.alloc_pods(n, 0, n)
    for i, req in enumerate(pod_requests):
        s.pod_flags[i] = (flags[i] if flags else COUNTED)
        s.pod_ns[i] = pod_ns[i] if pod_ns else 0
        s.pod_ctr_off[i + 1] = i + 1
        for d, v in req.items():
            s.ctr_req[i, d] = v
            s.ctr_present[i] |= np.uint32(1 << d)
    s.alloc_throttles(T, 1 if override else 0, T)
    for t in range(T):
        s.thr_flags[t] = S.THR_VALID | S.THR_RESPONSIBLE
        s.thr_ns[t] = 2
        s.thr_spec.set_row(t, {}, 0)
        s.thr_term_off[t + 1] = t + 1
    if row > 0:
        s.thr_ns[0] = 0
        s.thr_spec.set_row(0, {d: 1 << 40 for d in range(D)}, 1 << 40)
    s.thr_flags[row] |= S.THR_CLUSTER if cluster else 0
    s.thr_ns[row] = 0
    s.thr_spec.set_row(row, threshold, count)
    if reserved:
        s.thr_reserved.set_row(row, reserved[0], reserved[1])
    if override:
        s.thr_ovr_off[row + 1:] = 1
        s.ovr_thr.set_row(0, override[0], override[1])
    if stale:
        s.thr_used.set_row(row, {d: 1 << 30 for d in range(D)}, 1 << 30)
        s.thr_thrl_flag[row] = s.thr_thrl_has[row] = (1 << D) - 1
        s.thr_flags[row] |= S.THR_THROTTLED_POD
    return s


def line(m, k_star, D=2, dim=0, **kw):
    """Pod 0 pending, asking 1 of ``dim``; candidates 1 .. m running with 1 of ``dim`` each (and 2 of every other name, which
    the threshold does not name), threshold m + 1 - k_star: exactly k_star of them have to go -> (snapshot, 0, [1 .. m])."""
    other = {d: 2 for d in range(D) if d != dim}
    running = dict(other)
    running[dim] = 1
    snap = tiny([{dim: 1}] + [running] * m, {dim: m + 1 - k_star}, flags=[PENDING] + [COUNTED] * m, D=D, **kw)
    return snap, 0, list(range(1, m + 1))


def _interleaved():
    flags = [PENDING, PENDING, COUNTED, COUNTED | S.POD_FINISHED, COUNTED, S.POD_VALID | S.POD_SCHEDULED, COUNTED]
    return tiny([{0: 3}] + [{0: 4}] * 6, {0: 10}, flags=flags), 0, [1, 2, 3, 4, 5, 6]


def _error_candidate():
    # candidate 3 lives in a namespace without object: its own PreFilter is an error and the list ends before it
    return (tiny([{0: 3}] + [{0: 4}] * 5, {0: 10}, flags=[PENDING] + [COUNTED] * 5, pod_ns=[0, 0, 0, 1, 0, 0], cluster=True), 0, [1, 3, 2, 4, 5])


def _error_throttle_override():
    # The Throttle's second term does not convert and pod "other" reaches it: the reconcile is an error and the stored status
    # stays.  Nobody has reconciled yet (no calculatedAt), so the check reads spec (cpu 100) and not the override that is active
    # at `now` (cpu 5, less than the 6 the pending pod asks for): the pod passes as things stand.
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    for name, app, cpu, running in (("pending", "a", "6", False), ("victim", "a", "4", True), ("other", "b", "4", True)):
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": cpu}}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": app}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "thr", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "100"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}},
                                                    {"podSelector": {"matchExpressions": [{"key": "app", "operator": "Bogus"}]}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": "2026-02-01T00:00:00Z",
                                                      "threshold": {"resourceRequests": {"cpu": "5"}}}]}})
    return cs.build_pages()[0].snapshot, 0, [1]


DIRECTED = {
    # cpu is in `used` only through pod 1, with the value 0: step 3 (0 >= 0 on a Throttle) holds while the name is present and
    # falls away with its one contributor — the sums are 0 either way (the preemptor's negative request passes steps 1 and 4)
    "presence-through-one-victim": lambda: (tiny([{0: -1}, {0: 0}, {1: 1}], {0: 0}, flags=[PENDING, COUNTED, COUNTED]), 0, [2, 1]),
    "count-threshold-only": lambda: (tiny([{0: 1}] * 4, {}, count=2, flags=[PENDING] + [COUNTED] * 3), 0, [1, 2, 3]),
    "last-counted-pod": lambda: (tiny([{0: 1}] * 3, {}, count=1, flags=[PENDING, COUNTED, COUNTED]), 0, [1, 2]),
    "equality-throttle": lambda: (tiny([{0: 2}, {0: 2}, {0: 4}, {0: 4}], {0: 10}, flags=[PENDING] + [COUNTED] * 3), 0, [1, 2, 3]),
    "equality-clusterthrottle": lambda: (tiny([{0: 2}, {0: 2}, {0: 4}, {0: 4}], {0: 10}, cluster=True, flags=[PENDING] + [COUNTED] * 3), 0, [1, 2, 3]),
    "equality-step3-clusterthrottle": lambda: (tiny([{1: 1}, {0: 5}, {0: 5}, {0: 0, 1: 1}], {0: 10, 1: 1}, cluster=True,
                                                    flags=[PENDING] + [COUNTED] * 3), 0, [3, 1, 2]),
    "reserved": lambda: (tiny([{0: 1}] + [{0: 3}] * 3, {0: 10}, count=5, flags=[PENDING] + [COUNTED] * 3, reserved=({0: 4}, 2)), 0, [1, 2, 3]),
    "override-active-now": lambda: (tiny([{0: 1}] + [{0: 3}] * 3, {0: 100}, flags=[PENDING] + [COUNTED] * 3, override=({0: 5}, None)), 0, [1, 2, 3]),
    "stale-stored-status": lambda: (tiny([{0: 1}] + [{0: 3}] * 3, {0: 7}, count=9, flags=[PENDING] + [COUNTED] * 3, stale=True), 0, [1, 2, 3]),
    "error-throttle-override-active": _error_throttle_override,
    "uncounted-interleaved": _interleaved,
    "error-candidate-cuts": _error_candidate,
    "exceeds-threshold": lambda: (tiny([{0: 11}, {0: 4}, {0: 4}], {0: 10}, flags=[PENDING, COUNTED, COUNTED]), 0, [1, 2]),
    "already-passing": lambda: (tiny([{0: 1}, {0: 4}, {0: 4}], {0: 10}, flags=[PENDING, COUNTED, COUNTED]), 0, [1, 2]),
    "no-candidates": lambda: (tiny([{0: 3}, {0: 4}, {0: 4}, {0: 4}], {0: 10}, flags=[PENDING] + [COUNTED] * 3), 0, []),
}
