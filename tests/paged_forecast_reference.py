"""The reference of the paged admission forecast (kt_paged_forecast), shared by tests/test_paged_forecast_cpu.py and
tests/test_paged_forecast_gpu.py.

For every instant t_k: ``paged_preempt_reference.passes_without(snaps, oracle, p, [], now=t_k)`` — a copy of every page's
snapshot, the oracle's reconcile per page at t_k, the ``calc_updated`` and ``error`` bytes OR-ed over the pages
(status.calculatedThreshold is replaced as a whole), ``apply_status`` per page, the oracle's check per page and
``paging.combine_status`` — once per instant on the state as it is.  Verdict 2 at every instant for an invalid pod row or a
pod-level error of page 0's check.  Nothing here shares code with ``paging.paged_forecast_of`` or the kernel."""
import random

import numpy as np

import forecast_reference as FR
import paged_preempt_reference as PPR
import preempt_reference as PR
import test_manifest_model as TM
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState
from kube_throttler_amd.quantity import parse_rfc3339

NOW = FR.NOW


def reference_verdicts(snaps, oracle_mod, pods, instants, on_equal=False):
    """-> uint8 [len(pods)][len(instants)]: the verdict of PreFilter(pod) over all pages with every page reconciled at t_k."""
    pods = np.asarray(pods, np.int64)
    snap0 = snaps[0]
    out = np.zeros((len(pods), len(instants)), np.uint8)
    _, summary = oracle_mod.Oracle(snap0).check(rows=pods, on_equal=on_equal, want_status=False)
    for i, p in enumerate(pods):
        if not int(snap0.pod_flags[p]) & S.POD_VALID or (int(summary[i]) & 3) == S.VERDICT_ERROR:
            out[i, :] = S.VERDICT_ERROR
            continue
        for k, t in enumerate(instants):
            ok = PPR.passes_without(snaps, oracle_mod, int(p), [], now=t, on_equal=on_equal)
            out[i, k] = S.VERDICT_ALLOW if ok else S.VERDICT_BLOCK
    return out


def own_rows(snaps, oracle_mod, pods, instants, on_equal=False):
    """Every page on its own (forecast_reference.reference_verdicts per page snapshot) -> [uint8 [pods][instants]] per page."""
    return [FR.reference_verdicts(s, oracle_mod, pods, instants, on_equal) for s in snaps]


def or_of_pages(rows):
    """The per-page verdict rows combined as if the pages were independent: Error beats Block beats Success."""
    return np.maximum.reduce([np.asarray(r, np.uint8) for r in rows])


# ---- random wide clusters: forecast_reference.forecast_cluster's shape over 20 to 40 resource names ----
BASE = ["cpu", "memory", "amd.com/gpu"]
POD_QTY = ["0", "1", "1", "2", "3"]
SPEC_QTY_EXTRA = ["2", "8", "32"]
OVR_QTY_EXTRA = ["0", "2", "6", "64"]


def _names(n_names):
    return BASE + [f"example.com/r{k:02d}" for k in range(n_names - len(BASE))]


def _draw(r, names, base_values, extra_values, expect=3.0):
    """A resource list whose names are drawn from EVERY page independently (about ``expect`` of them)."""
    p = expect / len(names)
    base = dict(base_values)
    return {n: r.choice(base[n] if n in base else extra_values) for n in names if r.random() < p}


def _override(r, names, late_only=False):
    begin = r.choice(FR.OVERRIDE_TIMES)
    end = begin if r.random() < 0.1 else r.choice(FR.OVERRIDE_TIMES)  # (equal begin / end: active at exactly one instant)
    if begin and end and begin != "not-a-time" and end != "not-a-time" and r.random() < 0.7 and parse_rfc3339(end) < parse_rfc3339(begin):
        begin, end = end, begin
    if late_only:  # names of the later pages alone: the page that replaces the threshold is not page 0
        late = sorted(names)[S.KT_MAX_DIMS:]
        return {"begin": begin, "end": end, "threshold": {"resourceRequests": {r.choice(late): r.choice(OVR_QTY_EXTRA)}}}
    threshold = {}
    if r.random() < 0.35:
        threshold["resourceCounts"] = {"pod": r.choice([0, 2, 5, 40, 100])}
    rr = _draw(r, names, FR.OVR_QTY, OVR_QTY_EXTRA, 4.0)
    if rr or not threshold:
        threshold["resourceRequests"] = rr
    return {"begin": begin, "end": end, "threshold": threshold}


def wide_forecast_cluster(seed) -> ClusterState:
    r = random.Random(9973 * seed + 41)
    n_names = 20 + (5 * seed) % 21  # 20 .. 40: two or three pages, the last one mostly narrower than 16
    names = _names(n_names)
    cs = ClusterState()
    namespaces = ["ns0", "ns1", "ns2"]
    for n in namespaces:
        cs.add_namespace(n, {"zone": r.choice(["a", "b"]), "kubernetes.io/metadata.name": n})
    pod_namespaces = namespaces + (["ghost"] if seed % 4 == 0 else [])  # "ghost" has no Namespace object
    for i in range(r.randint(30, 50)):
        # the first pod names every resource with "0": the pages carry all n_names whatever the draws below
        zeros = {n: "0" for n in names} if i == 0 else {}
        spec = {"schedulerName": r.choice(["my-scheduler"] * 6 + ["default-scheduler"]),
                "containers": [{"name": f"c{k}", "resources": {"requests": dict(zeros, **_draw(r, names, TM.QTY.items(), POD_QTY, 9.0))}}
                               for k in range(r.randint(1, 2))]}
        phase = "Pending"
        if r.random() < 0.6:
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
        if r.random() < 0.4:
            threshold["resourceCounts"] = {"pod": r.choice([3, 12, 40, 40])}
        rr = _draw(r, names, FR.SPEC_QTY, SPEC_QTY_EXTRA, 5.0)
        if rr or not threshold:
            threshold["resourceRequests"] = rr
        spec = {"throttlerName": r.choice(["kube-throttler"] * 7 + ["someone-else"]), "selector": {"selectorTerms": terms}, "threshold": threshold}
        if r.random() < 0.8:
            spec["temporaryThresholdOverrides"] = [_override(r, names) for _ in range(r.randint(1, 3))]
        if seed % 2 == 0 and r.random() < 0.5:  # never reconciled: an override of a later page's name alone replaces the whole threshold
            spec.setdefault("temporaryThresholdOverrides", []).insert(0, _override(r, names, late_only=True))
        md = {"name": f"thr{i}"}
        if not cluster:
            md["namespace"] = r.choice(namespaces)
        cs.add({"kind": "ClusterThrottle" if cluster else "Throttle", "metadata": md, "spec": spec})
        if r.random() < 0.25:
            nn = (md.get("namespace", "") if not cluster else "") + "/" + md["name"]
            cs.reserved[("ClusterThrottle" if cluster else "Throttle", nn)] = {
                "resourceCounts": {"pod": 1}, "resourceRequests": {"cpu": r.choice(["100m", "500m"])}}
    return cs


def wide_case(seed, oracle_mod):
    """(page snapshots, pod rows): odd seeds with a status written back by a reconcile, even seeds never reconciled."""
    from test_paged_admit_cpu import write_status
    cs = wide_forecast_cluster(seed)
    if seed % 2:
        write_status(cs, oracle_mod)
    snaps = [b.snapshot for b in cs.build_pages()]
    return snaps, FR.forecast_pods(seed, snaps[0], n_pods=6)


# ---- directed cases: (page snapshots, pod row, instants, the joint answer written out) ----
OVR_END_TEXT = "2026-02-01T00:00:00Z"
OVR_END = parse_rfc3339(OVR_END_TEXT)
AROUND_END = [NOW, FR.shift(OVR_END, -1), OVR_END, FR.shift(OVR_END, 1), (OVR_END[0] + 86400, 0)]


def whole_threshold(r19_override="5", r19_request="1", n_extra=20, late="example.com/r19"):
    """tests/test_paged_preempt_cpu.whole_threshold_cluster with the override naming ``late``: r19_override: a never-reconciled
    Throttle, spec {cpu: 1}, an override {r19: 5} active until OVR_END; the pending pod asks cpu 2 (and ``r19_request`` of r19), a
    running pod holds cpu 1 and r19 1.  While the override is active page 1 replaces the threshold, and page 0 reads a calculated
    threshold that omits cpu: the pod passes.  From OVR_END + 1 ns on nothing differs from the empty stored threshold, spec
    {cpu: 1} is read again and the 2 asked exceed it."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    names = {f"example.com/r{k:02d}": "0" for k in range(n_extra)}
    for name, cpu, r19, running in (("pending", "2", r19_request, False), ("victim", "1", "1", True)):
        spec = {"schedulerName": "my-scheduler",
                "containers": [{"name": "c", "resources": {"requests": dict(names, cpu=cpu, **{late: r19})}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": "a"}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "thr", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "1"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": OVR_END_TEXT,
                                                      "threshold": {"resourceRequests": {late: r19_override}}}]}})
    return cs


def _snaps(cs):
    return [b.snapshot for b in cs.build_pages()]


def _error_throttle_wide():
    """preempt_reference._error_throttle_override widened to 20 names: the Throttle's second term does not convert and pod "other"
    reaches it, so the reconcile is an error and the stored status (never reconciled: spec) is read on every page at every
    instant.  spec names cpu 100 (page 0, passes) and r19 1 (page 1): the pending pod asks r19 2 — it never passes, whatever the
    override (cpu 5, r19 100) says."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    names = {f"example.com/r{k:02d}": "0" for k in range(20)}
    for name, app, cpu, r19, running in (("pending", "a", "6", "2", False), ("victim", "a", "4", "0", True), ("other", "b", "4", "0", True)):
        spec = {"schedulerName": "my-scheduler",
                "containers": [{"name": "c", "resources": {"requests": dict(names, cpu=cpu, **{"example.com/r19": r19})}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": app}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "thr", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "100", "example.com/r19": "1"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}},
                                                    {"podSelector": {"matchExpressions": [{"key": "app", "operator": "Bogus"}]}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": OVR_END_TEXT,
                                                      "threshold": {"resourceRequests": {"cpu": "5", "example.com/r19": "100"}}}]}})
    return cs


def _count_only():
    """Two pages of one name each under no name threshold; spec count 2 with two pods running blocks, the override's count 3
    between T1 and T2 (inclusive) lets the pod in: the pod count decides, and it is judged once."""
    flags = [PR.PENDING, PR.COUNTED, PR.COUNTED]
    snaps = PPR.pages_of([[{0: 1}] * 3, [{0: 2}] * 3], [{}, {}], flags, counts=[2, 2])
    return [FR.timed(s, 0, [(FR.T1, FR.T2, {}, 3)]) for s in snaps]


A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK
# name -> () -> (page snapshots, pod row, instants, (first, verdicts) of the cluster of all names)
DIRECTED = {
    # the case of whole_threshold's docstring: page 0 alone answers Block throughout, page 1 alone Success throughout
    "later-page-replaces-the-threshold": lambda: (_snaps(whole_threshold()), 0, AROUND_END, (0, [A, A, A, B, B])),
    # the replacing page holds nothing the pod requests (r19 request 0), r19 still in the override: the same answer
    "replacing-page-holds-nothing-the-pod-asks": lambda: (_snaps(whole_threshold(r19_request="0")), 0, AROUND_END, (0, [A, A, A, B, B])),
    "error-throttle-stopping-name-on-page-1": lambda: (_snaps(_error_throttle_wide()), 0, AROUND_END, (-1, [B] * 5)),
    "count-only-override": lambda: (_count_only(), 0, FR.EDGE, (2, [B, B, A, A, A, A, B, B, B])),
}
