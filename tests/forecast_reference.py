"""The reference of the admission forecast (kt_forecast_launch), shared by tests/test_forecast_cpu.py and tests/test_forecast_gpu.py.

For every instant t_k: a deep copy of the snapshot, the oracle's reconcile at t_k of the responsible rows written into the copy's
stored status for the rows without error, then the oracle's check of the pods — the pattern of preempt_reference.passes_without,
once per instant on the state as it is (never on top of the previous instant).  Nothing here shares code with
``paging.forecast_of`` or the kernel."""
import random

import numpy as np

import preempt_reference as PR
import test_manifest_model as TM
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState
from kube_throttler_amd.quantity import parse_rfc3339

NOW = PR.NOW
# the dozen override boundaries of the forecast window, all after NOW
BOUNDARY_TEXTS = ["2026-01-01T01:00:00Z", "2026-01-01T02:00:00Z", "2026-01-01T03:30:00Z", "2026-01-01T06:00:00Z", "2026-01-01T09:00:00+09:00",
                  "2026-01-01T12:00:00Z", "2026-01-01T18:00:00Z", "2026-01-01T22:00:00Z", "2026-01-02T00:00:00Z", "2026-01-02T06:00:00Z",
                  "2026-01-03T00:00:00Z", "2026-01-05T00:00:00Z"]
BOUNDARIES = sorted(parse_rfc3339(t) for t in BOUNDARY_TEXTS)
BEYOND = (BOUNDARIES[-1][0] + 86400, 0)


def shift(t, ns):
    """The instant t + ns nanoseconds (|ns| < 10^9)."""
    s, n = int(t[0]), int(t[1]) + ns
    return (s + n // 1_000_000_000, n % 1_000_000_000)


def instants_under_test(boundaries=BOUNDARIES, now=NOW, beyond=BEYOND):
    """now, every boundary, every boundary -+ 1 ns, and one instant beyond all of them — strictly ascending."""
    out = {tuple(now), tuple(beyond)}
    for b in boundaries:
        out |= {shift(b, -1), tuple(b), shift(b, 1)}
    return sorted(out)


INSTANTS = instants_under_test()


def state_at(snap, oracle_mod, t):
    """R_t: a copy of the snapshot with every responsible throttle reconciled at t (rows with an error keep their status)."""
    s = PR.copy_snapshot(snap)
    rows = PR.responsible_rows(s)
    if len(rows):
        r = oracle_mod.Oracle(s).reconcile(t, rows=rows)
        s.apply_status(r.used, r.calc, r.calc_updated, r.thrl_flag, r.thrl_has, r.thrl_pod, r.error, rows=rows)
    return s


def reference_verdicts(snap, oracle_mod, pods, instants, on_equal=False, states=None):
    """-> uint8 [len(pods)][len(instants)]: the verdict of PreFilter(pod) in R_{t_k}; an invalid pod row is an Error throughout."""
    pods = np.asarray(pods, np.int64)
    out = np.zeros((len(pods), len(instants)), np.uint8)
    valid = np.array([bool(int(snap.pod_flags[p]) & S.POD_VALID) for p in pods], bool)
    for k, t in enumerate(instants):
        s = states[k] if states is not None else state_at(snap, oracle_mod, t)
        _, summary = oracle_mod.Oracle(s).check(rows=pods, on_equal=on_equal, want_status=False)
        out[:, k] = np.where(valid, summary & 3, S.VERDICT_ERROR)
    return out


def first_of(verdicts):
    """Per row the first position whose verdict is Success, or -1."""
    return [next((k for k, v in enumerate(row) if int(v) == S.VERDICT_ALLOW), -1) for row in verdicts]


def flips(row) -> int:
    return sum(1 for a, b in zip(row[:-1], row[1:]) if int(a) != int(b))


# ---- random manifest clusters: preempt_cluster's shape, with temporaryThresholdOverrides on most throttles ----
OVERRIDE_TIMES = BOUNDARY_TEXTS + ["", "", "not-a-time"]
SPEC_QTY = (("cpu", ["2", "8", "20"]), ("memory", ["1Gi", "8Gi", "32Gi"]), ("amd.com/gpu", ["2", "8", "32"]))
# override thresholds: from below a single pod's request (cpu 100m .. 1 per container) to far above every sum
OVR_QTY = (("cpu", ["50m", "100m", "2", "20", "100"]), ("memory", ["32Mi", "1Gi", "64Gi"]), ("amd.com/gpu", ["0", "2", "64"]))


def _override(r):
    begin = r.choice(OVERRIDE_TIMES)
    end = begin if r.random() < 0.1 else r.choice(OVERRIDE_TIMES)  # (equal begin / end: active at exactly one instant)
    if begin and end and begin != "not-a-time" and end != "not-a-time" and r.random() < 0.7 and parse_rfc3339(end) < parse_rfc3339(begin):
        begin, end = end, begin
    threshold = {}
    if r.random() < 0.45:
        threshold["resourceCounts"] = {"pod": r.choice([0, 2, 5, 40, 100])}
    # names drawn independently of the spec's: an override may name a resource the spec does not, or omit one it does
    rr = {name: r.choice(vs) for name, vs in OVR_QTY if r.random() < 0.5}
    if rr or not threshold:
        threshold["resourceRequests"] = rr
    return {"begin": begin, "end": end, "threshold": threshold}


def forecast_cluster(seed) -> ClusterState:
    r = random.Random(6151 * seed + 29)
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
        if r.random() < 0.5:
            threshold["resourceCounts"] = {"pod": r.choice([3, 12, 40, 40])}
        rr = {name: r.choice(vs) for name, vs in SPEC_QTY if r.random() < 0.45}
        if rr or not threshold:
            threshold["resourceRequests"] = rr
        spec = {"throttlerName": r.choice(["kube-throttler"] * 7 + ["someone-else"]), "selector": {"selectorTerms": terms}, "threshold": threshold}
        if r.random() < 0.8:
            spec["temporaryThresholdOverrides"] = [_override(r) for _ in range(r.randint(1, 3))]
        md = {"name": f"thr{i}"}
        if not cluster:
            md["namespace"] = r.choice(namespaces)
        cs.add({"kind": "ClusterThrottle" if cluster else "Throttle", "metadata": md, "spec": spec})
        if r.random() < 0.25:
            nn = (md.get("namespace", "") if not cluster else "") + "/" + md["name"]
            cs.reserved[("ClusterThrottle" if cluster else "Throttle", nn)] = {
                "resourceCounts": {"pod": 1}, "resourceRequests": {"cpu": r.choice(["100m", "500m"])}}
    return cs


def forecast_pods(seed, snap, n_pods=8):
    """The pod rows under test: a random sample, pending and running pods alike."""
    r = random.Random(15485863 * seed + 3)
    rows = list(range(snap.n_pods))
    r.shuffle(rows)
    return sorted(rows[:n_pods])


# ---- snapshots built by hand: preempt_reference.tiny plus overrides with instants ----
T0 = NOW
T1, T2, T3, T4 = ((NOW[0] + 3600 * h, 0) for h in (1, 2, 3, 4))
BEGIN_PARSED = 0x2


def timed(snap, row, overrides):
    """Gives throttle row ``row`` of a ``PR.tiny`` snapshot (built without override) the list ``overrides``:
    (begin, end, {dim: value}, count[, flags]) with begin / end (seconds, nanoseconds) or None (the zero time)."""
    k = len(overrides)
    D = snap.D
    snap.ovr_begin_s = np.full(max(k, 1), S.ZERO_TIME_S, dtype=np.int64)
    snap.ovr_begin_ns = np.zeros(max(k, 1), dtype=np.int32)
    snap.ovr_end_s = np.full(max(k, 1), S.ZERO_TIME_S, dtype=np.int64)
    snap.ovr_end_ns = np.zeros(max(k, 1), dtype=np.int32)
    snap.ovr_flags = np.zeros(max(k, 1), dtype=np.uint8)
    snap.ovr_thr = S.Amounts(k, D)
    snap.thr_ovr_off[:] = 0
    snap.thr_ovr_off[row + 1:] = k
    for o, ov in enumerate(overrides):
        begin, end, values, count = ov[:4]
        if begin is not None:
            snap.ovr_begin_s[o], snap.ovr_begin_ns[o] = begin
        if end is not None:
            snap.ovr_end_s[o], snap.ovr_end_ns[o] = end
        snap.ovr_flags[o] = ov[4] if len(ov) > 4 else 0
        snap.ovr_thr.set_row(o, values, count)
    snap._keep = None
    return snap


def _run(threshold, count=None, n_running=2, each=4, ask=3, **kw):
    """Pod 0 pending and asking ``ask`` of name 0, pods 1 .. n_running running with ``each`` of it, under one throttle."""
    return PR.tiny([{0: ask}] + [{0: each}] * n_running, threshold, count=count, flags=[PR.PENDING] + [PR.COUNTED] * n_running, **kw)


def _error_throttle_timed():
    # preempt_reference's error throttle (its second term does not convert and pod "other" reaches it): the override that is
    # active over the whole window (cpu 5 < the 6 the pod asks) never reaches the check, the stored status (spec: cpu 100) stays
    snap, p, _ = PR.DIRECTED["error-throttle-override-active"]()
    return snap, p


# name -> () -> (snapshot, pod row, instants)
EDGE = [T0, shift(T1, -1), T1, shift(T1, 1), shift(T2, -1), T2, shift(T2, 1), T3, T4]
DIRECTED = {
    # used 8, the pod asks 3: spec 10 blocks (8 + 3 > 10), the override 100 lets it through from T1 to T2, both inclusive
    "window-opens-inclusive": lambda: (timed(_run({0: 10}), 0, [(T1, T2, {0: 100}, None)]), 0, EDGE),
    # the reverse: spec 100 passes, the override 10 blocks from T1 to T2 inclusive and no longer at T2 + 1 ns
    "window-closes-inclusive": lambda: (timed(_run({0: 100}), 0, [(T1, T2, {0: 10}, None)]), 0, EDGE),
    "open-ended-override": lambda: (timed(_run({0: 10}), 0, [(T2, None, {0: 100}, None)]), 0, EDGE),
    "begin-zero-until-end": lambda: (timed(_run({0: 100}), 0, [(None, T1, {0: 10}, None)]), 0, EDGE),
    "begin-equals-end": lambda: (timed(_run({0: 10}), 0, [(T2, T2, {0: 100}, None)]), 0, EDGE),
    # two overlapping overrides: the first wins name 0 (100: passes), the second supplies the count (2: two pods run -> blocked)
    "overlap-first-wins-second-supplies-count": lambda: (
        timed(_run({0: 10}), 0, [(T1, T3, {0: 100}, None), (T2, T4, {0: 5}, 2)]), 0, sorted(EDGE + [shift(T3, 1), shift(T4, 1)])),
    # the second override alone would block name 0 (5 < 8): where only it is active the pod is blocked, where the first is too, not
    "overlap-first-wins-per-name": lambda: (
        timed(_run({0: 10}), 0, [(T1, T2, {0: 100}, None), (T1, T3, {0: 5, 1: 7}, None)]), 0, sorted(EDGE + [shift(T3, 1)])),
    # an active override that omits name 0: the name becomes unthrottled (spec 10 blocked it)
    "override-omits-the-name": lambda: (timed(_run({0: 10}), 0, [(T1, T2, {1: 1}, None)]), 0, EDGE),
    # never reconciled, spec empty, the override (active from T1) empty too: the computed threshold equals the empty stored one by
    # value, nothing is replaced, calculatedAt stays zero and the check keeps reading spec
    "unreconciled-equal-to-empty-stored": lambda: (timed(_run({}), 0, [(T1, T2, {}, None)]), 0, EDGE),
    # ... and with a spec that blocks: the empty override equals the empty stored threshold, the check still reads spec (blocked),
    # although CalculateThreshold itself names nothing between T1 and T2
    "unreconciled-empty-override-keeps-spec": lambda: (timed(_run({0: 10}), 0, [(T1, T2, {}, None)]), 0, EDGE),
    "error-throttle-active-override": lambda: _error_throttle_timed() + (EDGE,),
    # an override threshold below the pod's own request: pod-requests-exceeds-threshold inside the window
    "override-below-the-request": lambda: (timed(_run({0: 100}), 0, [(T1, T2, {0: 2}, None)]), 0, EDGE),
    "never-passes": lambda: (timed(_run({0: 2}), 0, [(T1, T2, {0: 1}, None)]), 0, EDGE),
    # a parse error: never active, whatever its instants say; `begin` parsed (only `end` is bad) or not
    "parse-error-override": lambda: (timed(_run({0: 10}), 0, [(T1, None, {0: 100}, None, S.OVR_PARSE_ERROR | BEGIN_PARSED),
                                                             (None, None, {0: 100}, None, S.OVR_PARSE_ERROR)]), 0, EDGE),
    "parse-error-then-a-good-one": lambda: (timed(_run({0: 10}), 0, [(T1, None, {0: 5}, None, S.OVR_PARSE_ERROR | BEGIN_PARSED),
                                                                    (T2, T3, {0: 100}, None)]), 0, EDGE),
    # used 8 + 2 = 10: at exact equality step 4 passes only without on_equal; used 10 = threshold 10 between T1 and T2: step 3
    # of a Throttle is always on-equal, a ClusterThrottle's follows the caller
    "equality-throttle": lambda: (timed(_run({0: 10}, ask=2), 0, [(T1, T2, {0: 8}, None)]), 0, EDGE),
    "equality-clusterthrottle": lambda: (timed(_run({0: 10}, ask=2, cluster=True), 0, [(T1, T2, {0: 8}, None)]), 0, EDGE),
    # step 3 alone: used 4 + reserved 1 = the override's 5 (used alone is below it: not throttled), and the pod's negative request
    # passes steps 1 and 4 — a Throttle's step 3 is always on-equal, a ClusterThrottle's follows the caller
    "equality-step3-clusterthrottle": lambda: (
        timed(PR.tiny([{1: -1}, {1: 2}, {1: 2}], {1: 100}, cluster=True, flags=[PR.PENDING, PR.COUNTED, PR.COUNTED], reserved=({1: 1}, None)), 0,
              [(T1, T2, {1: 5}, None)]), 0, EDGE),
    "equality-step3-throttle": lambda: (
        timed(PR.tiny([{1: -1}, {1: 2}, {1: 2}], {1: 100}, flags=[PR.PENDING, PR.COUNTED, PR.COUNTED], reserved=({1: 1}, None)), 0,
              [(T1, T2, {1: 5}, None)]), 0, EDGE),
    # a stored status that says "throttled" with a large `used`: every R_t replaces it
    "stale-stored-status": lambda: (timed(_run({0: 10}, stale=True), 0, [(T1, T2, {0: 100}, 9)]), 0, EDGE),
    "count-only-override": lambda: (timed(_run({}, count=2), 0, [(T1, T2, {}, 3)]), 0, EDGE),
    "reserved": lambda: (timed(_run({0: 100}, reserved=({0: 4}, 1)), 0, [(T1, T2, {0: 14}, None), (T3, T4, {0: 15}, 4)]), 0,
                         EDGE + [shift(T4, 1)]),
    "no-throttle-affects-the-pod": lambda: (timed(_run({0: 1}, pod_ns=[2, 0, 0]), 0, [(T1, T2, {0: 0}, 0)]), 0, EDGE),
    "pod-in-a-namespace-without-object": lambda: (timed(_run({0: 100}, pod_ns=[1, 0, 0], cluster=True), 0, [(T1, T2, {0: 1}, None)]), 0, EDGE),
}
