"""The operational reference of the gang forecast (kt_forecast_gangs_launch), shared by tests/test_forecast_gangs_cpu.py and
tests/test_forecast_gangs_gpu.py.

For every instant t_k: forecast_reference.state_at — a copy of the snapshot with the oracle's reconcile at t_k written into the
stored status — then the oracle's in-order admission (PreFilter, and on Success Reserve) of the gang's members in that copy.  The
gang passes iff every member's verdict is Success; the blocker is the first member that is not.  Nothing here shares code with
``paging.forecast_gangs_of`` or the kernel."""
import functools
import random

import numpy as np

import forecast_reference as FR
import preempt_gangs_reference as GR
import preempt_reference as PR
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState

NONE = -1


def reference(snap, oracle_mod, members, instants, on_equal=False, states=None):
    """-> (first, verdicts [len(instants)], blockers [len(instants)]) of the one gang ``members`` (pod rows, in order)."""
    members = [int(p) for p in members]
    rows = np.asarray(members, np.int64)
    ok = GR.members_ok(snap, oracle_mod, members)
    verdicts, blockers = [], []
    for k, t in enumerate(instants):
        s = states[k] if states is not None else FR.state_at(snap, oracle_mod, t)
        _, summary, _ = oracle_mod.Oracle(s).admit(rows=rows, on_equal=on_equal)
        stopped = [j for j, p in enumerate(members) if int(summary[j]) & 3 or not int(snap.pod_flags[p]) & S.POD_VALID]
        blockers.append(stopped[0] if stopped else -1)
        verdicts.append(S.VERDICT_ERROR if not ok else S.VERDICT_BLOCK if stopped else S.VERDICT_ALLOW)
    return FR.first_of([verdicts])[0], verdicts, blockers


def members_and(snap, oracle_mod, members, instants, on_equal=False, states=None):
    """The AND of the members' own verdicts, each checked alone in the same states: what the gang's row would be if the
    members' forecasts composed."""
    own = FR.reference_verdicts(snap, oracle_mod, members, instants, on_equal, states=states)
    return [S.VERDICT_ALLOW if all(int(v) == S.VERDICT_ALLOW for v in own[:, k]) else S.VERDICT_BLOCK for k in range(len(instants))]


# ---- generator A: one throttle whose levels sit on the stairs the members climb ----
INST = sorted(set(FR.EDGE + [FR.shift(FR.T3, -1), FR.shift(FR.T3, 1), FR.shift(FR.T4, 1)]))
STAIR_SEEDS = list(range(60))


def stair_case(seed):
    r = random.Random(1000003 * seed + 17)
    D = r.choice([1, 2, 3]); g = r.randint(1, 5); n_run = r.randint(0, 4)
    def ask(lo):
        return {d: r.randint(lo, 3) for d in range(D) if r.random() < 0.7}
    members = [ask(0) for _ in range(g)]
    running = [ask(1) for _ in range(n_run)]
    used = [sum(q.get(d, 0) for q in running) for d in range(D)]
    def level(d, wide):
        j = r.randint(g - 1, g) if wide else r.randint(0, g)
        return max(0, used[d] + sum(q.get(d, 0) for q in members[:j]) + (r.choice([0, 1, 2]) if wide else r.choice([-1, 0, 0, 1])))
    def count_level(wide):
        return max(0, n_run + (g + r.choice([0, 1]) if wide else r.randint(0, g) + r.choice([-1, 0, 0, 1])))
    def amount(wide=False):
        vals = {d: level(d, wide) for d in range(D) if r.random() < 0.6}
        return vals, (count_level(wide) if r.random() < 0.4 else None)
    reserved = None
    if r.random() < 0.3:
        reserved = ({d: r.randint(0, 1) for d in range(D) if r.random() < 0.5}, r.choice([None, 1]))
    vals, cnt = amount()
    snap = PR.tiny(members + running, vals, count=cnt, cluster=r.random() < 0.5, flags=[PR.PENDING] * g + [PR.COUNTED] * n_run, D=D,
                   reserved=reserved, stale=r.random() < 0.2)
    T = [FR.T1, FR.T2, FR.T3, FR.T4]
    ovr = []
    for _ in range(r.randint(1, 3)):
        a, b = sorted(r.sample(range(4), 2)) if r.random() < 0.85 else (r.randrange(4),) * 2
        begin = None if r.random() < 0.1 else T[a]
        end = None if r.random() < 0.15 else T[b]
        v, c = amount(wide=r.random() < 0.5)
        ovr.append((begin, end, v, c))
    FR.timed(snap, 0, ovr)
    order = list(range(g)); r.shuffle(order)
    return snap, order, INST


@functools.lru_cache(maxsize=None)
def stair_reference(seed, oracle_mod):
    """(snapshot, members, instants, {on_equal: (first, verdicts, blockers)}, {on_equal: the AND of the members' own rows}) —
    computed once, never modified."""
    snap, members, inst = stair_case(seed)
    states = [FR.state_at(snap, oracle_mod, t) for t in inst]
    want = {eq: reference(snap, oracle_mod, members, inst, eq, states=states) for eq in (False, True)}
    alone = {eq: members_and(snap, oracle_mod, members, inst, eq, states=states) for eq in (False, True)}
    return snap, members, inst, want, alone


# ---- generator B: gangs on the manifest clusters of tests/test_forecast_cpu.py ----
def cluster_gangs(seed, snap, n_cases=4):
    """[member rows]: gangs of 1 .. 4 pending pods (the fourth gang, and clusters with too few pending pods, draw from all
    pods) — the drawing of ``preempt_gangs_reference.gang_cases``, without candidates."""
    r = random.Random(32452843 * seed + 11)
    pending = [p for p in range(snap.n_pods) if (int(snap.pod_flags[p]) & PR.COUNTED) == PR.PENDING]
    out = []
    for case in range(n_cases):
        size = r.choice([1, 2, 2, 3, 4])
        pool = pending if len(pending) >= size and case != 3 else list(range(snap.n_pods))
        out.append(r.sample(pool, size))
    return out


@functools.lru_cache(maxsize=None)
def cluster_reference(seed, oracle_mod):
    """(snapshot, gangs, {on_equal: [(first, verdicts, blockers) per gang]}, [a member of the gang is an Error or invalid]) over
    FR.INSTANTS — computed once, never modified."""
    from test_paged_admit_cpu import write_status
    cs = FR.forecast_cluster(seed)
    if seed % 2:
        write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1
    snap = pages[0].snapshot
    gangs = cluster_gangs(seed, snap)
    states = [FR.state_at(snap, oracle_mod, t) for t in FR.INSTANTS]
    want = {eq: [reference(snap, oracle_mod, g, FR.INSTANTS, eq, states=states) for g in gangs] for eq in (False, True)}
    bad = [not GR.members_ok(snap, oracle_mod, g) for g in gangs]
    return snap, gangs, want, bad


# ---- directed cases on snapshots built by hand: name -> () -> (snapshot, members, instants) ----
tiny, timed, PENDING, COUNTED = PR.tiny, FR.timed, PR.PENDING, PR.COUNTED
T1, T2, T3, T4, EDGE = FR.T1, FR.T2, FR.T3, FR.T4, FR.EDGE
P2C1 = [PENDING, PENDING, COUNTED]


def _example(threshold=None, window=None, **kw):
    """Two members asking 3 each, one running pod with 4: under 8 each member alone passes (4 + 3), the gang does not
    (4 + 3 + 3 > 8); the override 10 between T1 and T2 is the only window in which it starts."""
    snap = tiny([{0: 3}, {0: 3}, {0: 4}], {0: 8} if threshold is None else threshold, flags=P2C1, **kw)
    return timed(snap, 0, [(T1, T2, {0: 10} if window is None else window, None)])


def _not_responsible():
    snap = _example()
    snap.thr_flags[0] &= ~np.uint32(S.THR_RESPONSIBLE)
    return snap


def _invalid(position):
    snap = timed(tiny([{0: 1}] * 4, {0: 10}, flags=[PENDING] * 3 + [COUNTED]), 0, [(T1, T2, {0: 2}, None)])
    snap.pod_flags[0] = 0
    return snap, ([0, 1, 2] if position == 0 else [1, 2, 0]), EDGE


def _ghost(position):
    # pod 0 lives in a namespace without object: under a ClusterThrottle its PreFilter is an Error.  Inside the window (2) the
    # second valid member is stopped: with the Error member last the blocker moves in front of it
    snap = timed(tiny([{0: 1}] * 4, {0: 10}, cluster=True, flags=[PENDING] * 3 + [COUNTED], pod_ns=[1, 0, 0, 0]), 0, [(T1, T2, {0: 2}, None)])
    return snap, ([0, 1, 2] if position == 0 else [1, 2, 0]), EDGE


def _error_throttle():
    # The Throttle's second term does not convert and the running pod "other" reaches it: its reconcile is an error and the stored
    # status (never reconciled: spec cpu 10, nothing used) stays at every instant, whatever the override (cpu 100, active over the
    # whole window) says.  The first member (6) passes and reserves, the second (6 + 6 > 10) is stopped
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    for name, app, running in (("first", "a", False), ("second", "a", False), ("other", "b", True)):
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": "6"}}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": app}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "thr", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "10"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}},
                                                    {"podSelector": {"matchExpressions": [{"key": "app", "operator": "Bogus"}]}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": "2026-02-01T00:00:00Z",
                                                      "threshold": {"resourceRequests": {"cpu": "100"}}}]}})
    return cs.build_pages()[0].snapshot, [0, 1], EDGE


def _step3(cluster):
    # the first member (1) passes and reserves; inside the window (5) the second meets used 4 + reserved 1 = 5: step 3 of a
    # Throttle is always on-equal, a ClusterThrottle's follows the caller; its negative request passes steps 1 and 4
    snap = tiny([{1: 1}, {1: -1}, {1: 2}, {1: 2}], {1: 100}, cluster=cluster, flags=[PENDING] * 2 + [COUNTED] * 2)
    return timed(snap, 0, [(T1, T2, {1: 5}, None)]), [0, 1], EDGE


_ZERO = lambda: timed(tiny([{0: 0}, {0: -1}, {1: 1}, {1: 1}], {0: 5}, flags=[PENDING] * 2 + [COUNTED] * 2), 0, [(T1, T2, {0: 0}, None)])
_SIGNED = lambda: timed(tiny([{0: 5}, {0: -2}, {0: 4}], {0: 8}, flags=P2C1), 0, [(T3, T4, {0: 10}, None)])

DIRECTED = {
    "each-alone-passes-the-gang-only-in-the-window": lambda: (_example(), [0, 1], EDGE),
    # one pod runs, the count 2 admits one more: each member alone passes, the gang only under the override's 3
    "the-same-on-a-pod-count": lambda: (timed(tiny([{0: 1}] * 3, {}, count=2, flags=P2C1), 0, [(T1, T2, {}, 3)]), [0, 1], EDGE),
    # used 4, threshold 8: [5, -2] stops at the first member, [-2, 5] passes (4 - 2 + 5); between T3 and T4 (10) both pass
    "member-order-big-small": lambda: (_SIGNED(), [0, 1], EDGE + [FR.shift(T4, 1)]),
    "member-order-small-big": lambda: (_SIGNED(), [1, 0], EDGE + [FR.shift(T4, 1)]),
    # three members of 3: spec 5 stops the second, the override 7 the third, the override 2 the first, the override 9 nobody
    "the-blocker-moves-with-the-instant": lambda: (
        timed(tiny([{0: 3}] * 3, {0: 5}, flags=[PENDING] * 3), 0, [(T1, T1, {0: 7}, None), (T2, T2, {0: 2}, None), (T3, T3, {0: 9}, None)]),
        [0, 1, 2], EDGE),
    # the first member's zero-valued reservation makes name 0 PRESENT in reserved: inside the window (0) step 3 (0 >= 0 on a
    # Throttle) stops the second; in the other order nothing is present when the negative request is judged
    "zero-reservation-makes-present-in-the-window": lambda: (_ZERO(), [0, 1], EDGE),
    "zero-reservation-last": lambda: (_ZERO(), [1, 0], EDGE),
    # stored reserved 2: 4 + 2 + 3 > 8 stops the first member outside the window, 12 admits both (4 + 2 + 3 + 3)
    "stored-reserved-amounts": lambda: (_example(window={0: 12}, reserved=({0: 2}, 1)), [0, 1], EDGE),
    "stored-reserved-count": lambda: (
        timed(tiny([{0: 1}] * 3, {}, count=3, flags=P2C1, reserved=({}, 1)), 0, [(T1, T2, {}, 4)]), [0, 1], EDGE),
    "stale-stored-status": lambda: (_example(stale=True), [0, 1], EDGE),
    "error-throttle-stops-the-second-member-only": _error_throttle,
    "throttle-that-is-not-responsible": lambda: (_not_responsible(), [0, 1], EDGE),
    "equality-step3-throttle": lambda: _step3(False),
    "equality-step3-clusterthrottle": lambda: _step3(True),
    "member-without-namespace-object-first": lambda: _ghost(0),
    "member-without-namespace-object-last": lambda: _ghost(2),
    "invalid-member-row-first": lambda: _invalid(0),
    "invalid-member-row-last": lambda: _invalid(2),
    # the member in the middle lives in the empty namespace: no throttle affects it, it neither is checked nor reserves
    "member-no-throttle-affects": lambda: (
        timed(tiny([{0: 3}, {0: 3}, {0: 3}, {0: 4}], {0: 8}, flags=[PENDING] * 3 + [COUNTED], pod_ns=[0, 2, 0, 0]), 0, [(T1, T2, {0: 10}, None)]),
        [0, 1, 2], EDGE),
    "gang-no-throttle-affects": lambda: (_example(pod_ns=[2, 2, 0]), [0, 1], EDGE),
    # never reconciled, spec empty, the override empty too: nothing is replaced, the check keeps reading spec — which names nothing
    "unreconciled-empty-override-equals-empty-stored": lambda: (_example(threshold={}, window={}), [0, 1], EDGE),
    # ... and with a spec that stops the gang: the empty override is never read
    "unreconciled-empty-override-keeps-spec": lambda: (_example(window={}), [0, 1], EDGE),
}
