"""The operational reference of the elastic gang forecast (kt_forecast_gangs_elastic_launch), shared by
tests/test_forecast_gangs_elastic_cpu.py and tests/test_forecast_gangs_elastic_gpu.py.

For every instant t_k: forecast_reference.state_at — a copy of the snapshot with the oracle's reconcile at t_k written into the
stored status — then the oracle's in-order admission of the gang's members in that copy.  That admission walks past a member that
failed and reserves on Success only, so its summary words ARE the success list of the elastic walk; the rule (quorum, required
members, members that never succeed), the count, the verdict and the blocker are applied to that list here.  Nothing here shares
code with the kernel or with a host model."""
import functools
import random

import numpy as np

import forecast_gangs_reference as FG
import forecast_reference as FR
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState

A, B, ERR = S.VERDICT_ALLOW, S.VERDICT_BLOCK, S.VERDICT_ERROR


def never_succeeds(snap, oracle_mod, members):
    """Per member: its row is invalid, or the oracle's PreFilter of it is an Error (neither depends on the instant)."""
    _, summary = oracle_mod.Oracle(snap).check(rows=np.asarray(members, np.int64), want_status=False)
    return [not int(snap.pod_flags[p]) & S.POD_VALID or (int(w) & 3) == ERR for p, w in zip(members, summary)]


def successes(snap, oracle_mod, members, instants, on_equal=False, states=None):
    """[len(instants)][len(members)] bool: member j succeeds at t_k when the gang is walked in order in R_{t_k}."""
    rows = np.asarray([int(p) for p in members], np.int64)
    out = []
    for k, t in enumerate(instants):
        s = states[k] if states is not None else FR.state_at(snap, oracle_mod, t)
        _, summary, _ = oracle_mod.Oracle(s).admit(rows=rows, on_equal=on_equal)
        out.append([not int(summary[j]) & 3 and bool(int(snap.pod_flags[p]) & S.POD_VALID) for j, p in enumerate(rows)])
    return out


def rule(ok_lists, never, quorum, required):
    """The elastic rule on the success lists -> (first, verdicts, counts, blockers)."""
    size = len(never)
    required = [bool(x) for x in required] if required is not None else [False] * size
    out_of_reach = any(n and r for n, r in zip(never, required)) or size - sum(never) < quorum
    verdicts, counts, blockers = [], [], []
    for ok in ok_lists:
        count = sum(ok)
        failed = [j for j in range(size) if not ok[j]]
        failed_required = [j for j in failed if required[j]]
        passes = not out_of_reach and count >= quorum and not failed_required
        verdicts.append(ERR if out_of_reach else A if passes else B)
        counts.append(count)
        blockers.append(-1 if passes else failed_required[0] if failed_required else failed[0])
    return FR.first_of([verdicts])[0], verdicts, counts, blockers


def reference(snap, oracle_mod, members, quorum, required, instants, on_equal=False, states=None):
    """-> (first, verdicts, counts, blockers) of the one gang ``members`` (pod rows, in order) under the rule."""
    ok = successes(snap, oracle_mod, members, instants, on_equal, states)
    return rule(ok, never_succeeds(snap, oracle_mod, members), quorum, required)


# ---- the seeded rule of the generators' cases: case 0 is stair_case(seed), case 1 + g gang g of cluster_reference(seed) ----
def seeded_rule(seed, case, size):
    r = random.Random(7919 * seed + 31 * case + 5)
    quorum = r.randint(1, size)
    return quorum, [r.random() < 0.25 for _ in range(size)]


@functools.lru_cache(maxsize=None)
def stair_reference(seed, oracle_mod):
    """(snapshot, members, instants, quorum, required, {on_equal: (first, verdicts, counts, blockers)}, {on_equal: success lists})
    of generator A under the seeded rule — computed once, never modified."""
    snap, members, inst = FG.stair_case(seed)
    quorum, required = seeded_rule(seed, 0, len(members))
    states = [FR.state_at(snap, oracle_mod, t) for t in inst]
    never = never_succeeds(snap, oracle_mod, members)
    ok = {eq: successes(snap, oracle_mod, members, inst, eq, states) for eq in (False, True)}
    want = {eq: rule(ok[eq], never, quorum, required) for eq in (False, True)}
    return snap, members, inst, quorum, required, want, ok


@functools.lru_cache(maxsize=None)
def cluster_reference(seed, oracle_mod):
    """(snapshot, gangs, quorums, required lists, {on_equal: [(first, verdicts, counts, blockers) per gang]}, {on_equal: [success
    lists per gang]}) of generator B over FR.INSTANTS under the seeded rule — computed once, never modified."""
    snap, gangs, _, _ = FG.cluster_reference(seed, oracle_mod)
    rules = [seeded_rule(seed, 1 + g, len(members)) for g, members in enumerate(gangs)]
    states = [FR.state_at(snap, oracle_mod, t) for t in FR.INSTANTS]
    ok = {eq: [successes(snap, oracle_mod, m, FR.INSTANTS, eq, states) for m in gangs] for eq in (False, True)}
    want = {eq: [rule(ok[eq][g], never_succeeds(snap, oracle_mod, m), *rules[g]) for g, m in enumerate(gangs)] for eq in (False, True)}
    return snap, gangs, [q for q, _ in rules], [r for _, r in rules], want, ok


# ---- directed cases: name -> () -> (snapshot, members, quorum, required or None, instants) ----
EDGE = FR.EDGE
T1_TEXT, T2_TEXT = "2026-01-01T01:00:00Z", "2026-01-01T02:00:00Z"  # FR.T1, FR.T2
WINDOW = [k for k, t in enumerate(EDGE) if FR.T1 <= t <= FR.T2]


def _two_throttles(a_threshold, a_window, b_threshold, request):
    """Throttle A selects app=a and carries an override between T1 and T2, throttle B selects tier=x and nothing is used on either.
    m0 {app=a, tier=x}, m1 and m2 {app=b, tier=x}; every member asks ``request`` cpu."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    for name, app in (("m0", "a"), ("m1", "b"), ("m2", "b")):
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": app, "tier": "x"}},
                "spec": {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": request}}}]},
                "status": {"phase": "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "a", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": a_threshold,
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}}]},
                     "temporaryThresholdOverrides": [{"begin": T1_TEXT, "end": T2_TEXT, "threshold": a_window}]}})
    cs.add({"kind": "Throttle", "metadata": {"name": "b", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": b_threshold,
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"tier": "x"}}}]}}})
    pages = cs.build_pages()
    assert len(pages) == 1
    return pages[0].snapshot


def failed_member_reserves_nowhere():
    # outside the window m0 exceeds A (6 > 5) and therefore does NOT weigh on B: m1 passes (6 <= 10), m2 does not (12 > 10).
    # Inside, m0 passes both and reserves 6 on B: m1 and m2 are stopped there
    return _two_throttles({"resourceRequests": {"cpu": "5"}}, {"resourceRequests": {"cpu": "100"}}, {"resourceRequests": {"cpu": "10"}}, "6")


def failed_member_reserves_nowhere_on_a_count():
    # the same on the pod count: A admits no pod outside the window (1 > 0) and 100 inside, B admits one (the second meets a
    # reserved count of 1 at the threshold 1: step 3 of a Throttle is on-equal)
    return _two_throttles({"resourceCounts": {"pod": 0}}, {"resourceCounts": {"pod": 100}}, {"resourceCounts": {"pod": 1}}, "1")


def _by_window(inside, outside):
    return [inside if k in WINDOW else outside for k in range(len(EDGE))]


# name -> (build, members, quorum, required, the answer at on_equal=False derived by hand: (first, verdicts, counts, blockers))
NOWHERE = {
    "quorum-1": ([0, 1, 2], 1, None, (0, [A] * 9, [1] * 9, [-1] * 9)),
    # the override that lets the first member in shuts the required one out
    "quorum-1-m1-required": ([0, 1, 2], 1, [False, True, False], (0, _by_window(B, A), [1] * 9, _by_window(1, -1))),
    "quorum-2": ([0, 1, 2], 2, None, (-1, [B] * 9, [1] * 9, _by_window(1, 0))),
}


def _ghost(position):
    return FG.DIRECTED["member-without-namespace-object-first" if position == 0 else "member-without-namespace-object-last"]()


DIRECTED = {
    # a required Error member first / last: KT_VERDICT_ERROR throughout
    "required-error-member-first": lambda: _ghost(0)[:2] + (1, [True, False, False], EDGE),
    "required-error-member-last": lambda: _ghost(2)[:2] + (1, [False, False, True], EDGE),
    "required-invalid-member-last": lambda: FG.DIRECTED["invalid-member-row-last"]()[:2] + (1, [False, False, True], EDGE),
    # ... and not required: the two valid members decide (inside the window, 2, only one of them fits)
    "error-member-not-required-quorum-2": lambda: _ghost(0)[:2] + (2, None, EDGE),
    "error-member-not-required-quorum-1": lambda: _ghost(2)[:2] + (1, None, EDGE),
    # a quorum that only the Error member puts out of reach: 3 of 3 with one member that never succeeds
    "quorum-out-of-reach-by-the-error-member": lambda: _ghost(2)[:2] + (3, None, EDGE),
    "quorum-out-of-reach-by-the-invalid-member": lambda: FG.DIRECTED["invalid-member-row-first"]()[:2] + (3, None, EDGE),
    "gang-no-throttle-affects": lambda: FG.DIRECTED["gang-no-throttle-affects"]()[:2] + (2, [True, True], EDGE),
    "member-no-throttle-affects": lambda: FG.DIRECTED["member-no-throttle-affects"]()[:2] + (2, [False, True, False], EDGE),
    # the signed and zero-reservation cases of the gang forecast under quorum 1
    "member-order-big-small": lambda: FG.DIRECTED["member-order-big-small"]()[:2] + (1, None, EDGE + [FR.shift(FR.T4, 1)]),
    "member-order-small-big": lambda: FG.DIRECTED["member-order-small-big"]()[:2] + (1, None, EDGE + [FR.shift(FR.T4, 1)]),
    "zero-reservation-makes-present-in-the-window": lambda: FG.DIRECTED["zero-reservation-makes-present-in-the-window"]()[:2] + (1, None, EDGE),
    "zero-reservation-last": lambda: FG.DIRECTED["zero-reservation-last"]()[:2] + (1, None, EDGE),
    "the-blocker-moves-with-the-instant": lambda: FG.DIRECTED["the-blocker-moves-with-the-instant"]()[:2] + (2, [False, False, True], EDGE),
    "error-throttle-keeps-its-stored-status": lambda: FG.DIRECTED["error-throttle-stops-the-second-member-only"]()[:2] + (1, None, EDGE),
    "stored-reserved-amounts": lambda: FG.DIRECTED["stored-reserved-amounts"]()[:2] + (1, None, EDGE),
}
for _name, (_members, _quorum, _required, _) in NOWHERE.items():
    DIRECTED["nowhere-" + _name] = (lambda m=_members, q=_quorum, r=_required: (failed_member_reserves_nowhere(), m, q, r, EDGE))
    DIRECTED["nowhere-count-" + _name] = (lambda m=_members, q=_quorum, r=_required: (failed_member_reserves_nowhere_on_a_count(), m, q, r, EDGE))
