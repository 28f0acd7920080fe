"""The operational reference of the paged headroom forecast (kt_paged_headroom_forecast), shared by
tests/test_paged_headroom_forecast_cpu.py and tests/test_paged_headroom_forecast_gpu.py.

For every instant t_k: ``paged_forecast_gangs_reference.states_at`` — a copy of every page, the oracle's reconcile per page at t_k
with the ``calc_updated`` and ``error`` bytes OR-ed over the pages before ``apply_status``.  On a copy of that state the queue
``[p] * cap`` is walked as ``paged_forecast_gangs_reference.first_blocked_in`` walks a gang: the oracle's check per page, combined
with ``paging.combine_status``; on Success the oracle's admit of the one pod per page, stored as that copy's reserved rows.
copies = the position of the first copy that is not admitted (``cap``: none), limiting = the lowest row of that copy's COMBINED
status that is neither not-affected nor not-throttled (-1 at ``cap`` or on an Error).  Nothing here shares code with
``paging.paged_headroom_forecast_of`` or the kernel."""
import functools

import numpy as np

import forecast_reference as FR
import headroom_forecast_reference as HFR
import paged_forecast_gangs_reference as PFGR
import paged_forecast_reference as PFR
import paged_preempt_reference as PPR
import preempt_reference as PR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState

NOW, NONE, CAP = FR.NOW, -1, 16
PENDING, COUNTED = PR.PENDING, PR.COUNTED
T1, T2, T3, T4, EDGE = FR.T1, FR.T2, FR.T3, FR.T4, FR.EDGE
first_of = HFR.first_of


def walk(state, oracle_mod, p, cap, on_equal):
    """(copies, limiting) of the queue [p] * cap on a copy of the reconciled pages ``state``."""
    pages = [PR.copy_snapshot(s) for s in state]
    row = np.array([int(p)], np.int64)
    for j in range(cap):
        status = paging.combine_status([oracle_mod.Oracle(s).check(rows=row, on_equal=on_equal)[0] for s in pages])
        verdict = int(paging.verdicts(status)[0])
        if verdict == S.VERDICT_ERROR:
            return j, -1
        if verdict != S.VERDICT_ALLOW:
            return j, int(np.nonzero((status[0] != S.NOT_AFFECTED) & (status[0] != S.NOT_THROTTLED))[0][0])
        for s in pages:  # Reserve on every page: the page's own admission of the one pod, stored as the copy's reserved rows
            _, summary, reserved = oracle_mod.Oracle(s).admit(rows=row, on_equal=on_equal)
            assert not int(summary[0]) & 3, "a page's own verdict is Success whenever the combined one is"
            for t in range(s.n_thr):
                s.thr_reserved.v[t], s.thr_reserved.present[t] = reserved.v[t], reserved.present[t]
                s.thr_reserved.count[t], s.thr_reserved.has_count[t] = reserved.count[t], reserved.has_count[t]
    return cap, -1


def reference(snaps, oracle_mod, pods, instants, cap, on_equal=False, states=None):
    """-> (copies int64 [len(pods)][len(instants)], limiting int32 alike); an invalid pod row is 0 and -1 throughout, and so is a
    row whose PreFilter is an Error on page 0 (the walk stops at copy 0 with an Error)."""
    states = PFGR.states_at(snaps, oracle_mod, instants) if states is None else states
    copies = np.zeros((len(pods), len(instants)), np.int64)
    limiting = np.full((len(pods), len(instants)), -1, np.int32)
    for i, p in enumerate(pods):
        if not (0 <= int(p) < snaps[0].n_pods and int(snaps[0].pod_flags[int(p)]) & S.POD_VALID):
            continue
        for k in range(len(instants)):
            copies[i, k], limiting[i, k] = walk(states[k], oracle_mod, p, cap, on_equal)
    return copies, limiting


def min_of_pages(snaps, oracle_mod, pods, instants, cap, on_equal=False):
    """The pages' own single-engine references combined by minimum: what the copies would be if the pages' answers composed."""
    return np.minimum.reduce([HFR.reference(s, oracle_mod, pods, instants, cap, on_equal)[0] for s in snaps])


# ---- random wide clusters: paged_forecast_reference.wide_forecast_cluster with loosened thresholds ----
# (seed, factor): the thresholds of the cluster times ``factor`` (test_paged_admit_cpu.loosen).  The counts the REFERENCE alone gives
# over them stand beside test_paged_headroom_forecast_cpu.test_the_cases_are_not_vacuous.
CASES = [(3, 4), (8, 4), (10, 2), (12, 4), (19, 4), (32, 4), (46, 2)]
GPU_CASES = [(10, 2), (12, 4), (19, 4), (46, 2)]


def wide_case(seed, factor, oracle_mod):
    """(page snapshots, pod rows): odd seeds with a status written back by a reconcile, even seeds never reconciled."""
    from test_paged_admit_cpu import loosen, write_status
    cs = PFR.wide_forecast_cluster(seed)
    loosen(cs, factor)
    if seed % 2:
        write_status(cs, oracle_mod)
    snaps = [b.snapshot for b in cs.build_pages()]
    return snaps, FR.forecast_pods(seed, snaps[0], n_pods=6)


@functools.lru_cache(maxsize=None)
def wide_reference(seed, factor, oracle_mod):
    """(page snapshots, pod rows, {on_equal: (copies, limiting)} over FR.INSTANTS at CAP) — computed once, never modified."""
    snaps, pods = wide_case(seed, factor, oracle_mod)
    states = PFGR.states_at(snaps, oracle_mod, FR.INSTANTS)
    return snaps, pods, {eq: reference(snaps, oracle_mod, pods, FR.INSTANTS, CAP, eq, states=states) for eq in (False, True)}


# ---- directed cases: two pages of hand-built throttles; EDGE's positions 2 .. 5 lie in [T1, T2], 7 and 8 are T3 and T4 ----
IN = [2, 3, 4, 5]
RUN = [PENDING, COUNTED, COUNTED]  # pod 0 pending, two pods running


def _row(inside, outside, m=len(EDGE)):
    return [inside if k in IN else outside for k in range(m)]


def _timed(snaps, per_page, row=0):
    """``per_page[k]``: page k's override list for ``FR.timed`` — every page holds every override's times."""
    return [FR.timed(s, row, ov) for s, ov in zip(snaps, per_page)]


def both_accumulators():
    """``paged_forecast_reference.whole_threshold`` with numbers on both sides.  Page 0: the pod asks 3, two running pods hold 4
    each (`used` 8), spec {0: 14}; the stored calculatedThreshold is {0: 20} with calculatedAt unset.  Page 1 holds NOTHING the pod
    asks (its request there is empty; the running pods hold 1 under no spec) and stores an empty calculated threshold.  Two
    windows, in both of which page 0 computes {0: 20} — what it stores: it never says `differs` inside a window.
      [T1, T2]: page 1's override names {0: 5} != {}: the throttle is replaced as a whole, the CALCULATED threshold is read on every
                page: 8 + 3 (j + 1) <= 20: 4 copies (on_equal: < 20: 3).  The spec side would say 2.
      [T3, T4]: page 1's override names nothing, {} is what it stores: no page differs, calculatedAt is unset: SPEC is read: 8 + 3 (j +
                1) <= 14: 2 copies (on_equal: 1).  The calculated side would say 4.
      outside:  page 0 computes spec {0: 14} != its stored {0: 20}: replaced, the calculated threshold IS spec: 2 copies."""
    snaps = PPR.pages_of([[{0: 3}, {0: 4}, {0: 4}], [{}, {0: 1}, {0: 1}]], [{0: 14}, {}], RUN)
    snaps = _timed(snaps, [[(T1, T2, {0: 20}, None), (T3, T4, {0: 20}, None)], [(T1, T2, {0: 5}, None), (T3, T4, {}, None)]])
    snaps[0].thr_calc.set_row(0, {0: 20}, None)
    snaps[0]._keep = None
    return snaps, 0, EDGE + [FR.shift(T4, 1)]


def tie_across_pages():
    """Rows 0 and 1 both select the pod, which asks 3 of each page's name against a `used` of 8.  Row 0 is limited by page 0's name
    under 14 throughout: 2 copies.  Row 1 is limited by page 1's name: spec 11 (1 copy), 14 in [T1, T2] (2 copies): there both
    rows admit 2 and the LOWER row limits.  on_equal: 1 / 0 and 1."""
    s0 = PR.tiny([{0: 3}, {0: 4}, {0: 4}], {}, flags=RUN, D=1, T=2, row=1)
    s1 = PR.tiny([{0: 3}, {0: 4}, {0: 4}], {0: 11}, flags=RUN, D=1, T=2, row=1)
    s0.thr_spec.set_row(0, {0: 14}, None)
    return _timed([s0, s1], [[(T1, T2, {}, None)], [(T1, T2, {0: 14}, None)]], row=1), 0, EDGE


def count_then_a_name_of_the_last_page():
    """A pod count of 5 with two pods running: 2 + j + 1 <= 5: 3 copies (on_equal: 2), judged on page 0.  Page 1's name: the pod
    asks 3 against 8 under 30 (7 copies), under 14 in [T1, T2] (2 copies, on_equal 1): the count limits outside, the name inside."""
    snaps = PPR.pages_of([[{0: 1}] * 3, [{0: 3}, {0: 4}, {0: 4}]], [{}, {0: 30}], RUN, counts=[5, 5])
    return _timed(snaps, [[(T1, T2, {}, 5)], [(T1, T2, {0: 14}, 5)]]), 0, EDGE


def negative_request_on_page_1():
    """``headroom_forecast_reference``'s negative request as page 1: the pod asks 2 of name 0 (`used` 8 under 15: 3 copies, on_equal
    (15 - 8 - 1) // 2 = 3 too) and -1 of name 1 (`used` 4, reserved 1, under 100: the sums shrink, every copy passes).  In [T1, T2]
    name 1's threshold is 5 = used + reserved: step 3, always on-equal on a Throttle, stops copy 0."""
    s0 = PR.tiny([{0: 1}] * 3, {}, flags=RUN)
    s1 = PR.tiny([{0: 2, 1: -1}] + [{0: 4, 1: 2}] * 2, {0: 15, 1: 100}, flags=RUN, reserved=({1: 1}, None))
    return _timed([s0, s1], [[(T1, T2, {}, None)], [(T1, T2, {0: 13, 1: 5}, None)]]), 0, EDGE


def reserved_on_page_1_only():
    """Page 1's row alone holds a reserved amount, present for its name (4) and for the count (1).  The name: the pod asks 3
    against `used` 8 + 4 under 100 (cap), under 21 in [T1, T2]: (21 - 12) // 3 = 3 copies (on_equal 2; without the reserved 4 it
    would be 4).  The pod count is page 0's, whose reserved count is absent; the count threshold of 40 is out of reach of 16 copies
    either way (the pages of a real cluster never disagree about the reserved count, and the walk over per-page checks has no
    rule for pages that do)."""
    snaps = PPR.pages_of([[{0: 1}] * 3, [{0: 3}, {0: 4}, {0: 4}]], [{}, {0: 100}], RUN, counts=[40, 40])
    snaps[1].thr_reserved.set_row(0, {0: 4}, 1)
    return _timed(snaps, [[(T1, T2, {}, 40)], [(T1, T2, {0: 21}, 40)]]), 0, EDGE


def reserved_count_of_page_0():
    """The reserved count that is judged is page 0's: 3 there, two pods running, under 8: 2 + 3 + j + 1 <= 8: 3 copies (on_equal 2).
    In [T1, T2] page 1's name (3 against 8 under 14) admits 2 (on_equal 1)."""
    snaps = PPR.pages_of([[{0: 1}] * 3, [{0: 3}, {0: 4}, {0: 4}]], [{}, {0: 100}], RUN, counts=[8, 8])
    snaps[0].thr_reserved.set_row(0, {}, 3)
    return _timed(snaps, [[(T1, T2, {}, 8)], [(T1, T2, {0: 14}, 8)]]), 0, EDGE


def error_throttle_number_from_page_1():
    """``paged_forecast_reference._error_throttle_wide`` with room: the Throttle's second term does not convert and pod "other"
    reaches it, so its reconcile is an error and the stored status (never reconciled: spec, an empty `used`) is read on every page
    at every instant, whatever the override says.  spec cpu 100 (page 0: 6 (j + 1) <= 100 holds for all 16 copies) and r19 7 (page
    1: the pod asks 2: 2 (j + 1) <= 7: 3 copies; on_equal (7 - 1) // 2 = 3)."""
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
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "100", "example.com/r19": "7"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}},
                                                    {"podSelector": {"matchExpressions": [{"key": "app", "operator": "Bogus"}]}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": PFR.OVR_END_TEXT,
                                                      "threshold": {"resourceRequests": {"cpu": "5", "example.com/r19": "100"}}}]}})
    return [b.snapshot for b in cs.build_pages()], 0, PFR.AROUND_END


def _of_forecast(name):
    def build():
        snaps, p, instants, _ = PFR.DIRECTED[name]()
        return snaps, p, instants
    return build


def _same(copies, limiting):
    return {eq: (copies, limiting) for eq in (False, True)}


# name -> (builder of (page snapshots, pod row, instants), {on_equal: (copies, limiting)} at CAP, derived by hand above)
DIRECTED = {
    # the four snapshots of paged_forecast_reference.DIRECTED.  While the override {r19: 5} is active the pod's r19 request of 1 meets
    # `used` 1 under 5: 4 copies (on_equal 3); afterwards spec {cpu: 1} is below the 2 it asks
    "later-page-replaces-the-threshold": (_of_forecast("later-page-replaces-the-threshold"),
                                          {False: ([4, 4, 4, 0, 0], [0] * 5), True: ([3, 3, 3, 0, 0], [0] * 5)}),
    # ... and with an r19 request of 0 nothing of the calculated threshold is judged: all 16 copies
    "replacing-page-holds-nothing-the-pod-asks": (_of_forecast("replacing-page-holds-nothing-the-pod-asks"),
                                                  _same([16, 16, 16, 0, 0], [-1, -1, -1, 0, 0])),
    "error-throttle-stopping-name-on-page-1": (_of_forecast("error-throttle-stopping-name-on-page-1"), _same([0] * 5, [0] * 5)),
    # two pods run under a count of 2: nobody; under the override's 3 one copy (on_equal: 2 + 1 >= 3: nobody)
    "count-only-override": (_of_forecast("count-only-override"), {False: (_row(1, 0), [0] * 9), True: ([0] * 9, [0] * 9)}),
    "both-accumulators": (both_accumulators, {False: ([2, 2, 4, 4, 4, 4, 2, 2, 2, 2], [0] * 10), True: ([1, 1, 3, 3, 3, 3, 1, 1, 1, 1], [0] * 10)}),
    "tie-across-pages": (tie_across_pages, {False: (_row(2, 1), _row(0, 1)), True: (_row(1, 0), _row(0, 1))}),
    "count-then-a-name-of-the-last-page": (count_then_a_name_of_the_last_page, {False: (_row(2, 3), [0] * 9), True: (_row(1, 2), [0] * 9)}),
    "negative-request-on-page-1": (negative_request_on_page_1, _same(_row(0, 3), [0] * 9)),
    "reserved-on-page-1-only": (reserved_on_page_1_only, {False: (_row(3, 16), _row(0, -1)), True: (_row(2, 16), _row(0, -1))}),
    "reserved-count-of-page-0": (reserved_count_of_page_0, {False: (_row(2, 3), [0] * 9), True: (_row(1, 2), [0] * 9)}),
    "error-throttle-number-from-page-1": (error_throttle_number_from_page_1, _same([3] * 5, [0] * 5)),
}


@functools.lru_cache(maxsize=None)
def directed_reference(name, oracle_mod):
    """(page snapshots, pod row, instants, {on_equal: (copies list, limiting list)} from the reference) — computed once."""
    snaps, p, inst = DIRECTED[name][0]()
    states = PFGR.states_at(snaps, oracle_mod, inst)
    out = {}
    for eq in (False, True):
        copies, limiting = reference(snaps, oracle_mod, [p], inst, CAP, eq, states=states)
        out[eq] = (copies[0].tolist(), limiting[0].tolist())
    return snaps, p, inst, out
