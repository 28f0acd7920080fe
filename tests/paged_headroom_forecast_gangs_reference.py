"""The operational reference of the paged gang headroom forecast (kt_paged_headroom_forecast_gangs), shared by
tests/test_paged_headroom_forecast_gangs_cpu.py and tests/test_paged_headroom_forecast_gangs_gpu.py.

For every instant t_k: ``paged_forecast_gangs_reference.states_at`` — a copy of every page, the oracle's reconcile per page at t_k
with the ``calc_updated`` and ``error`` bytes OR-ed over the pages before ``apply_status``.  On a copy of that state ``cap``
consecutive copies of the gang are walked as ``paged_forecast_gangs_reference.first_blocked_in`` walks one: per member the oracle's
check per page, combined with ``paging.combine_status``; on Success the oracle's admit of the one pod per page, stored as that
copy's reserved rows, which persist from copy to copy.  copies = the index of the first copy with a stopped member (``cap``:
none), blocker = that member's place inside the gang, limiting = the lowest row of its COMBINED status that is neither
not-affected nor not-throttled (-1 on an Error).  A gang with an Error or invalid member reports 0 copies: the walk of copy 0 ends
at that member at the latest, and an earlier member that is stopped is the blocker.  Nothing here shares code with
``paging.paged_headroom_forecast_gangs_of`` or the kernel."""
import functools

import numpy as np

import forecast_reference as FR
import headroom_forecast_gangs_reference as HFGR
import paged_forecast_gangs_reference as PFGR
import paged_forecast_reference as PFR
import paged_preempt_reference as PPR
import preempt_reference as PR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState

NOW, NONE = FR.NOW, -1
CAP = 6          # the random cases' cap: chosen with CASES on the reference (the counts stand beside the CPU file's coverage test)
DIRECTED_CAP = 8
PENDING, COUNTED = PR.PENDING, PR.COUNTED
T1, T2, T3, T4, EDGE = FR.T1, FR.T2, FR.T3, FR.T4, FR.EDGE
first_of, queue_of, has_negative_request = HFGR.first_of, HFGR.queue_of, HFGR.has_negative_request


def _active(status_row, t):
    return int(status_row[t]) not in (S.NOT_AFFECTED, S.NOT_THROTTLED)


def walk(state, oracle_mod, members, cap, on_equal):
    """(copies, limiting, blocker position inside the gang, the limiting row's deciding amount lies off page 0) of ``cap``
    consecutive copies of ``members`` on a copy of the reconciled pages ``state``."""
    pages = [PR.copy_snapshot(s) for s in state]
    for j in range(cap):
        for i, p in enumerate(members):
            if not (0 <= p < pages[0].n_pods and int(pages[0].pod_flags[p]) & S.POD_VALID):
                return j, -1, i, False
            row = np.array([p], np.int64)
            own = [oracle_mod.Oracle(s).check(rows=row, on_equal=on_equal)[0] for s in pages]
            status = paging.combine_status(own)
            verdict = int(paging.verdicts(status)[0])
            if verdict == S.VERDICT_ERROR:
                return j, -1, i, False
            if verdict != S.VERDICT_ALLOW:
                t = int(np.nonzero((status[0] != S.NOT_AFFECTED) & (status[0] != S.NOT_THROTTLED))[0][0])
                return j, t, i, not _active(own[0][0], t)
            for s in pages:  # Reserve on every page: the page's own admission of the one pod, stored as the copy's reserved rows
                _, summary, reserved = oracle_mod.Oracle(s).admit(rows=row, on_equal=on_equal)
                assert not int(summary[0]) & 3, "a page's own verdict is Success whenever the combined one is"
                for t in range(s.n_thr):
                    s.thr_reserved.v[t], s.thr_reserved.present[t] = reserved.v[t], reserved.present[t]
                    s.thr_reserved.count[t], s.thr_reserved.has_count[t] = reserved.count[t], reserved.has_count[t]
    return cap, -1, -1, False


def reference(snaps, oracle_mod, members, instants, cap, want=1, on_equal=False, states=None, detail=False):
    """-> (first, copies [len(instants)], limiting [len(instants)], blocker positions inside the gang [len(instants)]) of the one
    gang ``members`` (pod rows, in order); ``detail``: a fifth list, "the deciding amount lies off page 0" per instant."""
    members = [int(p) for p in members]
    states = PFGR.states_at(snaps, oracle_mod, instants) if states is None else states
    rows = [walk(states[k], oracle_mod, members, cap, on_equal) for k in range(len(instants))]
    copies, limiting, blocker, off = ([r[i] for r in rows] for i in range(4))
    out = (first_of(copies, want), copies, limiting, blocker)
    return out + (off,) if detail else out


def as_fetched(per_gang, gangs, want):
    """[(copies, limiting, blocker inside the gang)] per gang -> (first [n_gangs], copies, limiting, blocker [n_gangs][m]) as the
    call hands them out: the blocker a queue position (gang_off[g] added)."""
    _, off = queue_of(gangs)
    first = [first_of(r[0], want) for r in per_gang]
    blocker = [[b + off[i] if b >= 0 else -1 for b in r[2]] for i, r in enumerate(per_gang)]
    return first, [list(r[0]) for r in per_gang], [list(r[1]) for r in per_gang], blocker


def own_states(snaps, oracle_mod, instants):
    """Per page, on its own: ``forecast_reference.state_at`` per instant (what ``headroom_forecast_gangs_reference.reference`` takes)."""
    return [[FR.state_at(s, oracle_mod, t) for t in instants] for s in snaps]


def min_of_pages(snaps, oracle_mod, members, instants, cap, on_equal=False, states=None):
    """The pages' own single-engine references combined by minimum: what the copies would be if the pages' answers composed."""
    states = own_states(snaps, oracle_mod, instants) if states is None else states
    rows = [HFGR.reference(s, oracle_mod, members, instants, cap, 1, on_equal, states=st)[1] for s, st in zip(snaps, states)]
    return [min(int(r[k]) for r in rows) for k in range(len(instants))]


# ---- random wide clusters: paged_forecast_reference.wide_forecast_cluster with loosened thresholds ----
# (seed, factor): the thresholds of the cluster times ``factor`` (test_paged_admit_cpu.loosen).  Chosen on the CPU, in a search of
# the seeds 0 .. 47 at the factors 2, 4, 8 and 16 and of the caps 4, 6 and 8, over the clusters without a negative request, so that
# the REFERENCE alone meets the conditions of test_paged_headroom_forecast_gangs_cpu.test_the_cases_are_not_vacuous.  (None of these
# clusters holds a negative request: wide_reference asserts it instead of filtering.)  Odd seeds — 13, 29, 37 — have a written-back
# status.  (12, 8) and (46, 4) meet every condition on their own; the page shapes are 16 + 12, 16 + 16 + 6, 16 + 6, 16 + 16 + 7,
# 16 + 16 + 5 and 16 + 16 + 8 names.
CASES = [(10, 4), (12, 8), (13, 8), (29, 4), (37, 4), (46, 4)]
GPU_CASES = [(10, 4), (12, 8), (37, 4), (46, 4)]


def wide_case(seed, factor, oracle_mod):
    """(page snapshots, gangs): odd seeds with a status written back by a reconcile, even seeds never reconciled."""
    return PFGR.wide_case(seed, factor, oracle_mod)


@functools.lru_cache(maxsize=None)
def wide_reference(seed, factor, oracle_mod, cap=CAP):
    """(page snapshots, gangs, {on_equal: [(copies, limiting, blocker inside the gang, off page 0) per gang]}) over FR.INSTANTS at
    ``cap`` — computed once, never modified."""
    snaps, gangs = wide_case(seed, factor, oracle_mod)
    assert not any(has_negative_request(s) for s in snaps), "the call refuses such pages: the seed does not belong in the list"
    states = PFGR.states_at(snaps, oracle_mod, FR.INSTANTS)
    want = {eq: [reference(snaps, oracle_mod, g, FR.INSTANTS, cap, 1, eq, states=states, detail=True)[1:] for g in gangs] for eq in (False, True)}
    return snaps, gangs, want


# ---- directed cases: two pages of hand-built throttles; EDGE's positions 2 .. 5 lie in [T1, T2], 7 and 8 are T3 and T4 ----
IN = [2, 3, 4, 5]
P2C1 = [PENDING, PENDING, COUNTED]
P2C2 = [PENDING, PENDING, COUNTED, COUNTED]
_timed = PFGR._timed


def _row(inside, outside, m=len(EDGE)):
    return [inside if k in IN else outside for k in range(m)]


def both_accumulators():
    """``another_page_replaces_the_threshold`` with numbers on both sides (``paged_headroom_forecast_reference.both_accumulators``
    for a gang).  Page 0: the members ask 2 and 1 (one copy reserves 3), two running pods hold 4 each (`used` 8), spec {0: 14}; the
    stored calculatedThreshold is {0: 20} with calculatedAt unset.  Page 1 holds NOTHING the members ask (the running pods hold 1
    under no spec) and stores an empty calculated threshold.  Two windows, in both of which page 0 computes {0: 20} — what it
    stores: it never says `differs` inside a window.
      [T1, T2]: page 1's override names {0: 5} != {}: the throttle is replaced as a whole, the CALCULATED threshold 20 is read on
                every page.  Copy j: member 1 meets 8 + 3 j + 3.  on_equal False: <= 20 up to j = 3; copy 4: member 0 meets used +
                reserved = 20 >= 20 at step 3 (always on-equal on a Throttle): 4 copies, blocker 0.  on_equal True: copy 3's member
                1 meets 20 >= 20: 3 copies, blocker 1.  The spec side would say 2 / 1.
      [T3, T4]: page 1's override names nothing, {} is what it stores: no page differs, calculatedAt is unset: SPEC 14 is read.
                on_equal False: copy 1's member 1 meets 14 > 14: no; copy 2's member 0 meets 8 + 6 = 14 >= 14 at step 3: 2 copies,
                blocker 0.  on_equal True: copy 1's member 1 meets 14 >= 14: 1 copy, blocker 1.
      outside:  page 0 computes spec {0: 14} != its stored {0: 20}: replaced, the calculated threshold IS spec: as [T3, T4]."""
    snaps = PPR.pages_of([[{0: 2}, {0: 1}, {0: 4}, {0: 4}], [{}, {}, {0: 1}, {0: 1}]], [{0: 14}, {}], P2C2)
    snaps = _timed(snaps, [[(T1, T2, {0: 20}, None), (T3, T4, {0: 20}, None)], [(T1, T2, {0: 5}, None), (T3, T4, {}, None)]])
    snaps[0].thr_calc.set_row(0, {0: 20}, None)
    snaps[0]._keep = None
    return snaps, [0, 1], EDGE + [FR.shift(T4, 1)]


def zero_reservation_makes_present():
    """``paged_forecast_gangs_reference.zero_reservation_makes_present`` without its negative request (the call refuses such
    pages), as ``headroom_forecast_gangs_reference``'s zero-valued name on page 1 (names 0 and 1): member 0 carries name 1 with value
    0, so from member 1 of copy 0 on the name is PRESENT in page 1's reserved row with value 0; in [T1, T2] the threshold names it
    with 0.  Nobody asks a non-zero amount of it, so it never decides: what decides is page 1's name 0 — both members ask 1, a
    running pod holds 2, under 12 inside and outside.  Copy j: member 1 meets 2 + 2 j + 2.  on_equal False: <= 12 up to j = 4; copy
    5's member 0 meets 12 >= 12 at step 3: 5 copies, blocker 0.  on_equal True: copy 4's member 1 meets 12 >= 12: 4 copies, blocker
    1.  Page 0 has one name under no threshold."""
    snap0 = PR.tiny([{0: 1}] * 3, {}, flags=P2C1)
    snap1 = PR.tiny([{0: 1, 1: 0}, {0: 1}, {0: 2}], {0: 12}, flags=P2C1)
    return _timed([snap0, snap1], [[(T1, T2, {}, None)], [(T1, T2, {0: 12, 1: 0}, None)]]), [0, 1], EDGE


def tie_across_pages():
    """Rows 0 and 1 both select the members, who ask 2 and 1 of each page's name against a `used` of 8.  Row 0 is limited by page
    0's name under 14 throughout: 2 copies and blocker 0 (on_equal: 1 and blocker 1), as [T3, T4] of ``both_accumulators``.  Row 1
    is limited by page 1's name: spec 11 — on_equal False: copy 0's member 1 meets 11 > 11: no; copy 1's member 0 meets 11 >= 11 at
    step 3: 1 copy, blocker 0; on_equal True: copy 0's member 1 meets 11 >= 11: 0 copies, blocker 1 — and 14 in [T1, T2]: there
    both rows report the same (copies, blocker) and the LOWER row limits."""
    reqs = [{0: 2}, {0: 1}, {0: 4}, {0: 4}]
    s0 = PR.tiny(reqs, {}, flags=P2C2, D=1, T=2, row=1)
    s1 = PR.tiny(reqs, {0: 11}, flags=P2C2, D=1, T=2, row=1)
    s0.thr_spec.set_row(0, {0: 14}, None)
    return [FR.timed(s, 1, ov) for s, ov in zip([s0, s1], [[(T1, T2, {}, None)], [(T1, T2, {0: 14}, None)]])], [0, 1], EDGE


def reserved_on_page_1_only():
    """Page 1's row alone holds a reserved amount, present for its name (4) and for the count (1).  The name: one copy reserves 3
    against `used` 8 + 4 under 100 (all 8 copies), under 21 in [T1, T2]: copy j's member 1 meets 12 + 3 j + 3.  on_equal False: <= 21
    up to j = 2; copy 3's member 0 meets 21 >= 21 at step 3: 3 copies, blocker 0 (without the reserved 4: 4 copies).  on_equal
    True: copy 2's member 1 meets 21 >= 21: 2 copies, blocker 1.  The pod count is page 0's, whose reserved count is absent; the
    count threshold of 40 is out of reach of 8 copies of two pods either way."""
    snaps = PPR.pages_of([[{0: 1}] * 4, [{0: 2}, {0: 1}, {0: 4}, {0: 4}]], [{}, {0: 100}], P2C2, counts=[40, 40])
    snaps[1].thr_reserved.set_row(0, {0: 4}, 1)
    return _timed(snaps, [[(T1, T2, {}, 40)], [(T1, T2, {0: 21}, 40)]]), [0, 1], EDGE


def reserved_count_of_page_0():
    """The reserved count that is judged is page 0's: 3 there, two pods running, under 8; one copy reserves 2.  on_equal False: copy
    1's member 1 meets used + reserved = 2 + 3 + 3 = 8 >= 8 at step 3: 1 copy, blocker 1.  on_equal True: copy 1's member 0 meets 2
    + 3 + 2 + 1 = 8 >= 8 at step 4: 1 copy, blocker 0.  Page 1's name (one copy reserves 3 against 8) is out of reach under 100;
    under 11 in [T1, T2] it reports (1 copy, blocker 0) at on_equal False — the earlier member wins the tie in copies — and (0
    copies, blocker 1) at on_equal True (``tie_across_pages``' row 1 outside its window)."""
    snaps = PPR.pages_of([[{0: 1}] * 4, [{0: 2}, {0: 1}, {0: 4}, {0: 4}]], [{}, {0: 100}], P2C2, counts=[8, 8])
    snaps[0].thr_reserved.set_row(0, {}, 3)
    return _timed(snaps, [[(T1, T2, {}, 8)], [(T1, T2, {0: 11}, 8)]]), [0, 1], EDGE


def error_throttle_number_from_page_1():
    """``paged_headroom_forecast_reference.error_throttle_number_from_page_1`` with two pending members: the Throttle's second term
    does not convert and pod "other" reaches it, so its reconcile is an error and the stored status (never reconciled: spec, an
    empty `used`) is read on every page at every instant, whatever the override says.  spec cpu 100 (page 0: one copy reserves 9:
    out of reach of 8 copies) and r19 7 (page 1: the members ask 2 and 1: copy 1's member 1 meets 6; copy 2's member 0 meets 6 + 2
    = 8 > 7 (and >= 7): 2 copies, blocker 0, at both on_equal values)."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    names = {f"example.com/r{k:02d}": "0" for k in range(20)}
    for name, app, cpu, r19, running in (("first", "a", "6", "2", False), ("second", "a", "3", "1", False), ("victim", "a", "4", "0", True),
                                         ("other", "b", "4", "0", True)):
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
    return [b.snapshot for b in cs.build_pages()], [0, 1], PFR.AROUND_END


def _same(copies, limiting, blocker):
    return {eq: (copies, limiting, blocker) for eq in (False, True)}


Z9, C = [0] * 9, DIRECTED_CAP
# name -> (builder of (page snapshots, members, instants), {on_equal: (copies, limiting, blocker inside the gang)} at DIRECTED_CAP),
# derived by hand: in the builders' texts above, and for the builders of paged_forecast_gangs_reference here
DIRECTED = {
    # page 1: `used` 4, the members ask 3 each.  Under spec 8 copy 0's member 1 meets 10 > 8.  Under 10: on_equal False copy 0
    # passes (10 > 10: no) and copy 1's member 0 meets used + reserved = 10 >= 10 at step 3; on_equal True copy 0's member 1 stops
    "reservation-on-the-second-page": (PFGR.reservation_on_the_second_page,
                                       {False: (_row(1, 0), Z9, _row(0, 1)), True: (Z9, Z9, [1] * 9)}),
    "another-page-replaces-the-threshold": (both_accumulators,
                                            {False: ([2, 2, 4, 4, 4, 4, 2, 2, 2, 2], [0] * 10, [0] * 10),
                                             True: ([1, 1, 3, 3, 3, 3, 1, 1, 1, 1], [0] * 10, [1] * 10)}),
    # outside page 1 stops member 0 (9 + 2 > 10); in [T1, T2] page 1 reads 20 and page 0 stops member 1 (8 + 1 + 2 > 10); at T3
    # both read 100: 8 copies reach 8 + 24 and 9 + 24
    "blocker-is-the-minimum-over-pages-per-instant": (PFGR.blocker_is_the_minimum_over_pages_per_instant,
                                                      _same([0] * 7 + [C, 0], [0] * 7 + [-1, 0], [0, 0, 1, 1, 1, 1, 0, -1, 0])),
    # a count of 2 with one pod running, 3 in [T1, T2].  Outside: the gang forecast's text.  Inside, on_equal False: copy 0 passes
    # (3 > 3: no), copy 1's member 0 meets used + reserved = 1 + 2 = 3 >= 3 at step 3; on_equal True: copy 0's member 1 meets 3 >= 3
    "count-judged-once": (PFGR.count_judged_once, {False: (_row(1, 0), Z9, _row(0, 1)), True: (Z9, Z9, _row(1, 0))}),
    # the stored status (an empty `used`) against spec 5: copy 0's member 1 meets 3 + 3 = 6 > 5
    "stored-on-one-page": (PFGR._stored_on_one_page(False), _same(Z9, Z9, [1] * 9)),
    # ... against the stored calculated threshold 6: on_equal False copy 0 passes (6 > 6: no) and copy 1's member 0 meets reserved 6
    # >= 6 at step 3; on_equal True copy 0's member 1 meets 6 >= 6
    "stored-on-one-page-calculated-at-on-page-0": (PFGR._stored_on_one_page(True),
                                                   {False: ([1] * 9, Z9, Z9), True: (Z9, Z9, [1] * 9)}),
    "zero-reservation-makes-present": (zero_reservation_makes_present, {False: ([5] * 9, Z9, Z9), True: ([4] * 9, Z9, [1] * 9)}),
    # 0 copies; outside member 0 passes and the bad member is the blocker (no limiting row), inside `used` 1 >= 1 stops member 0
    "invalid-member": (PFGR._bad_member(False), _same(Z9, _row(0, -1), _row(0, 1))),
    "error-member": (PFGR._bad_member(True), _same(Z9, _row(0, -1), _row(0, 1))),
    "tie-across-pages": (tie_across_pages, {False: (_row(2, 1), _row(0, 1), Z9), True: (_row(1, 0), _row(0, 1), [1] * 9)}),
    "reserved-on-page-1-only": (reserved_on_page_1_only,
                                {False: (_row(3, C), _row(0, -1), _row(0, -1)), True: (_row(2, C), _row(0, -1), _row(1, -1))}),
    "reserved-count-of-page-0": (reserved_count_of_page_0, {False: ([1] * 9, Z9, _row(0, 1)), True: (_row(0, 1), Z9, _row(1, 0))}),
    "error-throttle-number-from-page-1": (error_throttle_number_from_page_1, _same([2] * 5, [0] * 5, [0] * 5)),
}


@functools.lru_cache(maxsize=None)
def directed_reference(name, oracle_mod):
    """(page snapshots, members, instants, {on_equal: (copies, limiting, blocker inside the gang)} from the reference at
    DIRECTED_CAP) — computed once, never modified."""
    snaps, members, inst = DIRECTED[name][0]()
    states = PFGR.states_at(snaps, oracle_mod, inst)
    return snaps, members, inst, {eq: reference(snaps, oracle_mod, members, inst, DIRECTED_CAP, 1, eq, states=states)[1:] for eq in (False, True)}
