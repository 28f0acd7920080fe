"""The operational reference of the paged gang forecast (kt_paged_forecast_gangs), shared by
tests/test_paged_forecast_gangs_cpu.py and tests/test_paged_forecast_gangs_gpu.py.

For every instant t_k: ``paged_preempt_gangs_reference.first_blocked(snaps, oracle, members, [], now=t_k, on_equal)`` — a copy of
every page, the oracle's reconcile per page at t_k with the ``calc_updated`` and ``error`` bytes OR-ed over the pages before
``apply_status``, then the members admitted in order over every page, each admitted member reserving on every page.  The verdict is
Success iff nobody is stopped, the blocker is the first member that is; Error at every instant iff ``members_ok`` is false.  The
reconciled copies of an instant are computed once per case (``states``) and copied again for every gang, because the walk writes
the reservations into them.  Nothing here shares code with ``paging.paged_forecast_gangs_of`` or the kernel."""
import functools

import numpy as np

import forecast_gangs_reference as FGR
import forecast_reference as FR
import paged_forecast_reference as PFR
import paged_preempt_gangs_reference as PPGR
import paged_preempt_reference as PPR
import preempt_reference as PR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

NOW, NONE = FR.NOW, -1
A, B, ERR = S.VERDICT_ALLOW, S.VERDICT_BLOCK, S.VERDICT_ERROR
PENDING, COUNTED = PR.PENDING, PR.COUNTED
T1, T2, T3, T4, EDGE = FR.T1, FR.T2, FR.T3, FR.T4, FR.EDGE


def states_at(snaps, oracle_mod, instants):
    """Per instant the copies of every page with every responsible throttle reconciled at that instant (the OR-ed bytes)."""
    return [PPGR._without(snaps, oracle_mod, [], t) for t in instants]


def first_blocked_in(state, oracle_mod, members, on_equal):
    """``paged_preempt_gangs_reference.first_blocked`` from its second step on, on a copy of the reconciled pages ``state``: the
    position of the first member whose verdict over every page is not Success (None: the gang passes)."""
    copies = [PR.copy_snapshot(s) for s in state]
    for j, p in enumerate(members):
        if not int(copies[0].pod_flags[p]) & S.POD_VALID:
            return j
        row = np.array([int(p)], np.int64)
        status = paging.combine_status([oracle_mod.Oracle(s).check(rows=row, on_equal=on_equal)[0] for s in copies])
        if int(paging.verdicts(status)[0]) != A:
            return j
        for s in copies:  # Reserve on every page: the page's own admission of the one pod, stored as the copy's reserved rows
            _, summary, reserved = oracle_mod.Oracle(s).admit(rows=row, on_equal=on_equal)
            assert not int(summary[0]) & 3, "a page's own verdict is Success whenever the combined one is"
            for t in range(s.n_thr):
                s.thr_reserved.v[t], s.thr_reserved.present[t] = reserved.v[t], reserved.present[t]
                s.thr_reserved.count[t], s.thr_reserved.has_count[t] = reserved.count[t], reserved.has_count[t]
    return None


def reference(snaps, oracle_mod, members, instants, on_equal=False, states=None):
    """-> (first, verdicts [len(instants)], blockers [len(instants)]) of the one gang ``members`` (pod rows, in order)."""
    members = [int(p) for p in members]
    states = states_at(snaps, oracle_mod, instants) if states is None else states
    ok = PPGR.members_ok(snaps, oracle_mod, members)
    verdicts, blockers = [], []
    for k in range(len(instants)):
        b = first_blocked_in(states[k], oracle_mod, members, on_equal)
        blockers.append(-1 if b is None else b)
        verdicts.append(ERR if not ok else A if b is None else B)
    return next((k for k, v in enumerate(verdicts) if v == A), NONE), verdicts, blockers


def members_and(snaps, oracle_mod, members, instants, on_equal=False):
    """The AND of the members' own paged forecasts: what the gang's row would be if the members' forecasts composed."""
    own = PFR.reference_verdicts(snaps, oracle_mod, members, instants, on_equal)
    return [A if all(int(v) == A for v in own[:, k]) else B for k in range(len(instants))]


def own_states(snaps, oracle_mod, instants):
    """Per page, on its own: ``forecast_reference.state_at`` per instant (what ``forecast_gangs_reference.reference`` takes)."""
    return [[FR.state_at(s, oracle_mod, t) for t in instants] for s in snaps]


def pages_combined(snaps, oracle_mod, members, instants, on_equal=False, states=None):
    """The pages' own gang forecasts (the single-engine reference per page snapshot) combined as if the pages were independent:
    Error beats Block beats Success.  ``states``: ``own_states``, computed once per case."""
    states = own_states(snaps, oracle_mod, instants) if states is None else states
    rows = [FGR.reference(s, oracle_mod, members, instants, on_equal, states=st)[1] for s, st in zip(snaps, states)]
    return [max(int(r[k]) for r in rows) for k in range(len(instants))]


# ---- random wide clusters: paged_forecast_reference.wide_forecast_cluster with loosened thresholds ----
# (seed, factor): the thresholds of the cluster times ``factor`` (test_paged_admit_cpu.loosen).  Chosen on the CPU, in a search of the
# seeds 0 .. 44 at the factors 2, 4 and 8, so that the REFERENCE alone meets the counts of
# test_paged_forecast_gangs_cpu.test_the_cases_are_not_vacuous: at these factors gangs of several members sometimes fit, and the
# rows that neither the members' own forecasts nor the pages' own gang forecasts explain are rare (most seeds have none).
CASES = [(3, 4), (4, 4), (10, 2), (12, 4), (32, 4), (46, 2)]
GPU_CASES = [(10, 2), (12, 4), (32, 4), (46, 2)]


def wide_case(seed, factor, oracle_mod):
    """(page snapshots, gangs): odd seeds with a status written back by a reconcile, even seeds never reconciled."""
    from test_paged_admit_cpu import loosen, write_status
    cs = PFR.wide_forecast_cluster(seed)
    loosen(cs, factor)
    if seed % 2:
        write_status(cs, oracle_mod)
    snaps = [b.snapshot for b in cs.build_pages()]
    return snaps, FGR.cluster_gangs(seed, snaps[0])


@functools.lru_cache(maxsize=None)
def wide_reference(seed, factor, oracle_mod):
    """(page snapshots, gangs, {on_equal: [(first, verdicts, blockers) per gang]}, the reconciled copies per instant) over
    FR.INSTANTS — computed once, never modified."""
    snaps, gangs = wide_case(seed, factor, oracle_mod)
    states = states_at(snaps, oracle_mod, FR.INSTANTS)
    want = {eq: [reference(snaps, oracle_mod, g, FR.INSTANTS, eq, states=states) for g in gangs] for eq in (False, True)}
    return snaps, gangs, want, states


# ---- directed cases: two pages of one throttle, built by hand; EDGE's positions 2 .. 5 lie in [T1, T2] ----
IN, OUT = [2, 3, 4, 5], [0, 1, 6, 7, 8]


def _row(inside, outside, m=len(EDGE)):
    return [inside if k in IN else outside for k in range(m)]


def _timed(snaps, per_page):
    """``per_page[k]``: page k's override list for ``FR.timed`` — every page holds every override's times."""
    return [FR.timed(s, 0, ov) for s, ov in zip(snaps, per_page)]


def reservation_on_the_second_page():
    """The header's example on page 1: two members asking 3 each, one running pod with 4, spec 8, the override 10 in [T1, T2];
    page 0 carries 1 each under 100 (the override keeps it at 100).  Never reconciled, so spec / the override differ from the empty
    stored threshold at every instant and the calculated threshold is read.
      outside: member 0 meets 4 + 3 = 7 <= 8 and reserves 3; member 1 meets 4 + 3 + 3 = 10 > 8: blocker 1.
      inside:  member 1 meets 10 against 10: step 4 passes at on_equal False (10 > 10 is false) and stops at on_equal True.
    Each member alone passes everywhere (7 <= 8)."""
    flags = [PENDING, PENDING, COUNTED]
    snaps = PPR.pages_of([[{0: 1}] * 3, [{0: 3}, {0: 3}, {0: 4}]], [{0: 100}, {0: 8}], flags)
    return _timed(snaps, [[(T1, T2, {0: 100}, None)], [(T1, T2, {0: 10}, None)]]), [0, 1], EDGE


def another_page_replaces_the_threshold():
    """The gang version of ``paged_forecast_reference.whole_threshold``.  Page 0: spec {0: 1}, both members ask 2 (step 1 stops
    member 0 whenever spec is read).  Page 1: spec {}, the members ask 1, a running pod holds 1; the override names ONLY page 1's
    name (5) in [T1, T2].  Never reconciled: the stored calculated threshold is empty on both pages.
      inside:  page 0 computes {} — what it stores — but page 1 computes {0: 5} != {}: the throttle is replaced as a whole and
               reads the calculated threshold on EVERY page, which omits page 0's name: nothing stops the gang (1 + 1 + 1 <= 5).
      outside: page 0 computes spec {0: 1} != {}: replaced, spec's values are read, 2 > 1 stops member 0.
    Page 0's own gang forecast: inside the window nothing differs from its stored {}: it keeps reading spec and says blocked at
    every instant."""
    flags = [PENDING, PENDING, COUNTED]
    snaps = PPR.pages_of([[{0: 2}, {0: 2}, {0: 1}], [{0: 1}] * 3], [{0: 1}, {}], flags)
    return _timed(snaps, [[(T1, T2, {}, None)], [(T1, T2, {0: 5}, None)]]), [0, 1], EDGE


def blocker_is_the_minimum_over_pages_per_instant():
    """``paged_preempt_gangs_reference.blocker_is_the_minimum_over_pages`` with instants.  Page 0: `used` 8 under 10, the members
    ask 1 and 2: 8 + 1 passes, 8 + 1 + 2 = 11 > 10 stops member 1.  Page 1: `used` 9 under 10, they ask 2 and 1: 9 + 2 = 11 > 10
    stops member 0.
      outside:       min(1, 0) = 0.
      in [T1, T2]:   page 1 reads 20 (9 + 2 + 1 = 12 passes), page 0 still 10: blocker 1.
      at T3 exactly: both read 100: the gang passes.  T4: as outside."""
    flags = [PENDING, PENDING, COUNTED, COUNTED]
    snaps = PPR.pages_of([[{0: 1}, {0: 2}, {0: 4}, {0: 4}], [{0: 2}, {0: 1}, {0: 5}, {0: 4}]], [{0: 10}, {0: 10}], flags)
    return _timed(snaps, [[(T1, T2, {0: 10}, None), (T3, T3, {0: 100}, None)], [(T1, T2, {0: 20}, None), (T3, T3, {0: 100}, None)]]), [0, 1], EDGE


def count_judged_once():
    """A pod-count threshold of 2 alone, names on two pages under no threshold; one pod runs; the override raises the count to 3
    in [T1, T2].  The reserved count prefix is page 0's only.
      outside, on_equal False: member 0 meets 1 + 0 + 1 = 2 > 2: no; it reserves (count 1).  Member 1: step 3, always on-equal on a
               Throttle: 1 + 1 = 2 >= 2 stops it: blocker 1.
      outside, on_equal True:  member 0: step 4 is 2 >= 2: blocker 0.
      inside,  on_equal False: member 1: step 3 2 >= 3 no, step 4 3 > 3 no: the gang passes.
      inside,  on_equal True:  member 0: 2 >= 3 no; member 1: step 4 3 >= 3: blocker 1."""
    flags = [PENDING, PENDING, COUNTED]
    snaps = PPR.pages_of([[{0: 1}] * 3, [{0: 2}] * 3], [{}, {}], flags, counts=[2, 2])
    return _timed(snaps, [[(T1, T2, {}, 3)]] * 2), [0, 1], EDGE


def _stored_on_one_page(calc_at_on_page_0):
    """Page 0: the members ask 3 each, a running pod holds 4, spec {0: 5}, the override 100 in [T1, T2].  Page 1 names nothing (its
    pods ask 1 under no threshold) and its throttle row keeps its stored status — the row is marked invalid THERE alone, the one
    way two hand-built pages can disagree about it (an error byte on one page alone takes a `used` beyond int64 on that page,
    which the call refuses).  So the stored status is read on EVERY page at every instant, and the override never counts.
    Never reconciled: stored `used` is empty.
      calculatedAt unset: spec 5 is read.  Member 0: 3 <= 5, reserves 3; member 1: 3 + 3 = 6 > 5 (and >= 5): blocker 1 everywhere.
               (Reconciled, `used` 4 would stop member 0 outside the window and nobody inside.)
      calculatedAt set on page 0 only, stored calculated threshold {0: 6}: the stored calculated threshold is read on every page.
               Member 1 meets 6 against 6: passes at on_equal False (first = 0), stopped at on_equal True."""
    def build():
        flags = [PENDING, PENDING, COUNTED]
        snaps = PPR.pages_of([[{0: 3}, {0: 3}, {0: 4}], [{0: 1}] * 3], [{0: 5}, {}], flags)
        snaps = _timed(snaps, [[(T1, T2, {0: 100}, None)], [(T1, T2, {}, None)]])
        snaps[1].thr_flags[0] &= ~np.uint32(S.THR_VALID)
        if calc_at_on_page_0:
            snaps[0].thr_flags[0] |= np.uint32(S.THR_CALC_AT_NONZERO)
            snaps[0].thr_calc.set_row(0, {0: 6}, None)
        return snaps, [0, 1], EDGE
    return build


def zero_reservation_makes_present():
    """``forecast_gangs_reference``'s zero-reservation case as page 1 (names 0 and 1: member 0 carries name 0 with value 0, member
    1 asks -1 of it, the running pods hold name 1; spec {0: 5}, the override {0: 0} in [T1, T2]); page 0 has one name under no
    threshold.  Member 0 requests nothing that is judged and reserves the PRESENCE of page 1's name 0.
      inside:  member 1 meets threshold 0 with a present reserved 0: step 3 (0 >= 0, always on-equal on a Throttle) stops it.
      outside: 0 >= 5 no, -1 > 5 no: the gang passes."""
    flags = [PENDING] * 2 + [COUNTED] * 2
    snap0 = PR.tiny([{0: 1}] * 4, {}, flags=flags)
    snap1 = PR.tiny([{0: 0}, {0: -1}, {1: 1}, {1: 1}], {0: 5}, flags=flags)
    return _timed([snap0, snap1], [[(T1, T2, {}, None)], [(T1, T2, {0: 0}, None)]]), [0, 1], EDGE


def _bad_member(ghost):
    """Three members, the one in the MIDDLE is bad (``ghost``: it lives in a namespace without object and the throttle is a
    ClusterThrottle: its PreFilter is an Error; else its row is invalid on every page).  Page 1: every pod asks 1, one runs,
    spec 10, the override 1 in [T1, T2]; page 0: 1 each under 100.  Verdict Error at every instant.
      outside: member 0 passes (1 + 1 <= 10): the blocker is the bad member, 1.
      inside:  `used` 1 >= 1: the fresh reconcile says throttled (step 2): member 0 is stopped, blocker 0 — in front of the bad one."""
    def build():
        flags = [PENDING] * 3 + [COUNTED]
        kw = dict(cluster=True, pod_ns=[0, 1, 0, 0]) if ghost else {}
        snaps = PPR.pages_of([[{0: 1}] * 4, [{0: 1}] * 4], [{0: 100}, {0: 10}], flags, **kw)
        if not ghost:
            for s in snaps:
                s.pod_flags[1] = 0
        return _timed(snaps, [[(T1, T2, {0: 100}, None)], [(T1, T2, {0: 1}, None)]]), [0, 1, 2], EDGE
    return build


_BAD = {eq: (NONE, [ERR] * len(EDGE), _row(0, 1)) for eq in (False, True)}
# name -> (builder of (page snapshots, members, instants), {on_equal: (first, verdicts, blockers)}), derived by hand above
DIRECTED = {
    "reservation-on-the-second-page": (reservation_on_the_second_page,
                                       {False: (2, _row(A, B), _row(-1, 1)), True: (NONE, [B] * 9, [1] * 9)}),
    "another-page-replaces-the-threshold": (another_page_replaces_the_threshold,
                                            {eq: (2, _row(A, B), _row(-1, 0)) for eq in (False, True)}),
    "blocker-is-the-minimum-over-pages-per-instant": (blocker_is_the_minimum_over_pages_per_instant,
                                                      {eq: (7, [B] * 7 + [A, B], [0, 0, 1, 1, 1, 1, 0, -1, 0]) for eq in (False, True)}),
    "count-judged-once": (count_judged_once, {False: (2, _row(A, B), _row(-1, 1)), True: (NONE, [B] * 9, _row(1, 0))}),
    "stored-on-one-page": (_stored_on_one_page(False), {eq: (NONE, [B] * 9, [1] * 9) for eq in (False, True)}),
    "stored-on-one-page-calculated-at-on-page-0": (_stored_on_one_page(True),
                                                   {False: (0, [A] * 9, [-1] * 9), True: (NONE, [B] * 9, [1] * 9)}),
    "zero-reservation-makes-present": (zero_reservation_makes_present, {eq: (0, _row(B, A), _row(1, -1)) for eq in (False, True)}),
    "invalid-member": (_bad_member(False), _BAD),
    "error-member": (_bad_member(True), _BAD),
}


@functools.lru_cache(maxsize=None)
def directed_reference(name, oracle_mod):
    """(page snapshots, members, instants, {on_equal: (first, verdicts, blockers)} from the reference) — computed once."""
    snaps, members, inst = DIRECTED[name][0]()
    states = states_at(snaps, oracle_mod, inst)
    return snaps, members, inst, {eq: reference(snaps, oracle_mod, members, inst, eq, states=states) for eq in (False, True)}
