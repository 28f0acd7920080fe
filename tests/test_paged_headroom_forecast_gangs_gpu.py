"""kt_paged_headroom_forecast_gangs on the GPU: how many copies of a whole gang the throttles admit at each instant, over pages of
resource names (csrc/kt_kernels_headroom_forecast_gangs_paged.hip), held to tests/paged_headroom_forecast_gangs_reference.py (per
instant: oracle reconcile per page, OR of the bytes, then ``cap`` copies of the gang walked member by member over per-page oracle
checks and admits) and to ``paging.paged_headroom_forecast_gangs_of`` — exact, integers and bytes — for both isThrottledOnEqual
values.  The shapes are the smallest at which the kernel can still go wrong: one case per DT instantiation with the deciding name
on page 0 and on the last page, pages of unequal widths in both orders, instant blocks of 64 with the per-position triple carried
across pages, and the identities of the header."""
import functools

import numpy as np
import pytest

import forecast_reference as FR
import headroom_forecast_gangs_reference as HFGR
import paged_headroom_forecast_gangs_reference as R
import paged_headroom_forecast_reference as PHFR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

pytestmark = pytest.mark.gpu
NOW, CAP, DCAP = R.NOW, R.CAP, R.DIRECTED_CAP
P2C2 = R.P2C2


def _engines(snaps, **kw):
    return [E.Engine.for_snapshot(s, **kw) for s in snaps]


def _close(engs):
    for e in engs:
        e.close()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def ask(engs, gangs, inst, cap, want=1, on_equal=False, **kw):
    """All gangs in ONE call -> (first [n_gangs], copies, limiting, blocker [n_gangs][m]) as lists (None where left out)."""
    rows, off = R.queue_of(gangs)
    out = E.paged_headroom_forecast_gangs(engs, rows, off, inst, cap=cap, want=want, on_equal=on_equal, **kw)
    first, copies, limiting, blocker = out
    assert first.dtype == np.int64 and first.shape == (len(gangs),)
    for a, dt in ((copies, np.int64), (limiting, np.int32), (blocker, np.int64)):
        assert a is None or (a.dtype == dt and a.shape == (len(gangs), len(inst)))
    if blocker is not None:
        for g in range(len(gangs)):
            assert all(b == -1 or off[g] <= b < off[g + 1] for b in blocker[g].tolist()), (g, blocker[g].tolist())
    return tuple(None if a is None else a.tolist() for a in out)


def by_model(snaps, gangs, inst, cap, want=1, on_equal=False):
    ctx = paging.paged_preempt_context(snaps, inst[0])
    out = [paging.paged_headroom_forecast_gangs_of(snaps, g, inst, cap, want, on_equal, ctx=ctx) for g in gangs]
    return R.as_fetched([r[1:] for r in out], gangs, want)


def held_to_everything(snaps, oracle_mod, gangs, inst, cap=DCAP, want=1, on_equal=False, reference=None):
    """The engines' answer is the reference's and the model's -> (first, copies, limiting, blocker) as lists.  ``reference``:
    [(copies, limiting, blocker inside the gang)] per gang where it has been computed already."""
    if reference is None:
        states = R.PFGR.states_at(snaps, oracle_mod, inst)
        reference = [R.reference(snaps, oracle_mod, g, inst, cap, want, on_equal, states=states)[1:] for g in gangs]
    engs = _engines(snaps)
    try:
        got = ask(engs, gangs, inst, cap, want, on_equal)
    finally:
        _close(engs)
    assert got == R.as_fetched(reference, gangs, want), f"cap={cap} want={want} on_equal={on_equal}: the reference"
    assert got == by_model(snaps, gangs, inst, cap, want, on_equal), f"cap={cap} want={want} on_equal={on_equal}: the model"
    return got


# ---- kernel and model against the reference ----
@pytest.mark.parametrize("seed,factor", R.GPU_CASES)
def test_random_wide_clusters(seed, factor, oracle_mod):
    snaps, gangs, want = R.wide_reference(seed, factor, oracle_mod)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            expected = R.as_fetched([w[:3] for w in want[on_equal]], gangs, 2)
            got = ask(engs, gangs, FR.INSTANTS, CAP, 2, on_equal)  # all gangs of the cluster's cases in one call
            assert got == expected, f"seed {seed} on_equal={on_equal}"
            assert got == by_model(snaps, gangs, FR.INSTANTS, CAP, 2, on_equal)
            # every nullable output left out in turn: the others are the same bytes
            for k, name in ((1, "want_copies"), (2, "want_limiting"), (3, "want_blocker")):
                less = ask(engs, gangs, FR.INSTANTS, CAP, 2, on_equal, **{name: False})
                assert less[k] is None and [a for i, a in enumerate(less) if i != k] == [a for i, a in enumerate(got) if i != k], name
    finally:
        _close(engs)


@pytest.mark.parametrize("name", sorted(R.DIRECTED))
def test_directed(name, oracle_mod):
    snaps, members, inst, ref = R.directed_reference(name, oracle_mod)
    for on_equal in (False, True):
        answer = tuple(list(x) for x in R.DIRECTED[name][1][on_equal])
        assert ref[on_equal] == answer
        held_to_everything(snaps, oracle_mod, [members], inst, DCAP, 2, on_equal, reference=[answer])


# ---- shapes at which the kernel can go wrong ----
@pytest.mark.parametrize("widths", [(1, 1), (8, 3), (3, 16), (16, 3)], ids=lambda w: "x".join(map(str, w)))
def test_every_instantiation_and_unequal_widths(widths, oracle_mod):
    """One throttle over pages of these widths: the widest page picks the instantiation (D = 1: DT 4, 8: DT 8, 16: DT 16), and a
    three-name page stands beside a sixteen-name page in both orders.  The members ask 2 and 1 of the LAST name of page 0 and of
    the LAST name of the last page, `used` is 8 of each (the running pods hold 2 of every other name).  One copy reserves 3.
      outside:  page 0's name under 30 (7 copies), the last page's under 20: 4 copies, then copy 4's member 0 meets 8 + 12 >= 20 at
                step 3 (on_equal: copy 3's member 1 meets 20 >= 20: 3 copies, blocker 1): the last name of the last page decides.
      [T1, T2]: page 0's name under 14: 2 copies, blocker 0 (on_equal: 1, blocker 1): page 0 decides.
      [T3, T4]: the last page's name under 11: 1 copy, blocker 0 (on_equal: 0, blocker 1).
    The second gang holds the same members in the other order: the same copies, its blockers are queue positions 2 and 3."""
    d0, dl, last = widths[0] - 1, widths[-1] - 1, len(widths) - 1
    snaps, per_page = [], []
    for k, D in enumerate(widths):
        d = d0 if k == 0 else dl
        running = {x: 2 for x in range(D)}
        running[d] = 4
        snaps.append(PR.tiny([{d: 2}, {d: 1}, running, running], {d: 30 if k == 0 else 20}, flags=P2C2, D=D))
        per_page.append([(FR.T1, FR.T2, {d: 14 if k == 0 else 20}, None), (FR.T3, FR.T4, {d: 30 if k == 0 else 11}, None)])
    assert last == 1
    snaps = [FR.timed(s, 0, ov) for s, ov in zip(snaps, per_page)]
    assert tuple(s.D for s in snaps) == widths
    inst = FR.EDGE + [FR.shift(FR.T4, 1)]
    for on_equal, row, blk in ((False, [4, 4, 2, 2, 2, 2, 4, 1, 1, 4], 0), (True, [3, 3, 1, 1, 1, 1, 3, 0, 0, 3], 1)):
        first, copies, limiting, blocker = held_to_everything(snaps, oracle_mod, [[0, 1], [1, 0]], inst, DCAP, 4, on_equal)
        assert copies == [row, row] and limiting == [[0] * 10] * 2 and first == [-1 if on_equal else 0] * 2
        assert blocker[0] == [blk] * 10 and set(blocker[1]) <= {2, 3}


def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


@pytest.mark.parametrize("m,lo,hi", [(65, 64, 64), (65, 63, 64), (65, None, None), (130, 64, 100), (130, 128, 129), (130, 0, 129)])
def test_instant_blocks_the_triple_and_the_ballot(m, lo, hi, oracle_mod):
    """Two pages of one name each; rows 0 and 1 both select the two members, who ask 2 and 1 against a `used` of 8 on either page.
    Row 0's threshold of 15 on page 0 admits 2 copies throughout and stops the first member of the third (8 + 6 + 2 > 15).  Row 1's
    10 on PAGE 1 admits none: the second member is stopped by what the first reserved (8 + 2 + 1 > 10); its override 20 (4 copies)
    is active over positions lo .. hi of the m instants: there row 0 decides, elsewhere row 1."""
    inst = _seconds(m)
    times = (inst[lo], inst[hi]) if lo is not None else (FR.shift(inst[-1], 1), None)
    reqs = [{0: 2}, {0: 1}, {0: 4}, {0: 4}]
    s0 = PR.tiny(reqs, {}, flags=P2C2, D=1, T=2, row=1)
    s1 = PR.tiny(reqs, {0: 10}, flags=P2C2, D=1, T=2, row=1)
    s0.thr_spec.set_row(0, {0: 15}, None)
    snaps = [FR.timed(s0, 1, [times + ({}, None)]), FR.timed(s1, 1, [times + ({0: 20}, None)])]
    inside = [lo is not None and lo <= k <= hi for k in range(m)]
    reference = [R.reference(snaps, oracle_mod, [0, 1], inst, DCAP)[1:]]
    for want in (1, 2):
        first, copies, limiting, blocker = held_to_everything(snaps, oracle_mod, [[0, 1]], inst, DCAP, want, reference=reference)
        assert first == [lo if lo is not None else -1]
        assert copies[0] == [2 if x else 0 for x in inside]
        assert limiting[0] == [0 if x else 1 for x in inside]
        assert blocker[0] == [0 if x else 1 for x in inside]


# ---- the identities of the header ----
@pytest.mark.parametrize("name", sorted(HFGR.DIRECTED))
def test_one_page_is_the_single_engine_launch_on_its_directed_cases(name):
    """(P1)"""
    snap, members, inst = HFGR.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            one = eng.headroom_forecast_gangs(members, [0, len(members)], inst, cap=16, want=2, on_equal=on_equal)
            paged = E.paged_headroom_forecast_gangs([eng], members, [0, len(members)], inst, cap=16, want=2, on_equal=on_equal)
            assert [a.tobytes() for a in one] == [a.tobytes() for a in paged], f"{name} on_equal={on_equal}"
    finally:
        eng.close()


@pytest.mark.parametrize("seed", [1, 3])  # (clusters whose reference copies take at least three values)
def test_one_page_is_the_single_engine_launch(seed, oracle_mod):
    """(P1)"""
    snap, gangs, inst, _ = HFGR.cluster_case(seed, oracle_mod)
    rows, off = R.queue_of(gangs)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            one = eng.headroom_forecast_gangs(rows, off, inst, cap=HFGR.CAP, want=2, on_equal=on_equal)
            paged = E.paged_headroom_forecast_gangs([eng], rows, off, inst, cap=HFGR.CAP, want=2, on_equal=on_equal)
            assert [a.tobytes() for a in one] == [a.tobytes() for a in paged], f"seed {seed} on_equal={on_equal}"
            assert len(set(one[1].ravel().tolist())) >= 3
    finally:
        eng.close()


@pytest.mark.parametrize("seed,factor", PHFR.GPU_CASES[:2])
def test_a_gang_of_one_is_the_paged_headroom_forecast(seed, factor, oracle_mod):
    """(G1)"""
    snaps, pods = PHFR.wide_case(seed, factor, oracle_mod)
    n = len(pods)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            p_first, p_copies, p_limiting = E.paged_headroom_forecast(engs, pods, FR.INSTANTS, cap=PHFR.CAP, want=2, on_equal=on_equal)
            first, copies, limiting, blocker = E.paged_headroom_forecast_gangs(engs, pods, list(range(n + 1)), FR.INSTANTS, cap=PHFR.CAP,
                                                                               want=2, on_equal=on_equal)
            assert first.tobytes() == p_first.tobytes() and copies.tobytes() == p_copies.tobytes() and limiting.tobytes() == p_limiting.tobytes()
            own = np.arange(n, dtype=np.int64)[:, None]
            assert np.array_equal(blocker, np.where(copies < PHFR.CAP, own, -1))
            assert ((copies > 0) & (copies < PHFR.CAP)).any()
    finally:
        _close(engs)


@pytest.mark.parametrize("seed,factor", R.GPU_CASES[:2])
def test_cap_one_is_the_paged_gang_forecast(seed, factor, oracle_mod):
    """(G2)"""
    snaps, gangs = R.wide_case(seed, factor, oracle_mod)
    rows, off = R.queue_of(gangs)
    engs = _engines(snaps)
    try:
        seen = set()
        for on_equal in (False, True):
            f_first, verdicts, f_blocker = E.paged_forecast_gangs(engs, rows, off, FR.INSTANTS, on_equal)
            first, copies, _, blocker = E.paged_headroom_forecast_gangs(engs, rows, off, FR.INSTANTS, cap=1, want=1, on_equal=on_equal)
            assert np.array_equal(copies == 1, verdicts == S.VERDICT_ALLOW) and np.array_equal(copies == 0, verdicts != S.VERDICT_ALLOW)
            assert first.tobytes() == f_first.tobytes() and blocker.tobytes() == f_blocker.tobytes()
            seen |= set(verdicts.ravel().tolist())
        assert {S.VERDICT_ALLOW, S.VERDICT_BLOCK} <= seen
    finally:
        _close(engs)


@functools.lru_cache(maxsize=None)
def _pages_agree(seed, factor, t, oracle_mod):
    """The precondition of (G3) from the per-page oracle reconciles at t: for every responsible throttle every page's calc_updated
    and error byte equals the OR over the pages, and the stored calculatedAt flags agree -> (page snapshots, gangs)."""
    snaps, gangs = R.wide_case(seed, factor, oracle_mod)
    rows = PR.responsible_rows(snaps[0])
    results = [oracle_mod.Oracle(s).reconcile(t, rows=rows) for s in snaps]
    updated = [np.asarray(r.calc_updated[:len(rows)]) != 0 for r in results]
    error = [np.asarray(r.error[:len(rows)]) != 0 for r in results]
    stored = [(s.thr_flags[rows] & np.uint32(S.THR_CALC_AT_NONZERO)) != 0 for s in snaps]
    for per_page in (updated, error, stored):
        assert all(np.array_equal(x, np.logical_or.reduce(per_page)) for x in per_page), (seed, factor, t)
    return snaps, gangs


# (seed, factor) of R.CASES whose pages agree at NOW: found on the CPU with _pages_agree
@pytest.mark.parametrize("seed,factor", [(10, 4), (37, 4)])
def test_single_instant_behind_an_applied_reconcile_is_the_paged_gang_headroom(seed, factor, oracle_mod):
    """(G3)"""
    snaps, gangs = _pages_agree(seed, factor, NOW, oracle_mod)
    rows, off = R.queue_of(gangs)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            E.paged_reconcile(engs, NOW, apply=True)
            _, copies, limiting, blocker = E.paged_headroom_forecast_gangs(engs, rows, off, [NOW], cap=CAP, on_equal=on_equal)
            h_copies, h_limiting, h_blocker = E.paged_headroom_gangs(engs, rows, off, CAP, on_equal)
            assert copies[:, 0].tobytes() == h_copies.tobytes() and limiting[:, 0].tobytes() == h_limiting.tobytes()
            assert blocker[:, 0].tobytes() == h_blocker.tobytes()
    finally:
        _close(engs)


def test_single_instant_where_the_calculated_at_flags_disagree(oracle_mod):
    """(G3), second part: after kt_paged_reconcile(APPLY) page 1 holds the replaced threshold {r19: 5} with calculatedAt set and
    page 0 (whose own byte says nothing to replace) may not.  This call follows the forecast — the throttle has been replaced once
    some page says so — and is held to the reference on snapshots with both flags set: the pod asks 1 of r19 against a `used` of 1
    under 5: 4 copies, then the fifth meets 1 + 4 >= 5 at step 3."""
    from test_paged_forecast_cpu import flags_disagree
    snaps, p, inst, _ = R.PFR.DIRECTED["later-page-replaces-the-threshold"]()
    both, _, _ = flags_disagree(oracle_mod, both=True)
    want = R.reference(both, oracle_mod, [p], [NOW], DCAP)
    assert want == (0, [4], [0], [0])
    engs = _engines(snaps)
    try:
        _, replaced, _ = E.paged_reconcile(engs, NOW, apply=True)
        assert replaced.tolist() == [1]
        assert ask(engs, [[p]], [NOW], DCAP) == ([0], [[4]], [[0]], [[0]])
    finally:
        _close(engs)
    one, p, _ = flags_disagree(oracle_mod, both=False)
    assert [bool(int(s.thr_flags[0]) & S.THR_CALC_AT_NONZERO) for s in one] == [False, True]
    engs = _engines(one)
    try:
        assert ask(engs, [[p]], [NOW], DCAP) == ([0], [[4]], [[0]], [[0]])
    finally:
        _close(engs)


def test_the_dry_run_and_the_slots(oracle_mod):
    """(G4) and the slot rules: reserved amounts and the stored status of every page are unchanged, a pending kt_aggregate_launch
    keeps its sums, every page's reconcile report is dropped, all four forecast fetches of page 0 answer NOT_READY and a pending
    preempt result of page 0 stays fetchable."""
    snaps, members, inst, ref = R.directed_reference("reservation-on-the-second-page", oracle_mod)
    answer = R.as_fetched([ref[False]], [members], 1)
    engs = _engines(snaps)
    other_inst = [NOW, (NOW[0] + 60, 0)]
    try:
        reserved = [e.fetch_reserved() for e in engs]
        plain = [e.reconcile(NOW, apply=False) for e in engs]
        want_pre = [a.copy() for a in engs[0].preempt([0], [2], NOW)]
        for launch in (lambda: engs[0].forecast_launch([0], other_inst), lambda: engs[0].headroom_forecast_launch([0], other_inst, DCAP),
                       lambda: engs[0].forecast_gangs_launch([0], [0, 1], other_inst),
                       lambda: engs[0].headroom_forecast_gangs_launch([0], [0, 1], other_inst, DCAP)):
            launch()
            engs[0].preempt_launch([0], [2], NOW)
            for e in engs:
                e.reconcile_launch(NOW, apply=False)
            engs[1].aggregate_launch()
            assert ask(engs, [members], inst, DCAP) == answer
            # handed out by the call: no forecast result of any kind is pending on page 0
            assert _code(lambda: engs[0].forecast_fetch(1, len(other_inst))) == -5
            assert _code(lambda: engs[0].forecast_gangs_fetch(1, len(other_inst))) == -5
            assert _code(lambda: engs[0].headroom_forecast_fetch(1, len(other_inst))) == -5
            assert _code(lambda: engs[0].headroom_forecast_gangs_fetch(1, len(other_inst))) == -5
            assert [a.tobytes() for a in engs[0].preempt_fetch(1, 1)] == [a.tobytes() for a in want_pre]
            for e in engs:
                assert _code(e.reconcile_fetch) == -5  # every page's reconcile report is dropped
            engs[1].finalize_launch(NOW, apply=False)  # page 1's pending aggregate kept its sums
            got = engs[1].reconcile_fetch()
            assert got.used.v.tobytes() == plain[1].used.v.tobytes() and got.used.present.tobytes() == plain[1].used.present.tobytes()
        # a dry run: reserved amounts and the stored status of every page are unchanged
        for e, before, dry in zip(engs, reserved, plain):
            after = e.fetch_reserved()
            for f in ("v", "present", "count", "has_count"):
                assert getattr(after, f).tobytes() == getattr(before, f).tobytes()
            again = e.reconcile(NOW, apply=False)
            assert again.calc_updated.tobytes() == dry.calc_updated.tobytes() and again.used.v.tobytes() == dry.used.v.tobytes()
        # a larger call grows page 0's result buffers behind an unfetched launch
        engs[0].headroom_forecast_gangs_launch([0], [0, 1], other_inst, DCAP)
        big = _seconds(130)
        first, copies, limiting, blocker = ask(engs, [members, [1, 0]] * 20, big, DCAP)
        assert len(copies) == 40 and all(len(r) == 130 for r in copies) and all(r == copies[0] for r in copies[0::2])
        assert (first[0], copies[0], limiting[0], blocker[0]) == paging.paged_headroom_forecast_gangs_of(snaps, members, big, DCAP)
    finally:
        _close(engs)


def test_refusals_in_order_and_what_a_refused_call_leaves_alone(oracle_mod):
    snaps, members, inst, ref = R.directed_reference("reservation-on-the-second-page", oracle_mod)
    n = snaps[0].n_pods
    engs = _engines(snaps)
    other = E.Engine.for_snapshot(PR.tiny([{0: 1}] * n, {0: 10}, T=3, row=2, D=1))
    inc = E.Engine.for_snapshot(snaps[1], kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    rows, off = np.array(members, np.int64), np.array([0, len(members)], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    call = lambda es, a, g, b, cap=DCAP, want=1: E.paged_headroom_forecast_gangs(es, a, g, b, cap=cap, want=want)
    raw = lambda hs_, k, n_, r, s_, ns_: L.kt_paged_headroom_forecast_gangs(hs_, k, n_, r, 1, off.ctypes.data, 2, s_, ns_, 0, DCAP, 1, None, None,
                                                                             None, None)
    last = lambda: L.kt_last_error(engs[0]._h)

    def every_refusal():
        # 1. the page array, the pages, n
        assert raw(None, 2, 2, rows.ctypes.data, s2.ctypes.data, n2.ctypes.data) == -1
        assert raw(hs, 0, 2, rows.ctypes.data, s2.ctypes.data, n2.ctypes.data) == -1
        assert raw(hs, 2, -1, rows.ctypes.data, s2.ctypes.data, n2.ctypes.data) == -1
        # 2. the instants and a missing array, in front of cap
        assert _code(lambda: call(engs, members, [0, 2], [])) == -1
        assert _code(lambda: call(engs, members, [0, 2], [FR.T2, FR.T1], cap=0)) == -1 and b"ascending" in last()
        assert _code(lambda: call(engs, members, [0, 2], [(NOW[0], 1_000_000_000)])) == -1
        assert raw(hs, 2, 2, None, s2.ctypes.data, n2.ctypes.data) == -1
        assert raw(hs, 2, 2, rows.ctypes.data, None, n2.ctypes.data) == -1
        # 3. cap, then want, in front of the gang offsets
        for cap, w in ((0, 1), (E.HEADROOM_MAX_CAP + 1, 1), (DCAP, 0), (DCAP, DCAP + 1)):
            assert _code(lambda: call(engs, members, [0, 3], inst, cap=cap, want=w)) == -1
        assert _code(lambda: call(engs, members, [0, 3], inst, cap=0, want=0)) == -1 and b"paged headroom forecast gangs: cap = 0" in last()
        assert _code(lambda: call(engs, members, [0, 3], inst, want=DCAP + 1)) == -1 and b"paged headroom forecast gangs: want" in last()
        # 4. the gang offsets and a pod twice within one gang, in front of the page set
        assert _code(lambda: call([engs[0], other], members, [0, 3], inst)) == -1
        assert _code(lambda: call([engs[0], other], members, [1, 2], inst)) == -1
        assert _code(lambda: call([engs[0], other], [0, 0], [0, 2], inst)) == -1 and b"twice" in last()
        # 5. the page set and the rows
        assert _code(lambda: call([engs[0], other], members, [0, 2], inst)) == -1            # different throttle-row counts
        assert _code(lambda: call([engs[0], engs[0]], members, [0, 2], inst)) == -1          # an engine named twice
        engs[1].set_exchange_world(2)
        assert _code(lambda: call(engs, [0, 99], [0, 2], inst)) == -2                        # ... in front of what is unsupported
        # 6. n_gangs x n_inst > 2^31
        assert _code(lambda: call(engs, np.zeros(2**16 + 1, np.int64), np.arange(2**16 + 2), _seconds(2**15))) == -2
        # 7. an engine, asked of every page
        assert _code(lambda: call(engs, members, [0, 2], inst)) == -7
        engs[1].set_exchange_world(1)
        assert _code(lambda: call([engs[0], inc], members, [0, 2], inst)) == -7              # KT_VARIANT_INCREMENTAL
        engs[1].set_wide_sums(1)  # found out by that page's sums kernel, the one thing that runs before the refusal
        assert _code(lambda: call(engs, members, [0, 2], inst)) == -7
        engs[1].set_wide_sums(0)

    try:
        want_check = [a.copy() for a in engs[0].check(rows=np.arange(n), on_equal=False)]
        want_rec = engs[0].reconcile(NOW, apply=False)
        want_pre = [a.copy() for a in engs[0].preempt([0], [2], NOW)]
        want_hf = [a.copy() for a in engs[0].headroom_forecast_gangs(members, [0, 2], inst, cap=DCAP)]
        # a pending check and a pending reconcile report of page 0 ...
        engs[0].check_launch(n, want_status=True)
        engs[0].reconcile_launch(NOW, apply=False)
        every_refusal()
        got = engs[0].reconcile_fetch()
        assert got.used.v.tobytes() == want_rec.used.v.tobytes() and got.calc_updated.tobytes() == want_rec.calc_updated.tobytes()
        status, summary = engs[0].check_fetch(n, True)
        assert status.tobytes() == want_check[0].tobytes() and summary.tobytes() == want_check[1].tobytes()
        # ... and a pending forecast result and a pending preempt result
        engs[0].headroom_forecast_gangs_launch(members, [0, 2], inst, DCAP)
        engs[0].preempt_launch([0], [2], NOW)
        every_refusal()
        assert [a.tobytes() for a in engs[0].preempt_fetch(1, 1)] == [a.tobytes() for a in want_pre]
        assert [a.tobytes() for a in engs[0].headroom_forecast_gangs_fetch(1, len(inst))] == [a.tobytes() for a in want_hf]
        # n == 0 with no gangs: KT_OK, nothing launched; n == 0 with a gang: refused
        first, copies, limiting, blocker = call(engs, [], [0], inst)
        assert first.shape == (0,) and copies.shape == limiting.shape == blocker.shape == (0, len(inst))
        assert _code(lambda: call(engs, [], [0, 0], inst)) == -1
        # the same pod in two gangs is allowed
        assert call(engs, [0, 0], [0, 1, 2], inst)[1].shape == (2, len(inst))
    finally:
        _close(engs + [other, inc])


def test_a_negative_request_on_any_page_is_refused_last(oracle_mod):
    """8.: the search over the copies rests on sums that only grow; the message names the pod-by-pod call, which serves such pages."""
    snaps, p, inst = PHFR.DIRECTED["negative-request-on-page-1"][0]()
    assert not R.has_negative_request(snaps[0]) and R.has_negative_request(snaps[1])
    engs = _engines(snaps)
    try:
        assert _code(lambda: E.paged_headroom_forecast_gangs(engs, [p], [0, 1], inst, cap=DCAP)) == -7
        text = E.lib().kt_last_error(engs[1]._h)
        assert b"page 1 has been fed a negative request" in text and b"(kt_paged_headroom_forecast serves such pages pod by pod)" in text
        assert E.paged_headroom_forecast(engs, [p], inst, cap=PHFR.CAP)[1].tolist() == [PHFR.DIRECTED["negative-request-on-page-1"][1][False][0]]
    finally:
        _close(engs)


def test_paged_engine_headroom_forecast_gangs(oracle_mod):
    import paged_forecast_reference as PFR
    import forecast_gangs_reference as FGR
    from test_paged_admit_cpu import loosen
    cs = PFR.wide_forecast_cluster(46)
    loosen(cs, 4)
    pages = cs.build_pages()
    snaps = [b.snapshot for b in pages]
    assert len(snaps) == 3
    gangs = FGR.cluster_gangs(46, snaps[0])
    rows, off = R.queue_of(gangs)
    pe = paging.PagedEngine(pages)
    try:
        for on_equal in (False, True):
            got = pe.headroom_forecast_gangs(rows, off, FR.INSTANTS, cap=CAP, want=3, on_equal=on_equal)
            assert tuple(a.tolist() for a in got) == by_model(snaps, gangs, FR.INSTANTS, CAP, 3, on_equal)
    finally:
        pe.close()
