"""kt_paged_headroom_forecast on the GPU: how many copies of a pod the throttles admit at each instant, over pages of resource
names, held to tests/paged_headroom_forecast_reference.py (per instant: oracle reconcile per page, OR of the bytes, then the queue
[pod] * cap walked over per-page oracle checks and admits) and to ``paging.paged_headroom_forecast_of`` — exact, integers and
bytes — for both isThrottledOnEqual values."""
import functools

import numpy as np
import pytest

import forecast_reference as FR
import paged_headroom_forecast_reference as R
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

pytestmark = pytest.mark.gpu
NOW, CAP = R.NOW, R.CAP
RUN = R.RUN


def _engines(snaps, **kw):
    return [E.Engine.for_snapshot(s, **kw) for s in snaps]


def _close(engs):
    for e in engs:
        e.close()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def held_to_everything(snaps, oracle_mod, pods, instants, on_equal=False, want=1, cap=CAP, reference=None):
    """The engines' answer is the reference's and the closed form's -> (first list, copies, limiting)."""
    w_copies, w_limiting = R.reference(snaps, oracle_mod, pods, instants, cap, on_equal) if reference is None else reference
    engs = _engines(snaps)
    try:
        first, copies, limiting = E.paged_headroom_forecast(engs, pods, instants, cap=cap, want=want, on_equal=on_equal)
    finally:
        _close(engs)
    assert copies.dtype == np.int64 and limiting.dtype == np.int32 and first.dtype == np.int64
    assert np.array_equal(copies, w_copies), f"on_equal={on_equal}: copies"
    assert np.array_equal(limiting, w_limiting), f"on_equal={on_equal}: limiting"
    assert first.tolist() == R.first_of(w_copies, want), f"on_equal={on_equal}: first"
    ctx = paging.paged_preempt_context(snaps, instants[0])
    for i, p in enumerate(pods):
        assert paging.paged_headroom_forecast_of(snaps, p, instants, cap, want, on_equal, ctx=ctx) == (int(first[i]), copies[i].tolist(), limiting[i].tolist())
    return first.tolist(), copies, limiting


@pytest.mark.parametrize("seed,factor", R.GPU_CASES)
def test_random_wide_clusters(seed, factor, oracle_mod):
    snaps, pods, want = R.wide_reference(seed, factor, oracle_mod)
    ctx = paging.paged_preempt_context(snaps, NOW)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            w_copies, w_limiting = want[on_equal]
            # all pods of the cluster's cases in one call
            first, copies, limiting = E.paged_headroom_forecast(engs, pods, FR.INSTANTS, cap=CAP, want=2, on_equal=on_equal)
            assert np.array_equal(copies, w_copies) and np.array_equal(limiting, w_limiting), f"seed {seed} on_equal={on_equal}"
            assert first.tolist() == R.first_of(w_copies, 2), f"seed {seed} on_equal={on_equal}"
            for i, p in enumerate(pods):
                assert paging.paged_headroom_forecast_of(snaps, p, FR.INSTANTS, CAP, 2, on_equal, ctx=ctx) == (
                    int(first[i]), copies[i].tolist(), limiting[i].tolist())
            f2, none_c, l2 = E.paged_headroom_forecast(engs, pods, FR.INSTANTS, cap=CAP, want=2, on_equal=on_equal, want_copies=False)
            assert none_c is None and f2.tobytes() == first.tobytes() and l2.tobytes() == limiting.tobytes()
            f3, c3, none_l = E.paged_headroom_forecast(engs, pods, FR.INSTANTS, cap=CAP, want=2, on_equal=on_equal, want_limiting=False)
            assert none_l is None and f3.tobytes() == first.tobytes() and c3.tobytes() == copies.tobytes()
    finally:
        _close(engs)


@pytest.mark.parametrize("name", sorted(R.DIRECTED))
def test_directed(name, oracle_mod):
    snaps, p, inst, ref = R.directed_reference(name, oracle_mod)
    for on_equal in (False, True):
        answer = R.DIRECTED[name][1][on_equal]
        assert ref[on_equal] == (list(answer[0]), list(answer[1]))
        want = (np.array([answer[0]], np.int64), np.array([answer[1]], np.int32))
        held_to_everything(snaps, oracle_mod, [p], inst, on_equal, want=2, reference=want)


def test_directed_calculated_at_flags_disagree(oracle_mod):
    """After kt_paged_reconcile(APPLY) page 1 holds the replaced threshold with calculatedAt set and page 0 (whose own byte says
    nothing to replace) may not; the answer is the one with both set."""
    from test_paged_forecast_cpu import flags_disagree
    snaps, p, inst, ref = R.directed_reference("later-page-replaces-the-threshold", oracle_mod)
    answer = (0, [4, 4, 4, 0, 0], [0] * 5)
    both, _, _ = flags_disagree(oracle_mod, both=True)
    w_copies, w_limiting = R.reference(both, oracle_mod, [p], inst, CAP)
    assert (R.first_of(w_copies, 1)[0], w_copies[0].tolist(), w_limiting[0].tolist()) == answer

    def ask(engs):
        first, copies, limiting = E.paged_headroom_forecast(engs, [p], inst, cap=CAP)
        return int(first[0]), copies[0].tolist(), limiting[0].tolist()
    engs = _engines(snaps)
    try:
        assert [int(e.reconcile(NOW, apply=False).calc_updated[0]) for e in engs] == [0, 1]  # the pages' own bytes disagree
        assert ask(engs) == answer
        _, replaced, _ = E.paged_reconcile(engs, NOW, apply=True)
        assert replaced.tolist() == [1]
        assert ask(engs) == answer
    finally:
        _close(engs)
    # ... and with the snapshots' flags set by hand on page 1 alone
    one, p, inst = flags_disagree(oracle_mod, both=False)
    engs = _engines(one)
    try:
        assert ask(engs) == answer
    finally:
        _close(engs)


# ---- shapes at which the kernel can go wrong ----
def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


WINDOWS = [(0, 0), (63, 63), (64, 64), (63, 64), (64, 100), (128, 129), (None, None)]
BLOCKS = sorted({(m, lo, hi) for m in (1, 63, 64, 65, 130) for lo, hi in WINDOWS + [(0, m - 1)] if hi is None or hi < m},
                key=lambda c: (c[0], -1 if c[1] is None else c[1], -1 if c[2] is None else c[2]))


@pytest.mark.parametrize("m,lo,hi", BLOCKS)
def test_instant_blocks_and_the_ballot(m, lo, hi, oracle_mod):
    """Two pages of one name each; rows 0 and 1 both select the pod, which asks 3 against a `used` of 8 on either page.  Row 0's
    threshold of 15 on page 0 admits 2 copies throughout.  Row 1's 10 on PAGE 1 admits none; its override 20 (4 copies) is active
    over positions lo .. hi of the m instants: there row 0 limits, elsewhere row 1."""
    inst = _seconds(m)
    times = (inst[lo], inst[hi]) if lo is not None else (FR.shift(inst[-1], 1), None)
    s0 = PR.tiny([{0: 3}, {0: 4}, {0: 4}], {}, flags=RUN, D=1, T=2, row=1)
    s1 = PR.tiny([{0: 3}, {0: 4}, {0: 4}], {0: 10}, flags=RUN, D=1, T=2, row=1)
    s0.thr_spec.set_row(0, {0: 15}, None)
    snaps = [FR.timed(s0, 1, [times + ({}, None)]), FR.timed(s1, 1, [times + ({0: 20}, None)])]
    inside = [lo is not None and lo <= k <= hi for k in range(m)]
    reference = R.reference(snaps, oracle_mod, [0], inst, CAP)
    for want in (1, 2):
        first, copies, limiting = held_to_everything(snaps, oracle_mod, [0], inst, want=want, reference=reference)
        assert first == [lo if lo is not None else -1]
        assert copies[0].tolist() == [2 if x else 0 for x in inside]
        assert limiting[0].tolist() == [0 if x else 1 for x in inside]


@pytest.mark.parametrize("widths", [(1, 1), (8, 3), (3, 16), (16, 16, 2)], ids=lambda w: "x".join(map(str, w)))
def test_every_instantiation_and_unequal_widths(widths, oracle_mod):
    """One throttle over pages of these widths.  The pod asks 3 of the LAST name of page 0 and of the LAST name of the LAST page,
    `used` is 8 of each (the running pods hold 2 of every other name, the pod 1 of the names of a middle page, under no threshold).
      outside:  page 0's name under 30 (7 copies), the last page's under 20: 4 copies (on_equal 3): the last name of the last page.
      [T1, T2]: page 0's name under 14: 2 copies (on_equal 1): page 0 decides.
      [T3, T4]: the last page's name under 11: 1 copy (on_equal 0)."""
    d0, dl, last = widths[0] - 1, widths[-1] - 1, len(widths) - 1
    snaps, per_page = [], []
    for k, D in enumerate(widths):
        d = d0 if k == 0 else dl if k == last else None
        running = {x: 2 for x in range(D)}
        ask = {x: 1 for x in range(D)}
        spec = {}
        if d is not None:
            running[d], ask, spec = 4, {d: 3}, {d: 30 if k == 0 else 20}
        snaps.append(PR.tiny([ask, running, running], spec, flags=RUN, D=D))
        per_page.append([(FR.T1, FR.T2, {d: 14 if k == 0 else 20} if d is not None else {}, None),
                         (FR.T3, FR.T4, {d: 30 if k == 0 else 11} if d is not None else {}, None)])
    snaps = [FR.timed(s, 0, ov) for s, ov in zip(snaps, per_page)]
    assert tuple(s.D for s in snaps) == widths
    inst = FR.EDGE + [FR.shift(FR.T4, 1)]
    for on_equal, row in ((False, [4, 4, 2, 2, 2, 2, 4, 1, 1, 4]), (True, [3, 3, 1, 1, 1, 1, 3, 0, 0, 3])):
        first, copies, limiting = held_to_everything(snaps, oracle_mod, [0, 1], inst, on_equal, want=4)
        assert copies[0].tolist() == row and limiting[0].tolist() == [0] * 10 and first[0] == (-1 if on_equal else 0)


def _many_throttles(rows_spec, timed_row, window, T=1030):
    """Two pages of one name each; T throttles affect pod 0 (`used` 8 on either page, it asks 3 of each), all under thresholds
    nothing reaches but ``rows_spec`` = {row: (page, threshold)}; ``window``: the threshold of ``timed_row``'s PAGE 1 name in
    [T1, T2]."""
    snaps = [FR._run({0: 1 << 40}, T=T, row=T - 1, D=1) for _ in range(2)]
    for s in snaps:
        for t in range(T - 1):
            s.thr_ns[t] = 0
            s.thr_spec.set_row(t, {0: 1 << 40}, 1 << 40)
    for t, (k, v) in rows_spec.items():
        snaps[k].thr_spec.set_row(t, {0: v}, None)
    return [FR.timed(snaps[0], timed_row, [(FR.T1, FR.T2, {}, None)]), FR.timed(snaps[1], timed_row, [(FR.T1, FR.T2, {0: window}, None)])]


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect the pod — more than one chunk of the LDS list holds; only the last row's override on PAGE 1 decides."""
    snaps = _many_throttles({1029: (1, 10)}, 1029, 20)
    assert len(paging.affected_throttles(snaps[0], 0)[1]) == 1030
    first, copies, limiting = held_to_everything(snaps, oracle_mod, [0], FR.EDGE[:8], want=4)
    assert first == [2] and copies[0].tolist() == [0, 0, 4, 4, 4, 4, 0, 0]
    assert limiting[0].tolist() == [1029] * 8


@pytest.mark.parametrize("low,high", [(500, 1029), (5, 32)], ids=["different-chunks", "list-order-reversed"])
def test_tying_throttles_report_the_lower_row(low, high, oracle_mod):
    """Two deciding throttles among 1030: ``low`` admits 2 copies throughout by a page-0 name, ``high`` 1 copy by a page-1 name, and
    2 between T1 and T2 — a tie, and the lower row is the limiting one.  (5, 32): the chunk list holds row 32 in front of row 5 (it
    is filled round by round, one marked byte per lane and round), so "first seen wins" would report 32."""
    snaps = _many_throttles({low: (0, 14), high: (1, 11)}, high, 14)
    first, copies, limiting = held_to_everything(snaps, oracle_mod, [0], FR.EDGE[:8], want=2)
    assert first == [2] and copies[0].tolist() == [1, 1, 2, 2, 2, 2, 1, 1]
    assert limiting[0].tolist() == [high, high, low, low, low, low, high, high]


def test_more_pods_than_workgroups(oracle_mod):
    """2100 pods x 3 instants in one call over two pages: the grid (2048 workgroups at the most) strides."""
    n = 2100
    asks = [(1, 2, 3, 12)[i % 4] for i in range(n)]
    flags = [PR.PENDING] * n + [PR.COUNTED] * 2
    s0 = PR.tiny([{0: 1}] * (n + 2), {}, flags=flags, D=1)
    s1 = PR.tiny([{0: a} for a in asks] + [{0: 4}] * 2, {0: 10}, flags=flags, D=1)
    snaps = [FR.timed(s0, 0, [(FR.T1, FR.T2, {}, None)]), FR.timed(s1, 0, [(FR.T1, FR.T2, {0: 19}, None)])]
    inst = [FR.T0, FR.T1, FR.T3]
    engs = _engines(snaps)
    try:
        first, copies, limiting = E.paged_headroom_forecast(engs, list(range(n)), inst, cap=CAP, want=3)
    finally:
        _close(engs)
    sample = list(range(0, n, 21))
    assert len(sample) == 100 and sample[-1] >= 2048
    w_copies, w_limiting = R.reference(snaps, oracle_mod, sample, inst, CAP)
    assert np.array_equal(copies[sample], w_copies) and np.array_equal(limiting[sample], w_limiting)
    assert first[sample].tolist() == R.first_of(w_copies, 3)
    # spec 10 against used 8: room for 2; the override's 19: room for 11
    by_ask = {1: [2, 11, 2], 2: [1, 5, 1], 3: [0, 3, 0], 12: [0, 0, 0]}
    assert copies.tolist() == [by_ask[a] for a in asks]
    assert first.tolist() == [{1: 1, 2: 1, 3: 1, 12: -1}[a] for a in asks]
    assert (limiting == 0).all()


# ---- the identities of the header ----
@pytest.mark.parametrize("seed", [1, 4, 5])
def test_one_page_is_the_single_engine_launch(seed, oracle_mod):
    """(P1)"""
    from test_forecast_cpu import forecast_case
    snap, pods, _ = forecast_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            one = eng.headroom_forecast(pods, FR.INSTANTS, cap=CAP, want=2, on_equal=on_equal)
            paged = E.paged_headroom_forecast([eng], pods, FR.INSTANTS, cap=CAP, want=2, on_equal=on_equal)
            assert [a.tobytes() for a in one] == [a.tobytes() for a in paged], f"seed {seed} on_equal={on_equal}"
    finally:
        eng.close()


@pytest.mark.parametrize("seed,factor", R.GPU_CASES[:2])
def test_cap_one_is_the_paged_forecast(seed, factor, oracle_mod):
    """(I1)"""
    snaps, pods = R.wide_case(seed, factor, oracle_mod)
    engs = _engines(snaps)
    try:
        seen = set()
        for on_equal in (False, True):
            f_first, verdicts = E.paged_forecast(engs, pods, FR.INSTANTS, on_equal)
            first, copies, limiting = E.paged_headroom_forecast(engs, pods, FR.INSTANTS, cap=1, want=1, on_equal=on_equal)
            assert np.array_equal(copies == 1, verdicts == S.VERDICT_ALLOW) and np.array_equal(copies == 0, verdicts != S.VERDICT_ALLOW)
            assert first.tobytes() == f_first.tobytes()
            assert (limiting[verdicts != S.VERDICT_BLOCK] == -1).all() and (limiting[verdicts == S.VERDICT_BLOCK] >= 0).all()
            seen |= set(verdicts.ravel().tolist())
        assert {S.VERDICT_ALLOW, S.VERDICT_BLOCK} <= seen
    finally:
        _close(engs)


@functools.lru_cache(maxsize=None)
def _pages_agree(seed, factor, t, oracle_mod):
    """The precondition of (I2) from the per-page oracle reconciles at t: for every responsible throttle every page's calc_updated
    and error byte equals the OR over the pages, and the stored calculatedAt flags agree -> (page snapshots, replaced rows)."""
    snaps, _ = R.wide_case(seed, factor, oracle_mod)
    rows = PR.responsible_rows(snaps[0])
    results = [oracle_mod.Oracle(s).reconcile(t, rows=rows) for s in snaps]
    updated = [np.asarray(r.calc_updated[:len(rows)]) != 0 for r in results]
    error = [np.asarray(r.error[:len(rows)]) != 0 for r in results]
    stored = [(s.thr_flags[rows] & np.uint32(S.THR_CALC_AT_NONZERO)) != 0 for s in snaps]
    for per_page in (updated, error, stored):
        assert all(np.array_equal(x, np.logical_or.reduce(per_page)) for x in per_page), (seed, factor, t)
    return snaps, int(updated[0].sum())


# (seed, factor) of R.CASES whose pages agree at NOW and at FR.BOUNDARIES[5]: found on the CPU with _pages_agree.  Replaced rows: 3 and
# 3 on (10, 2), never reconciled; 0 and 2 on (19, 4), whose status was written back at NOW.
@pytest.mark.parametrize("seed,factor", [(10, 2), (19, 4)])
@pytest.mark.parametrize("at", ["now", "boundary"])
def test_single_instant_behind_an_applied_reconcile_is_the_paged_headroom(seed, factor, at, oracle_mod):
    """(I2), at NOW and at a boundary inside a window."""
    t = NOW if at == "now" else FR.BOUNDARIES[5]
    snaps, _ = _pages_agree(seed, factor, t, oracle_mod)
    everyone = np.arange(snaps[0].n_pods, dtype=np.int64)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            E.paged_reconcile(engs, t, apply=True)
            _, copies, limiting = E.paged_headroom_forecast(engs, everyone, [t], cap=CAP, on_equal=on_equal)
            h_copies, h_limiting = E.paged_headroom(engs, everyone, CAP, on_equal)
            assert copies[:, 0].tobytes() == h_copies.tobytes() and limiting[:, 0].tobytes() == h_limiting.tobytes()
            assert len(set(copies[:, 0].tolist())) >= 3
    finally:
        _close(engs)


def test_the_largest_cap_against_a_threshold_of_two_to_the_62_on_page_1():
    """headroom_fit's bisection at full width, against the closed form alone (no queue of 2^31 pods can be walked): `used` 8 on
    page 1, the pod asks 2^32 of its name, the override's threshold is 2^62 + 8 — 2^30 copies, one fewer with on_equal."""
    cap = E.HEADROOM_MAX_CAP
    s0 = FR.timed(PR.tiny([{0: 1}] * 3, {}, flags=RUN, D=1), 0, [(FR.T1, FR.T2, {}, None)])
    s1 = FR.timed(FR._run({0: 10}, ask=2**32, D=1), 0, [(FR.T1, FR.T2, {0: 2**62 + 8}, None)])
    window = [0, 0, 1, 1, 1, 1, 0, 0, 0]
    engs = _engines([s0, s1])
    try:
        for on_equal, copies in ((False, 2**30), (True, 2**30 - 1)):
            got = E.paged_headroom_forecast(engs, [0], FR.EDGE, cap=cap, want=2**30, on_equal=on_equal)
            assert got[1][0].tolist() == [copies * w for w in window] and got[2][0].tolist() == [0] * 9
            assert got[0].tolist() == [-1 if on_equal else 2]
            assert paging.paged_headroom_forecast_of([s0, s1], 0, FR.EDGE, cap, 2**30, on_equal) == (
                int(got[0][0]), got[1][0].tolist(), got[2][0].tolist())
    finally:
        _close(engs)


# ---- refusals in their order, and what a refused call leaves alone ----
def test_refusals_in_order_and_what_a_refused_call_leaves_alone(oracle_mod):
    snaps, p, inst, ref = R.directed_reference("later-page-replaces-the-threshold", oracle_mod)
    n = snaps[0].n_pods
    engs = _engines(snaps)
    other = E.Engine.for_snapshot(PR.tiny([{0: 1}] * n, {0: 10}, T=3, row=2, D=1))
    inc = E.Engine.for_snapshot(snaps[1], kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    rows = np.array([p], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    call = lambda es, a, b, cap=CAP, want=1: E.paged_headroom_forecast(es, a, b, cap=cap, want=want)
    raw = lambda hs_, k, n_, r, m, s_, ns_: L.kt_paged_headroom_forecast(hs_, k, n_, r, m, s_, ns_, 0, CAP, 1, None, None, None)
    said = lambda word: any(word in L.kt_last_error(e._h) for e in engs)

    def every_refusal():
        # 1. the page array, the pages, n
        assert raw(None, 2, 0, None, 2, s2.ctypes.data, n2.ctypes.data) == -1
        assert raw(hs, 0, 0, None, 2, s2.ctypes.data, n2.ctypes.data) == -1
        assert raw(hs, 2, -1, rows.ctypes.data, 2, s2.ctypes.data, n2.ctypes.data) == -1
        # 2. the instants and a missing array, in front of cap
        assert _code(lambda: call(engs, [p], [])) == -1
        assert _code(lambda: call(engs, [p], [FR.T1, FR.T1])) == -1
        assert _code(lambda: call(engs, [p], [FR.T2, FR.T1])) == -1
        assert _code(lambda: call(engs, [p], [(NOW[0], 1_000_000_000)])) == -1
        assert _code(lambda: call(engs, [p], [(NOW[0], -1)])) == -1
        assert raw(hs, 2, 1, None, 2, s2.ctypes.data, n2.ctypes.data) == -1
        assert raw(hs, 2, 1, rows.ctypes.data, 2, None, n2.ctypes.data) == -1
        assert raw(hs, 2, 1, rows.ctypes.data, 2, s2.ctypes.data, None) == -1
        assert _code(lambda: call(engs, [p], [FR.T2, FR.T1], cap=0)) == -1 and said(b"ascending")
        # 3. cap, then want, in front of the page set and a pod row no page holds
        for cap, w in ((0, 1), (-3, 1), (E.HEADROOM_MAX_CAP + 1, 1), (CAP, 0), (CAP, CAP + 1), (CAP, -1)):
            assert _code(lambda: call(engs, [99], inst, cap=cap, want=w)) == -1
        assert _code(lambda: call([engs[0], other], [p], inst, cap=0)) == -1 and b"paged headroom forecast: cap" in L.kt_last_error(engs[0]._h)
        assert _code(lambda: call(engs, [p], inst, cap=0, want=0)) == -1 and b"cap = 0" in L.kt_last_error(engs[0]._h)
        assert _code(lambda: call(engs, [p], inst, want=CAP + 1)) == -1 and b"paged headroom forecast: want" in L.kt_last_error(engs[0]._h)
        # 4. the page set and the rows
        assert _code(lambda: call([engs[0], other], [p], inst)) == -1                      # different throttle-row counts
        assert _code(lambda: call([engs[0], engs[0]], [p], inst)) == -1                    # an engine named twice
        engs[1].set_exchange_world(2)
        assert _code(lambda: call(engs, [99], inst)) == -2                                 # ... in front of what is unsupported
        # 5. n x n_inst > 2^31
        many = np.zeros(2**16 + 1, np.int64)
        assert _code(lambda: call(engs, many, _seconds(2**15))) == -2
        # 6. an engine, asked of every page
        assert _code(lambda: call(engs, [p], inst)) == -7
        engs[1].set_exchange_world(1)
        assert _code(lambda: call([engs[0], inc], [p], inst)) == -7                        # KT_VARIANT_INCREMENTAL
        # `used` of page 1 wider than int64: found out by that page's sums kernel, the one thing that runs before the refusal
        engs[1].set_wide_sums(1)
        assert _code(lambda: call(engs, [p], inst)) == -7
        engs[1].set_wide_sums(0)

    try:
        want_check = [a.copy() for a in engs[0].check(rows=np.arange(n), on_equal=False)]
        want_rec = engs[0].reconcile(NOW, apply=False)
        want_pre = [a.copy() for a in engs[0].preempt([p], [1], NOW)]
        want_hf = [a.copy() for a in engs[0].headroom_forecast([p], inst, cap=CAP)]
        # a pending check and a pending reconcile report of page 0 ...
        engs[0].check_launch(n, want_status=True)
        engs[0].reconcile_launch(NOW, apply=False)
        every_refusal()
        got = engs[0].reconcile_fetch()
        assert got.used.v.tobytes() == want_rec.used.v.tobytes() and got.calc_updated.tobytes() == want_rec.calc_updated.tobytes()
        status, summary = engs[0].check_fetch(n, True)
        assert status.tobytes() == want_check[0].tobytes() and summary.tobytes() == want_check[1].tobytes()
        # ... and a pending forecast result and a pending preempt result (each takes the check slot: not pending beside a check)
        engs[0].headroom_forecast_launch([p], inst, CAP)
        engs[0].preempt_launch([p], [1], NOW)
        every_refusal()
        assert [a.tobytes() for a in engs[0].preempt_fetch(1, 1)] == [a.tobytes() for a in want_pre]
        assert [a.tobytes() for a in engs[0].headroom_forecast_fetch(1, len(inst))] == [a.tobytes() for a in want_hf]
        # n == 0: KT_OK, nothing launched
        first, copies, limiting = call(engs, [], inst)
        assert first.shape == (0,) and copies.shape == (0, len(inst)) and limiting.shape == (0, len(inst))
    finally:
        _close(engs + [other, inc])
    # n x throttle_rows beyond 2^31 bytes of matrix: refused on the host, nothing is allocated
    wide = _engines([FR._run({0: 10}, T=1030, row=1029), FR._run({0: 10}, T=1030, row=1029)])
    try:
        assert _code(lambda: call(wide, np.zeros(2**31 // 1030 + 1, np.int64), [NOW])) == -2
        assert call(wide, [0], [NOW])[1].tolist() == [[0]]
    finally:
        _close(wide)


def test_slots_after_a_successful_call_and_the_dry_run(oracle_mod):
    """The slot rules, and (I3)."""
    snaps, p, inst, ref = R.directed_reference("later-page-replaces-the-threshold", oracle_mod)
    answer = (0,) + ref[False]
    engs = _engines(snaps)
    other_inst = [NOW, (NOW[0] + 60, 0)]

    def ask(pods, instants):
        first, copies, limiting = E.paged_headroom_forecast(engs, pods, instants, cap=CAP)
        return int(first[0]), copies[0].tolist(), limiting[0].tolist()
    try:
        reserved = [e.fetch_reserved() for e in engs]
        plain = [e.reconcile(NOW, apply=False) for e in engs]
        want_pre = [a.copy() for a in engs[0].preempt([p], [1], NOW)]
        for launch in (lambda: engs[0].forecast_launch([p], other_inst), lambda: engs[0].headroom_forecast_launch([p], other_inst, CAP),
                       lambda: engs[0].forecast_gangs_launch([p], [0, 1], other_inst)):
            launch()
            engs[0].preempt_launch([p], [1], NOW)
            for e in engs:
                e.reconcile_launch(NOW, apply=False)
            engs[1].aggregate_launch()
            assert ask([p], inst) == answer
            # handed out by the call: no forecast result of any kind is pending on page 0
            assert _code(lambda: engs[0].forecast_fetch(1, len(other_inst))) == -5
            assert _code(lambda: engs[0].forecast_gangs_fetch(1, len(other_inst))) == -5
            assert _code(lambda: engs[0].headroom_forecast_fetch(1, len(other_inst))) == -5
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
            assert e.reconcile(NOW, apply=False).calc_updated.tobytes() == dry.calc_updated.tobytes()
        # a larger call grows page 0's result buffers behind an unfetched launch
        engs[0].headroom_forecast_launch([p], other_inst, CAP)
        big = _seconds(130)
        first, copies, limiting = E.paged_headroom_forecast(engs, [p, 1] * 40, big, cap=CAP)
        assert copies.shape == (80, 130) and limiting.shape == (80, 130) and (copies[0::2] == copies[0]).all()
        assert (int(first[0]), copies[0].tolist(), limiting[0].tolist()) == paging.paged_headroom_forecast_of(snaps, p, big, CAP)
    finally:
        _close(engs)


def test_paged_engine_headroom_forecast(oracle_mod):
    import paged_forecast_reference as PFR
    from test_paged_admit_cpu import loosen
    cs = PFR.wide_forecast_cluster(46)
    loosen(cs, 2)
    pages = cs.build_pages()
    snaps = [b.snapshot for b in pages]
    assert len(snaps) == 3
    pods = FR.forecast_pods(46, snaps[0], n_pods=6)
    pe = paging.PagedEngine(pages)
    try:
        ctx = paging.paged_preempt_context(snaps, NOW)
        for on_equal in (False, True):
            first, copies, limiting = pe.headroom_forecast(pods, FR.INSTANTS, cap=CAP, want=3, on_equal=on_equal)
            for i, q in enumerate(pods):
                assert (int(first[i]), copies[i].tolist(), limiting[i].tolist()) == paging.paged_headroom_forecast_of(
                    snaps, q, FR.INSTANTS, CAP, 3, on_equal, ctx=ctx)
    finally:
        pe.close()
