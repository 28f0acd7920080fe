"""kt_paged_forecast on the GPU: the first passing instant over pages of resource names, held to
tests/paged_forecast_reference.py (per instant: oracle reconcile per page, OR of the bytes, oracle check per page, combine) —
exact, bytes and integers — for both isThrottledOnEqual values."""
import numpy as np
import pytest

import forecast_reference as FR
import paged_forecast_reference as PFR
import paged_preempt_reference as PPR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_paged_forecast_cpu import SEEDS, flags_disagree, paged_case

pytestmark = pytest.mark.gpu
NOW = PFR.NOW
A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK


def _engines(snaps, **kw):
    return [E.Engine.for_snapshot(s, **kw) for s in snaps]


def _close(engs):
    for e in engs:
        e.close()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def held_to_the_reference(snaps, oracle_mod, pods, instants, on_equals=(False, True)):
    """The engines' answer is the reference's and the closed form's -> (first list, verdicts) of the last on_equal."""
    engs = _engines(snaps)
    try:
        for on_equal in on_equals:
            want = PFR.reference_verdicts(snaps, oracle_mod, pods, instants, on_equal)
            first, verdicts = E.paged_forecast(engs, pods, instants, on_equal)
            assert np.array_equal(verdicts, want), f"on_equal={on_equal}"
            assert first.tolist() == FR.first_of(want), f"on_equal={on_equal}"
            for i, p in enumerate(pods):
                assert paging.paged_forecast_of(snaps, p, instants, on_equal) == (int(first[i]), verdicts[i].tolist())
    finally:
        _close(engs)
    return first.tolist(), verdicts


@pytest.mark.parametrize("seed", SEEDS)
def test_random_wide_clusters(seed, oracle_mod):
    snaps, pods, want = paged_case(seed, oracle_mod)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            first, verdicts = E.paged_forecast(engs, pods, FR.INSTANTS, on_equal)  # all pods of the cluster's cases in one call
            assert np.array_equal(verdicts, want[on_equal]), f"seed {seed} on_equal={on_equal}"
            assert first.tolist() == FR.first_of(want[on_equal]), f"seed {seed} on_equal={on_equal}"
            only_first, none = E.paged_forecast(engs, pods, FR.INSTANTS, on_equal, want_verdicts=False)
            assert none is None and only_first.tolist() == first.tolist()
    finally:
        _close(engs)


@pytest.mark.parametrize("name", sorted(PFR.DIRECTED))
def test_directed(name, oracle_mod):
    snaps, p, instants, answer = PFR.DIRECTED[name]()
    first, verdicts = held_to_the_reference(snaps, oracle_mod, [p], instants, on_equals=(False,))
    assert (first[0], verdicts[0].tolist()) == answer


def test_directed_calculated_at_flags_disagree(oracle_mod):
    """Case 5 with the library's own reconcile: after kt_paged_reconcile(APPLY) page 1 holds the replaced threshold with
    calculatedAt set and page 0 (whose own byte says nothing to replace) may not; the answer is the one with both set."""
    snaps, p, instants, answer = PFR.DIRECTED["later-page-replaces-the-threshold"]()
    both, _, _ = flags_disagree(oracle_mod, both=True)
    want = PFR.reference_verdicts(both, oracle_mod, [p], instants)
    assert (FR.first_of(want)[0], want[0].tolist()) == answer == (0, [A, A, A, B, B])
    engs = _engines(snaps)
    try:
        assert [int(e.reconcile(NOW, apply=False).calc_updated[0]) for e in engs] == [0, 1]  # the pages' own bytes disagree
        first, verdicts = E.paged_forecast(engs, [p], instants)
        assert (int(first[0]), verdicts[0].tolist()) == answer
        _, replaced, _ = E.paged_reconcile(engs, NOW, apply=True)
        assert replaced.tolist() == [1]
        first, verdicts = E.paged_forecast(engs, [p], instants)
        assert (int(first[0]), verdicts[0].tolist()) == answer
    finally:
        _close(engs)
    # ... and with the snapshots' flags set by hand on page 1 alone
    one, p, instants = flags_disagree(oracle_mod, both=False)
    engs = _engines(one)
    try:
        first, verdicts = E.paged_forecast(engs, [p], instants)
        assert (int(first[0]), verdicts[0].tolist()) == answer
    finally:
        _close(engs)


@pytest.mark.parametrize("seed", [1, 4, 5])
def test_one_page_is_the_single_engine_launch(seed, oracle_mod):
    from test_forecast_cpu import forecast_case
    snap, pods, _ = forecast_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            one = eng.forecast(pods, FR.INSTANTS, on_equal)
            paged = E.paged_forecast([eng], pods, FR.INSTANTS, on_equal)
            assert [a.tobytes() for a in one] == [a.tobytes() for a in paged], f"seed {seed} on_equal={on_equal}"
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(PPR.DIRECTED))
def test_single_instant_agrees_with_paged_preempt_prefix_zero(name):
    snaps, p, _ = PPR.DIRECTED[name]()
    rows = list(range(snaps[0].n_pods))
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            prefix, _ = E.paged_preempt(engs, rows, [], NOW, on_equal)
            first, _ = E.paged_forecast(engs, rows, [NOW], on_equal)
            assert ((first == 0) == (prefix == 0)).all(), (first.tolist(), prefix.tolist())
    finally:
        _close(engs)


def test_single_instant_agrees_with_paged_preempt_on_a_wide_cluster(oracle_mod):
    snaps, _, _ = paged_case(SEEDS[0], oracle_mod)
    rows = list(range(snaps[0].n_pods))
    engs = _engines(snaps)
    try:
        prefix, _ = E.paged_preempt(engs, rows, [], NOW)
        first, _ = E.paged_forecast(engs, rows, [NOW])
        assert ((first == 0) == (prefix == 0)).all() and (first == 0).any() and (first != 0).any()
    finally:
        _close(engs)


# ---- shapes at which the kernel can go wrong: two pages (one case: three), tiny otherwise ----
def two_pages(times, values1, spec1, ask=3, each=4, D0=1, D1=1, dim1=0, T=1, row=0):
    """Pod 0 pending, two pods running.  Page 0 (D0 names): name 0 under no threshold, the overrides name nothing of it.  Page 1
    (D1 names): the pod asks ``ask`` of name ``dim1``, the running pods hold ``each``, spec ``spec1``, the overrides
    ``values1[j]`` over ``times[j]`` = (begin, end).  Every page holds every override's times."""
    flags = [PR.PENDING, PR.COUNTED, PR.COUNTED]
    s0 = PR.tiny([{0: 1}] * 3, {}, flags=flags, D=D0, T=T, row=row)
    s1 = PR.tiny([{dim1: ask}] + [{dim1: each}] * 2, spec1, flags=flags, D=D1, T=T, row=row)
    FR.timed(s0, row, [(b, e, {}, None) for b, e in times])
    FR.timed(s1, row, [(b, e, v, None) for (b, e), v in zip(times, values1)])
    return [s0, s1]


def widened(m):
    """FR.instants_under_test widened with -+2 ns, -+3 ns, ... around every boundary: the first m of them, strictly ascending."""
    out = set(FR.instants_under_test())
    j = 2
    while len(out) < m + 8:
        for b in FR.BOUNDARIES:
            out |= {FR.shift(b, -j), FR.shift(b, j)}
        j += 1
    return sorted(out)[:m]


@pytest.mark.parametrize("m,lo,hi", [(65, 64, 64), (65, 63, 64), (130, 70, 100), (130, 128, 129), (130, None, None)])
def test_instant_blocks(m, lo, hi, oracle_mod):
    """Spec 10 on page 1 blocks the pod (8 + 3 > 10); the override 100 is active over positions lo .. hi of the m instants: the
    first pass sits in the second or third block of 64 lanes."""
    inst = widened(m)
    assert len(inst) == m
    times = [(inst[lo], inst[hi])] if lo is not None else [(FR.shift(inst[-1], 1), None)]
    snaps = two_pages(times, [{0: 100}], {0: 10})
    first, verdicts = held_to_the_reference(snaps, oracle_mod, [0], inst, on_equals=(False,))
    assert first == [lo if lo is not None else -1]
    assert verdicts[0].tolist() == [A if lo is not None and lo <= k <= hi else B for k in range(m)]


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect the pod — more than one chunk of the LDS list holds; only the last row's override on PAGE 1 decides."""
    T = 1030
    snaps = two_pages([(FR.T1, FR.T2)], [{0: 100}], {0: 10}, T=T, row=T - 1)
    for s in snaps:
        for t in range(T - 1):
            s.thr_ns[t] = 0
            s.thr_spec.set_row(t, {d: 1 << 40 for d in range(s.D)}, 1 << 40)
        s._keep = None
    assert len(paging.affected_throttles(snaps[0], 0)[1]) == T
    first, verdicts = held_to_the_reference(snaps, oracle_mod, [0], FR.EDGE[:8], on_equals=(False,))
    assert first == [2] and verdicts[0].tolist() == [B, B, A, A, A, A, B, B]


def test_more_pods_than_workgroups(oracle_mod):
    """2050 pods over 2048 one-wave workgroups: two of them take a second turn."""
    n = 2050
    flags = [PR.PENDING] * 4 + [PR.COUNTED] * 2
    asks = [1, 2, 3, 12]
    s0 = PR.tiny([{0: 1}] * 6, {}, flags=flags, D=1)
    s1 = PR.tiny([{0: a} for a in asks] + [{0: 4}] * 2, {0: 10}, flags=flags, D=1)
    inst = [FR.T0, FR.T1, FR.shift(FR.T2, 1)]
    snaps = [FR.timed(s0, 0, [(FR.T1, FR.T2, {}, None)]), FR.timed(s1, 0, [(FR.T1, FR.T2, {0: 11}, None)])]
    rows = [(i + (i >= 2048)) % 4 for i in range(n)]
    want = PFR.reference_verdicts(snaps, oracle_mod, [0, 1, 2, 3], inst)
    assert FR.first_of(want) == [0, 0, 1, -1]
    engs = _engines(snaps)
    try:
        first, verdicts = E.paged_forecast(engs, rows, inst)
    finally:
        _close(engs)
    assert np.array_equal(verdicts, want[rows]) and first.tolist() == [FR.first_of(want)[r] for r in rows]


def test_a_narrow_page_under_the_widest_bucket(oracle_mod):
    """Pages of D = 16 and D = 4 in one call: name 3 of the narrow page decides under the DT = 16 form."""
    snaps = two_pages([(FR.T1, FR.T2), (FR.T3, FR.T4)], [{3: 100}, {3: 100, 1: 1}], {3: 10}, D0=16, D1=4, dim1=3)
    snaps[0].thr_spec.set_row(0, {15: 1 << 30}, None)
    snaps[0]._keep = None
    assert [s.D for s in snaps] == [16, 4]
    first, _ = held_to_the_reference(snaps, oracle_mod, [0, 1], FR.EDGE + [FR.shift(FR.T4, 1)])
    assert first[0] == 2


def test_three_pages_the_last_decides(oracle_mod):
    flags = [PR.PENDING, PR.COUNTED, PR.COUNTED]
    times = [(FR.T1, FR.T2)]
    snaps = two_pages(times, [{}], {}, D0=16, D1=16)
    last = PR.tiny([{2: 3}] + [{2: 4}] * 2, {2: 10}, flags=flags, D=3)
    snaps.append(FR.timed(last, 0, [(FR.T1, FR.T2, {2: 100}, None)]))
    first, verdicts = held_to_the_reference(snaps, oracle_mod, [0], FR.EDGE)
    assert first == [2] and verdicts[0].tolist() == [B, B, A, A, A, A, B, B, B]


# ---- refusals, and what a refused call leaves alone ----
def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


def test_refusals_and_what_a_refused_call_leaves_alone(oracle_mod):
    snaps, p, inst, answer = PFR.DIRECTED["later-page-replaces-the-threshold"]()
    n = snaps[0].n_pods
    engs = _engines(snaps)
    other = E.Engine.for_snapshot(PR.tiny([{0: 1}] * n, {0: 10}, T=3, row=2, D=1))
    inc = E.Engine.for_snapshot(snaps[1], kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    rows = np.array([p], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    call = lambda es, a, b, **kw: E.paged_forecast(es, a, b, **kw)
    raw = lambda hs_, k, n_, r, m, s_, ns_: L.kt_paged_forecast(hs_, k, n_, r, m, s_, ns_, 0, None, None)

    def every_refusal():
        # the page set
        assert _code(lambda: call([engs[0], other], [p], inst)) == -1                      # different throttle-row counts
        assert _code(lambda: call([engs[0], engs[0]], [p], inst)) == -1                    # an engine named twice
        assert raw(None, 2, 0, None, 2, s2.ctypes.data, n2.ctypes.data) == -1
        assert raw(hs, 0, 0, None, 2, s2.ctypes.data, n2.ctypes.data) == -1
        # the arguments
        assert _code(lambda: call(engs, [p], [])) == -1                                    # n_inst < 1
        assert _code(lambda: call(engs, [p], [FR.T1, FR.T1])) == -1                        # not STRICTLY ascending
        assert _code(lambda: call(engs, [p], [FR.T2, FR.T1])) == -1
        assert _code(lambda: call(engs, [p], [(NOW[0], 5), (NOW[0], 4)])) == -1
        assert _code(lambda: call(engs, [p], [(NOW[0], 1_000_000_000)])) == -1             # inst_ns outside [0, 10^9)
        assert _code(lambda: call(engs, [p], [(NOW[0], -1)])) == -1
        assert raw(hs, 2, 1, None, 2, s2.ctypes.data, n2.ctypes.data) == -1                # missing arrays
        assert raw(hs, 2, 1, rows.ctypes.data, 2, None, n2.ctypes.data) == -1
        assert raw(hs, 2, 1, rows.ctypes.data, 2, s2.ctypes.data, None) == -1
        assert raw(hs, 2, -1, rows.ctypes.data, 2, s2.ctypes.data, n2.ctypes.data) == -1
        assert _code(lambda: call(engs, [99], inst)) == -2                                 # a pod row no page holds
        many = np.zeros(2**16 + 1, np.int64)
        assert _code(lambda: call(engs, many, _seconds(2**15))) == -2                      # n x n_inst > 2^31
        # an engine, asked of every page
        assert _code(lambda: call([engs[0], inc], [p], inst)) == -7                        # KT_VARIANT_INCREMENTAL
        engs[1].set_exchange_world(2)
        assert _code(lambda: call(engs, [p], inst)) == -7
        engs[1].set_exchange_world(1)
        # `used` of page 1 wider than int64: found out by that page's sums kernel, the one thing that runs before the refusal
        engs[1].set_wide_sums(1)
        assert _code(lambda: call(engs, [p], inst)) == -7
        engs[1].set_wide_sums(0)

    try:
        want_check = [a.copy() for a in engs[0].check(rows=np.arange(n), on_equal=False)]
        want_rec = engs[0].reconcile(NOW, apply=False)
        want_pre = [a.copy() for a in engs[0].preempt([p], [1], NOW)]
        want_fc = [a.copy() for a in engs[0].forecast([p], inst)]
        # a pending check and a pending reconcile report of page 0 ...
        engs[0].check_launch(n, want_status=True)
        engs[0].reconcile_launch(NOW, apply=False)
        every_refusal()
        got = engs[0].reconcile_fetch()
        assert got.used.v.tobytes() == want_rec.used.v.tobytes() and got.calc_updated.tobytes() == want_rec.calc_updated.tobytes()
        status, summary = engs[0].check_fetch(n, True)
        assert status.tobytes() == want_check[0].tobytes() and summary.tobytes() == want_check[1].tobytes()
        # ... and a pending forecast and a pending preempt result (each takes the check slot: they cannot be pending beside a check)
        engs[0].forecast_launch([p], inst)
        engs[0].preempt_launch([p], [1], NOW)
        every_refusal()
        assert [a.tobytes() for a in engs[0].preempt_fetch(1, 1)] == [a.tobytes() for a in want_pre]
        assert [a.tobytes() for a in engs[0].forecast_fetch(1, len(inst))] == [a.tobytes() for a in want_fc]
        import torch
        # pages on different devices: needs a second GPU, so this case does not run on a one-GPU machine (paged_same_cluster's
        # refusal, shared with kt_paged_admit)
        if torch.cuda.device_count() >= 2:
            far = E.Engine.for_snapshot(snaps[1], device=1)
            try:
                assert _code(lambda: call([engs[0], far], [p], inst)) == -7
            finally:
                far.close()
        # n == 0: KT_OK, nothing launched; out_verdicts == NULL
        first, verdicts = call(engs, [], inst)
        assert first.shape == (0,) and verdicts.shape == (0, len(inst))
        first, none = call(engs, [p], inst, want_verdicts=False)
        assert none is None and first.tolist() == [answer[0]]
    finally:
        _close(engs + [other, inc])
    # n x throttle_rows beyond 2^31 bytes of matrix: refused on the host, nothing is allocated
    wide = _engines([FR._run({0: 10}, T=1030, row=1029), FR._run({0: 10}, T=1030, row=1029)])
    try:
        assert _code(lambda: call(wide, np.zeros(2**31 // 1030 + 1, np.int64), [NOW])) == -2
        assert call(wide, [0], [NOW])[0].tolist() == [-1]
    finally:
        _close(wide)


def test_slots_after_a_successful_call(oracle_mod):
    snaps, p, inst, answer = PFR.DIRECTED["later-page-replaces-the-threshold"]()
    engs = _engines(snaps)
    other_inst = [NOW, (NOW[0] + 60, 0)]
    try:
        reserved = [e.fetch_reserved() for e in engs]
        plain = [e.reconcile(NOW, apply=False) for e in engs]
        want_pre = [a.copy() for a in engs[0].preempt([p], [1], NOW)]
        engs[0].forecast_launch([p], other_inst)
        engs[0].preempt_launch([p], [1], NOW)
        for e in engs:
            e.reconcile_launch(NOW, apply=False)
        engs[1].aggregate_launch()
        first, verdicts = E.paged_forecast(engs, [p], inst)
        assert (int(first[0]), verdicts[0].tolist()) == answer
        assert _code(lambda: engs[0].forecast_fetch(1, len(other_inst))) == -5  # handed out by the call: nothing is pending
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
        engs[0].forecast_launch([p], other_inst)
        big = widened(130)
        first, verdicts = E.paged_forecast(engs, [p, 1] * 40, big)
        assert verdicts.shape == (80, 130) and (verdicts[0::2] == verdicts[0]).all()
        assert (int(first[0]), verdicts[0].tolist()) == paging.paged_forecast_of(snaps, p, big)
    finally:
        _close(engs)


def test_paged_engine_forecast_and_override_instants(oracle_mod):
    cs = PFR.wide_forecast_cluster(46)
    pages = cs.build_pages()
    snaps = [b.snapshot for b in pages]
    assert len(snaps) == 3
    pods = FR.forecast_pods(46, snaps[0], n_pods=6)
    pe = paging.PagedEngine(pages)
    try:
        ctx = paging.paged_preempt_context(snaps, NOW)
        for on_equal in (False, True):
            first, verdicts = pe.forecast(pods, FR.INSTANTS, on_equal)
            for i, q in enumerate(pods):
                assert (int(first[i]), verdicts[i].tolist()) == paging.paged_forecast_of(snaps, q, FR.INSTANTS, on_equal, ctx=ctx)
        want = paging.override_instants_of(snaps[0], NOW, FR.BEYOND)
        assert want and pe.override_instants(NOW, FR.BEYOND) == (want, len(want))
        assert all(paging.override_instants_of(s, NOW, FR.BEYOND) == want for s in snaps)
        assert pe.override_instants(NOW, FR.BEYOND, cap=2) == (want[:2], len(want))
    finally:
        pe.close()
