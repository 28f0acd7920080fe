"""The headroom forecast on the GPU: Engine.headroom_forecast (kt_headroom_forecast_launch / kt_headroom_forecast_fetch,
csrc/kt_kernels_headroom_forecast.hip) against the reference of tests/headroom_forecast_reference.py (per instant: a copy of the
snapshot, the oracle's reconcile, the oracle's admit of [pod] * cap) and ``paging.headroom_forecast_of``; first, copies and
limiting compared bit for bit.  The shapes are the smallest at which the kernel can still go wrong: instant blocks of 64 with
the per-position accumulators and the ballot across them, deciding throttles in the second chunk of the affected-throttle list
and in an order the list does not keep, one case per DT instantiation (D = 1, 8, 16), more pods than the grid has workgroups."""
import os
import subprocess

import numpy as np
import pytest

import forecast_reference as FR
import headroom_forecast_reference as HR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_forecast_cpu import forecast_case
from test_headroom_forecast_cpu import SEEDS, headroom_forecast_case

pytestmark = pytest.mark.gpu
NOW = FR.NOW
CAP = HR.CAP
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def held_to_everything(snap, oracle_mod, pods, instants, on_equal=False, cap=CAP, want=1):
    eng = E.Engine.for_snapshot(snap)
    try:
        first, copies, limiting = eng.headroom_forecast(pods, instants, cap=cap, want=want, on_equal=on_equal)
    finally:
        eng.close()
    assert first.dtype == np.int64 and copies.dtype == np.int64 and limiting.dtype == np.int32
    w_copies, w_limiting = HR.reference(snap, oracle_mod, pods, instants, cap, on_equal)
    assert copies.shape == w_copies.shape and np.array_equal(copies, w_copies), (copies.tolist(), w_copies.tolist())
    assert np.array_equal(limiting, w_limiting), (limiting.tolist(), w_limiting.tolist())
    assert first.tolist() == HR.first_of(w_copies, want)
    ctx = paging.preempt_context(snap, instants[0])
    for i, p in enumerate(pods):
        assert paging.headroom_forecast_of(snap, p, instants, cap, want, on_equal, ctx=ctx) == (int(first[i]), copies[i].tolist(), limiting[i].tolist())
    return first.tolist(), copies, limiting


@pytest.mark.parametrize("seed", SEEDS)
def test_random_manifest_clusters(seed, oracle_mod):
    snap, pods, want = headroom_forecast_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, NOW)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            first, copies, limiting = eng.headroom_forecast(pods, FR.INSTANTS, cap=CAP, want=2, on_equal=on_equal)
            assert np.array_equal(copies, want[on_equal][0]), f"seed {seed} on_equal={on_equal}"
            assert np.array_equal(limiting, want[on_equal][1]), f"seed {seed} on_equal={on_equal}"
            assert first.tolist() == HR.first_of(want[on_equal][0], 2)
            for i, p in enumerate(pods):
                assert paging.headroom_forecast_of(snap, p, FR.INSTANTS, CAP, 2, on_equal, ctx=ctx) == (
                    int(first[i]), copies[i].tolist(), limiting[i].tolist())
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FR.DIRECTED) + sorted(HR.DIRECTED))
def test_directed(name, oracle_mod):
    snap, p, instants = (FR.DIRECTED[name] if name in FR.DIRECTED else HR.DIRECTED[name])()
    for on_equal in (False, True):
        held_to_everything(snap, oracle_mod, [p], instants, on_equal)


def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


@pytest.mark.parametrize("m,lo,hi", [(1, 0, 0), (1, None, None), (63, 62, 62), (64, 63, 63), (65, 64, 64), (65, 63, 64), (130, 64, 100),
                                     (130, 100, 128), (130, 128, 129), (130, 129, 129), (130, None, None), (130, 0, 129)])
def test_instant_blocks_accumulators_and_the_ballot(m, lo, hi, oracle_mod):
    """Rows 0 and 1 both select the pod; used 8, it asks 3.  Row 0's cpu 15 admits 2 copies throughout.  Row 1's cpu 10 admits
    none; its override 20 (4 copies) is active over positions lo .. hi of the m instants: there row 0 limits, elsewhere row 1."""
    inst = _seconds(m)
    ovr = [(inst[lo], inst[hi], {0: 20}, None)] if lo is not None else [(FR.shift(inst[-1], 1), None, {0: 20}, None)]
    snap = PR.tiny([{0: 3}] + [{0: 4}] * 2, {0: 10}, flags=[PR.PENDING] + [PR.COUNTED] * 2, T=2, row=1)
    snap.thr_spec.set_row(0, {0: 15}, None)
    FR.timed(snap, 1, ovr)
    inside = [lo is not None and lo <= k <= hi for k in range(m)]
    for want in (1, 2):
        first, copies, limiting = held_to_everything(snap, oracle_mod, [0], inst, want=want)
        assert first == [lo if lo is not None else -1]
        assert copies[0].tolist() == [2 if x else 0 for x in inside]
        assert limiting[0].tolist() == [0 if x else 1 for x in inside]


@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    d = D - 1
    other = {x: 2 for x in range(D) if x != d}
    running = dict(other)
    running[d] = 4
    snap = PR.tiny([{d: 3}] + [running] * 2, {d: 10}, flags=[PR.PENDING, PR.COUNTED, PR.COUNTED], D=D)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {d: 20}, None), (FR.T3, FR.T4, {d: 100, (d + 1) % D: 1} if D > 1 else {d: 9}, None)])
    for on_equal in (False, True):
        first, copies, _ = held_to_everything(snap, oracle_mod, [0, 1], FR.EDGE + [FR.shift(FR.T4, 1)], on_equal)
        assert first[0] == 2 and copies[0].tolist()[:7] == [0, 0, 3 if on_equal else 4, 3 if on_equal else 4] + [3 if on_equal else 4] * 2 + [0]


def _many_throttles(rows_spec, timed_row, overrides, T=1030):
    """T throttles affect pod 0 (used 8, it asks 3), all but ``rows_spec`` = {row: cpu threshold} with thresholds nothing reaches."""
    snap = FR._run({0: rows_spec[T - 1] if T - 1 in rows_spec else 1 << 40}, T=T, row=T - 1)
    for t in range(T - 1):
        snap.thr_ns[t] = 0
        snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    for t, v in rows_spec.items():
        snap.thr_spec.set_row(t, {0: v}, None)
    return FR.timed(snap, timed_row, overrides)


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect the pod — more than one chunk of the LDS list holds; only the last row's override decides."""
    snap = _many_throttles({1029: 10}, 1029, [(FR.T1, FR.T2, {0: 20}, None)])
    first, copies, limiting = held_to_everything(snap, oracle_mod, [0], FR.EDGE[:8], want=4)
    assert first == [2] and copies[0].tolist() == [0, 0, 4, 4, 4, 4, 0, 0]
    assert limiting[0].tolist() == [1029] * 8
    assert len(paging.affected_throttles(snap, 0)[1]) == 1030


@pytest.mark.parametrize("low,high", [(500, 1029), (5, 32)], ids=["different-chunks", "list-order-reversed"])
def test_tying_throttles_report_the_lower_row(low, high, oracle_mod):
    """Two deciding throttles among 1030: ``low`` admits 2 copies throughout, ``high`` 1 copy, and 2 between T1 and T2 — a tie, and
    the lower row is the limiting one.  (5, 32): the chunk list holds row 32 in front of row 5 (it is filled round by round, one
    marked byte per lane and round), so "first seen wins" would report 32."""
    snap = _many_throttles({low: 14, high: 11}, high, [(FR.T1, FR.T2, {0: 14}, None)])
    first, copies, limiting = held_to_everything(snap, oracle_mod, [0], FR.EDGE[:8], want=2)
    assert first == [2] and copies[0].tolist() == [1, 1, 2, 2, 2, 2, 1, 1]
    assert limiting[0].tolist() == [high, high, low, low, low, low, high, high]


def test_more_pods_than_workgroups(oracle_mod):
    """2100 pods x 3 instants in one launch: the grid (2048 workgroups at the most) strides."""
    n = 2100
    asks = [(1, 2, 3, 12)[i % 4] for i in range(n)]
    snap = PR.tiny([{0: a} for a in asks] + [{0: 4}] * 2, {0: 10}, flags=[PR.PENDING] * n + [PR.COUNTED] * 2)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {0: 19}, None)])
    inst = [FR.T0, FR.T1, FR.T3]
    eng = E.Engine.for_snapshot(snap)
    try:
        first, copies, limiting = eng.headroom_forecast(list(range(n)), inst, cap=CAP, want=3)
    finally:
        eng.close()
    sample = list(range(0, n, 21))
    assert len(sample) == 100 and sample[-1] >= 2048
    w_copies, w_limiting = HR.reference(snap, oracle_mod, sample, inst, CAP)
    assert np.array_equal(copies[sample], w_copies) and np.array_equal(limiting[sample], w_limiting)
    assert first[sample].tolist() == HR.first_of(w_copies, 3)
    # spec 10 against used 8: room for 2; the override's 19: room for 11
    by_ask = {1: [2, 11, 2], 2: [1, 5, 1], 3: [0, 3, 0], 12: [0, 0, 0]}
    assert copies.tolist() == [by_ask[a] for a in asks]
    assert first.tolist() == [{1: 1, 2: 1, 3: 1, 12: -1}[a] for a in asks]
    assert (limiting == 0).all()


@pytest.mark.parametrize("seed", SEEDS[:4])
def test_cap_one_is_the_forecast(seed, oracle_mod):
    """(I1)"""
    snap, pods, _ = forecast_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            f_first, verdicts = eng.forecast(pods, FR.INSTANTS, on_equal)
            first, copies, limiting = eng.headroom_forecast(pods, FR.INSTANTS, cap=1, want=1, on_equal=on_equal)
            assert np.array_equal(copies == 1, verdicts == S.VERDICT_ALLOW) and np.array_equal(copies == 0, verdicts != S.VERDICT_ALLOW)
            assert first.tobytes() == f_first.tobytes()
            assert (limiting[verdicts != S.VERDICT_BLOCK] == -1).all() and (limiting[verdicts == S.VERDICT_BLOCK] >= 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("seed", SEEDS[:2])
def test_single_instant_behind_an_applied_reconcile_is_the_headroom(seed, oracle_mod):
    """(I2), at NOW and at a boundary inside the window."""
    snap, _, _ = forecast_case(seed, oracle_mod)
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    eng = E.Engine.for_snapshot(snap)
    try:
        for t in (NOW, FR.BOUNDARIES[5]):
            for on_equal in (False, True):
                eng.reconcile(t, apply=True)
                _, copies, limiting = eng.headroom_forecast(everyone, [t], cap=CAP, on_equal=on_equal)
                h_copies, h_limiting = eng.headroom(everyone, cap=CAP, on_equal=on_equal)
                assert copies[:, 0].tobytes() == h_copies.tobytes() and limiting[:, 0].tobytes() == h_limiting.tobytes()
    finally:
        eng.close()


def _rise_and_fall():
    # used 8, the pod asks 3: spec 10 admits nobody, 20 four copies (T1 .. T2), 100 all sixteen (T3 .. T4)
    snap = FR.timed(FR._run({0: 10}), 0, [(FR.T1, FR.T2, {0: 20}, None), (FR.T3, FR.T4, {0: 100}, None)])
    return snap, FR.EDGE + [FR.shift(FR.T4, 1)]


def test_want(oracle_mod):
    snap, inst = _rise_and_fall()
    for want, first in ((1, 2), (4, 2), (5, 7), (CAP, 7)):
        got, copies, _ = held_to_everything(snap, oracle_mod, [0], inst, want=want)
        assert got == [first] and copies[0].tolist() == [0, 0, 4, 4, 4, 4, 0, CAP, CAP, 0]


def test_the_largest_cap_against_a_threshold_of_two_to_the_62():
    """headroom_fit's bisection at full width, against the closed form alone (no queue of 2^31 pods can be walked; the expected
    numbers are written out in tests/test_headroom_forecast_cpu.py): used 8, the pod asks 2^32, the override's threshold is
    2^62 + 8 — 2^30 copies, one fewer with on_equal."""
    cap = E.HEADROOM_MAX_CAP
    snap = FR.timed(FR._run({0: 10}, ask=2**32), 0, [(FR.T1, FR.T2, {0: 2**62 + 8}, None)])
    window = [0, 0, 1, 1, 1, 1, 0, 0, 0]
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal, copies in ((False, 2**30), (True, 2**30 - 1)):
            got = eng.headroom_forecast([0], FR.EDGE, cap=cap, want=2**30, on_equal=on_equal)
            assert got[1][0].tolist() == [copies * w for w in window] and got[2][0].tolist() == [0] * 9
            assert got[0].tolist() == [-1 if on_equal else 2]
            assert paging.headroom_forecast_of(snap, 0, FR.EDGE, cap, 2**30, on_equal) == (int(got[0][0]), got[1][0].tolist(), got[2][0].tolist())
    finally:
        eng.close()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def test_validation_in_order_and_what_a_refused_call_leaves_alone(oracle_mod):
    snap, inst = _rise_and_fall()
    p = 0
    want = HR.reference(snap, oracle_mod, [p], inst, CAP)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    rows = np.array([p], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    hf = lambda pods, instants, cap=CAP, want=1: eng.headroom_forecast(pods, instants, cap=cap, want=want)
    try:
        assert _code(lambda: eng.headroom_forecast_fetch(1, len(inst))) == -5  # KT_ERR_NOT_READY

        def every_refusal():
            # 1. the instants and a missing array
            assert _code(lambda: hf([p], [])) == -1
            assert _code(lambda: hf([p], [FR.T1, FR.T1])) == -1
            assert _code(lambda: hf([p], [FR.T2, FR.T1])) == -1
            assert _code(lambda: hf([p], [(NOW[0], 1_000_000_000)])) == -1
            assert _code(lambda: hf([p], [(NOW[0], -1)])) == -1
            assert L.kt_headroom_forecast_launch(eng._h, 1, None, 2, s2.ctypes.data, n2.ctypes.data, 0, CAP, 1, None) == -1
            assert L.kt_headroom_forecast_launch(eng._h, 1, rows.ctypes.data, 2, None, n2.ctypes.data, 0, CAP, 1, None) == -1
            assert L.kt_headroom_forecast_launch(eng._h, 1, rows.ctypes.data, 2, s2.ctypes.data, None, 0, CAP, 1, None) == -1
            assert L.kt_headroom_forecast_launch(eng._h, -1, rows.ctypes.data, 2, s2.ctypes.data, n2.ctypes.data, 0, CAP, 1, None) == -1
            # ... in front of cap: the message names the instants
            assert _code(lambda: hf([p], [FR.T2, FR.T1], cap=0)) == -1 and b"ascending" in L.kt_last_error(eng._h)
            # 2. cap and want, in front of a pod row outside the table
            for cap, w in ((0, 1), (-3, 1), (E.HEADROOM_MAX_CAP + 1, 1), (CAP, 0), (CAP, CAP + 1), (CAP, -1)):
                assert _code(lambda: hf([99], inst, cap=cap, want=w)) == -1
            assert _code(lambda: hf([p], inst, cap=0)) == -1 and b"cap" in L.kt_last_error(eng._h)
            # 3. out of range, in front of what is unsupported
            eng.set_exchange_world(2)
            assert _code(lambda: hf([99], inst)) == -2
            assert _code(lambda: hf([-1], inst)) == -2
            many = np.zeros(2**16 + 1, np.int64)
            assert _code(lambda: hf(many, _seconds(2**15))) == -2                                # n x n_inst > 2^31
            # 4. unsupported
            assert _code(lambda: hf([p], inst)) == -7
            eng.set_exchange_world(1)
            eng.set_wide_sums(1)
            assert _code(lambda: hf([p], inst)) == -7                                            # `used` wider than int64
            eng.set_wide_sums(0)

        def fetched_is_wanted():
            first, copies, limiting = eng.headroom_forecast_fetch(1, len(inst))
            assert np.array_equal(copies, want[0]) and np.array_equal(limiting, want[1]) and first.tolist() == HR.first_of(want[0], 5)

        # a refused call leaves a pending result fetchable ...
        eng.headroom_forecast_launch([p], inst, CAP, 5)
        every_refusal()
        fetched_is_wanted()
        # ... and a pending check and a pending reconcile report (a launch that is accepted takes both: see the slot rules)
        eng.reconcile_launch(NOW, apply=False)
        eng.check_launch(snap.n_pods, want_status=True)
        every_refusal()
        eng.check_fetch(snap.n_pods, True)
        eng.reconcile_fetch()
        assert _code(lambda: inc.headroom_forecast([p], inst, cap=CAP)) == -7
        wide_rows = E.Engine.for_snapshot(FR._run({0: 10}, T=1030, row=1029))
        try:
            assert _code(lambda: wide_rows.headroom_forecast(np.zeros(2**31 // 1030 + 1, np.int64), [NOW], cap=CAP)) == -2  # n x throttle_rows
            assert wide_rows.headroom_forecast([0], [NOW], cap=CAP)[1].tolist() == [[0]]
        finally:
            wide_rows.close()
        # n == 0: KT_OK, nothing launched; the nullable outputs; the largest cap
        eng.headroom_forecast_launch([], inst, CAP)
        assert [x.tolist() for x in eng.headroom_forecast_fetch(0, len(inst))] == [[], [], []]
        eng.headroom_forecast_launch([p], inst, CAP, 5)
        first, none_c, none_l = eng.headroom_forecast_fetch(1, len(inst), want_copies=False, want_limiting=False)
        assert none_c is None and none_l is None and first.tolist() == [7]
        first, copies, _ = hf([p], inst, cap=E.HEADROOM_MAX_CAP, want=30)
        assert copies[0].tolist() == [0, 0, 4, 4, 4, 4, 0, 30, 30, 0] and first.tolist() == [7]
    finally:
        eng.close()
        inc.close()


def test_slot_rules_and_dry_run(oracle_mod):
    snap, pods, want = headroom_forecast_case(SEEDS[0], oracle_mod)
    m = len(FR.INSTANTS)
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    cands = [int(c) for c in everyone if c != pods[0]]
    gang_off = [0, len(pods)]
    eng = E.Engine.for_snapshot(snap)

    def fetch_ok():
        _, copies, limiting = eng.headroom_forecast_fetch(len(pods), m)
        return np.array_equal(copies, want[False][0]) and np.array_equal(limiting, want[False][1])
    try:
        # (I3) a dry run: what reads the stored status and the reserved amounts sees them unchanged
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = [x.copy() for eq in (False, True) for x in eng.headroom(everyone, cap=E.HEADROOM_MAX_CAP, on_equal=eq)]
        res_before = eng.fetch_reserved()
        plain = eng.reconcile(NOW, apply=False)
        prefix = eng.preempt([pods[0]], cands, NOW)[0].tolist()
        # the launch takes the check slot and the reconcile result buffers
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        eng.headroom_forecast_launch(pods, FR.INSTANTS, CAP)
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == -5
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves the result fetchable
        eng.aggregate_launch()
        eng.headroom_forecast_launch(pods, FR.INSTANTS, CAP)
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        assert fetch_ok()
        # the three kinds of the one pending forecast result: only the launch's own fetch reads it
        eng.headroom_forecast_launch(pods, FR.INSTANTS, CAP)
        assert _code(lambda: eng.forecast_fetch(len(pods), m)) == -5
        assert _code(lambda: eng.forecast_gangs_fetch(1, m)) == -5
        assert fetch_ok()
        eng.forecast_launch(pods, FR.INSTANTS)
        assert _code(lambda: eng.headroom_forecast_fetch(len(pods), m)) == -5
        eng.forecast_fetch(len(pods), m)
        eng.forecast_gangs_launch(pods, gang_off, FR.INSTANTS)
        assert _code(lambda: eng.headroom_forecast_fetch(1, m)) == -5
        eng.forecast_gangs_fetch(1, m)
        # a preempt result survives the launch, and the other way round
        eng.preempt_launch([pods[0]], cands, NOW)
        eng.headroom_forecast_launch(pods, FR.INSTANTS, CAP)
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == prefix
        assert fetch_ok()
        eng.headroom_forecast_launch(pods, FR.INSTANTS, CAP)
        eng.preempt_launch([pods[0]], cands, NOW)
        assert fetch_ok()
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == prefix
        # a later user of the check slot drops it
        eng.headroom_forecast_launch(pods, FR.INSTANTS, CAP)
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.headroom_forecast_fetch(len(pods), m)) == -5
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        room_after = [x for eq in (False, True) for x in eng.headroom(everyone, cap=E.HEADROOM_MAX_CAP, on_equal=eq)]
        res_after = eng.fetch_reserved()
        again = eng.reconcile(NOW, apply=False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, room_after))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
            assert getattr(plain.used, f).tobytes() == getattr(again.used, f).tobytes()
        assert plain.thrl_flag.tobytes() == again.thrl_flag.tobytes()
    finally:
        eng.close()


def test_host_plugin_scale_after():
    """The plugin mirror's ScaleAfter against a twin plugin that, per boundary, reconciles and counts PreFilter + Reserve of fresh
    same-shape pods (tests/cpp/host_plugin_scale_after_test.cpp)."""
    host = os.path.join(ROOT, "kube_throttler_amd", "host")
    subprocess.check_call(["make", "-C", host, "host_plugin_scale_after_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(host, "host_plugin_scale_after_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
