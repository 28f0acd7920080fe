"""The admission forecast on the GPU: Engine.forecast (kt_forecast_launch / kt_forecast_fetch, csrc/kt_kernels_forecast.hip)
against the reference of tests/forecast_reference.py (per instant: a copy of the snapshot, the oracle's reconcile, the oracle's
check) and ``paging.forecast_of``, verdict bytes and first position compared bit for bit.  The shapes are the smallest at which
the kernel can still go wrong: instant blocks of 64 and the ballot across them, a deciding throttle in the second chunk of the
affected-throttle list, one case per DT instantiation (D = 1, 8, 16), several pods in one launch."""
import numpy as np
import pytest

import forecast_reference as FR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_forecast_cpu import SEEDS, forecast_case

pytestmark = pytest.mark.gpu
NOW = FR.NOW
A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK


def held_to_everything(snap, oracle_mod, pods, instants, on_equal=False, eng=None):
    own = eng is None
    eng = E.Engine.for_snapshot(snap) if own else eng
    try:
        first, verdicts = eng.forecast(pods, instants, on_equal)
    finally:
        if own:
            eng.close()
    want = FR.reference_verdicts(snap, oracle_mod, pods, instants, on_equal)
    assert verdicts.shape == want.shape and np.array_equal(verdicts, want), (verdicts.tolist(), want.tolist())
    assert first.tolist() == FR.first_of(want)
    for i, p in enumerate(pods):
        assert paging.forecast_of(snap, p, instants, on_equal) == (int(first[i]), verdicts[i].tolist())
    return first.tolist(), verdicts


@pytest.mark.parametrize("seed", SEEDS)
def test_random_manifest_clusters(seed, oracle_mod):
    snap, pods, want = forecast_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            first, verdicts = eng.forecast(pods, FR.INSTANTS, on_equal)
            assert np.array_equal(verdicts, want[on_equal]), f"seed {seed} on_equal={on_equal}"
            assert first.tolist() == FR.first_of(want[on_equal])
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FR.DIRECTED))
def test_directed(name, oracle_mod):
    snap, p, instants = FR.DIRECTED[name]()
    for on_equal in (False, True):
        held_to_everything(snap, oracle_mod, [p], instants, on_equal)


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_single_instant_agrees_with_preempt_prefix_zero(name, oracle_mod):
    snap, p, cands = PR.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            prefix, _ = eng.preempt([p], cands, NOW, on_equal)
            first, _ = eng.forecast([p], [NOW], on_equal)
            assert (int(first[0]) == 0) == (int(prefix[0]) == 0)
    finally:
        eng.close()


def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


@pytest.mark.parametrize("m,lo,hi", [(1, 0, 0), (1, None, None), (63, 62, 62), (64, 63, 63), (65, 64, 64), (65, 63, 64), (130, 64, 100),
                                     (130, 128, 129), (130, 129, 129), (130, None, None), (130, 0, 129)])
def test_instant_blocks_and_the_ballot(m, lo, hi, oracle_mod):
    """Spec 10 blocks the pod (8 + 3 > 10); the override 100 is active over positions lo .. hi of the m instants."""
    inst = _seconds(m)
    ovr = [(inst[lo], inst[hi], {0: 100}, None)] if lo is not None else [(FR.shift(inst[-1], 1), None, {0: 100}, None)]
    snap = FR.timed(FR._run({0: 10}), 0, ovr)
    first, verdicts = held_to_everything(snap, oracle_mod, [0], inst)
    assert first == [lo if lo is not None else -1]
    assert verdicts[0].tolist() == [A if lo is not None and lo <= k <= hi else B for k in range(m)]


@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    d = D - 1
    other = {x: 2 for x in range(D) if x != d}
    running = dict(other)
    running[d] = 4
    snap = PR.tiny([{d: 3}] + [running] * 2, {d: 10}, flags=[PR.PENDING, PR.COUNTED, PR.COUNTED], D=D)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {d: 100}, None), (FR.T3, FR.T4, {d: 100, (d + 1) % D: 1} if D > 1 else {d: 9}, None)])
    for on_equal in (False, True):
        first, _ = held_to_everything(snap, oracle_mod, [0, 1], FR.EDGE + [FR.shift(FR.T4, 1)], on_equal)
        assert first[0] == 2


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect the pod — more than one chunk of the LDS list holds; only the last row's override decides."""
    T = 1030
    snap = FR._run({0: 10}, T=T, row=T - 1)
    for t in range(T - 1):
        snap.thr_ns[t] = 0
        snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    FR.timed(snap, T - 1, [(FR.T1, FR.T2, {0: 100}, None)])
    first, verdicts = held_to_everything(snap, oracle_mod, [0], FR.EDGE[:8])
    assert first == [2] and verdicts[0].tolist() == [B, B, A, A, A, A, B, B]
    assert len(paging.affected_throttles(snap, 0)[1]) == T


def test_seventy_pods_in_one_launch(oracle_mod):
    n = 70
    asks = [(1, 2, 3, 12)[i % 4] for i in range(n)]
    snap = PR.tiny([{0: a} for a in asks] + [{0: 4}] * 2, {0: 10}, flags=[PR.PENDING] * n + [PR.COUNTED] * 2)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {0: 11}, None)])
    first, verdicts = held_to_everything(snap, oracle_mod, list(range(n)), FR.EDGE)
    assert {asks[i]: first[i] for i in range(n)} == {1: 0, 2: 0, 3: 2, 12: -1}


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def test_validation_and_what_a_refused_call_leaves_alone(oracle_mod):
    snap, p, inst = FR.DIRECTED["window-opens-inclusive"]()
    want = FR.reference_verdicts(snap, oracle_mod, [p], inst)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    rows = np.array([p], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    try:
        assert _code(lambda: eng.forecast_fetch(1, len(inst))) == -5  # KT_ERR_NOT_READY

        def every_refusal():
            assert _code(lambda: eng.forecast([p], [])) == -1                                    # n_inst < 1
            assert _code(lambda: eng.forecast([p], [FR.T1, FR.T1])) == -1                        # not STRICTLY ascending
            assert _code(lambda: eng.forecast([p], [FR.T2, FR.T1])) == -1
            assert _code(lambda: eng.forecast([p], [(NOW[0], 5), (NOW[0], 4)])) == -1
            assert _code(lambda: eng.forecast([p], [(NOW[0], 1_000_000_000)])) == -1             # inst_ns outside [0, 10^9)
            assert _code(lambda: eng.forecast([p], [(NOW[0], -1)])) == -1
            assert L.kt_forecast_launch(eng._h, 1, None, 2, s2.ctypes.data, n2.ctypes.data, 0, None) == -1  # missing arrays
            assert L.kt_forecast_launch(eng._h, 1, rows.ctypes.data, 2, None, n2.ctypes.data, 0, None) == -1
            assert L.kt_forecast_launch(eng._h, 1, rows.ctypes.data, 2, s2.ctypes.data, None, 0, None) == -1
            assert L.kt_forecast_launch(eng._h, -1, rows.ctypes.data, 2, s2.ctypes.data, n2.ctypes.data, 0, None) == -1
            assert _code(lambda: eng.forecast([99], inst)) == -2                                 # a pod row outside the capacity
            many = np.zeros(2**16 + 1, np.int64)
            assert _code(lambda: eng.forecast(many, _seconds(2**15))) == -2                      # n x n_inst > 2^31
            eng.set_exchange_world(2)
            assert _code(lambda: eng.forecast([p], inst)) == -7                                  # KT_ERR_UNSUPPORTED
            eng.set_exchange_world(1)
            eng.set_wide_sums(1)
            assert _code(lambda: eng.forecast([p], inst)) == -7                                  # `used` wider than int64
            eng.set_wide_sums(0)

        # a refused call leaves a pending forecast fetchable ...
        eng.forecast_launch([p], inst)
        every_refusal()
        first, verdicts = eng.forecast_fetch(1, len(inst))
        assert np.array_equal(verdicts, want) and first.tolist() == FR.first_of(want)
        # ... and a pending check and a pending reconcile report (a forecast that is launched takes both: see the slot rules)
        eng.reconcile_launch(NOW, apply=False)
        eng.check_launch(snap.n_pods, want_status=True)
        every_refusal()
        eng.check_fetch(snap.n_pods, True)
        eng.reconcile_fetch()
        assert _code(lambda: inc.forecast([p], inst)) == -7
        wide_rows = E.Engine.for_snapshot(FR._run({0: 10}, T=1030, row=1029))
        try:
            assert _code(lambda: wide_rows.forecast(np.zeros(2**31 // 1030 + 1, np.int64), [NOW])) == -2  # n x throttle_rows > 2^31
            assert wide_rows.forecast([0], [NOW])[0].tolist() == [-1]
        finally:
            wide_rows.close()
        # n == 0: KT_OK, nothing launched; out_verdicts == NULL
        eng.forecast_launch([], inst)
        assert eng.forecast_fetch(0, len(inst))[0].tolist() == []
        first, none = eng.forecast([p], inst, want_verdicts=False)
        assert none is None and first.tolist() == FR.first_of(want)
    finally:
        eng.close()
        inc.close()


def _stored_readback(eng, rows):
    """What reads the stored status quantitatively: the headroom query (see tests/test_preempt_gpu.py)."""
    out = []
    for eq in (False, True):
        out += list(eng.headroom(rows, cap=E.HEADROOM_MAX_CAP, on_equal=eq))
    return out


def test_slot_rules_and_dry_run(oracle_mod):
    snap, pods, want = forecast_case(SEEDS[0], oracle_mod)
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    cands = [int(c) for c in everyone if c != pods[0]]
    eng = E.Engine.for_snapshot(snap)
    try:
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = _stored_readback(eng, everyone)
        res_before = eng.fetch_reserved()
        plain = eng.reconcile(NOW, apply=False)
        prefix = eng.preempt([pods[0]], cands, NOW)[0].tolist()
        # the launch takes the check slot and the reconcile result buffers
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        eng.forecast_launch(pods, FR.INSTANTS)
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == -5
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves the forecast fetchable
        eng.aggregate_launch()
        eng.forecast_launch(pods, FR.INSTANTS)
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        assert np.array_equal(eng.forecast_fetch(len(pods), len(FR.INSTANTS))[1], want[False])
        # a forecast and a preempt result are independent: one launch of each, in either order, and both are fetchable
        eng.forecast_launch(pods, FR.INSTANTS, on_equal=True)
        eng.preempt_launch([pods[0]], cands, NOW)
        assert np.array_equal(eng.forecast_fetch(len(pods), len(FR.INSTANTS))[1], want[True])
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == prefix
        eng.preempt_launch([pods[0]], cands, NOW)
        eng.forecast_launch(pods, FR.INSTANTS)
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == prefix
        assert np.array_equal(eng.forecast_fetch(len(pods), len(FR.INSTANTS))[1], want[False])
        # a later user of the check slot drops it
        eng.forecast_launch(pods, FR.INSTANTS)
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.forecast_fetch(len(pods), len(FR.INSTANTS))) == -5
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        res_after = eng.fetch_reserved()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, _stored_readback(eng, everyone)))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("seed", SEEDS[:4])
def test_override_instants(seed, oracle_mod):
    snap, _, _ = forecast_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        want = paging.override_instants_of(snap, NOW, FR.BEYOND)
        assert eng.override_instants(NOW, FR.BEYOND) == (want, len(want))
        mid = FR.BOUNDARIES[5]
        assert eng.override_instants(mid, FR.BEYOND)[0] == paging.override_instants_of(snap, mid, FR.BEYOND)
        assert eng.override_instants(NOW, mid)[0] == paging.override_instants_of(snap, NOW, mid)
        if len(want) > 2:
            assert eng.override_instants(NOW, FR.BEYOND, cap=2) == (want[:2], len(want))  # the earliest, and the full count
        assert eng.override_instants(NOW, FR.BEYOND, cap=0) == ([], len(want))
        total = E.C.c_int64(-1)
        assert E.lib().kt_override_instants(eng._h, NOW[0], NOW[1], FR.BEYOND[0], FR.BEYOND[1], 3, None, None, E.C.byref(total)) == -1
    finally:
        eng.close()


def test_override_instants_directed():
    snap = FR.timed(FR._run({0: 10}), 0, [(FR.T1, FR.T2, {0: 100}, None), (None, (FR.T3[0], 999_999_999), {0: 1}, None),
                                           (FR.T4, None, {0: 1}, None, S.OVR_PARSE_ERROR | FR.BEGIN_PARSED)])
    eng = E.Engine.for_snapshot(snap)
    try:
        assert eng.override_instants(FR.T0, FR.BEYOND)[0] == [FR.T1, FR.shift(FR.T2, 1), (FR.T3[0] + 1, 0)]
        assert eng.override_instants(FR.T1, FR.T2) == ([], 0)
    finally:
        eng.close()
