"""kt_paged_preempt_gangs on the GPU: a gang's victim prefix, blocker and reprieve pass over pages of resource names, held to
tests/paged_preempt_gangs_reference.py (delete, oracle reconcile per page, OR of the bytes, in-order admission with a reservation
on every page) — exact, integers and bytes — with and without KT_PREEMPT_REPRIEVE, for both isThrottledOnEqual values."""
import os

import numpy as np
import pytest

import paged_preempt_gangs_reference as PGR
import paged_preempt_reference as PPR
import preempt_gangs_reference as GR
import preempt_gangs_reprieve_reference as GRR
import preempt_reference as PR
import reprieve_reference as RR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from test_paged_preempt_gangs_cpu import CASES, paged_gang_case, reference_answers
from test_paged_preempt_cpu import whole_threshold_cluster
from test_paged_preempt_gpu import _error_throttle_wide

pytestmark = pytest.mark.gpu
NOW = PGR.NOW
NONE = E.PREEMPT_NONE
INVALID, RANGE, NOT_READY, UNSUPPORTED = -1, -2, -5, -7


def _engines(snaps, **kw):
    return [E.Engine.for_snapshot(s, **kw) for s in snaps]


def _close(engs):
    for e in engs:
        e.close()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def _both(engs, rows, off, cands, on_equal=False):
    """-> (prefix [g], prefix mask [g][m], reprieved victims [g][m], blocker [g]); the two calls agree on prefix and blocker."""
    prefix, mask, blocker = E.paged_preempt_gangs(engs, rows, off, cands, NOW, on_equal)
    again, walked, blocker2 = E.paged_preempt_gangs(engs, rows, off, cands, NOW, on_equal, reprieve=True)
    assert prefix.tolist() == again.tolist() and blocker.tolist() == blocker2.tolist()
    return prefix, mask, walked, blocker


def _one(engs, ms, cands, on_equal=False):
    """One gang -> (prefix, mask, reprieved, blocker) as Python values."""
    prefix, mask, walked, blocker = _both(engs, ms, [0, len(ms)], cands, on_equal)
    return int(prefix[0]), mask[0].tolist(), walked[0].tolist(), int(blocker[0])


def held_to_the_reference(snaps, oracle_mod, ms, cands, on_equals=(False, True)):
    engs = _engines(snaps)
    out = []
    try:
        for on_equal in on_equals:
            want = PGR.reference(snaps, oracle_mod, ms, cands, NOW, on_equal)
            k, mask, walked, blocker = _one(engs, ms, cands, on_equal)
            assert (k, walked, blocker) == want, f"on_equal={on_equal}"
            PGR.check_victims(snaps, oracle_mod, ms, cands, k, mask, NOW, on_equal)
            assert (k, mask, blocker) == paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal)
            out.append(want)
    finally:
        _close(engs)
    return out


@pytest.mark.parametrize("seed,factor", CASES)
def test_random_wide_clusters(seed, factor):
    _, snaps, cases = paged_gang_case(seed, factor)
    assert len(snaps) >= 3
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            for (ms, cands), (k, walked, b) in zip(cases, reference_answers(seed, factor, on_equal)):
                got = _one(engs, ms, cands, on_equal)
                assert (got[0], got[2], got[3]) == (k, walked, b), f"seed {seed} gang {ms} on_equal={on_equal}"
                assert (got[0], got[1], got[3]) == paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal), f"seed {seed} gang {ms}: mask"
        # every gang of the seed that shares no pod with the last candidate list, in one call: one wave each
        cands = cases[-1][1]
        gangs = [ms for ms, _ in cases if not set(ms) & set(cands)]
        rows = [p for ms in gangs for p in ms]
        off = np.cumsum([0] + [len(ms) for ms in gangs])
        prefix, mask, walked, blocker = _both(engs, rows, off, cands)
        for g, ms in enumerate(gangs):
            want = paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, reprieve=True)
            local = int(blocker[g]) - int(off[g]) if blocker[g] >= 0 else -1  # (a queue position -> a position in the gang)
            assert (int(prefix[g]), walked[g].tolist(), local) == want, f"seed {seed} gang {ms}"
    finally:
        _close(engs)


@pytest.mark.parametrize("name", sorted(PGR.DIRECTED))
def test_directed(name, oracle_mod):
    build, table = PGR.DIRECTED[name]
    snaps, ms, cands = build()
    for on_equal, want in zip((False, True), held_to_the_reference(snaps, oracle_mod, ms, cands)):
        if on_equal in table:
            t_prefix, _, t_walked, t_blocker = table[on_equal]
            assert want[0] == t_prefix and (t_walked is None or want[1] == t_walked) and (t_blocker is None or want[2] == t_blocker), name


@pytest.mark.parametrize("name", sorted(PPR.DIRECTED))
def test_a_gang_of_one_answers_what_kt_paged_preempt_answers(name):
    snaps, p, cands = PPR.DIRECTED[name]()
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            for reprieve in (False, True):
                k, victims = E.paged_preempt(engs, [p], cands, NOW, on_equal, reprieve=reprieve)
                gk, gv, gb = E.paged_preempt_gangs(engs, [p], [0, 1], cands, NOW, on_equal, reprieve=reprieve)
                assert gk.tobytes() == k.tobytes() and gv.tobytes() == victims.tobytes(), f"{name} {on_equal} {reprieve}"
                assert gb.tolist() == [-1 if int(k[0]) == 0 else 0]
    finally:
        _close(engs)


def test_the_calculated_threshold_is_read_as_a_whole(oracle_mod):
    snaps = [b.snapshot for b in whole_threshold_cluster().build_pages()]
    assert held_to_the_reference(snaps, oracle_mod, [0], [1])[0] == (1, [1], 0)


@pytest.mark.parametrize("blocked", [False, True])
def test_an_error_throttle_keeps_its_stored_status_on_every_page(blocked, oracle_mod):
    snaps, p, cands = _error_throttle_wide(blocked)
    assert len(snaps) == 2
    want = held_to_the_reference(snaps, oracle_mod, [p], cands)
    assert want[0] == ((NONE, [0], 0) if blocked else (0, [0], -1))


def test_candidates_across_blocks_on_the_second_page(oracle_mod):
    """70 candidates, the binding name on page 1: the carries of the second block of 64 are that page's."""
    snaps, ms, cands = PGR.big_last_on_the_second_page(70)
    want = paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, reprieve=True)
    assert want[0] == 69 and sum(want[1]) == 1
    assert PGR.reference_prefix(snaps, oracle_mod, ms, cands) == (want[0], want[2])
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            k, mask, walked, blocker = _one(engs, ms, cands, on_equal)
            assert (k, mask, blocker) == paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal)
            assert (k, walked, blocker) == paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal, reprieve=True)
    finally:
        _close(engs)


def test_a_long_list_and_the_hbm_workspace(oracle_mod):
    """70 affecting throttles with binding names on both pages, the three pending pods as one gang: the list takes more than one
    entry per lane; with KT_REPRIEVE_LDS_CAP=16 (read when the engine is created and on kt_debug_reload_env) it lives in page 0's
    workspace."""
    snaps, ms, cands = PGR.long_list_gang()
    gangs = [ms, ms[::-1], ms[:2]]
    rows = [p for g in gangs for p in g]
    off = np.cumsum([0] + [len(g) for g in gangs])
    want = [paging.paged_preempt_gangs_of(snaps, g, cands, NOW, reprieve=True) for g in gangs]
    assert all(k > 1 and sum(v) < k for k, v, _ in want)
    assert PGR.reference(snaps, oracle_mod, gangs[2], cands) == want[2]
    engs = _engines(snaps)
    try:
        in_lds = _both(engs, rows, off, cands)
    finally:
        _close(engs)
    assert "KT_REPRIEVE_LDS_CAP" not in os.environ
    os.environ["KT_REPRIEVE_LDS_CAP"] = "16"
    try:
        engs = _engines(snaps)
    finally:
        del os.environ["KT_REPRIEVE_LDS_CAP"]
    try:
        in_hbm = _both(engs, rows, off, cands)
        again = _both(engs, rows, off, cands)  # the workspace is reused
        engs[0].reload_env()  # the switch is gone: back in LDS
        back = _both(engs, rows, off, cands)
    finally:
        _close(engs)
    for a, b, c, d in zip(in_lds, in_hbm, back, again):
        assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
    assert [(int(k), v.tolist()) for k, v in zip(in_lds[0], in_lds[2])] == [(k, v) for k, v, _ in want]


def test_throttle_rows_beyond_one_chunk(oracle_mod):
    """1030 throttle rows: the union list takes two chunks of 1024 matrix bytes; two seeds of ``reprieve_reference.wide`` as two pages."""
    s0, pre, cands = RR.wide(6, 12, D=3, T=1030, seed=0, n_pre=2)
    s1, _, _ = RR.wide(6, 12, D=3, T=1030, seed=5, n_pre=2)
    snaps, ms = [s0, s1], list(pre)
    want = held_to_the_reference(snaps, oracle_mod, ms, cands, on_equals=(False,))
    assert want[0][0] > 0


def test_a_sixteen_name_page_beside_a_three_name_page(oracle_mod):
    snaps, ms, cands = PGR.unequal_widths_gang()
    want = held_to_the_reference(snaps, oracle_mod, ms, cands)
    assert want[0][0] > 0


def test_more_gangs_than_workgroups():
    """2500 gangs over 2048 one-wave workgroups: 452 of them take a second turn."""
    n = 2500
    snaps, pre, cands = PPR.long_list(L=6, m=40, n_pre=4)
    kinds = [[0, 1], [1, 0], [2], [3, 2, 1]]
    pick = [(i + (i >= 2048)) % 4 for i in range(n)]
    rows = [p for i in pick for p in kinds[i]]
    off = np.cumsum([0] + [len(kinds[i]) for i in pick])
    want = [paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, reprieve=True) for ms in kinds]
    engs = _engines(snaps)
    try:
        prefix, victims, blocker = E.paged_preempt_gangs(engs, rows, off, cands, NOW, reprieve=True)
        only_prefix = E.paged_preempt_gangs(engs, rows, off, cands, NOW, want_victims=False)
    finally:
        _close(engs)
    assert only_prefix[1] is None and only_prefix[0].tolist() == prefix.tolist() and only_prefix[2].tolist() == blocker.tolist()
    local = np.where(blocker >= 0, blocker - off[:-1], -1)
    for r in range(4):
        sel = np.array(pick) == r
        assert (prefix[sel] == want[r][0]).all() and (victims[sel] == np.array(want[r][1], np.uint8)).all() and (local[sel] == want[r][2]).all()


@pytest.mark.parametrize("seed", range(4))
def test_one_page_is_the_single_engine_launch(seed):
    snap = PR.preempt_cluster(seed).build_pages()[0].snapshot
    cases = GR.gang_cases(seed, snap)
    eng = E.Engine.for_snapshot(snap)
    try:
        for ms, cands in cases:
            for on_equal in (False, True):
                for reprieve in (False, True):
                    one = eng.preempt_gangs(ms, [0, len(ms)], cands, NOW, on_equal, reprieve=reprieve)
                    paged = E.paged_preempt_gangs([eng], ms, [0, len(ms)], cands, NOW, on_equal, reprieve=reprieve)
                    assert [a.tobytes() for a in one] == [a.tobytes() for a in paged], f"seed {seed} gang {ms} {on_equal} {reprieve}"
        # all gangs that share no pod with the last list, in one call
        cands = cases[-1][1]
        gangs = [ms for ms, _ in cases if not set(ms) & set(cands)]
        rows = [p for ms in gangs for p in ms]
        off = np.cumsum([0] + [len(ms) for ms in gangs])
        for reprieve in (False, True):
            one = eng.preempt_gangs(rows, off, cands, NOW, reprieve=reprieve)
            paged = E.paged_preempt_gangs([eng], rows, off, cands, NOW, reprieve=reprieve)
            assert [a.tobytes() for a in one] == [a.tobytes() for a in paged]
    finally:
        eng.close()


def test_one_page_is_the_single_engine_launch_on_the_shapes():
    for make in (lambda: GRR.gang_wide(65, 40, g=3), lambda: GRR.gang_big_last(70, T=1030, row=1029, D=5, dim=4),
                 lambda: GR.DIRECTED["zero-reservation-makes-present"][0](), lambda: GRR.DIRECTED["count-threshold"][0]()):
        snap, ms, cands = make()
        ms = list(ms)
        eng = E.Engine.for_snapshot(snap)
        try:
            for reprieve in (False, True):
                assert [a.tobytes() for a in eng.preempt_gangs(ms, [0, len(ms)], cands, NOW, reprieve=reprieve)] == \
                    [a.tobytes() for a in E.paged_preempt_gangs([eng], ms, [0, len(ms)], cands, NOW, reprieve=reprieve)]
        finally:
            eng.close()


def test_validation():
    snaps, ms, cands = PGR.reserved_prefix_on_the_second_page()
    other_rows = PR.tiny([{0: 1}] * 6, {0: 10}, T=3, row=2, D=1)
    engs = _engines(snaps)
    other = E.Engine.for_snapshot(other_rows)
    inc = E.Engine.for_snapshot(snaps[1], kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    call = lambda es, rows, off, cs, **kw: E.paged_preempt_gangs(es, rows, off, cs, NOW, **kw)
    go = lambda rows, off, cs, es=None: _code(lambda: call(engs if es is None else es, rows, off, cs))
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    a, off = np.array(ms + cands, np.int64), np.array([0, 2], np.int64)
    raw = lambda hs_, k, n, rows, ng, off_, m, cs, flags=0: L.kt_paged_preempt_gangs(hs_, k, n, rows, ng, off_, m, cs, 0, 0, 0, flags, None, None, None)
    try:
        # the page set
        assert go(ms, [0, 2], cands, [engs[0], other]) == INVALID  # different throttle-row counts
        assert go(ms, [0, 2], cands, [engs[0], engs[0]]) == INVALID  # an engine named twice
        assert raw(None, 2, 0, None, 0, None, 0, None) == INVALID
        assert raw(hs, 0, 0, None, 0, None, 0, None) == INVALID
        import torch
        # pages on different devices: needs a second GPU, so this case does NOT run on a one-GPU machine
        if torch.cuda.device_count() >= 2:
            far = E.Engine.for_snapshot(snaps[1], device=1)
            try:
                assert go(ms, [0, 2], cands, [engs[0], far]) == UNSUPPORTED
            finally:
                far.close()
        # the flags
        assert raw(hs, 2, 2, a.ctypes.data, 1, off.ctypes.data, 4, a[2:].ctypes.data, flags=0x2) == INVALID
        # the gang_off defects of kt_admit_gangs_launch
        assert go(ms, [1, 2], cands) == INVALID        # gang_off[0] != 0
        assert go(ms, [0, 1, 1, 2], cands) == INVALID  # an empty gang
        assert go(ms, [0, 2, 1, 2], cands) == INVALID  # descending
        assert go(ms, [0, 1], cands) == INVALID        # gang_off[n_gangs] != n
        assert go(ms, [0], cands) == INVALID           # no gangs for a queue of two pods
        assert raw(hs, 2, 2, a.ctypes.data, 1, None, 4, a[2:].ctypes.data) == INVALID  # gang_off missing
        assert raw(hs, 2, 2, None, 1, off.ctypes.data, 4, a[2:].ctypes.data) == INVALID  # pod_rows missing
        assert raw(hs, 2, 2, a.ctypes.data, 1, off.ctypes.data, 4, None) == INVALID  # cand_rows missing
        assert raw(hs, 2, 2, a.ctypes.data, 1, off.ctypes.data, -1, None) == INVALID  # n_cand < 0
        assert raw(hs, 2, 2, a.ctypes.data, -1, off.ctypes.data, 4, a[2:].ctypes.data) == INVALID  # n_gangs < 0
        assert raw(hs, 2, -1, None, 0, None, 0, None) == INVALID  # n < 0
        assert go([0, 1, 0], [0, 3], cands) == INVALID  # a pod twice within one gang
        assert go(ms, [0, 2], [2, 3, 1]) == INVALID     # a member that is also a candidate
        assert go(ms, [0, 2], [2, 3, 2]) == INVALID     # a candidate named twice
        assert go(ms, [0, 2], [2, 99]) == RANGE         # a row no page holds
        assert go([0, 99], [0, 2], cands) == RANGE
        # an engine, asked of every page
        assert go(ms, [0, 2], cands, [engs[0], inc]) == UNSUPPORTED  # KT_VARIANT_INCREMENTAL
        engs[1].set_exchange_world(2)
        assert go(ms, [0, 2], cands) == UNSUPPORTED
        engs[1].set_exchange_world(1)
        engs[1].set_wide_sums(1)
        assert go(ms, [0, 2], cands) == UNSUPPORTED
        engs[1].set_wide_sums(0)
        # n == 0 only with n_gangs == 0: KT_OK, nothing is launched; n_cand == 0 answers 0 or KT_PREEMPT_NONE, with blockers
        prefix, victims, blocker = call(engs, [], [0], cands)
        assert prefix.shape == (0,) and victims.shape == (0, len(cands)) and blocker.shape == (0,)
        prefix, victims, blocker = call(engs, [0, 1, 0], [0, 2, 3], [], reprieve=True)
        assert (prefix.tolist(), blocker.tolist()) == ([NONE, NONE], [0, 2]) and victims.shape == (2, 0)
        assert [paging.paged_preempt_gangs_of(snaps, g, [], NOW) for g in ([0, 1], [0])] == [(NONE, [], 0)] * 2
        # a pod may be in several gangs
        prefix, victims, blocker = call(engs, [0, 1, 1, 0], [0, 2, 4], cands, reprieve=True)
        assert (prefix.tolist(), victims.tolist(), blocker.tolist()) == ([2, 2], [[1, 1, 0, 0]] * 2, [0, 2])
    finally:
        _close(engs + [other, inc])
    # n_cand == 0 with a gang that passes and one that does not: 0 and KT_PREEMPT_NONE, the blocker of the second
    snaps = PGR.DIRECTED["zero-reservation-on-the-second-page"][0]()[0]
    engs = _engines(snaps)
    try:
        prefix, victims, blocker = call(engs, [1, 0, 0, 1], [0, 2, 4], [])
        assert (prefix.tolist(), blocker.tolist()) == ([0, NONE], [-1, 3]) and victims.shape == (2, 0)
    finally:
        _close(engs)
    # (n + n_cand) x throttle_rows beyond 2^31 bytes of matrix: refused on the host, nothing is allocated
    wide = [RR.big_last(6, T=1030, row=1029)[0], RR.big_last(6, T=1030, row=1029)[0]]
    engs = _engines(wide)
    try:
        many = np.zeros(2**31 // 1030 + 1, np.int64)
        assert _code(lambda: call(engs, many, np.arange(len(many) + 1), [1, 2])) == RANGE
        assert _code(lambda: call(engs, many[:-1], np.arange(len(many)), [1, 2, 3, 4, 5])) == RANGE  # (only the sum of the two)
    finally:
        _close(engs)


def test_a_refused_call_leaves_every_slot_alone():
    snaps, ms, cands = PGR.reserved_prefix_on_the_second_page()
    engs = _engines(snaps)
    n = snaps[0].n_pods
    try:
        want_check = engs[0].check(rows=np.arange(n), on_equal=False)
        want_rec = engs[1].reconcile(NOW, apply=False)
        want_pre = [a.copy() for a in engs[0].preempt_gangs(ms, [0, 2], cands, NOW)]

        def refused():
            assert _code(lambda: E.paged_preempt_gangs(engs, ms, [0, 2], [2, 3, 2], NOW)) == INVALID
            assert _code(lambda: E.paged_preempt_gangs(engs, ms, [0, 1, 1, 2], cands, NOW)) == INVALID
            # `used` of page 1 wider than int64: found out by that page's sums kernel, the one thing that runs before the refusal
            engs[1].set_wide_sums(1)
            assert _code(lambda: E.paged_preempt_gangs(engs, ms, [0, 2], cands, NOW, reprieve=True)) == UNSUPPORTED
            engs[1].set_wide_sums(0)

        engs[0].check_launch(n, want_status=True)
        engs[1].reconcile_launch(NOW, apply=False)
        refused()
        got = engs[1].reconcile_fetch()
        assert got.used.v.tobytes() == want_rec.used.v.tobytes() and got.calc_updated.tobytes() == want_rec.calc_updated.tobytes()
        status, summary = engs[0].check_fetch(n, True)
        assert status.tobytes() == want_check[0].tobytes() and summary.tobytes() == want_check[1].tobytes()
        engs[0].preempt_gangs_launch(ms, [0, 2], cands, NOW)  # (takes page 0's check slot: the two cannot be pending together)
        refused()
        assert [a.tobytes() for a in engs[0].preempt_gangs_fetch(1, len(cands))] == [a.tobytes() for a in want_pre]
    finally:
        _close(engs)


def test_slots_after_a_successful_call():
    snaps, ms, cands = PGR.reserved_prefix_on_the_second_page()
    engs = _engines(snaps)
    n = snaps[0].n_pods
    instants = [NOW, (NOW[0] + 60, 0)]
    try:
        reserved = [e.fetch_reserved() for e in engs]
        checked = [E.paged_check(engs, n, on_equal=eq)[0].copy() for eq in (False, True)]
        want_forecast = [a.copy() for a in engs[0].forecast([0], instants)]
        plain = [e.reconcile(NOW, apply=False) for e in engs]
        engs[0].forecast_launch([0], instants)
        engs[0].preempt_gangs_launch(ms, [0, 2], cands, NOW)
        for e in engs:
            e.reconcile_launch(NOW, apply=False)
        engs[1].aggregate_launch()
        prefix, victims, blocker = E.paged_preempt_gangs(engs, ms, [0, 2], cands, NOW, reprieve=True)
        assert (prefix.tolist(), victims.tolist(), blocker.tolist()) == ([2], [[1, 1, 0, 0]], [0])
        assert [a.tobytes() for a in engs[0].forecast_fetch(1, len(instants))] == [a.tobytes() for a in want_forecast]
        # handed out by the call: nothing is pending, for either fetch
        assert _code(lambda: engs[0].preempt_gangs_fetch(1, len(cands))) == NOT_READY
        assert _code(lambda: engs[0].preempt_fetch(1, len(cands))) == NOT_READY
        for e in engs:
            assert _code(e.reconcile_fetch) == NOT_READY  # every page's reconcile report is dropped
        engs[1].finalize_launch(NOW, apply=False)  # page 1's pending aggregate kept its sums
        got = engs[1].reconcile_fetch()
        assert got.used.v.tobytes() == plain[1].used.v.tobytes() and got.used.present.tobytes() == plain[1].used.present.tobytes()
        # a dry run: reserved amounts and the stored status of every page are unchanged
        for e, before in zip(engs, reserved):
            after = e.fetch_reserved()
            for f in ("v", "present", "count", "has_count"):
                assert getattr(after, f).tobytes() == getattr(before, f).tobytes()
        assert all(np.array_equal(c, E.paged_check(engs, n, on_equal=eq)[0]) for c, eq in zip(checked, (False, True)))
    finally:
        _close(engs)
