"""The gang preemption query on the GPU: Engine.preempt_gangs (kt_preempt_gangs_launch / kt_preempt_gangs_fetch,
csrc/kt_kernels_preempt_gangs.hip) against the reference of tests/preempt_gangs_reference.py (delete the prefix, reconcile and
admit the gang in order with the oracle, for every k) and ``paging.preempt_gangs_of``.  Prefix, victim mask and blocker are
compared bit for bit.  The shapes are the smallest at which the kernel can still go wrong: candidate blocks of 64 and their
carries under a reserved prefix, a blocking throttle in the second chunk of the union list, one case per DT instantiation, a gang
longer than a wave, more gangs than workgroups."""
import functools

import numpy as np
import pytest

import preempt_gangs_reference as GR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from test_preempt_cpu import SEEDS
from test_preempt_gangs_cpu import gang_case

pytestmark = pytest.mark.gpu
NOW = PR.NOW
INVALID, RANGE, NOT_READY, UNSUPPORTED = -1, -2, -5, -7


def launch(eng, gangs, cands, on_equal=False):
    """All ``gangs`` (lists of member rows) in one launch -> (prefix, victims, blocker as a position in its own gang)."""
    rows = [p for ms in gangs for p in ms]
    off = np.cumsum([0] + [len(ms) for ms in gangs])
    prefix, victims, blocker = eng.preempt_gangs(rows, off, cands, NOW, on_equal)
    assert victims.shape == (len(gangs), len(cands))
    local = [int(b) - int(off[g]) if b >= 0 else -1 for g, b in enumerate(blocker)]
    assert all(b == -1 or 0 <= b < len(ms) for b, ms in zip(local, gangs))
    return prefix.tolist(), victims, local


def held_to_everything(snap, oracle_mod, members, cands, on_equal=False, eng=None):
    own = eng is None
    eng = E.Engine.for_snapshot(snap) if own else eng
    try:
        prefix, victims, blocker = launch(eng, [members], cands, on_equal)
    finally:
        if own:
            eng.close()
    want = GR.reference(snap, oracle_mod, members, cands, NOW, on_equal)
    model = paging.preempt_gangs_of(snap, members, cands, NOW, on_equal)
    assert (prefix[0], blocker[0]) == want == (model[0], model[2]), (prefix[0], blocker[0], want, model[0], model[2])
    assert victims[0].tolist() == model[1]
    GR.check_victims(snap, oracle_mod, members, cands, want[0], victims[0], NOW, on_equal)
    return want[0]


@functools.lru_cache(maxsize=None)
def shared_list_case(seed, oracle_mod):
    """The gangs of a seed over ONE candidate list (the longest case's, without any gang's members) and their references."""
    snap, cases, _, _ = gang_case(seed, oracle_mod)
    gangs = [ms for ms, _ in cases]
    everyone = {p for ms in gangs for p in ms}
    cands = [c for c in max((cs for _, cs in cases), key=len) if c not in everyone]
    want = {eq: [GR.reference(snap, oracle_mod, ms, cands, NOW, eq) for ms in gangs] for eq in (False, True)}
    return gangs, cands, want


@pytest.mark.parametrize("seed", SEEDS[::3])
def test_random_manifest_clusters(seed, oracle_mod):
    snap, cases, want, _ = gang_case(seed, oracle_mod)
    gangs, cands, want_shared = shared_list_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, NOW)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            for (ms, cs), (k, b) in zip(cases, want[on_equal]):  # the cases of the CPU suite, each over its own list
                prefix, victims, blocker = launch(eng, [ms], cs, on_equal)
                model = paging.preempt_gangs_of(snap, ms, cs, NOW, on_equal, ctx=ctx)
                assert (prefix[0], blocker[0]) == (k, b) == (model[0], model[2]), f"seed {seed} on_equal={on_equal} gang {ms} over {cs}"
                assert victims[0].tolist() == model[1]
            prefix, victims, blocker = launch(eng, gangs, cands, on_equal)  # all gangs of the seed in one launch
            for g, ms in enumerate(gangs):
                model = paging.preempt_gangs_of(snap, ms, cands, NOW, on_equal, ctx=ctx)
                assert (prefix[g], blocker[g]) == want_shared[on_equal][g] == (model[0], model[2]), f"seed {seed} on_equal={on_equal} gang {ms}"
                assert victims[g].tolist() == model[1]
                GR.check_victims(snap, oracle_mod, ms, cands, prefix[g], victims[g], NOW, on_equal)
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(GR.DIRECTED))
def test_directed(name, oracle_mod):
    build, want, _ = GR.DIRECTED[name]
    snap, ms, cands = build()
    for i, on_equal in enumerate((False, True)):
        assert held_to_everything(snap, oracle_mod, ms, cands, on_equal) == want[i]


def gang_line(m, k_star, g=2, D=2, dim=0, **kw):
    """``g`` pending members asking 1 of ``dim`` each; candidates g .. g + m - 1 running with 1 of ``dim`` each (and 2 of every
    other name, which the threshold does not name); threshold m + g - k_star: the last member passes with its g - 1 predecessors
    reserved exactly when k_star candidates are gone -> (snapshot, members, candidates)."""
    other = {d: 2 for d in range(D) if d != dim}
    running = dict(other)
    running[dim] = 1
    snap = PR.tiny([{dim: 1}] * g + [running] * m, {dim: m + g - k_star}, flags=[PR.PENDING] * g + [PR.COUNTED] * m, D=D, **kw)
    return snap, list(range(g)), list(range(g, g + m))


@pytest.mark.parametrize("m,k_star", [(63, 63), (64, 64), (65, 65), (130, 65), (130, 129), (130, 130)])
def test_candidate_blocks_and_carries(m, k_star, oracle_mod):
    snap, ms, cands = gang_line(m, k_star)
    assert held_to_everything(snap, oracle_mod, ms, cands) == k_star
    # each member alone needs one victim less: the reserved prefix is what moves the answer
    assert paging.preempt_of(snap, ms[1], cands, NOW)[0] == k_star - 1


@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    snap, ms, cands = gang_line(70, 66, D=D, dim=D - 1)
    for on_equal in (False, True):
        assert held_to_everything(snap, oracle_mod, ms, cands, on_equal) == 66 + on_equal


@pytest.mark.parametrize("T,row", [(70, 67), (1030, 1029)])
def test_blocking_throttle_in_the_second_list_chunk(T, row, oracle_mod):
    snap, ms, cands = gang_line(5, 3, T=T, row=row)
    assert held_to_everything(snap, oracle_mod, ms, cands) == 3


def test_a_gang_of_seventy_members(oracle_mod):
    # 70 members of 1 under a threshold of 100 with 65 running 1s: the last member meets 69 reserved, 30 may stay
    snap, ms, cands = gang_line(65, 35, g=70)
    assert held_to_everything(snap, oracle_mod, ms, cands) == 35
    # ... and with a member in the middle that asks more than the threshold the gang has no prefix; the blocker is that member
    asks = [1] * 70
    asks[66] = 101
    snap = PR.tiny([{0: a} for a in asks] + [{0: 1}] * 65, {0: 100}, flags=[PR.PENDING] * 70 + [PR.COUNTED] * 65)
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, _, blocker = launch(eng, [ms], cands)
    finally:
        eng.close()
    assert (prefix, blocker) == ([-1], [35])  # (in S_0 the 65 running pods leave room for 35 members)
    assert paging.preempt_gangs_of(snap, ms, cands, NOW)[::2] == (-1, 35)


def test_more_gangs_than_workgroups_equal_the_single_query(oracle_mod):
    """The launch caps its grid at 2048 workgroups of one wave: with 2100 gangs of one pod 52 waves take a second turn.  A gang
    of one pod reports exactly what kt_preempt_launch reports for that pod."""
    m, n = 70, 2100
    asks = (1, 2, 3, 12)
    snap = PR.tiny([{0: a} for a in asks] + [{0: 1}] * m, {0: 10}, flags=[PR.PENDING] * 4 + [PR.COUNTED] * m)
    cands = list(range(4, 4 + m))
    rows = [(i + (i >= 2048)) % 4 for i in range(n)]  # the turns of one wave differ
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims, blocker = eng.preempt_gangs(rows, np.arange(n + 1), cands, NOW)
        single, single_victims = eng.preempt(rows, cands, NOW)
    finally:
        eng.close()
    assert single.tolist() == [(61, 62, 63, -1)[r] for r in rows]
    assert np.array_equal(prefix, single) and np.array_equal(victims, single_victims)
    assert blocker.tolist() == list(range(n))  # nobody passes in S_0: every gang's one member blocks it


def test_gangs_sharing_a_launch_are_answered_independently(oracle_mod):
    # [0, 1] needs 4 victims; were gangs a queue, its reservations would push the repeats further out
    snap, ms, cands = GR.DIRECTED["two-members-throttle"][0]()
    gangs = [[0, 1], [1], [0, 1], [1, 0], [0], [0, 1]]
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims, blocker = launch(eng, gangs, cands)
    finally:
        eng.close()
    assert prefix == [4, 3, 4, 4, 3, 4] and blocker == [0, 0, 0, 0, 0, 0]
    assert all(victims[g].tolist() == [1] * prefix[g] + [0] * (6 - prefix[g]) for g in range(len(gangs)))
    for g, members in enumerate(gangs):
        assert prefix[g] == GR.reference(snap, oracle_mod, members, cands)[0]


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def _refusals(eng, inc, wide_rows, many):
    """Every refusal with its code, on an engine whose pending results the caller then fetches."""
    ms, cands = [0, 1], [2, 3, 4]
    go = lambda rows, off, cs, e=eng: _code(lambda: e.preempt_gangs(rows, off, cs, NOW))
    # the gang_off defects of kt_admit_gangs_launch
    assert go(ms, [1, 2], cands) == INVALID     # gang_off[0] != 0
    assert go(ms, [0, 1, 1, 2], cands) == INVALID  # an empty gang
    assert go(ms, [0, 2, 1, 2], cands) == INVALID  # descending
    assert go(ms, [0, 1], cands) == INVALID     # gang_off[n_gangs] != n
    assert go(ms, [0], cands) == INVALID        # no gangs for a queue of two pods
    L, a = E.lib(), np.array(ms + cands, np.int64)
    off = np.array([0, 2], np.int64)
    assert L.kt_preempt_gangs_launch(eng._h, 2, a.ctypes.data, 1, None, 3, a[2:].ctypes.data, 0, 0, 0, None) == INVALID  # gang_off missing
    assert L.kt_preempt_gangs_launch(eng._h, 2, None, 1, off.ctypes.data, 3, a[2:].ctypes.data, 0, 0, 0, None) == INVALID  # pod_rows missing
    assert L.kt_preempt_gangs_launch(eng._h, 2, a.ctypes.data, 1, off.ctypes.data, 3, None, 0, 0, 0, None) == INVALID  # cand_rows missing
    assert L.kt_preempt_gangs_launch(eng._h, 2, a.ctypes.data, 1, off.ctypes.data, -1, None, 0, 0, 0, None) == INVALID  # n_cand < 0
    assert L.kt_preempt_gangs_launch(eng._h, 2, a.ctypes.data, -1, off.ctypes.data, 3, a[2:].ctypes.data, 0, 0, 0, None) == INVALID
    assert go([0, 1, 0], [0, 3], cands) == INVALID  # a pod twice within one gang
    assert go(ms, [0, 2], [2, 3, 1]) == INVALID     # a member that is also a candidate
    assert go(ms, [0, 2], [2, 3, 2]) == INVALID     # a candidate named twice
    assert go(ms, [0, 2], [2, 99]) == RANGE
    assert go([0, 99], [0, 2], cands) == RANGE
    assert go(ms, [0, 2], cands, inc) == UNSUPPORTED
    eng.set_exchange_world(2)
    assert go(ms, [0, 2], cands) == UNSUPPORTED
    eng.set_exchange_world(1)
    eng.set_wide_sums(1)
    assert go(ms, [0, 2], cands) == UNSUPPORTED
    eng.set_wide_sums(0)
    # the 2^31 matrix rule, by n x throttle_rows and by the sum of the two alone: refused on the host, nothing is allocated
    assert go(many, np.arange(len(many) + 1), [2, 3], wide_rows) == RANGE
    assert len(many[:-1]) * 1030 <= 2**31 < (len(many[:-1]) + 5) * 1030
    assert go(many[:-1], np.arange(len(many)), [2, 3, 4, 5, 6], wide_rows) == RANGE  # (only the sum of the two)


def test_refusals_leave_pending_results_alone():
    snap, ms, cands = gang_line(5, 3)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    wide_rows = E.Engine.for_snapshot(gang_line(5, 3, T=1030, row=1029)[0])
    many = np.zeros(2**31 // 1030 + 1, np.int64)
    try:
        assert _code(lambda: eng.preempt_gangs_fetch(1, 5)) == NOT_READY
        # a pending check and a pending reconcile report survive every refused call
        plain_status, plain_summary = eng.check(n=snap.n_pods, want_status=True)
        plain = eng.reconcile(NOW, apply=False)
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        _refusals(eng, inc, wide_rows, many)
        status, summary = eng.check_fetch(snap.n_pods, True)
        assert np.array_equal(status, plain_status) and np.array_equal(summary, plain_summary)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.count, plain.used.count)
        # ... and so does a pending preempt result, of either kind
        eng.preempt_launch([1], cands, NOW)
        _refusals(eng, inc, wide_rows, many)
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == [2]
        eng.preempt_gangs_launch(ms, [0, 2], cands, NOW)
        _refusals(eng, inc, wide_rows, many)
        prefix, victims, blocker = eng.preempt_gangs_fetch(1, len(cands))
        assert (prefix.tolist(), victims.tolist(), blocker.tolist()) == ([3], [[1, 1, 1, 0, 0]], [0])
        # n == 0 is allowed only with n_gangs == 0: KT_OK, nothing is launched
        eng.preempt_gangs_launch([], [0], cands, NOW)
        assert eng.preempt_gangs_fetch(0, len(cands))[0].tolist() == []
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == RANGE
        assert wide_rows.preempt_gangs([0, 1], [0, 2], [2, 3, 4, 5, 6], NOW)[0].tolist() == [3]
    finally:
        eng.close()
        inc.close()
        wide_rows.close()


def test_slot_rules_and_dry_run(oracle_mod):
    snap, cases, want, _ = gang_case(SEEDS[0], oracle_mod)
    i = max(range(len(cases)), key=lambda c: len(cases[c][1]))
    (ms, cands), (k, b) = cases[i], want[False][i]
    off = [0, len(ms)]
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    eng = E.Engine.for_snapshot(snap)
    try:
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = [x.copy() for eq in (False, True) for x in eng.headroom(everyone, cap=E.HEADROOM_MAX_CAP, on_equal=eq)]
        res_before = eng.fetch_reserved()
        # the launch takes the check slot and the reconcile report, exactly as kt_preempt_launch does
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        eng.preempt_gangs_launch(ms, off, cands, NOW)
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == NOT_READY
        assert _code(lambda: eng.reconcile_fetch()) == NOT_READY
        # the three launches share the one pending preempt result, and each fetch reads only its own kind
        assert _code(lambda: eng.preempt_fetch(1, len(cands))) == NOT_READY
        prefix, _, blocker = eng.preempt_gangs_fetch(1, len(cands))
        assert (int(prefix[0]), int(blocker[0])) == (k, b)
        single = eng.preempt([ms[0]], cands, NOW)[0].tolist()
        eng.preempt_gangs_launch(ms, off, cands, NOW)
        eng.preempt_launch([ms[0]], cands, NOW)
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == NOT_READY
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == single
        eng.preempt_reprieve_launch([ms[0]], cands, NOW)
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == NOT_READY
        eng.preempt_gangs_launch(ms, off, cands, NOW)
        assert _code(lambda: eng.preempt_fetch(1, len(cands))) == NOT_READY
        # a pending forecast stays fetchable behind a gang launch
        first = eng.forecast(ms, [NOW], False)[0].tolist()
        eng.forecast_launch(ms, [NOW], False)
        eng.preempt_gangs_launch(ms, off, cands, NOW)
        assert eng.forecast_fetch(len(ms), 1)[0].tolist() == first
        assert int(eng.preempt_gangs_fetch(1, len(cands))[0][0]) == k
        # a later user of the check slot drops the pending result
        eng.preempt_gangs_launch(ms, off, cands, NOW)
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == NOT_READY
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        room_after = [x for eq in (False, True) for x in eng.headroom(everyone, cap=E.HEADROOM_MAX_CAP, on_equal=eq)]
        res_after = eng.fetch_reserved()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(room_before, room_after))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()
