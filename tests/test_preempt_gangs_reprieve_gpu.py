"""The gang reprieve pass on the GPU: Engine.preempt_gangs(reprieve=True) (kt_preempt_gangs_reprieve_launch /
kt_preempt_gangs_fetch, csrc/kt_kernels_preempt_gangs_reprieve.hip) against the reference of
tests/preempt_gangs_reprieve_reference.py (the walk on delete + oracle reconcile + oracle in-order admission) on the random
manifest clusters and the directed table, and against ``paging.preempt_gangs_of(reprieve=True)`` — which
tests/test_preempt_gangs_reprieve_cpu.py holds to that reference — on the shapes where the oracle walk would be slow.  Prefix,
victim bytes and blocker are compared bit for bit.  The shapes are the smallest at which the kernel can still go wrong: masked
victims across blocks of 64 candidates, lists of 1, 64, 65 and 200 entries (several per lane), entries from both chunks of the
matrix row, the 65-entry list again in the HBM workspace, one case per DT instantiation, a gang longer than a wave, more gangs
than workgroups."""
import functools
import os

import numpy as np
import pytest

import preempt_gangs_reference as GR
import preempt_gangs_reprieve_reference as GRR
import preempt_reference as PR
import reprieve_reference as RR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from test_preempt_cpu import SEEDS
from test_preempt_gangs_reprieve_cpu import gang_reprieve_case

pytestmark = pytest.mark.gpu
NOW = PR.NOW
INVALID, RANGE, NOT_READY, UNSUPPORTED = -1, -2, -5, -7


def launch(eng, gangs, cands, on_equal=False, reprieve=True):
    """All ``gangs`` (lists of member rows) in one launch -> (prefix, victims, blocker as a position in its own gang)."""
    rows = [p for ms in gangs for p in ms]
    off = np.cumsum([0] + [len(ms) for ms in gangs])
    prefix, victims, blocker = eng.preempt_gangs(rows, off, cands, NOW, on_equal, reprieve=reprieve)
    assert victims.shape == (len(gangs), len(cands))
    local = [int(b) - int(off[g]) if b >= 0 else -1 for g, b in enumerate(blocker)]
    return prefix.tolist(), victims, local


def held_to_the_model(snap, gangs, cands, on_equal=False, eng=None):
    """One launch over ``gangs`` against ``preempt_gangs_of`` with and without the walk -> (prefix, reprieved victims)."""
    own = eng is None
    eng = E.Engine.for_snapshot(snap) if own else eng
    try:
        prefix, victims, blocker = launch(eng, gangs, cands, on_equal)
        plain = launch(eng, gangs, cands, on_equal, reprieve=False)
    finally:
        if own:
            eng.close()
    ctx = paging.preempt_context(snap, NOW)
    for g, ms in enumerate(gangs):
        k, v, b = paging.preempt_gangs_of(snap, ms, cands, NOW, on_equal, ctx=ctx, reprieve=True)
        assert (prefix[g], victims[g].tolist(), blocker[g]) == (k, v, b), f"gang {g} {ms} on_equal={on_equal}"
        assert (plain[0][g], plain[1][g].tolist(), plain[2][g]) == paging.preempt_gangs_of(snap, ms, cands, NOW, on_equal, ctx=ctx)
    return np.array(prefix), victims


def held_to_everything(snap, oracle_mod, members, cands, on_equal=False):
    prefix, victims = held_to_the_model(snap, [members], cands, on_equal)
    k, v, _ = GRR.reference(snap, oracle_mod, members, cands, NOW, on_equal)
    assert (int(prefix[0]), victims[0].tolist()) == (k, v), (members, on_equal)
    GR.check_victims(snap, oracle_mod, members, cands, k, victims[0], NOW, on_equal)
    return k, v


@functools.lru_cache(maxsize=None)
def shared_list_case(seed, oracle_mod):
    """The gangs of a seed over ONE candidate list (the longest case's, without any gang's members) and their references."""
    snap, cases, _, _ = gang_reprieve_case(seed, oracle_mod)
    gangs = [ms for ms, _ in cases]
    everyone = {p for ms in gangs for p in ms}
    cands = [c for c in max((cs for _, cs in cases), key=len) if c not in everyone]
    want = {eq: [GRR.reference(snap, oracle_mod, ms, cands, NOW, eq) for ms in gangs] for eq in (False, True)}
    return gangs, cands, want


@pytest.mark.parametrize("seed", SEEDS[::3])
def test_random_manifest_clusters(seed, oracle_mod):
    snap, cases, want, walked = gang_reprieve_case(seed, oracle_mod)
    gangs, cands, want_shared = shared_list_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, NOW)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            for (ms, cs), (k, b), v in zip(cases, want[on_equal], walked[on_equal]):  # each gang over its own list
                prefix, victims, blocker = launch(eng, [ms], cs, on_equal)
                assert (prefix[0], victims[0].tolist(), blocker[0]) == (k, v, b), f"seed {seed} on_equal={on_equal} gang {ms} over {cs}"
                assert (k, v, b) == paging.preempt_gangs_of(snap, ms, cs, NOW, on_equal, ctx=ctx, reprieve=True)
            prefix, victims, blocker = launch(eng, gangs, cands, on_equal)  # all gangs of the seed in one launch
            for g, ms in enumerate(gangs):
                got = (prefix[g], victims[g].tolist(), blocker[g])
                assert got == want_shared[on_equal][g], f"seed {seed} on_equal={on_equal} gang {ms}"
                assert got == paging.preempt_gangs_of(snap, ms, cands, NOW, on_equal, ctx=ctx, reprieve=True)
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(GRR.DIRECTED))
def test_directed(name, oracle_mod):
    build, prefixes, victims = GRR.DIRECTED[name]
    snap, ms, cands = build()
    for i, on_equal in enumerate((False, True)):
        assert held_to_everything(snap, oracle_mod, ms, cands, on_equal) == (prefixes[i], victims[i])


@pytest.mark.parametrize("m", [63, 64, 65, 130])
def test_masked_victims_across_candidate_blocks(m):
    snap, ms, cands = GRR.gang_big_last(m)
    for on_equal in (False, True):
        prefix, victims = held_to_the_model(snap, [ms], cands, on_equal)
        # the big pod stays out, and with on_equal the small one that was walked last
        assert prefix.tolist() == [m - 1] and victims[0].tolist() == [int(on_equal)] + [0] * (m - 3) + [1, 0]
    # each member alone lets one more small pod back than the gang does
    assert sum(paging.preempt_of(snap, ms[1], cands, NOW, True, reprieve=True)[1]) == 1


@pytest.mark.parametrize("L,D,g", [(1, 1, 2), (64, 3, 3), (65, 3, 2), (200, 3, 3)])
def test_list_lengths(L, D, g):
    snap, ms, cands = GRR.gang_wide(L, 40, g=g, D=D)
    prefix, victims = held_to_the_model(snap, [ms], cands)
    assert prefix[0] > 1 and victims[0].sum() < prefix[0]  # somebody is reprieved


def test_entries_from_both_chunks_of_the_matrix_row():
    snap, ms, cands = GRR.gang_wide(5, 40, g=2, D=3, T=1030)
    prefix, victims = held_to_the_model(snap, [ms], cands)
    assert prefix[0] > 1 and victims[0].sum() < prefix[0]


def test_the_list_in_the_hbm_workspace_gives_the_same_bytes():
    """KT_REPRIEVE_LDS_CAP (read when the engine is created and on kt_debug_reload_env) lowers the list capacity of LDS: the
    65-entry list then lives in the engine's workspace — same code, same bytes."""
    snap, ms, cands = GRR.gang_wide(65, 40, g=3, D=3)
    gangs = [ms, ms[:2], ms[1:]]
    in_lds = held_to_the_model(snap, gangs, cands)
    assert "KT_REPRIEVE_LDS_CAP" not in os.environ
    os.environ["KT_REPRIEVE_LDS_CAP"] = "16"
    try:
        eng = E.Engine.for_snapshot(snap)
    finally:
        del os.environ["KT_REPRIEVE_LDS_CAP"]
    try:
        in_hbm = held_to_the_model(snap, gangs, cands, eng=eng)
        again = held_to_the_model(snap, gangs[::-1], cands, on_equal=True, eng=eng)  # the workspace is reused
        eng.reload_env()  # the switch is gone: back in LDS
        back = held_to_the_model(snap, gangs, cands, eng=eng)
    finally:
        eng.close()
    for a, b, c in zip(in_lds, in_hbm, back):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert (again[0] > 0).all()


@pytest.mark.parametrize("D", [3, 5, 9])
def test_every_instantiation(D):
    snap, ms, cands = GRR.gang_wide(12, 70, g=2, D=D)
    for on_equal in (False, True):
        prefix, victims = held_to_the_model(snap, [ms], cands, on_equal)
        assert prefix[0] > 1 and victims[0].sum() < prefix[0]
    snap, ms, cands = GRR.gang_big_last(70, D=D, dim=D - 1)
    assert held_to_the_model(snap, [ms], cands)[1][0].tolist() == [0] * 68 + [1, 0]


def test_a_gang_of_seventy_members(oracle_mod):
    """70 members of 1 under a threshold of 110; 34 running 1s, a pod of 36, 30 more 1s: `used` (100) has to come down to 40 for
    the last member, who meets 69 reserved — only with the 36 gone (prefix 35, `used` 30), and ten of the small ones before it,
    the last ones first, come back.  Built like gang_line(65, 35, g=70) of the prefix suite, with slack behind the big pod."""
    running = [{0: 1}] * 34 + [{0: 36}] + [{0: 1}] * 30
    snap = PR.tiny([{0: 1}] * 70 + running, {0: 110}, flags=[PR.PENDING] * 70 + [PR.COUNTED] * 65)
    ms, cands = list(range(70)), list(range(70, 135))
    assert held_to_everything(snap, oracle_mod, ms, cands) == (35, [1] * 24 + [0] * 10 + [1] + [0] * 30)


def test_more_gangs_than_workgroups():
    """2500 gangs — five distinct ones over the four pending pods, cycled, the second lap shifted by one — over 40 candidates:
    the grid is capped at 2048 one-wave workgroups, 452 of them take a second turn on the same LDS state."""
    n = 2500
    snap, pre, cands = GRR.gang_wide(6, 40, g=4, D=3)
    distinct = [[0, 1], [1, 2], [2, 3, 0], [3], [0, 1, 2, 3]]
    which = [(i + (i >= 2048)) % len(distinct) for i in range(n)]
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims, blocker = launch(eng, [distinct[w] for w in which], cands)
    finally:
        eng.close()
    ctx = paging.preempt_context(snap, NOW)
    want = [paging.preempt_gangs_of(snap, ms, cands, NOW, ctx=ctx, reprieve=True) for ms in distinct]
    assert all(k > 0 for k, _, _ in want) and len({tuple(v) for _, v, _ in want}) > 1  # (the turns of one wave differ)
    assert prefix == [want[w][0] for w in which] and blocker == [want[w][2] for w in which]
    assert np.array_equal(victims, np.array([want[w][1] for w in which], np.uint8))


@pytest.mark.parametrize("name", sorted(RR.DIRECTED))
def test_gangs_of_one_equal_the_single_reprieve(name):
    snap, p, cands = RR.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            single = eng.preempt([p], cands, NOW, on_equal, reprieve=True)
            prefix, victims, _ = eng.preempt_gangs([p], [0, 1], cands, NOW, on_equal, reprieve=True)
            assert prefix.tobytes() == single[0].tobytes() and victims.tobytes() == single[1].tobytes(), (name, on_equal)
    finally:
        eng.close()


def test_no_candidates_and_nobody_with_a_positive_prefix():
    snap, pre, cands = GRR.gang_wide(6, 40, g=4, D=3)
    gangs = [pre[:2], pre[2:]]
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims, _ = launch(eng, gangs, [])  # n_cand == 0
        assert prefix == [-1, -1] and victims.shape == (2, 0)
        prefix, victims, _ = launch(eng, gangs, cands[:1])  # one candidate is not enough: every prefix is -1
        assert prefix == [-1, -1] and not victims.any()
    finally:
        eng.close()
    snap = PR.tiny([{0: 1}, {0: 1}, {0: 4}, {0: 4}], {0: 10}, flags=[PR.PENDING] * 2 + [PR.COUNTED] * 2)
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims, blocker = launch(eng, [[0, 1], [1]], [2, 3])  # everybody passes already: prefix 0
        assert prefix == [0, 0] and blocker == [-1, -1] and not victims.any()
    finally:
        eng.close()


def test_plain_gang_launches_are_unchanged_between_reprieve_launches():
    snap, ms, cands = GRR.gang_wide(65, 40, g=3, D=3)
    gangs = [ms, ms[:2]]
    eng = E.Engine.for_snapshot(snap)
    try:
        first = launch(eng, gangs, cands, reprieve=False)
        walked = launch(eng, gangs, cands)
        second = launch(eng, gangs, cands, reprieve=False)
        eng.preempt_gangs_reprieve_launch(ms[:1], [0, 1], cands[:20], NOW, True)
        third = launch(eng, gangs, cands, reprieve=False)
        again = launch(eng, gangs, cands)
    finally:
        eng.close()
    for x in (second, third):
        assert x[0] == first[0] and x[1].tobytes() == first[1].tobytes() and x[2] == first[2]
    assert walked[0] == first[0] == again[0] and walked[2] == first[2] and walked[1].tobytes() == again[1].tobytes()
    assert (walked[1] <= first[1]).all() and walked[1].sum() < first[1].sum()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def _refusals(eng, inc, wide_rows, many):
    """Every refusal of kt_preempt_gangs_launch with its code, asked of the reprieved launch, on an engine whose pending results
    the caller then fetches."""
    ms, cands = [0, 1], [2, 3, 4]
    go = lambda rows, off, cs, e=eng: _code(lambda: e.preempt_gangs(rows, off, cs, NOW, reprieve=True))
    # the gang_off defects of kt_admit_gangs_launch
    assert go(ms, [1, 2], cands) == INVALID     # gang_off[0] != 0
    assert go(ms, [0, 1, 1, 2], cands) == INVALID  # an empty gang
    assert go(ms, [0, 2, 1, 2], cands) == INVALID  # descending
    assert go(ms, [0, 1], cands) == INVALID     # gang_off[n_gangs] != n
    assert go(ms, [0], cands) == INVALID        # no gangs for a queue of two pods
    fn, a = E.lib().kt_preempt_gangs_reprieve_launch, np.array(ms + cands, np.int64)
    off = np.array([0, 2], np.int64)
    assert fn(eng._h, 2, a.ctypes.data, 1, None, 3, a[2:].ctypes.data, 0, 0, 0, None) == INVALID  # gang_off missing
    assert fn(eng._h, 2, None, 1, off.ctypes.data, 3, a[2:].ctypes.data, 0, 0, 0, None) == INVALID  # pod_rows missing
    assert fn(eng._h, 2, a.ctypes.data, 1, off.ctypes.data, 3, None, 0, 0, 0, None) == INVALID  # cand_rows missing
    assert fn(eng._h, 2, a.ctypes.data, 1, off.ctypes.data, -1, None, 0, 0, 0, None) == INVALID  # n_cand < 0
    assert fn(eng._h, 2, a.ctypes.data, -1, off.ctypes.data, 3, a[2:].ctypes.data, 0, 0, 0, None) == INVALID
    assert fn(None, 0, None, 0, None, 0, None, 0, 0, 0, None) == INVALID
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
    assert go(many[:-1], np.arange(len(many)), [2, 3, 4, 5, 6], wide_rows) == RANGE  # (only the sum of the two)


def test_refusals_leave_pending_results_alone():
    snap, ms, cands = GRR.gang_big_last(6)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    wide_rows = E.Engine.for_snapshot(GRR.gang_big_last(6, T=1030, row=1029)[0])
    many = np.zeros(2**31 // 1030 + 1, np.int64)
    want = ([5], [[0, 0, 0, 0, 1, 0]], [0])
    try:
        assert _code(lambda: eng.preempt_gangs_fetch(1, 6)) == NOT_READY
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
        # ... and so does a pending preempt result, of every kind
        eng.preempt_reprieve_launch([1], cands, NOW)
        _refusals(eng, inc, wide_rows, many)
        assert [x.tolist() for x in eng.preempt_fetch(1, len(cands))] == [[5], [[0, 0, 0, 0, 1, 0]]]
        eng.preempt_gangs_launch(ms, [0, 2], cands, NOW)
        _refusals(eng, inc, wide_rows, many)
        assert [x.tolist() for x in eng.preempt_gangs_fetch(1, len(cands))] == [[5], [[1, 1, 1, 1, 1, 0]], [0]]
        eng.preempt_gangs_reprieve_launch(ms, [0, 2], cands, NOW)
        _refusals(eng, inc, wide_rows, many)
        assert tuple(x.tolist() for x in eng.preempt_gangs_fetch(1, len(cands))) == want
        # n == 0 is allowed only with n_gangs == 0: KT_OK, nothing is launched
        eng.preempt_gangs_reprieve_launch([], [0], cands, NOW)
        assert eng.preempt_gangs_fetch(0, len(cands))[0].tolist() == []
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == RANGE
        assert tuple(x.tolist() for x in wide_rows.preempt_gangs(ms, [0, 2], cands, NOW, reprieve=True)) == want
    finally:
        eng.close()
        inc.close()
        wide_rows.close()


def test_slot_rules_and_dry_run():
    snap, ms, cands = GRR.gang_wide(6, 40, g=3, D=3)
    off = [0, len(ms)]
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    eng = E.Engine.for_snapshot(snap)
    try:
        want = [x.copy() for x in eng.preempt_gangs(ms, off, cands, NOW, reprieve=True)]
        unwalked = [x.copy() for x in eng.preempt_gangs(ms, off, cands, NOW)]
        assert want[0].tobytes() == unwalked[0].tobytes() and want[2].tobytes() == unwalked[2].tobytes() and want[1].sum() < unwalked[1].sum()
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        res_before = eng.fetch_reserved()
        # the launch takes the check slot and the reconcile report, exactly as kt_preempt_gangs_launch does
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        eng.preempt_gangs_reprieve_launch(ms, off, cands, NOW)
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == NOT_READY
        assert _code(lambda: eng.reconcile_fetch()) == NOT_READY
        # the four launches share the one pending preempt result, and each fetch reads only its own kind
        assert _code(lambda: eng.preempt_fetch(1, len(cands))) == NOT_READY
        assert [x.tobytes() for x in eng.preempt_gangs_fetch(1, len(cands))] == [x.tobytes() for x in want]
        eng.preempt_gangs_reprieve_launch(ms, off, cands, NOW)
        eng.preempt_reprieve_launch([ms[0]], cands, NOW)
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == NOT_READY
        single = eng.preempt_fetch(1, len(cands))
        eng.preempt_gangs_reprieve_launch(ms, off, cands, NOW)
        eng.preempt_launch([ms[0]], cands, NOW)
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == NOT_READY
        assert eng.preempt_fetch(1, len(cands))[0].tobytes() == single[0].tobytes()
        # a plain gang launch between two reprieve launches returns the unreprieved mask
        eng.preempt_gangs_reprieve_launch(ms, off, cands, NOW)
        eng.preempt_gangs_launch(ms, off, cands, NOW)
        assert [x.tobytes() for x in eng.preempt_gangs_fetch(1, len(cands))] == [x.tobytes() for x in unwalked]
        eng.preempt_gangs_reprieve_launch(ms, off, cands, NOW)
        assert [x.tobytes() for x in eng.preempt_gangs_fetch(1, len(cands))] == [x.tobytes() for x in want]
        # a pending forecast stays fetchable behind the launch
        first = eng.forecast(ms, [NOW], False)[0].tolist()
        eng.forecast_launch(ms, [NOW], False)
        eng.preempt_gangs_reprieve_launch(ms, off, cands, NOW)
        assert eng.forecast_fetch(len(ms), 1)[0].tolist() == first
        assert [x.tobytes() for x in eng.preempt_gangs_fetch(1, len(cands))] == [x.tobytes() for x in want]
        # a later user of the check slot drops the pending result
        eng.preempt_gangs_reprieve_launch(ms, off, cands, NOW)
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.preempt_gangs_fetch(1, len(cands))) == NOT_READY
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        res_after = eng.fetch_reserved()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()
