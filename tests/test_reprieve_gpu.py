"""The reprieve pass on the GPU: Engine.preempt(reprieve=True) (kt_preempt_reprieve_launch / kt_preempt_fetch,
csrc/kt_kernels_reprieve.hip) against the reference of tests/reprieve_reference.py (the walk on delete + oracle reconcile +
oracle check) on the random manifest clusters and the directed cases, and against ``paging.preempt_of(reprieve=True)`` — which
tests/test_reprieve_cpu.py holds to that reference — on the shapes where the oracle walk would be slow.  Prefix and victim bytes
are compared bit for bit.  The shapes are the smallest at which the kernel can still go wrong: masked victims across blocks of
64 candidates, lists of 1, 64, 65 and about 200 entries (several per lane), entries from both chunks of the matrix row, the
65-entry list again in the HBM workspace, one case per DT instantiation, more preemptors than workgroups."""
import os

import numpy as np
import pytest

import preempt_reference as PR
import reprieve_reference as RR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from test_preempt_cpu import SEEDS
from test_reprieve_cpu import reprieve_case

pytestmark = pytest.mark.gpu
NOW = PR.NOW


def held_to_the_model(snap, pre, cands, on_equal=False, eng=None):
    """The launch over the preemptors ``pre`` against ``preempt_of`` with and without the walk -> (prefix, reprieved victims)."""
    own = eng is None
    eng = E.Engine.for_snapshot(snap) if own else eng
    try:
        prefix, victims = eng.preempt(pre, cands, NOW, on_equal, reprieve=True)
        plain = eng.preempt(pre, cands, NOW, on_equal)
    finally:
        if own:
            eng.close()
    ctx = paging.preempt_context(snap, NOW)
    assert victims.shape == (len(pre), len(cands))
    for i, p in enumerate(pre):
        k, v = paging.preempt_of(snap, p, cands, NOW, on_equal, ctx=ctx, reprieve=True)
        assert (int(prefix[i]), victims[i].tolist()) == (k, v), f"preemptor {i} (pod {p}) on_equal={on_equal}"
        assert (int(plain[0][i]), plain[1][i].tolist()) == paging.preempt_of(snap, p, cands, NOW, on_equal, ctx=ctx)
    return prefix, victims


@pytest.mark.parametrize("seed", SEEDS)
def test_random_manifest_clusters(seed, oracle_mod):
    snap, cases, want, walked = reprieve_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            for (p, cands), k, v in zip(cases, want[on_equal], walked[on_equal]):
                prefix, victims = eng.preempt([p], cands, NOW, on_equal, reprieve=True)
                assert int(prefix[0]) == k and victims[0].tolist() == v, f"seed {seed} on_equal={on_equal} pod{p} over {cands}"
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(set(PR.DIRECTED) | set(RR.DIRECTED)))
def test_directed(name, oracle_mod):
    snap, p, cands = (RR.DIRECTED.get(name) or PR.DIRECTED[name])()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            prefix, victims = eng.preempt([p], cands, NOW, on_equal, reprieve=True)
            assert (int(prefix[0]), victims[0].tolist()) == RR.reference(snap, oracle_mod, p, cands, NOW, on_equal)
    finally:
        eng.close()


def test_the_example_of_the_issue():
    snap, p, cands = RR.DIRECTED["one-one-six"]()
    eng = E.Engine.for_snapshot(snap)
    try:
        assert [x.tolist() for x in eng.preempt([p], cands, NOW)] == [[3], [[1, 1, 1]]]
        assert [x.tolist() for x in eng.preempt([p], cands, NOW, reprieve=True)] == [[3], [[0, 0, 1]]]
    finally:
        eng.close()


@pytest.mark.parametrize("m", [63, 64, 65, 130])
def test_masked_victims_across_candidate_blocks(m):
    snap, p, cands = RR.big_last(m)
    for on_equal in (False, True):
        prefix, victims = held_to_the_model(snap, [p], cands, on_equal)
        assert int(prefix[0]) == m - 1 and victims[0].tolist() == ([1] if on_equal else [0]) + [0] * (m - 3) + [1, 0]


@pytest.mark.parametrize("L,D", [(1, 1), (64, 3), (65, 3), (200, 3)])
def test_list_lengths(L, D):
    snap, pre, cands = RR.wide(L, 40, D=D, n_pre=3)
    prefix, victims = held_to_the_model(snap, pre, cands)
    assert (prefix > 1).all() and (victims.sum(axis=1) < prefix).all()  # somebody is reprieved, for every preemptor


def test_entries_from_both_chunks_of_the_matrix_row():
    snap, pre, cands = RR.wide(5, 40, D=3, T=1030, n_pre=2)
    prefix, victims = held_to_the_model(snap, pre, cands)
    assert (prefix > 1).all() and (victims.sum(axis=1) < prefix).all()


def test_the_list_in_the_hbm_workspace_gives_the_same_bytes():
    """KT_REPRIEVE_LDS_CAP (read when the engine is created and on kt_debug_reload_env) lowers the list capacity of LDS: the
    65-entry list then lives in the engine's workspace — same code, same bytes."""
    snap, pre, cands = RR.wide(65, 40, D=3, n_pre=3)
    in_lds = held_to_the_model(snap, pre, cands)
    assert "KT_REPRIEVE_LDS_CAP" not in os.environ
    os.environ["KT_REPRIEVE_LDS_CAP"] = "16"
    try:
        eng = E.Engine.for_snapshot(snap)
    finally:
        del os.environ["KT_REPRIEVE_LDS_CAP"]
    try:
        in_hbm = held_to_the_model(snap, pre, cands, eng=eng)
        again = held_to_the_model(snap, pre[::-1], cands, on_equal=True, eng=eng)  # the workspace is reused
        eng.reload_env()  # the switch is gone: back in LDS
        back = held_to_the_model(snap, pre, cands, eng=eng)
    finally:
        eng.close()
    for a, b, c in zip(in_lds, in_hbm, back):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert (again[0] > 0).all()


@pytest.mark.parametrize("D", [3, 5, 9])
def test_every_instantiation(D):
    snap, pre, cands = RR.wide(12, 70, D=D, n_pre=2)
    for on_equal in (False, True):
        prefix, victims = held_to_the_model(snap, pre, cands, on_equal)
        assert (prefix > 1).all() and (victims.sum(axis=1) < prefix).all()
    snap, p, cands = RR.big_last(70, D=D, dim=D - 1)
    assert held_to_the_model(snap, [p], cands)[1][0].tolist() == [0] * 68 + [1, 0]


def test_more_preemptors_than_workgroups():
    """2500 preemptors — the four pending pods over and over, the second lap shifted by one — over 40 candidates: the grid is
    capped at 2048 one-wave workgroups, 452 of them take a second turn on the same LDS state."""
    n = 2500
    snap, pre, cands = RR.wide(6, 40, D=3, n_pre=4)
    rows = [(i + (i >= 2048)) % 4 for i in range(n)]
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims = eng.preempt(rows, cands, NOW, reprieve=True)
    finally:
        eng.close()
    ctx = paging.preempt_context(snap, NOW)
    want = [paging.preempt_of(snap, p, cands, NOW, ctx=ctx, reprieve=True) for p in pre]
    assert len({tuple(v) for _, v in want}) > 1  # (the turns of one wave differ)
    assert prefix.tolist() == [want[r][0] for r in rows]
    assert np.array_equal(victims, np.array([want[r][1] for r in rows], np.uint8))


def test_no_candidates_and_nobody_with_a_positive_prefix():
    snap, pre, cands = RR.wide(6, 40, D=3, n_pre=4)
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims = eng.preempt(pre, [], NOW, reprieve=True)  # n_cand == 0
        assert prefix.tolist() == [-1] * 4 and victims.shape == (4, 0)
        prefix, victims = eng.preempt(pre, cands[:1], NOW, reprieve=True)  # one candidate is not enough: every prefix is -1
        assert prefix.tolist() == [-1] * 4 and not victims.any()
    finally:
        eng.close()
    snap = PR.tiny([{0: 1}, {0: 1}, {0: 4}, {0: 4}], {0: 10}, flags=[PR.PENDING] * 2 + [PR.COUNTED] * 2)
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims = eng.preempt([0, 1], [2, 3], NOW, reprieve=True)  # everybody passes already: prefix 0
        assert prefix.tolist() == [0, 0] and not victims.any()
    finally:
        eng.close()


def test_prefix_launches_are_unchanged_between_reprieve_launches():
    snap, pre, cands = RR.wide(65, 40, D=3, n_pre=3)
    eng = E.Engine.for_snapshot(snap)
    try:
        first = eng.preempt(pre, cands, NOW)
        walked = eng.preempt(pre, cands, NOW, reprieve=True)
        second = eng.preempt(pre, cands, NOW)
        eng.preempt_reprieve_launch(pre[:1], cands[:20], NOW, True)
        third = eng.preempt(pre, cands, NOW)
        again = eng.preempt(pre, cands, NOW, reprieve=True)
    finally:
        eng.close()
    for a, b, c in zip(first, second, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert walked[0].tobytes() == first[0].tobytes() == again[0].tobytes() and walked[1].tobytes() == again[1].tobytes()
    assert (walked[1] <= first[1]).all() and walked[1].sum() < first[1].sum()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def test_validation_and_not_ready():
    snap, p, cands = RR.big_last(6)
    walk = lambda eng, a, b, **kw: eng.preempt(a, b, NOW, reprieve=True, **kw)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    try:
        assert _code(lambda: eng.preempt_fetch(1, 6)) == -5  # KT_ERR_NOT_READY
        assert _code(lambda: walk(eng, [0], [1, 2, 0])) == -1  # a preemptor that is a candidate
        assert _code(lambda: walk(eng, [0], [1, 2, 1])) == -1  # a candidate named twice
        assert _code(lambda: walk(eng, [0], [1, 99])) == -2
        assert E.lib().kt_preempt_reprieve_launch(eng._h, 1, np.array([0], np.int64).ctypes.data, -1, None, 0, 0, 0, None) == -1
        assert E.lib().kt_preempt_reprieve_launch(eng._h, 1, None, 0, None, 0, 0, 0, None) == -1  # a missing row array
        assert E.lib().kt_preempt_reprieve_launch(None, 0, None, 0, None, 0, 0, 0, None) == -1
        assert _code(lambda: walk(inc, [0], [1, 2])) == -7  # KT_ERR_UNSUPPORTED
        eng.set_exchange_world(2)
        assert _code(lambda: walk(eng, [0], [1, 2])) == -7
        eng.set_exchange_world(1)
        # (n + n_cand) x throttle_rows beyond 2^31 bytes of matrix, by either product: refused on the host, nothing is allocated
        wide_rows = E.Engine.for_snapshot(RR.big_last(6, T=1030, row=1029)[0])
        try:
            many = np.zeros(2**31 // 1030 + 1, np.int64)
            assert _code(lambda: walk(wide_rows, many, [1, 2])) == -2  # KT_ERR_OUT_OF_RANGE (n x throttle_rows)
            assert _code(lambda: walk(wide_rows, many[:-1], [1, 2, 3, 4, 5])) == -2  # (only the sum of the two)
            assert [x.tolist() for x in walk(wide_rows, [0], cands)] == [[5], [[0, 0, 0, 0, 1, 0]]]
        finally:
            wide_rows.close()
        # `used` wider than int64: refused, and a refused call leaves the check slot and a pending result to whoever holds them
        eng.check_launch(snap.n_pods, want_status=True)
        eng.set_wide_sums(1)
        assert _code(lambda: walk(eng, [0], [1, 2])) == -7
        eng.set_wide_sums(0)
        eng.check_fetch(snap.n_pods, True)
        eng.preempt_reprieve_launch([0], cands, NOW)
        assert _code(lambda: walk(eng, [0], [1, 1])) == -1
        assert [x.tolist() for x in eng.preempt_fetch(1, len(cands))] == [[5], [[0, 0, 0, 0, 1, 0]]]
        eng.preempt_reprieve_launch([], cands, NOW)  # n == 0: KT_OK, nothing launched
        assert eng.preempt_fetch(0, len(cands))[0].tolist() == []
        assert _code(lambda: eng.preempt_fetch(1, len(cands))) == -2  # more than the last launch had
    finally:
        eng.close()
        inc.close()


def test_slot_rules(oracle_mod):
    snap, pre, cands = RR.wide(6, 40, D=3, n_pre=2)
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    eng = E.Engine.for_snapshot(snap)
    try:
        want = [x.copy() for x in eng.preempt(pre, cands, NOW, reprieve=True)]
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        res_before = eng.fetch_reserved()
        plain = eng.reconcile(NOW, apply=False)
        # the launch takes the check slot and the reconcile result buffers
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        eng.preempt_reprieve_launch(pre, cands, NOW)
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == -5
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a kt_check served by the few-pod path runs beside the slot and leaves it fetchable; any other kt_check takes the slot
        served = eng.few_checks_served()
        eng.check_atomic(rows=everyone[:2], want_status=False)
        if eng.few_checks_served() > served:
            assert [a.tobytes() for a in eng.preempt_fetch(2, len(cands))] == [a.tobytes() for a in want]
        else:
            assert _code(lambda: eng.preempt_fetch(2, len(cands))) == -5
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves it fetchable
        eng.aggregate_launch()
        eng.preempt_reprieve_launch(pre, cands, NOW)
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        assert [a.tobytes() for a in eng.preempt_fetch(2, len(cands))] == [a.tobytes() for a in want]
        # the two kinds of launch share the one pending result: the later one is what is fetched
        eng.preempt_reprieve_launch(pre, cands, NOW)
        eng.preempt_launch(pre, cands, NOW)
        assert eng.preempt_fetch(2, len(cands))[1].sum() > want[1].sum()
        # a pending headroom launch is dropped, and a later user of the check slot drops the result
        eng.headroom_launch(2, pre, E.HEADROOM_MAX_CAP, False)
        eng.preempt_reprieve_launch(pre, cands, NOW)
        assert _code(lambda: eng.headroom_fetch(2)) == -5
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.preempt_fetch(2, len(cands))) == -5
        # a dry run: the stored status and the reserved amounts are unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        res_after = eng.fetch_reserved()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()
