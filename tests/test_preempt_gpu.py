"""The preemption query on the GPU: Engine.preempt (kt_preempt_launch / kt_preempt_fetch, csrc/kt_kernels_preempt.hip) against
the reference of tests/preempt_reference.py (delete the prefix, reconcile and check with the oracle, for every k),
``paging.preempt_of`` and the engine's own composed path on a scratch engine (kt_delete_pods + kt_reconcile_launch(APPLY) +
kt_check per step).  Prefix and victim mask are compared bit for bit.  The shapes are the smallest at which the kernel can
still go wrong: candidate blocks of 64 and their carries, a blocking throttle in the second chunk of the affected-throttle
list, one case per DT instantiation (D = 1, 8, 16), more preemptors than ... one (the grid strides per preemptor)."""
import numpy as np
import pytest

import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_preempt_cpu import SEEDS, preempt_case

pytestmark = pytest.mark.gpu
NOW = PR.NOW


def composed_prefix(snap, p, cands, on_equal):
    """What a caller does today, on a scratch engine: delete a candidate, reconcile every throttle, check the pod again."""
    eng = E.Engine.for_snapshot(snap)
    try:
        if not int(snap.pod_flags[p]) & S.POD_VALID:
            return -1
        _, summary = eng.check(rows=np.array(list(cands) + [p], np.int64), want_status=False)
        if int(summary[-1]) & 3 == S.VERDICT_ERROR:
            return -1
        m_eff = next((j for j, c in enumerate(cands) if not int(snap.pod_flags[c]) & S.POD_VALID or int(summary[j]) & 3 == S.VERDICT_ERROR),
                     len(cands))
        for k in range(m_eff + 1):
            if k:
                eng.delete_pods(np.array([cands[k - 1]], np.int64))
            eng.reconcile(NOW, apply=True)
            _, s = eng.check(rows=np.array([p], np.int64), on_equal=on_equal, want_status=False)
            if int(s[0]) & 3 == S.VERDICT_ALLOW:
                return k
        return -1
    finally:
        eng.close()


def held_to_everything(snap, oracle_mod, p, cands, on_equal=False, composed=True, eng=None):
    own = eng is None
    eng = E.Engine.for_snapshot(snap) if own else eng
    try:
        prefix, victims = eng.preempt([p], cands, NOW, on_equal)
    finally:
        if own:
            eng.close()
    want = PR.reference_prefix(snap, oracle_mod, p, cands, NOW, on_equal)
    model = paging.preempt_of(snap, p, cands, NOW, on_equal)
    assert int(prefix[0]) == want == model[0], (int(prefix[0]), want, model[0])
    assert victims.shape == (1, len(cands)) and victims[0].tolist() == model[1]
    PR.check_victims(snap, oracle_mod, p, cands, want, victims[0], NOW, on_equal)
    if composed:
        assert composed_prefix(snap, p, cands, on_equal) == want
    return want


@pytest.mark.parametrize("seed", SEEDS[::3])
def test_random_manifest_clusters(seed, oracle_mod):
    snap, cases, want = preempt_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, NOW)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            for (p, cands), k in zip(cases, want[on_equal]):
                prefix, victims = eng.preempt([p], cands, NOW, on_equal)
                model = paging.preempt_of(snap, p, cands, NOW, on_equal, ctx=ctx)
                assert int(prefix[0]) == k == model[0], f"seed {seed} on_equal={on_equal} pod{p} over {cands}"
                assert victims[0].tolist() == model[1]
        p, cands = max(cases, key=lambda c: len(c[1]))
        assert composed_prefix(snap, p, cands, False) == want[False][cases.index((p, cands))]
    finally:
        eng.close()


@pytest.mark.parametrize("m,k_star", [(1, 1), (63, 63), (64, 64), (65, 64), (65, 65), (130, 64), (130, 65), (130, 129), (130, 130)])
def test_candidate_blocks_and_carries(m, k_star, oracle_mod):
    snap, p, cands = PR.line(m, k_star)
    assert held_to_everything(snap, oracle_mod, p, cands, composed=m <= 65 or k_star == 130) == k_star


@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    snap, p, cands = PR.line(70, 66, D=D, dim=D - 1)
    for on_equal in (False, True):
        assert held_to_everything(snap, oracle_mod, p, cands, on_equal, composed=not on_equal) == 66 + on_equal


def test_blocking_throttle_in_the_second_list_chunk(oracle_mod):
    snap, p, cands = PR.line(5, 3, T=1030, row=1029)
    assert held_to_everything(snap, oracle_mod, p, cands) == 3


def test_seventy_preemptors_in_one_launch(oracle_mod):
    # preemptors 0..69 ask 1, 2, 3 or 12 (more than the threshold: never); candidates 70..134 run with 1 each, threshold 10
    m, n = 65, 70
    asks = [(1, 2, 3, 12)[i % 4] for i in range(n)]
    snap = PR.tiny([{0: a} for a in asks] + [{0: 1}] * m, {0: 10}, flags=[PR.PENDING] * n + [PR.COUNTED] * m)
    cands = list(range(n, n + m))
    want = {a: PR.reference_prefix(snap, oracle_mod, asks.index(a), cands, NOW) for a in set(asks)}
    assert want[12] == -1 and want[1] == 56 and want[3] == 58
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims = eng.preempt(list(range(n)), cands, NOW)
        one, _ = eng.preempt([3], cands, NOW, want_victims=False)
    finally:
        eng.close()
    assert prefix.tolist() == [want[a] for a in asks] and int(one[0]) == -1
    for i in range(n):
        assert victims[i].tolist() == [int(j < prefix[i]) for j in range(m)]


def test_more_preemptors_than_workgroups(oracle_mod):
    """The launch caps its grid at 2048 workgroups of one wave: with 2500 preemptors (the four pending pods, over and over) 452
    waves take a second turn — the victim row is zeroed again and the affected-throttle list in LDS is rewritten."""
    m, n = 70, 2500
    asks = (1, 2, 3, 12)
    snap = PR.tiny([{0: a} for a in asks] + [{0: 1}] * m, {0: 10}, flags=[PR.PENDING] * 4 + [PR.COUNTED] * m)
    cands = list(range(4, 4 + m))
    want = [PR.reference_prefix(snap, oracle_mod, i, cands, NOW) for i in range(4)]
    assert want == [61, 62, 63, -1]
    # the turns of one wave differ: preemptor i and i + 2048 are different pods (2048 % 4 == 0, so shift the second lap by one)
    rows = [(i + (i >= 2048)) % 4 for i in range(n)]
    eng = E.Engine.for_snapshot(snap)
    try:
        prefix, victims = eng.preempt(rows, cands, NOW)
    finally:
        eng.close()
    assert prefix.tolist() == [want[r] for r in rows]
    assert np.array_equal(victims, (np.arange(m)[None, :] < prefix[:, None]).astype(np.uint8))


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_directed(name, oracle_mod):
    snap, p, cands = PR.DIRECTED[name]()
    for on_equal in (False, True):
        held_to_everything(snap, oracle_mod, p, cands, on_equal)


def test_directed_cases_are_not_vacuous(oracle_mod):
    def ref(name, eq=False):
        snap, p, cands = PR.DIRECTED[name]()
        return PR.reference_prefix(snap, oracle_mod, p, cands, NOW, eq)

    assert ref("equality-throttle", False) == 1 and ref("equality-throttle", True) == 2
    assert ref("equality-step3-clusterthrottle", False) != ref("equality-step3-clusterthrottle", True)
    assert ref("exceeds-threshold") == -1 and ref("already-passing") == 0 and ref("no-candidates") == -1
    assert ref("presence-through-one-victim") == 2 and ref("error-candidate-cuts") == -1 and ref("uncounted-interleaved") == 4
    assert ref("error-throttle-override-active") == 0  # (the override's threshold would make it -1)
    assert ref("override-active-now") >= 1 and ref("stale-stored-status") >= 1 and ref("reserved") >= 1


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def test_validation_and_not_ready():
    snap, p, cands = PR.line(5, 3)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    try:
        assert _code(lambda: eng.preempt_fetch(1, 5)) == -5  # KT_ERR_NOT_READY
        assert _code(lambda: eng.preempt([0], [1, 2, 0], NOW)) == -1  # a preemptor that is a candidate
        assert _code(lambda: eng.preempt([0], [1, 2, 1], NOW)) == -1  # a candidate named twice
        assert _code(lambda: eng.preempt([0], [1, 99], NOW)) == -2
        assert E.lib().kt_preempt_launch(eng._h, 1, np.array([0], np.int64).ctypes.data, -1, None, 0, 0, 0, None) == -1
        assert _code(lambda: inc.preempt([0], [1, 2], NOW)) == -7  # KT_ERR_UNSUPPORTED
        eng.set_exchange_world(2)
        assert _code(lambda: eng.preempt([0], [1, 2], NOW)) == -7
        eng.set_exchange_world(1)
        # (n + n_cand) x throttle_rows beyond 2^31 bytes of matrix, by either product: refused on the host, nothing is allocated
        wide_rows = E.Engine.for_snapshot(PR.line(5, 3, T=1030, row=1029)[0])
        try:
            many = np.zeros(2**31 // 1030 + 1, np.int64)
            assert _code(lambda: wide_rows.preempt(many, [1, 2], NOW)) == -2  # KT_ERR_OUT_OF_RANGE (n x throttle_rows)
            assert len(many[:-1]) * 1030 <= 2**31 < (len(many[:-1]) + 5) * 1030
            assert _code(lambda: wide_rows.preempt(many[:-1], [1, 2, 3, 4, 5], NOW)) == -2  # (only the sum of the two)
            assert wide_rows.preempt([0], [1, 2, 3, 4, 5], NOW)[0].tolist() == [3]
        finally:
            wide_rows.close()
        # `used` wider than int64: refused, and a refused call leaves the check slot to the launch that holds it
        eng.check_launch(snap.n_pods, want_status=True)
        eng.set_wide_sums(1)
        assert _code(lambda: eng.preempt([0], [1, 2], NOW)) == -7
        eng.set_wide_sums(0)
        eng.check_fetch(snap.n_pods, True)
        eng.preempt_launch([], cands, NOW)  # n == 0: KT_OK, nothing launched
        assert eng.preempt_fetch(0, len(cands))[0].tolist() == []
        prefix, _ = eng.preempt([0], cands, NOW)
        assert prefix.tolist() == [3]
    finally:
        eng.close()
        inc.close()


def _stored_readback(eng, rows):
    """The engine has no call that hands out the stored status.  What reads it QUANTITATIVELY is the headroom query: the copies
    that still fit are (calculatedThreshold - used - reserved) / request per name and for the pod count, and the limiting row
    names the throttle — a stored `used` or calculatedThreshold that moved without flipping a verdict moves these."""
    out = []
    for eq in (False, True):
        out += list(eng.headroom(rows, cap=E.HEADROOM_MAX_CAP, on_equal=eq))
    return out


def test_slot_rule_and_dry_run(oracle_mod):
    snap, cases, want = preempt_case(SEEDS[0], oracle_mod)
    p, cands = max(cases, key=lambda c: len(c[1]))
    k = want[False][cases.index((p, cands))]
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    eng = E.Engine.for_snapshot(snap)
    try:
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = _stored_readback(eng, everyone)
        res_before = eng.fetch_reserved()
        plain = eng.reconcile(NOW, apply=False)
        # the launch takes the check slot and the reconcile result buffers
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        eng.preempt_launch([p], cands, NOW)
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == -5
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a kt_check served by the few-pod path runs beside the slot and leaves it fetchable; any other kt_check takes the slot
        served = eng.few_checks_served()
        eng.check_atomic(rows=everyone[:2], want_status=False)
        if eng.few_checks_served() > served:
            assert eng.preempt_fetch(1, len(cands))[0].tolist() == [k]
        else:
            assert _code(lambda: eng.preempt_fetch(1, len(cands))) == -5
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves it fetchable
        eng.aggregate_launch()
        eng.preempt_launch([p], cands, NOW)
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == [k]
        # a later user of the check slot drops it
        eng.preempt_launch([p], cands, NOW)
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.preempt_fetch(1, len(cands))) == -5
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        res_after = eng.fetch_reserved()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, _stored_readback(eng, everyone)))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()
