"""kt_paged_preempt on the GPU: the victim prefix and its reprieve pass over pages of resource names, held to
tests/paged_preempt_reference.py (delete, oracle reconcile per page, OR of the bytes, oracle check per page, combine) — exact,
integers and bytes — with and without KT_PREEMPT_REPRIEVE, for both isThrottledOnEqual values where cheap."""
import os

import numpy as np
import pytest

import paged_preempt_reference as PPR
import preempt_reference as PR
import reprieve_reference as RR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd.objects import ClusterState
from test_paged_preempt_cpu import SEEDS, paged_case, reference_answers, whole_threshold_cluster

pytestmark = pytest.mark.gpu
NOW = PPR.NOW
NONE = E.PREEMPT_NONE


def _engines(snaps, **kw):
    return [E.Engine.for_snapshot(s, **kw) for s in snaps]


def _close(engs):
    for e in engs:
        e.close()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def _both(engs, pre, cands, on_equal=False):
    """-> (prefix [n], prefix mask [n][m], reprieved victims [n][m]); the two calls agree on the prefix."""
    prefix, mask = E.paged_preempt(engs, pre, cands, NOW, on_equal)
    again, walked = E.paged_preempt(engs, pre, cands, NOW, on_equal, reprieve=True)
    assert prefix.tolist() == again.tolist()
    return prefix, mask, walked


def held_to_the_reference(snaps, oracle_mod, p, cands, on_equals=(False, True), engs=None):
    own = engs is None
    engs = _engines(snaps) if own else engs
    out = []
    try:
        for on_equal in on_equals:
            want = PPR.reference(snaps, oracle_mod, p, cands, NOW, on_equal)
            prefix, mask, walked = _both(engs, [p], cands, on_equal)
            assert (int(prefix[0]), walked[0].tolist()) == want, f"on_equal={on_equal}"
            PPR.check_victims(snaps, oracle_mod, p, cands, int(prefix[0]), mask[0], NOW, on_equal)
            assert (int(prefix[0]), mask[0].tolist()) == paging.paged_preempt_of(snaps, p, cands, NOW, on_equal)
            out.append(want)
    finally:
        if own:
            _close(engs)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_random_wide_clusters(seed, oracle_mod):
    _, snaps, cases = paged_case(seed)
    assert len(snaps) >= 3
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            for (p, cands), (k, walked) in zip(cases, reference_answers(seed, on_equal)):
                prefix, mask, got = _both(engs, [p], cands, on_equal)
                assert (int(prefix[0]), got[0].tolist()) == (k, walked), f"seed {seed} pod {p} on_equal={on_equal}"
                assert (k, mask[0].tolist()) == paging.paged_preempt_of(snaps, p, cands, NOW, on_equal), f"seed {seed} pod {p}: mask"
        # all preemptors of one candidate list in one call: one wave each
        p0, cands = cases[-1]
        pre = [q for q in range(snaps[0].n_pods) if q not in cands]
        if pre:
            prefix, mask, got = _both(engs, pre, cands)
            for i, q in enumerate(pre):
                assert (int(prefix[i]), got[i].tolist()) == paging.paged_preempt_of(snaps, q, cands, NOW, reprieve=True), f"seed {seed} pod {q}"
    finally:
        _close(engs)


def test_the_calculated_threshold_is_read_as_a_whole(oracle_mod):
    cs = whole_threshold_cluster()
    snaps = [b.snapshot for b in cs.build_pages()]
    assert PPR.reference(snaps, oracle_mod, 0, [1]) == (1, [1])
    engs = _engines(snaps)
    try:
        # the pages' own bytes disagree; page 0 on its own byte keeps spec {cpu: 1} and answers KT_PREEMPT_NONE
        assert [int(e.reconcile(NOW, apply=False).calc_updated[0]) for e in engs] == [0, 1]
        assert engs[0].preempt([0], [1], NOW)[0].tolist() == [NONE]
        for reprieve in (False, True):
            prefix, victims = E.paged_preempt(engs, [0], [1], NOW, reprieve=reprieve)
            assert (prefix.tolist(), victims.tolist()) == ([1], [[1]])
        # between a kt_paged_reconcile(APPLY) and the host's write-back the stored calculatedAt flags differ between the pages
        _, replaced, _ = E.paged_reconcile(engs, NOW, apply=True)
        assert replaced.tolist() == [1]
        assert [int(e.reconcile(NOW, apply=False).calc_updated[0]) for e in engs] == [0, 0]  # nothing left to replace on either
        for reprieve in (False, True):
            prefix, victims = E.paged_preempt(engs, [0], [1], NOW, reprieve=reprieve)
            assert (prefix.tolist(), victims.tolist()) == ([1], [[1]])
    finally:
        _close(engs)


@pytest.mark.parametrize("name", sorted(PPR.DIRECTED))
def test_directed(name, oracle_mod):
    snaps, p, cands = PPR.DIRECTED[name]()
    held_to_the_reference(snaps, oracle_mod, p, cands)


def test_the_directed_answers():
    for make, want, walked in ((PPR.non_monotone, 3, None), (PPR.second_page_line, 66, None), (PPR.count_only, 2, [1, 1, 0]),
                               (PPR.reprieve_across_pages, 2, [1, 1, 0, 0])):
        snaps, p, cands = make()
        engs = _engines(snaps)
        try:
            prefix, mask, got = _both(engs, [p], cands)
            assert prefix.tolist() == [want], make.__name__
            if walked is not None:
                assert got[0].tolist() == walked, make.__name__
        finally:
            _close(engs)


def _error_throttle_wide(blocked):
    """The cluster of preempt_reference._error_throttle_override widened to 20 names (two pages): the Throttle's reconcile is an
    error (pod "other" reaches a term that does not convert), so it keeps its stored status on every page.  As stored — never
    reconciled, no calculatedAt — the check reads spec: cpu 100 lets the pending pod through although the override active at
    `now` says 5; ``blocked``: spec names r19 with 0 on page 1, which the pending pod's 1 exceeds whoever is deleted."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    extra = {f"example.com/r{k:02d}": "1" for k in range(20)}
    for name, app, cpu, running in (("pending", "a", "6", False), ("victim", "a", "4", True), ("other", "b", "4", True)):
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": dict(extra, cpu=cpu)}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": app}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    threshold = {"cpu": "100"}
    if blocked:
        threshold["example.com/r19"] = "0"
    cs.add({"kind": "Throttle", "metadata": {"name": "thr", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": threshold},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}},
                                                    {"podSelector": {"matchExpressions": [{"key": "app", "operator": "Bogus"}]}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": "2026-02-01T00:00:00Z",
                                                      "threshold": {"resourceRequests": {"cpu": "5"}}}]}})
    return [b.snapshot for b in cs.build_pages()], 0, [1]


@pytest.mark.parametrize("blocked", [False, True])
def test_an_error_throttle_keeps_its_stored_status_on_every_page(blocked, oracle_mod):
    snaps, p, cands = _error_throttle_wide(blocked)
    assert len(snaps) == 2
    want = held_to_the_reference(snaps, oracle_mod, p, cands)
    assert want[0] == ((NONE if blocked else 0), [0])


def test_a_long_list_and_the_hbm_workspace(oracle_mod):
    """70 affecting throttles with binding names on both pages: the list takes more than one entry per lane; with
    KT_REPRIEVE_LDS_CAP=16 (read when the engine is created and on kt_debug_reload_env) it lives in page 0's workspace."""
    snaps, pre, cands = PPR.long_list()
    want = [paging.paged_preempt_of(snaps, p, cands, NOW, reprieve=True) for p in pre]
    assert all(k > 1 and sum(v) < k for k, v in want)
    assert PPR.reference(snaps, oracle_mod, pre[0], cands) == want[0]
    engs = _engines(snaps)
    try:
        in_lds = _both(engs, pre, cands)
    finally:
        _close(engs)
    assert "KT_REPRIEVE_LDS_CAP" not in os.environ
    os.environ["KT_REPRIEVE_LDS_CAP"] = "16"
    try:
        engs = _engines(snaps)
    finally:
        del os.environ["KT_REPRIEVE_LDS_CAP"]
    try:
        in_hbm = _both(engs, pre, cands)
        again = _both(engs, pre[::-1], cands)  # the workspace is reused
        engs[0].reload_env()  # the switch is gone: back in LDS
        back = _both(engs, pre, cands)
    finally:
        _close(engs)
    for a, b, c, d in zip(in_lds, in_hbm, back, again):
        assert a.tobytes() == b.tobytes() == c.tobytes() == d[::-1].tobytes()
    assert [(int(k), v.tolist()) for k, v in zip(in_lds[0], in_lds[2])] == want


@pytest.mark.parametrize("seed", range(4))
def test_one_page_is_the_single_engine_launch(seed):
    snap = PR.preempt_cluster(seed).build_pages()[0].snapshot
    cases = PR.preempt_cases(seed, snap)
    eng = E.Engine.for_snapshot(snap)
    try:
        for p, cands in cases:
            for on_equal in (False, True):
                for reprieve in (False, True):
                    one = eng.preempt([p], cands, NOW, on_equal, reprieve=reprieve)
                    paged = E.paged_preempt([eng], [p], cands, NOW, on_equal, reprieve=reprieve)
                    assert [a.tobytes() for a in one] == [a.tobytes() for a in paged], f"seed {seed} pod {p} {on_equal} {reprieve}"
        cands = cases[-1][1]
        pre = [q for q in range(snap.n_pods) if q not in cands]
        for reprieve in (False, True):
            one = eng.preempt(pre, cands, NOW, reprieve=reprieve)
            paged = E.paged_preempt([eng], pre, cands, NOW, reprieve=reprieve)
            assert [a.tobytes() for a in one] == [a.tobytes() for a in paged]
    finally:
        eng.close()
    for make in (lambda: RR.wide(65, 40, D=3, n_pre=3), lambda: RR.big_last(70, T=1030, row=1029, D=5, dim=4)):
        snap, pre, cands = make()
        pre = pre if isinstance(pre, list) else [pre]
        eng = E.Engine.for_snapshot(snap)
        try:
            for reprieve in (False, True):
                assert [a.tobytes() for a in eng.preempt(pre, cands, NOW, reprieve=reprieve)] == \
                    [a.tobytes() for a in E.paged_preempt([eng], pre, cands, NOW, reprieve=reprieve)]
        finally:
            eng.close()


def test_more_preemptors_than_workgroups():
    """2500 preemptors over 2048 one-wave workgroups: 452 of them take a second turn."""
    n = 2500
    snaps, pre, cands = PPR.long_list(L=6, m=40, n_pre=4)
    rows = [(i + (i >= 2048)) % 4 for i in range(n)]
    want = [paging.paged_preempt_of(snaps, p, cands, NOW, reprieve=True) for p in range(4)]
    engs = _engines(snaps)
    try:
        prefix, victims = E.paged_preempt(engs, rows, cands, NOW, reprieve=True)
        only_prefix = E.paged_preempt(engs, rows, cands, NOW, want_victims=False)
    finally:
        _close(engs)
    assert only_prefix[1] is None and only_prefix[0].tolist() == prefix.tolist()
    for i in (0, 1, 2, 3, 2047, 2048, 2049, 2499):
        assert (int(prefix[i]), victims[i].tolist()) == want[rows[i]], i
    for r in range(4):
        sel = np.array(rows) == r
        assert (prefix[sel] == want[r][0]).all() and (victims[sel] == np.array(want[r][1], np.uint8)).all()


def test_validation():
    snaps, p, cands = PPR.reprieve_across_pages()
    other_rows = PR.tiny([{0: 1}] * 6, {0: 10}, T=3, row=2, D=1)
    engs = _engines(snaps)
    other = E.Engine.for_snapshot(other_rows)
    inc = E.Engine.for_snapshot(snaps[1], kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    call = lambda es, a, b, **kw: E.paged_preempt(es, a, b, NOW, **kw)
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    one = np.array([0], np.int64)
    try:
        # the page set
        assert _code(lambda: call([engs[0], other], [0], cands)) == -1  # different throttle-row counts
        assert _code(lambda: call([engs[0], engs[0]], [0], cands)) == -1  # an engine named twice
        assert L.kt_paged_preempt(None, 2, 0, None, 0, None, 0, 0, 0, 0, None, None) == -1
        assert L.kt_paged_preempt(hs, 0, 0, None, 0, None, 0, 0, 0, 0, None, None) == -1
        import torch
        # pages on different devices: needs a second GPU, so this case does NOT run on a one-GPU machine (the CI box is one) and the
        # refusal — paged_same_cluster's, shared with kt_paged_admit — stays unexercised there
        if torch.cuda.device_count() >= 2:
            far = E.Engine.for_snapshot(snaps[1], device=1)
            try:
                assert _code(lambda: call([engs[0], far], [0], cands)) == -7
            finally:
                far.close()
        # the arguments
        assert _code(lambda: call(engs, [0], [2, 3, 0])) == -1  # a preemptor that is a candidate
        assert _code(lambda: call(engs, [0], [2, 3, 2])) == -1  # a candidate named twice
        assert _code(lambda: call(engs, [0], [2, 99])) == -2  # a row no page holds
        assert L.kt_paged_preempt(hs, 2, 1, one.ctypes.data, -1, None, 0, 0, 0, 0, None, None) == -1  # n_cand < 0
        assert L.kt_paged_preempt(hs, 2, 1, None, 0, None, 0, 0, 0, 0, None, None) == -1  # a missing row array
        assert L.kt_paged_preempt(hs, 2, -1, None, 0, None, 0, 0, 0, 0, None, None) == -1
        assert L.kt_paged_preempt(hs, 2, 1, one.ctypes.data, 0, None, 0, 0, 0, 0x2, None, None) == -1  # an unknown flag
        # an engine, asked of every page
        assert _code(lambda: call([engs[0], inc], [0], cands)) == -7  # KT_VARIANT_INCREMENTAL
        engs[1].set_exchange_world(2)
        assert _code(lambda: call(engs, [0], cands)) == -7
        engs[1].set_exchange_world(1)
        # n == 0 launches nothing; n_cand == 0 answers 0 or KT_PREEMPT_NONE
        prefix, victims = call(engs, [], cands)
        assert prefix.shape == (0,) and victims.shape == (0, len(cands))
        prefix, victims = call(engs, [0, 1], [], reprieve=True)
        assert prefix.tolist() == [paging.paged_preempt_of(snaps, q, [], NOW)[0] for q in (0, 1)] and NONE in prefix.tolist() and victims.shape == (2, 0)
        prefix, victims = call(engs, [0], cands, reprieve=True)
        assert (prefix.tolist(), victims.tolist()) == ([2], [[1, 1, 0, 0]])
    finally:
        _close(engs + [other, inc])
    # (n + n_cand) x throttle_rows beyond 2^31 bytes of matrix: refused on the host, nothing is allocated
    wide = [RR.big_last(6, T=1030, row=1029)[0], RR.big_last(6, T=1030, row=1029)[0]]
    engs = _engines(wide)
    try:
        many = np.zeros(2**31 // 1030 + 1, np.int64)
        assert _code(lambda: call(engs, many, [1, 2])) == -2
        assert _code(lambda: call(engs, many[:-1], [1, 2, 3, 4, 5])) == -2  # (only the sum of the two)
    finally:
        _close(engs)


def test_a_refused_call_leaves_every_slot_alone():
    snaps, p, cands = PPR.reprieve_across_pages()
    engs = _engines(snaps)
    n = snaps[0].n_pods
    try:
        want_check = engs[0].check(rows=np.arange(n), on_equal=False)
        want_rec = engs[1].reconcile(NOW, apply=False)
        want_pre = [a.copy() for a in engs[0].preempt([p], cands, NOW)]
        def refused():
            assert _code(lambda: E.paged_preempt(engs, [0], [2, 3, 2], NOW)) == -1
            # `used` of page 1 wider than int64: found out by that page's sums kernel, the one thing that runs before the refusal
            engs[1].set_wide_sums(1)
            assert _code(lambda: E.paged_preempt(engs, [0], cands, NOW, reprieve=True)) == -7
            engs[1].set_wide_sums(0)

        engs[0].check_launch(n, want_status=True)
        engs[1].reconcile_launch(NOW, apply=False)
        refused()
        got = engs[1].reconcile_fetch()
        assert got.used.v.tobytes() == want_rec.used.v.tobytes() and got.calc_updated.tobytes() == want_rec.calc_updated.tobytes()
        status, summary = engs[0].check_fetch(n, True)
        assert status.tobytes() == want_check[0].tobytes() and summary.tobytes() == want_check[1].tobytes()
        engs[0].preempt_launch([p], cands, NOW)  # (takes page 0's check slot: the two cannot be pending together)
        refused()
        assert [a.tobytes() for a in engs[0].preempt_fetch(1, len(cands))] == [a.tobytes() for a in want_pre]
    finally:
        _close(engs)


def test_slots_after_a_successful_call():
    snaps, p, cands = PPR.reprieve_across_pages()
    engs = _engines(snaps)
    n = snaps[0].n_pods
    everyone = np.arange(n, dtype=np.int64)
    instants = [NOW, (NOW[0] + 60, 0)]
    try:
        reserved = [e.fetch_reserved() for e in engs]
        checked = [E.paged_check(engs, n, on_equal=eq)[0].copy() for eq in (False, True)]
        want_forecast = [a.copy() for a in engs[0].forecast([p], instants)]
        plain = [e.reconcile(NOW, apply=False) for e in engs]
        engs[0].forecast_launch([p], instants)
        engs[0].preempt_launch([p], cands, NOW)
        for e in engs:
            e.reconcile_launch(NOW, apply=False)
        engs[1].aggregate_launch()
        prefix, victims = E.paged_preempt(engs, [p], cands, NOW, reprieve=True)
        assert (prefix.tolist(), victims.tolist()) == ([2], [[1, 1, 0, 0]])
        assert [a.tobytes() for a in engs[0].forecast_fetch(1, len(instants))] == [a.tobytes() for a in want_forecast]
        assert _code(lambda: engs[0].preempt_fetch(1, len(cands))) == -5  # handed out by the call: nothing is pending
        for e in engs:
            assert _code(e.reconcile_fetch) == -5  # every page's reconcile report is dropped
        engs[1].finalize_launch(NOW, apply=False)  # page 1's pending aggregate kept its sums
        got = engs[1].reconcile_fetch()
        assert got.used.v.tobytes() == plain[1].used.v.tobytes() and got.used.present.tobytes() == plain[1].used.present.tobytes()
        # a dry run: reserved amounts and the stored status of every page are unchanged
        for e, before in zip(engs, reserved):
            after = e.fetch_reserved()
            for f in ("v", "present", "count", "has_count"):
                assert getattr(after, f).tobytes() == getattr(before, f).tobytes()
        assert all(np.array_equal(a, E.paged_check(engs, n, on_equal=eq)[0]) for a, eq in zip(checked, (False, True)))
    finally:
        _close(engs)
