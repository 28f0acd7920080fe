"""kt_paged_admit on the device: admission queues over more than 16 resource names (kube_throttler_amd.paging.PagedEngine.admit),
held to the manifest-level reference of tests/test_paged_admit_cpu.py, to kt_admit_launch on one page, and with the state
of all pages beyond LDS."""
import copy

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from manifest_model import Model
from oracle import kt_oracle as O
from test_paged_admit_cpu import PAGED_SEEDS, VERDICT_NAME, admission_case, model_admit, reserved_totals, row_of
from test_paging_cpu import responsible_rows

pytestmark = pytest.mark.gpu
NOW = (1767225600, 0)


@pytest.mark.parametrize("on_equal", [False, True])
@pytest.mark.parametrize("seed", PAGED_SEEDS)
def test_paged_admit_equals_the_manifest_model(seed, on_equal, oracle_mod):
    cs, queue = admission_case(seed, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) >= 3
    names = pages[0].thr_names
    after = copy.deepcopy(cs)
    want = model_admit(after, queue, on_equal)
    eng = paging.PagedEngine(pages)
    try:
        for commit in (False, True):  # the dry run leaves the reserved amounts as they were: the same answers twice
            status, verdict = eng.admit(np.array(queue, np.int64), on_equal=on_equal, commit=commit)
            for k, (v, st) in enumerate(want):
                where = f"seed {seed} commit={commit} pos {k} pod{queue[k]}"
                assert VERDICT_NAME[int(verdict[k])] == v, where
                assert row_of(status[k], names) == st, where
        totals = reserved_totals(after)
        got = eng.fetch_reserved()
        for t, nn in enumerate(names):
            assert got[t] == totals.get(nn, {}), f"seed {seed}: reserved of {nn}"
        # a following check sees the committed reservations
        status, verdict = eng.check(on_equal=on_equal)
        model = Model(after)
        for i, p in enumerate(after.pods):
            v, st = model.check(p, on_equal)
            assert VERDICT_NAME[int(verdict[i])] == v, f"seed {seed} pod{i} after commit"
            if v != "error":
                assert row_of(status[i], names) == st, f"seed {seed} pod{i} after commit"
    finally:
        eng.close()


def test_paged_admit_equals_the_manifest_model_with_hbm_state():
    """The same distinct pages with every page's state in the HBM scratch buffer (kt_admit<DT, false>): the hook is
    read once per process, so the cases run in a child."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, KT_ADMIT_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__, "-k",
                        "test_paged_admit_equals_the_manifest_model and not hbm"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _workload(n_thr, D=8, seed=61, head_room=2):
    snap = W.generate(W.small(seed=seed, n_pods=3000, n_thr=n_thr, n_cluster=n_thr // 2, D=D))
    T = snap.n_thr
    # head-room: the queue fills the throttles up on the way (the more throttles affect a pod, the more it needs)
    snap.thr_spec.v[:T] = snap.thr_spec.v[:T] * head_room + 1
    snap.thr_spec.count[:T] = snap.thr_spec.count[:T] * head_room + 3
    snap.thr_ovr_off[:] = 0
    rows = responsible_rows(snap)  # the stored status: an oracle reconcile, as UpdateStatus persists it
    want = O.Oracle(snap).reconcile(NOW, rows=rows)
    snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    return snap, np.random.default_rng(seed).permutation(pending)[:1200].astype(np.int64)


def _identical_pages(n_thr, n_pages, D=8, head_room=2):
    """One snapshot loaded into n_pages engines: combining identical pages is the identity, so kt_paged_admit must answer
    exactly what kt_admit_launch answers on one of them."""
    snap, queue = _workload(n_thr, D, head_room=head_room)
    one = E.Engine.for_snapshot(snap)
    pages = [E.Engine.for_snapshot(snap) for _ in range(n_pages)]
    try:
        for commit in (False, True):
            st1, sm1 = one.admit(queue, commit=commit)
            stp, smp = E.paged_admit(pages, queue, commit=commit)
            np.testing.assert_array_equal(stp, st1)
            np.testing.assert_array_equal(smp, sm1)
        verdict = S.summary_fields(sm1)[0]
        assert (verdict == S.VERDICT_ALLOW).any() and (verdict == S.VERDICT_BLOCK).any()
        r1 = one.fetch_reserved()
        for e in pages:
            rp = e.fetch_reserved()
            for f in ("v", "present", "count", "has_count"):
                np.testing.assert_array_equal(getattr(rp, f), getattr(r1, f), err_msg=f)
    finally:
        for e in [one] + pages:
            e.close()


def test_one_page_is_kt_admit_launch():
    _identical_pages(64, 1)


def test_two_launches_back_to_back_then_one_fetch():
    """kt_admit_launch is asynchronous and reads its page descriptor from device memory, copied there from engine-owned host
    storage: a second launch that follows without a fetch must neither disturb the first one's copy nor be disturbed by it.  The
    one fetch returns the SECOND queue's result, equal to what a fresh engine gives for that queue."""
    snap, queue = _workload(64)
    first, second = queue[:700], queue[500:][::-1].copy()  # different queues, overlapping, different lengths
    eng, fresh = E.Engine.for_snapshot(snap), E.Engine.for_snapshot(snap)
    try:
        for q in (first, second):  # dry runs: the reserved amounts stay as loaded
            eng._ck(E.lib().kt_admit_launch(eng._h, len(q), q.ctypes.data, 0, 0, None))
        status, summary = eng.check_fetch(len(second), want_status=True)
        want_status, want_summary = fresh.admit(second, commit=False)
        np.testing.assert_array_equal(summary, want_summary)
        np.testing.assert_array_equal(status, want_status)
        verdict = S.summary_fields(summary)[0]
        assert (verdict == S.VERDICT_ALLOW).any() and (verdict == S.VERDICT_BLOCK).any()
    finally:
        eng.close()
        fresh.close()


def test_state_beyond_lds_lives_in_hbm():
    # 4 pages x 800 throttle rows x (8 x 8 + 16) bytes = 256 KB of state > 160 KiB of LDS; one page alone fits
    _identical_pages(800, 4, head_room=10)


def test_refusals_and_the_empty_queue():
    a = E.Engine.for_snapshot(W.generate(W.small(seed=3, n_pods=200, n_thr=16, n_cluster=8)))
    b = E.Engine.for_snapshot(W.generate(W.small(seed=4, n_pods=200, n_thr=24, n_cluster=8)))
    try:
        with pytest.raises(E.EngineError) as ex:
            E.paged_admit([a, b], np.arange(10))
        assert ex.value.code == -1  # different throttle-row counts
        with pytest.raises(E.EngineError) as ex:
            E.paged_admit([a, a], np.arange(10))
        assert ex.value.code == -1  # the same engine twice
        status, summary = E.paged_admit([a], np.arange(0))
        assert status.shape[0] == 0 and summary.shape == (0,)
    finally:
        a.close()
        b.close()


def test_a_page_with_wide_sums_is_refused():
    """As kt_admit_launch: a stored `used` beyond int64 (tests/test_engine_gpu.py::test_wide_sums) is not admitted."""
    snap = W.generate(W.small(seed=45, n_pods=64, n_thr=6, n_cluster=3, D=3))
    first = snap.pod_ctr_off[:snap.n_pods]
    nc = int(snap.pod_ctr_off[snap.n_pods])
    snap.ctr_req[:nc, 0] = 0
    snap.ctr_req[first, 0] = 1 << 59
    snap.ctr_present[first] |= 1
    wide = E.Engine.for_snapshot(snap)
    plain = E.Engine.for_snapshot(W.generate(W.small(seed=46, n_pods=64, n_thr=6, n_cluster=3, D=3)))
    try:
        wide.reconcile(NOW, apply=True)
        with pytest.raises(E.EngineError) as one:
            wide.admit(np.arange(8))
        with pytest.raises(E.EngineError) as ex:
            E.paged_admit([plain, wide], np.arange(8))
        assert ex.value.code == one.value.code == -7
    finally:
        wide.close()
        plain.close()
