"""Gang admission on the device (kt_admit_gangs_launch / kt_paged_admit_gangs, the kt_admit_gangs kernels): held to
``model_admit_gangs`` of tests/test_gang_admit_cpu.py on its cases (one page through Engine.admit_gangs, >= 3 pages through
PagedEngine.admit_gangs, state in LDS and in HBM), directed cases for the presence rollback and for the shapes where the walk
takes another path, identity with plain admission, validation, and the C++ plugin mirror's AdmitGangs."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from kube_throttler_amd.objects import ClusterState
from test_gang_admit_cpu import GANG_CASES, gang_case, model_admit_gangs
from test_paged_admit_cpu import VERDICT_NAME, reserved_totals, row_of, write_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")


def _verdicts(summary):
    return np.where(summary == 2, S.VERDICT_ERROR, np.where((summary & 1) != 0, S.VERDICT_BLOCK, S.VERDICT_ALLOW)).astype(np.uint8)


def _admit_gangs(eng, queue, off, on_equal, commit):
    """One page: Engine.admit_gangs (kt_admit_gangs_launch + the two fetches); more: PagedEngine.admit_gangs."""
    if len(eng.engines) == 1:
        status, summary, admitted = eng.engines[0].admit_gangs(np.array(queue, np.int64), off, on_equal=on_equal, commit=commit)
        return status, _verdicts(summary), admitted
    return eng.admit_gangs(np.array(queue, np.int64), off, on_equal=on_equal, commit=commit)


def _hold_to_model(cs, queue, off, on_equal, label, min_pages=1):
    """Dry run, then commit: per-pod status row and verdict, the gang byte, and every throttle's reserved amount on every page
    (absent names and an absent count included) against the reference; after the dry run the reserved amounts are unchanged."""
    pages = cs.build_pages()
    assert len(pages) >= min_pages
    names = pages[0].thr_names
    after = copy.deepcopy(cs)
    want, want_admitted = model_admit_gangs(after, queue, off, on_equal)
    eng = paging.PagedEngine(pages)
    try:
        before = reserved_totals(cs)
        for commit in (False, True):
            status, verdict, admitted = _admit_gangs(eng, queue, off, on_equal, commit)
            for k, (v, st) in enumerate(want):
                where = f"{label} on_equal={on_equal} commit={commit} pos {k} pod{queue[k]}"
                assert VERDICT_NAME[int(verdict[k])] == v, where
                if v != "error":
                    assert row_of(status[k], names) == st, where
            assert [bool(x) for x in admitted] == want_admitted, f"{label} on_equal={on_equal} commit={commit}"
            totals = reserved_totals(after) if commit else before
            got = eng.fetch_reserved()
            for t, nn in enumerate(names):
                assert got[t] == totals.get(nn, {}), f"{label} commit={commit}: reserved of {nn}"
        return want, want_admitted
    finally:
        eng.close()


@pytest.mark.parametrize("on_equal", [False, True])
@pytest.mark.parametrize("seed,wide", GANG_CASES)
def test_gangs_equal_the_manifest_model(seed, wide, on_equal, oracle_mod):
    cs, queue, off = gang_case(seed, wide, oracle_mod)
    _hold_to_model(cs, queue, off, on_equal, f"seed {seed} wide={wide}", min_pages=3 if wide else 1)


def test_gangs_equal_the_manifest_model_with_hbm_state():
    """The same cases with the state in the HBM scratch buffer (kt_admit_gangs<DT, false>): the hook is read once per process,
    so they run in a child."""
    env = dict(os.environ, KT_ADMIT_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__, "-k",
                        "(test_gangs_equal_the_manifest_model and not hbm) or test_presence or test_shapes"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- directed cases --------------------------------------------------------------------------------------------------------
def _pod(name, requests, ns="ns0", labels=None):
    return {"kind": "Pod", "metadata": {"name": name, "namespace": ns, "labels": dict(labels or {"app": "job"})},
            "spec": {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": dict(requests)}}]},
            "status": {"phase": "Pending"}}


def _throttle(name, threshold, app="job"):
    return {"kind": "Throttle", "metadata": {"name": name, "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": app}}}]},
                     "threshold": threshold}}


def _cluster(pods, n_match=1, n_other=0, extra_names=0):
    """n_other throttles that select nothing in the queue, then n_match that select the job pods (2 pods, 1 cpu each);
    extra_names more resource names in the first one's threshold (the engine's D)."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    for p in pods:
        cs.add(p)
    for i in range(n_other):  # first: the job's throttles get the highest rows
        cs.add(_throttle(f"u{i:04d}", {"resourceCounts": {"pod": 1}}, app="other"))
    for i in range(n_match):
        rr = {"cpu": "1"}
        if i == 0:
            rr.update({f"example.com/r{k:02d}": "100" for k in range(extra_names)})
        cs.add(_throttle(f"t{i:04d}", {"resourceCounts": {"pod": 2}, "resourceRequests": rr}))
    return cs


def _abcd():
    # A: cpu only; B: cpu + memory; C: blocked by the count of 2; D: 700m, fits only when A and B are gone
    return [_pod("A", {"cpu": "400m"}), _pod("B", {"cpu": "400m", "memory": "64Mi"}), _pod("C", {"cpu": "100m"}),
            _pod("D", {"cpu": "700m"})]


def test_presence_goes_back_with_the_gang(oracle_mod):
    """[A, B, C] on an empty reserved table: A and B reserve (B brings `memory` in, both the count), C is blocked by the count:
    after the commit the throttle's reserved amount reads back with no names and no count."""
    cs = _cluster(_abcd()[:3])
    write_status(cs, oracle_mod)
    want, admitted = _hold_to_model(cs, [0, 1, 2], [0, 3], False, "presence")
    assert [v for v, _ in want] == ["allow", "allow", "block"] and admitted == [False]
    pages = cs.build_pages()
    eng = E.Engine.for_snapshot(pages[0].snapshot)
    try:
        _, _, adm = eng.admit_gangs(np.arange(3), [0, 3], commit=True)
        assert list(adm) == [0]
        r = eng.fetch_reserved()
        assert not r.present[:1].any() and not r.has_count[:1].any()
        assert pages[0].amount_to_dict(r, 0) == {}
    finally:
        eng.close()


def test_presence_subtraction_is_undone_not_added_again(oracle_mod):
    """The single-pod gang D behind [A, B, C] fits only if A's and B's amounts are gone."""
    cs = _cluster(_abcd())
    write_status(cs, oracle_mod)
    want, admitted = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], False, "undo")
    assert [v for v, _ in want] == ["allow", "allow", "block", "allow"] and admitted == [False, True]


@pytest.mark.parametrize("n_match,n_other,extra_names", [(17, 0, 0), (5, 0, 14), (17, 1023, 0)],
                         ids=["17-throttles-D4", "5-throttles-D16", "1040-throttles"])
def test_shapes_where_the_walk_takes_another_path(n_match, n_other, extra_names, oracle_mod):
    """More affected throttles than one pass of lanes holds (64 / DT: 16 for D <= 4, 4 for D = 16), and T > 1024: the row is
    listed in a second 16-bytes-per-lane chunk, in the rollback too (the job's throttles hold the rows from 1023 on)."""
    cs = _cluster(_abcd(), n_match, n_other, extra_names)
    write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1 and pages[0].snapshot.D == (16 if extra_names else 2)
    if n_other:
        rows = [t for t, nn in enumerate(pages[0].thr_names) if "/t" in nn]
        assert len(pages[0].thr_names) == 1040 and min(rows) == 1023 and max(rows) == 1039
    want, admitted = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], False, "shape")
    assert [v for v, _ in want] == ["allow", "allow", "block", "allow"] and admitted == [False, True]
    assert all(len(st) == n_match for _, st in want)


def test_shapes_error_member_and_failing_ends(oracle_mod):
    """A gang with an Error member (unknown namespace) in the middle, behind an admitted one; a gang whose first and last
    members fail (the first asks for more than the threshold) around two that reserve; D is admitted behind both."""
    a, b, c, d = _abcd()
    ghost = _pod("G", {"cpu": "100m"}, ns="ghost")
    big = _pod("X", {"cpu": "2"})
    a2, b2 = _pod("A2", {"cpu": "400m"}), _pod("B2", {"cpu": "400m", "memory": "64Mi"})
    cs = _cluster([a, ghost, b, big, a2, b2, c, d])
    write_status(cs, oracle_mod)
    queue, off = list(range(8)), [0, 3, 7, 8]  # [A G B] [X A2 B2 C] [D]
    want, admitted = _hold_to_model(cs, queue, off, False, "ends")
    assert [v for v, _ in want] == ["allow", "error", "allow", "block", "allow", "allow", "block", "allow"]
    assert admitted == [False, False, True]


# ---- identity --------------------------------------------------------------------------------------------------------------
def _workload(n_thr=64, D=8, seed=61, head_room=2):
    from oracle import kt_oracle as O
    from test_paging_cpu import responsible_rows
    snap = W.generate(W.small(seed=seed, n_pods=3000, n_thr=n_thr, n_cluster=n_thr // 2, D=D))
    T = snap.n_thr
    snap.thr_spec.v[:T] = snap.thr_spec.v[:T] * head_room + 1
    snap.thr_spec.count[:T] = snap.thr_spec.count[:T] * head_room + 3
    snap.thr_ovr_off[:] = 0
    rows = responsible_rows(snap)
    want = O.Oracle(snap).reconcile((1767225600, 0), rows=rows)
    snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    return snap, np.random.default_rng(seed).permutation(pending)[:600].astype(np.int64)


def _same_reserved(a, b):
    for f in ("v", "present", "count", "has_count"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


def test_gangs_of_one_pod_are_plain_admission():
    snap, queue = _workload()
    plain, gang, paged = (E.Engine.for_snapshot(snap) for _ in range(3))
    try:
        ones = np.arange(len(queue) + 1)
        for commit in (False, True):
            st1, sm1 = plain.admit(queue, commit=commit)
            st2, sm2, adm = gang.admit_gangs(queue, ones, commit=commit)
            np.testing.assert_array_equal(st2, st1)
            np.testing.assert_array_equal(sm2, sm1)
            np.testing.assert_array_equal(adm, (sm1 == 0).astype(np.uint8))
        assert adm.any() and not adm.all()
        _same_reserved(gang.fetch_reserved(), plain.fetch_reserved())
        # one page of kt_paged_admit_gangs is kt_admit_gangs_launch: gangs of 1..7 pods
        cut = np.unique(np.concatenate([[0, len(queue)], np.random.default_rng(7).integers(1, len(queue), len(queue) // 4)]))
        fresh = E.Engine.for_snapshot(snap)
        try:
            for commit in (False, True):
                a = fresh.admit_gangs(queue, cut, commit=commit)
                b = E.paged_admit_gangs([paged], queue, cut, commit=commit)
                for x, y in zip(a, b):
                    np.testing.assert_array_equal(x, y)
            assert a[2].any() and not a[2].all()
            _same_reserved(fresh.fetch_reserved(), paged.fetch_reserved())
        finally:
            fresh.close()
    finally:
        for e in (plain, gang, paged):
            e.close()


# ---- validation ------------------------------------------------------------------------------------------------------------
def test_refused_offsets_leave_the_reserved_amounts_alone():
    snap, queue = _workload()
    queue = queue[:10]
    eng = E.Engine.for_snapshot(snap)
    try:
        before = eng.fetch_reserved()
        with pytest.raises(E.EngineError) as ex:
            eng.admit_gangs_fetch(1)
        assert ex.value.code == -5  # KT_ERR_NOT_READY: no gang launch yet
        for off in ([1, 10], [0, 4, 9], [0, 4, 4, 10], [0, 6, 4, 10], [0, 4, 12]):
            with pytest.raises(E.EngineError) as ex:
                eng.admit_gangs(queue, off, commit=True)
            assert ex.value.code == -1, off  # KT_ERR_INVALID_ARGUMENT
            with pytest.raises(E.EngineError) as ex:
                E.paged_admit_gangs([eng], queue, off, commit=True)
            assert ex.value.code == -1, off
        with pytest.raises(E.EngineError) as ex:
            eng.admit_gangs(queue, [0], commit=True)  # no gangs for a queue that is not empty
        assert ex.value.code == -1
        with pytest.raises(E.EngineError) as ex:
            eng.admit_gangs_fetch(1)  # a refused launch leaves nothing to fetch
        assert ex.value.code == -5
        _same_reserved(eng.fetch_reserved(), before)
        status, summary, adm = eng.admit_gangs(queue[:0], [0])  # the empty queue
        assert summary.shape == (0,) and adm.shape == (0,)
        status, summary, adm = eng.admit_gangs(queue, [0, 4, 10])
        assert adm.shape == (2,)
        eng.admit(queue)  # a plain launch drops the pending gang result
        with pytest.raises(E.EngineError) as ex:
            eng.admit_gangs_fetch(2)
        assert ex.value.code == -5
    finally:
        eng.close()


def test_the_empty_gang_is_named():
    snap, queue = _workload()
    eng = E.Engine.for_snapshot(snap)
    try:
        with pytest.raises(E.EngineError) as ex:
            eng.admit_gangs(queue[:10], [0, 4, 4, 10])
        assert ex.value.code == -1 and "gang 1 is empty" in str(ex.value)
    finally:
        eng.close()


def test_a_page_with_wide_sums_is_refused():
    """As kt_admit_launch and kt_paged_admit (tests/test_paged_admit_gpu.py): a stored `used` beyond int64 is not admitted."""
    snap = W.generate(W.small(seed=45, n_pods=64, n_thr=6, n_cluster=3, D=3))
    first = snap.pod_ctr_off[:snap.n_pods]
    nc = int(snap.pod_ctr_off[snap.n_pods])
    snap.ctr_req[:nc, 0] = 0
    snap.ctr_req[first, 0] = 1 << 59
    snap.ctr_present[first] |= 1
    wide = E.Engine.for_snapshot(snap)
    plain = E.Engine.for_snapshot(W.generate(W.small(seed=46, n_pods=64, n_thr=6, n_cluster=3, D=3)))
    try:
        wide.reconcile((1767225600, 0), apply=True)
        with pytest.raises(E.EngineError) as one:
            wide.admit(np.arange(8))
        with pytest.raises(E.EngineError) as gang:
            wide.admit_gangs(np.arange(8), [0, 3, 8])
        with pytest.raises(E.EngineError) as ex:
            E.paged_admit_gangs([plain, wide], np.arange(8), [0, 3, 8])
        assert ex.value.code == gang.value.code == one.value.code == -7
    finally:
        wide.close()
        plain.close()


# ---- the C++ plugin mirror ---------------------------------------------------------------------------------------------------
def test_host_plugin_gangs():
    """KubeThrottler::AdmitGangs against PreFilter / Reserve / Unreserve on a twin (tests/cpp/host_plugin_gang_test.cpp)."""
    exe = os.path.join(HOST, "host_plugin_gang_test")
    subprocess.check_call(["make", "-C", HOST, "host_plugin_gang_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
