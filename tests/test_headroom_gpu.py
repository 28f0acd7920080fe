"""Headroom on the device (kt_headroom_launch / kt_paged_headroom, the kt_headroom kernels): held to the admission walk of
tests/test_headroom_cpu.py on its cases (one page through Engine.headroom, >= 3 pages through PagedEngine.headroom), to the
engine's own dry-run admission of ``[pod] * cap``, to the C oracle's repeated-row admit where the grid strides, the matrix row
has a second chunk and at every DT bucket, to the manifest model on directed cases, plus refusals, the rules of the check slot,
and the C++ plugin mirror's Headroom."""
import copy
import os
import subprocess

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from kube_throttler_amd.objects import ClusterState
from oracle import kt_oracle as O
from test_headroom_cpu import CAP, HEADROOM_CASES, headroom_by_walk, headroom_case
from test_paged_admit_cpu import write_status
from test_paged_admit_gpu import _workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")


def _headroom(pages, rows, cap, on_equal):
    """One page: Engine.headroom (kt_headroom_launch + kt_headroom_fetch); more: PagedEngine.headroom (kt_paged_headroom)."""
    eng = paging.PagedEngine(pages)
    try:
        rows = np.asarray(rows, np.int64)
        if len(pages) == 1:
            return eng.engines[0].headroom(rows, cap=cap, on_equal=on_equal)
        return eng.headroom(rows, cap, on_equal=on_equal)
    finally:
        eng.close()


@pytest.mark.parametrize("on_equal", [False, True])
@pytest.mark.parametrize("seed,wide", HEADROOM_CASES)
def test_headroom_equals_the_admission_walk(seed, wide, on_equal, oracle_mod):
    """Every pod of the cluster: the queue pods and the pods PreFilter answers with an error."""
    cs, pages, queue, want = headroom_case(seed, wide, oracle_mod)
    assert (len(pages) >= 3) if wide else (len(pages) == 1)
    n = len(cs.pods)
    copies, limiting = _headroom(pages, np.arange(n), CAP, on_equal)
    assert copies.dtype == np.int64 and limiting.dtype == np.int32
    for i in range(n):
        assert (int(copies[i]), int(limiting[i])) == want[on_equal][i][:2], f"seed {seed} wide={wide} on_equal={on_equal} pod{i}"


# ---- the engine against itself, and against the oracle's repeated-row admit ------------------------------------------------
def _leading_success(summary):
    bad = np.nonzero(summary != 0)[0]
    return int(bad[0]) if len(bad) else len(summary)


def _oracle_headroom(o, p, cap, on_equal=False):
    """(copies, limiting) by the C oracle's admit of [p] * cap (it adds the pod's amount once per queue position)."""
    status, summary, _ = o.admit(rows=np.full(cap, p, np.int64), on_equal=on_equal)
    k = _leading_success(summary)
    if k == cap or summary[k] == 2:
        return k, -1
    return k, int(np.nonzero((status[k] != S.NOT_AFFECTED) & (status[k] != S.NOT_THROTTLED))[0][0])


def test_headroom_is_the_dry_run_admission_of_repeated_rows():
    snap, queue = _workload(64)
    eng = E.Engine.for_snapshot(snap)
    try:
        pods = queue[:50]
        before = eng.fetch_reserved()
        copies, limiting = eng.headroom(pods, cap=16)
        after = eng.fetch_reserved()
        for f in ("v", "present", "count", "has_count"):
            np.testing.assert_array_equal(getattr(after, f), getattr(before, f), err_msg=f)
        for k, p in enumerate(pods):
            status, summary = eng.admit(np.full(16, p, np.int64), commit=False)
            c = _leading_success(summary)
            assert int(copies[k]) == c, f"pod {p}"
            lim = -1 if c == 16 else int(np.nonzero((status[c] != S.NOT_AFFECTED) & (status[c] != S.NOT_THROTTLED))[0][0])
            assert int(limiting[k]) == lim, f"pod {p}"
        assert (copies == 0).any() and ((copies > 0) & (copies < 16)).any()
    finally:
        eng.close()


@pytest.mark.parametrize("n_thr,D", [(64, 3), (64, 8), (64, 16), (1100, 8)], ids=["D3", "D8", "D16", "1100-throttles"])
def test_grid_stride_chunk_boundary_and_dt_buckets(n_thr, D):
    """Every pod row of the workload in one launch — 3000 pods, more than the grid has waves — against the oracle on a sample
    of 200; D = 3, 8 and 16 reach the three DT buckets; 1100 throttle rows put a second 1024-byte chunk in the matrix row."""
    snap, queue = _workload(n_thr, D=D, head_room=10 if n_thr > 1024 else 2)
    assert snap.n_pods == 3000 and snap.D == D
    o = O.Oracle(snap)
    sample = np.random.default_rng(5).permutation(queue)[:200]
    if n_thr > 1024:  # pods affected by throttles on both sides of the chunk boundary come first
        assert snap.n_thr >= n_thr
        st, _ = o.check(rows=queue)
        both = queue[(st[:, :1024] != 0).any(axis=1) & (st[:, 1024:] != 0).any(axis=1)]
        assert len(both) >= 10
        sample = np.concatenate([both[:60], sample[:140]])
    eng = E.Engine.for_snapshot(snap)
    try:
        copies, limiting = eng.headroom(n=snap.n_pods, cap=16)
        got = [(int(copies[p]), int(limiting[p])) for p in sample]
        want = [_oracle_headroom(o, int(p), 16) for p in sample]
        assert got == want
        assert len({c for c, _ in want}) >= 3  # zero, the cap and something between
        if n_thr > 1024:
            assert any(t >= 0 for _, t in want[:60])  # some of the pods on both sides are stopped by a throttle
        some = sample[:40]  # listed rows in another order give the same answers
        c2, l2 = eng.headroom(some[::-1].copy(), cap=16, on_equal=True)
        assert [(int(a), int(b)) for a, b in zip(c2[::-1], l2[::-1])] == [_oracle_headroom(o, int(p), 16, True) for p in some]
    finally:
        eng.close()


# ---- directed cases --------------------------------------------------------------------------------------------------------
def _pod(name, requests, ns="ns0", app="job", node=None):
    p = {"kind": "Pod", "metadata": {"name": name, "namespace": ns, "labels": {"app": app}},
         "spec": {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": dict(requests)}}]},
         "status": {"phase": "Running" if node else "Pending"}}
    if node:
        p["spec"]["nodeName"] = node
    return p


def _throttle(kind, threshold, overrides=None):
    sel = {"podSelector": {"matchLabels": {"app": "job"}}}
    md = {"name": "t0"}
    if kind == "Throttle":
        md["namespace"] = "ns0"
    else:
        sel["namespaceSelector"] = {"matchLabels": {"kubernetes.io/metadata.name": "ns0"}}
    spec = {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [sel]}, "threshold": threshold}
    if overrides:
        spec["temporaryThresholdOverrides"] = overrides
    return {"kind": kind, "metadata": md, "spec": spec}


def _cluster(kind, threshold, pods, overrides=None, reserved=None):
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    for p in pods:
        cs.add(p)
    cs.add(_throttle(kind, threshold, overrides))
    if reserved:
        cs.reserved[(kind, ("ns0" if kind == "Throttle" else "") + "/t0")] = reserved
    return cs


GPU_NAME = "example.com/gpu"
DIRECTED = {
    # used + k x request meets the threshold exactly: step 4 lets the copy through unless on_equal; a Throttle's step 3 then
    # stops the next copy as `active`, a ClusterThrottle's only with on_equal
    "exact": ({"resourceRequests": {"cpu": "1"}}, [_pod("half", {"cpu": "500m"}), _pod("quarter", {"cpu": "250m"}), _pod("third", {"cpu": "300m"})]),
    "exact-with-used": ({"resourceRequests": {"cpu": "2"}}, [_pod("run", {"cpu": "1"}, node="n1"), _pod("half", {"cpu": "500m"}), _pod("one", {"cpu": "1"})]),
    "count-only": ({"resourceCounts": {"pod": 3}}, [_pod("run", {"cpu": "1"}, node="n1"), _pod("a", {"cpu": "100m"}), _pod("b", {})]),
    # copy 0 meets a name that is neither used nor reserved (step 3 does not fire), the copies behind it brought it in
    "name-not-yet-present": ({"resourceRequests": {"cpu": "4", GPU_NAME: "2"}}, [_pod("run", {"cpu": "1"}, node="n1"), _pod("g", {GPU_NAME: "1"}), _pod("g2", {GPU_NAME: "2", "cpu": "1"})]),
    "name-the-threshold-lacks": ({"resourceRequests": {"cpu": "1"}}, [_pod("mem", {"memory": "1Gi"}), _pod("both", {"memory": "1Gi", "cpu": "300m"})]),
    # the running pod fills cpu: status.throttled says cpu; a zero request for cpu is not a request
    "zero-request-and-throttled-name": ({"resourceRequests": {"cpu": "1", "memory": "1Gi"}},
                                        [_pod("run", {"cpu": "1"}, node="n1"), _pod("zero", {"cpu": "0", "memory": "256Mi"}), _pod("cpu", {"cpu": "100m"})]),
    "throttled-pod-flag": ({"resourceCounts": {"pod": 1}}, [_pod("run", {"cpu": "1"}, node="n1"), _pod("a", {"cpu": "100m"})]),
    "request-above-threshold": ({"resourceCounts": {"pod": 5}, "resourceRequests": {"cpu": "1"}}, [_pod("big", {"cpu": "2"}), _pod("fits", {"cpu": "1"})]),
    "count-and-names": ({"resourceCounts": {"pod": 3}, "resourceRequests": {"cpu": "1", "memory": "1Gi"}},
                        [_pod("cpu-first", {"cpu": "500m", "memory": "100Mi"}), _pod("count-first", {"cpu": "100m", "memory": "100Mi"}), _pod("mem-first", {"cpu": "100m", "memory": "600Mi"})]),
}


def _hold_to_walk(cs, oracle_mod, label, cap=CAP, engine_hook=None, model_cs=None):
    """Every pod, both on_equal values: Engine.headroom on the cluster's one page against the walk -> {on_equal: [(copies, limiting)]}."""
    write_status(cs, oracle_mod)
    if model_cs is not None:
        write_status(model_cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1
    ref = model_cs if model_cs is not None else cs
    eng = E.Engine.for_snapshot(pages[0].snapshot)
    out = {}
    try:
        if engine_hook:
            engine_hook(eng)
        n = len(cs.pods)
        for on_equal in (False, True):
            copies, limiting = eng.headroom(np.arange(n), cap=cap, on_equal=on_equal)
            got = [(int(copies[i]), int(limiting[i])) for i in range(n)]
            want = [headroom_by_walk(ref, pages[0].thr_names, i, on_equal, cap)[:2] for i in range(n)]
            print(label, "on_equal", on_equal, "got", got, "want", want)
            assert got == want, f"{label} on_equal={on_equal}"
            out[on_equal] = got
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["Throttle", "ClusterThrottle"])
@pytest.mark.parametrize("case", sorted(DIRECTED))
def test_directed_cases(case, kind, oracle_mod):
    threshold, pods = DIRECTED[case]
    got = _hold_to_walk(_cluster(kind, copy.deepcopy(threshold), copy.deepcopy(pods)), oracle_mod, f"{case} {kind}")
    if case == "exact":  # pods: half, quarter, third
        assert got[False] == [(2, 0), (4, 0), (3, 0)] and got[True] == [(1, 0), (3, 0), (3, 0)]
    if case == "count-only":  # pods: run (scheduled: a further copy is one more pod), a, b
        assert got[False][1:] == [(2, 0), (2, 0)] and got[True][1:] == [(1, 0), (1, 0)]
    if case == "name-the-threshold-lacks":
        assert got[False] == [(CAP, -1), (3, 0)]
    if case == "zero-request-and-throttled-name":
        assert got[False][1:] == [(4, 0), (0, 0)]
    if case == "throttled-pod-flag":
        assert got[False][1] == (0, 0) and got[True][1] == (0, 0)
    if case == "request-above-threshold":
        assert got[False] == [(0, 0), (1, 0)] and got[True] == [(0, 0), (0, 0)]


@pytest.mark.parametrize("kind", ["Throttle", "ClusterThrottle"])
def test_negative_request(kind, oracle_mod):
    """A negative request never grows the sums: it limits at copy 0 or — a Throttle's step 3, which fires on equality whatever
    on_equal says, once copy 0 made the name present — at copy 1; otherwise every copy passes."""
    pods = [_pod("neg", {"cpu": "-1"}), _pod("neg2", {"cpu": "-2"})]
    got = _hold_to_walk(_cluster(kind, {"resourceRequests": {"cpu": "-1"}}, pods), oracle_mod, f"negative {kind}")
    assert got[False][0] == ((1, 0) if kind == "Throttle" else (CAP, -1))
    assert got[True][0] == (0, 0) and got[False][1] == (CAP, -1)


@pytest.mark.parametrize("kind", ["Throttle", "ClusterThrottle"])
def test_an_active_override_is_the_threshold(kind, oracle_mod):
    ovr = [{"begin": "2025-12-01T00:00:00Z", "end": "2026-02-01T00:00:00Z", "threshold": {"resourceRequests": {"cpu": "2"}}}]
    got = _hold_to_walk(_cluster(kind, {"resourceRequests": {"cpu": "1"}}, [_pod("half", {"cpu": "500m"})], overrides=ovr),
                        oracle_mod, f"override {kind}")
    assert got[False] == [(4, 0)] and got[True] == [(3, 0)]


@pytest.mark.parametrize("kind", ["Throttle", "ClusterThrottle"])
def test_reserved_amounts_set_with_kt_set_reserved(kind, oracle_mod):
    threshold = {"resourceCounts": {"pod": 6}, "resourceRequests": {"cpu": "2", "memory": "1Gi"}}
    pods = [_pod("half", {"cpu": "500m"}), _pod("mem", {"memory": "300Mi"}), _pod("both", {"cpu": "100m", "memory": "100Mi"})]
    reserved = {"resourceCounts": {"pod": 2}, "resourceRequests": {"cpu": "700m"}}
    plain = _cluster(kind, threshold, pods)
    with_reserved = _cluster(kind, copy.deepcopy(threshold), copy.deepcopy(pods), reserved=reserved)
    tab = with_reserved.build_pages()[0].snapshot.thr_reserved  # the same names, so the same dimensions

    def feed(eng):
        before = eng.headroom(np.arange(3), cap=CAP)[0]
        eng.set_reserved(np.arange(1, dtype=np.int32), tab)
        after = eng.headroom(np.arange(3), cap=CAP)[0]
        assert (after <= before).all() and (after < before).any()
    got = _hold_to_walk(plain, oracle_mod, f"reserved {kind}", engine_hook=feed, model_cs=with_reserved)
    assert got[False] == [(2, 0), (3, 0), (4, 0)]


def test_pods_without_an_answer_from_any_throttle(oracle_mod):
    """A pod no throttle affects: (cap, -1); a pod in a namespace that does not exist (PreFilter is an error) and a pod row that
    holds no pod: (0, -1)."""
    pods = [_pod("job", {"cpu": "500m"}), _pod("other", {"cpu": "500m"}, app="other"), _pod("ghost", {"cpu": "500m"}, ns="ghost")]
    cs = _cluster("ClusterThrottle", {"resourceRequests": {"cpu": "1"}}, pods)
    got = _hold_to_walk(cs, oracle_mod, "no answer", cap=7)
    assert got[False] == [(2, 0), (7, -1), (0, -1)]
    snap = cs.build_pages()[0].snapshot
    eng = E.Engine.for_snapshot(snap, pod_capacity=8)
    try:
        copies, limiting = eng.headroom(np.array([5, 0, 7]), cap=7)
        assert list(copies) == [0, 2, 0] and list(limiting) == [-1, 0, -1]
    finally:
        eng.close()


# ---- refusals and the check slot ---------------------------------------------------------------------------------------------
def test_refusals_and_the_check_slot():
    snap, queue = _workload(64)
    queue = queue[:10]
    eng = E.Engine.for_snapshot(snap)
    other = E.Engine.for_snapshot(W.generate(W.small(seed=4, n_pods=200, n_thr=24, n_cluster=8)))
    try:
        before = eng.fetch_reserved()
        with pytest.raises(E.EngineError) as ex:
            eng.headroom_fetch(1)
        assert ex.value.code == -5  # KT_ERR_NOT_READY: no launch yet
        for cap in (0, -3, 1 << 31):
            with pytest.raises(E.EngineError) as ex:
                eng.headroom(queue, cap=cap)
            assert ex.value.code == -1, cap  # KT_ERR_INVALID_ARGUMENT
            with pytest.raises(E.EngineError) as ex:
                E.paged_headroom([eng], queue, cap)
            assert ex.value.code == -1, cap
        with pytest.raises(E.EngineError) as ex:
            eng.headroom_fetch(1)  # a refused launch leaves nothing to fetch
        assert ex.value.code == -5
        copies, limiting = eng.headroom(queue[:0], cap=4)  # n == 0
        assert copies.shape == (0,) and limiting.shape == (0,)
        copies, limiting = E.paged_headroom([eng], queue[:0], 4)
        assert copies.shape == (0,) and limiting.shape == (0,)
        want = eng.headroom(queue, cap=E.HEADROOM_MAX_CAP)  # the largest cap
        assert (want[0] <= E.HEADROOM_MAX_CAP).all() and (want[0] >= 0).all()
        eng.headroom_launch(len(queue), queue, cap=9)
        got = eng.headroom_fetch(len(queue), want_limiting=False)  # out_limiting is nullable
        assert got[1] is None and (got[0] == np.minimum(want[0], 9)).all()
        eng.headroom_launch(len(queue), queue, cap=9)
        eng._ck(E.lib().kt_admit_launch(eng._h, len(queue), queue.ctypes.data, 0, 0, None))  # takes the check slot
        with pytest.raises(E.EngineError) as ex:
            eng.headroom_fetch(len(queue))
        assert ex.value.code == -5
        eng.check_launch(len(queue), queue)
        eng.headroom_launch(len(queue), queue, cap=9)  # ... and a headroom launch drops a pending check launch
        with pytest.raises(E.EngineError) as ex:
            eng.check_fetch(len(queue))
        assert ex.value.code == -5
        with pytest.raises(E.EngineError) as ex:
            eng.headroom_fetch(len(queue) + 1)
        assert ex.value.code == -2  # more than were launched
        a, b = eng.headroom_fetch(len(queue))
        assert (a == got[0]).all()
        one = E.paged_headroom([eng], queue, 9)  # one page of kt_paged_headroom is kt_headroom_launch + kt_headroom_fetch
        assert (one[0] == a).all() and (one[1] == b).all()
        with pytest.raises(E.EngineError) as ex:
            E.paged_headroom([eng, other], queue, 9)
        assert ex.value.code == -1  # different throttle-row counts
        with pytest.raises(E.EngineError) as ex:
            E.paged_headroom([eng, eng], queue, 9)
        assert ex.value.code == -1  # the same engine twice
        after = eng.fetch_reserved()
        for f in ("v", "present", "count", "has_count"):
            np.testing.assert_array_equal(getattr(after, f), getattr(before, f), err_msg=f)
    finally:
        eng.close()
        other.close()


def test_a_page_with_wide_sums_is_refused():
    """As kt_admit_launch (tests/test_paged_admit_gpu.py): a stored `used` beyond int64 is not read."""
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
            wide.headroom(np.arange(8), cap=4)
        with pytest.raises(E.EngineError) as ex:
            E.paged_headroom([plain, wide], np.arange(8), 4)
        assert ex.value.code == one.value.code == -7
    finally:
        wide.close()
        plain.close()


# ---- the C++ plugin mirror ---------------------------------------------------------------------------------------------------
def test_host_plugin_headroom():
    """KubeThrottler::Headroom against counting PreFilter + Reserve of fresh same-shape pods on a twin
    (tests/cpp/host_plugin_headroom_test.cpp)."""
    exe = os.path.join(HOST, "host_plugin_headroom_test")
    subprocess.check_call(["make", "-C", HOST, "host_plugin_headroom_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
