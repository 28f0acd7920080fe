"""Elastic gang admission on the device (kt_admit_gangs_elastic_launch / kt_paged_admit_gangs_elastic, the kt_admit_gangs_elastic
kernels): held to ``model_admit_gangs_elastic`` of tests/test_gang_admit_elastic_cpu.py on its cases and seeded rules (one page
through Engine.admit_gangs_elastic, >= 3 pages through PagedEngine.admit_gangs_elastic, state in LDS and in HBM), directed cases for
the kept partial gang, the required member and the shapes where the walk takes another path, the identities with all-or-nothing and
plain admission, validation, the slot rules, degenerate shapes, and the C++ plugin mirror's AdmitElasticGangs."""
import copy
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import workload as W
from kube_throttler_amd.objects import ClusterState
from test_gang_admit_cpu import GANG_CASES, gang_case, model_admit_gangs
from test_gang_admit_elastic_cpu import elastic_case, model_admit_gangs_elastic
from test_gang_admit_gpu import _abcd, _cluster, _pod, _same_reserved, _throttle, _verdicts, _workload
from test_paged_admit_cpu import VERDICT_NAME, reserved_totals, row_of, write_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "kube_throttler_amd", "host")
INVALID_ARGUMENT, NOT_READY = -1, -5


def _admit_elastic(eng, queue, off, mins, req, on_equal, commit):
    """One page: Engine.admit_gangs_elastic (the launch + the two fetches); more: PagedEngine.admit_gangs_elastic."""
    rq = None if req is None else np.array(req, bool)
    if len(eng.engines) == 1:
        status, summary, members = eng.engines[0].admit_gangs_elastic(np.array(queue, np.int64), off, mins, rq, on_equal=on_equal, commit=commit)
        return status, _verdicts(summary), members
    return eng.admit_gangs_elastic(np.array(queue, np.int64), off, mins, rq, on_equal=on_equal, commit=commit)


def _hold_to_model(cs, queue, off, mins, req, on_equal, label, min_pages=1):
    """Dry run, then commit: per-pod status row and verdict, the members per gang, and every throttle's reserved amount on every
    page (absent names and an absent count included) against the reference; after the dry run the reserved amounts are unchanged.
    -> (the reference's per-pod answers, its members per gang, the committed reserved amounts per throttle name)"""
    pages = cs.build_pages()
    assert len(pages) >= min_pages
    names = pages[0].thr_names
    after = copy.deepcopy(cs)
    want, want_members = model_admit_gangs_elastic(after, queue, off, mins, req, on_equal)
    eng = paging.PagedEngine(pages)
    try:
        before = reserved_totals(cs)
        for commit in (False, True):
            status, verdict, members = _admit_elastic(eng, queue, off, mins, req, on_equal, commit)
            for k, (v, st) in enumerate(want):
                where = f"{label} on_equal={on_equal} commit={commit} pos {k} pod{queue[k]}"
                assert VERDICT_NAME[int(verdict[k])] == v, where
                if v != "error":
                    assert row_of(status[k], names) == st, where
            assert [int(x) for x in members] == want_members, f"{label} on_equal={on_equal} commit={commit}"
            totals = reserved_totals(after) if commit else before
            got = eng.fetch_reserved()
            for t, nn in enumerate(names):
                assert got[t] == totals.get(nn, {}), f"{label} commit={commit}: reserved of {nn}"
        return want, want_members, dict(zip(names, got))
    finally:
        eng.close()


# ---- model parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_equal", [False, True])
@pytest.mark.parametrize("seed,wide", GANG_CASES)
def test_elastic_gangs_equal_the_manifest_model(seed, wide, on_equal, oracle_mod):
    cs, queue, off, mins, req = elastic_case(seed, wide, oracle_mod)
    _hold_to_model(cs, queue, off, mins, req, on_equal, f"seed {seed} wide={wide}", min_pages=3 if wide else 1)


def test_elastic_gangs_equal_the_manifest_model_with_hbm_state():
    """The same cases, the required member that fails and the shapes with the state in the HBM scratch buffer
    (kt_admit_gangs_elastic<DT, false>): the hook is read once per process, so they run in a child."""
    env = dict(os.environ, KT_ADMIT_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__, "-k",
                        "(test_elastic_gangs_equal_the_manifest_model and not hbm) or test_required or test_kept or test_shapes"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- directed cases ----------------------------------------------------------------------------------------------------------
def _verdicts_of(want):
    return [v for v, _ in want]


def test_kept_partial_gang_blocks_the_pod_behind_it(oracle_mod):
    """[A, B, C] with a quorum of 2 on an empty reserved table: A and B reserve (B brings `memory` in, both the count), C is blocked
    by the count of 2 and never stores: the gang stays with 2 members, the reserved amount reads back A + B with `memory` present
    and a count of 2, and D behind it is blocked.  With a quorum of 3 it is all-or-nothing admission: rolled back, D is admitted."""
    cs = _cluster(_abcd())
    write_status(cs, oracle_mod)
    want, members, reserved = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [2, 1], None, False, "kept partial")
    assert _verdicts_of(want) == ["allow", "allow", "block", "block"] and members == [2, 0]
    (r,) = reserved.values()
    assert r == {"resourceCounts": {"pod": 2}, "resourceRequests": {"cpu": Fraction(4, 5), "memory": Fraction(64 << 20)}}
    want, members, reserved = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [3, 1], None, False, "all or nothing")
    assert _verdicts_of(want) == ["allow", "allow", "block", "allow"] and members == [0, 1]
    assert want == model_admit_gangs(copy.deepcopy(cs), [0, 1, 2, 3], [0, 3, 4], False)[0]
    (r,) = reserved.values()
    assert r == {"resourceCounts": {"pod": 1}, "resourceRequests": {"cpu": Fraction(7, 10)}}


def test_required_member_that_fails_rolls_the_gang_back(oracle_mod):
    """[X (2 cpu: more than the threshold, required), A, B] with a quorum of 2: two members succeed, the gang is rolled back all
    the same — the reserved amount reads back with no names and no count — and D behind it is admitted."""
    a, b, _, d = _abcd()
    cs = _cluster([_pod("X", {"cpu": "2"}), a, b, d])
    write_status(cs, oracle_mod)
    want, members, reserved = _hold_to_model(cs, [0, 1, 2], [0, 3], [2], [True, False, False], False, "required alone")
    assert _verdicts_of(want) == ["block", "allow", "allow"] and members == [0]
    assert list(reserved.values()) == [{}]
    pages = cs.build_pages()
    eng = E.Engine.for_snapshot(pages[0].snapshot)
    try:
        _, _, m = eng.admit_gangs_elastic(np.arange(3), [0, 3], [2], [True, False, False], commit=True)
        assert list(m) == [0]
        r = eng.fetch_reserved()
        assert not r.present[:1].any() and not r.has_count[:1].any()
    finally:
        eng.close()
    want, members, _ = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [2, 1], [True, False, False, False], False, "required")
    assert _verdicts_of(want) == ["block", "allow", "allow", "allow"] and members == [0, 1]
    # without the flag the same gang stays, and D does not fit behind A + B
    want, members, _ = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [2, 1], None, False, "not required")
    assert _verdicts_of(want) == ["block", "allow", "allow", "block"] and members == [2, 0]


def test_error_member_counts_as_failed(oracle_mod):
    """An Error member (unknown namespace) in the middle: not required, the gang stays with the 2 that succeeded; required, it is
    rolled back."""
    a, b, _, d = _abcd()
    cs = _cluster([a, _pod("G", {"cpu": "100m"}, ns="ghost"), b, d])
    write_status(cs, oracle_mod)
    want, members, _ = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [2, 1], None, False, "error member")
    assert _verdicts_of(want) == ["allow", "error", "allow", "block"] and members == [2, 0]
    want, members, _ = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [2, 1], [False, True, False, False], False, "required error member")
    assert _verdicts_of(want) == ["allow", "error", "allow", "allow"] and members == [0, 1]


@pytest.mark.parametrize("n_match,n_other,extra_names", [(17, 0, 0), (5, 0, 14), (17, 1023, 0)],
                         ids=["17-throttles-D4", "5-throttles-D16", "1040-throttles"])
def test_shapes_where_the_walk_takes_another_path(n_match, n_other, extra_names, oracle_mod):
    """More affected throttles than one pass of lanes holds (64 / DT: 16 for D <= 4, 4 for D = 16), and T > 1024 (the row is listed
    in a second 16-bytes-per-lane chunk): [A, B, C] with a quorum of 2 stays with 2 members on every throttle, D is blocked on all
    of them."""
    cs = _cluster(_abcd(), n_match, n_other, extra_names)
    write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1 and pages[0].snapshot.D == (16 if extra_names else 2)
    if n_other:
        rows = [t for t, nn in enumerate(pages[0].thr_names) if "/t" in nn]
        assert len(pages[0].thr_names) == 1040 and min(rows) == 1023 and max(rows) == 1039
    want, members, reserved = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [2, 1], None, False, "shape")
    assert _verdicts_of(want) == ["allow", "allow", "block", "block"] and members == [2, 0]
    assert all(len(st) == n_match for _, st in want)
    assert all(s != "not-throttled" for s in want[3][1].values())  # D is blocked on every one of them
    assert sum(1 for r in reserved.values() if r.get("resourceCounts") == {"pod": 2}) == n_match


def test_wide_verdict_depends_on_a_kept_partial_gang(oracle_mod):
    """Three pages by hand: the throttle names cpu, 40 example.com names and (through B) memory; r39, which decides, lives on the last
    page.  [A, B, C] with a quorum of 2: A and B take the 4 of r39, C is blocked there and the gang stays; D's verdict behind it is
    `block` only because the partial gang was kept (all-or-nothing admission rolls it back and admits D)."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    r39 = "example.com/r39"
    for p in (_pod("A", {"cpu": "400m", r39: "2"}), _pod("B", {"cpu": "400m", "memory": "64Mi", r39: "2"}), _pod("C", {"cpu": "100m", r39: "1"}),
              _pod("D", {"cpu": "100m", r39: "1"})):
        cs.add(p)
    rr = {"cpu": "10", **{f"example.com/r{k:02d}": "100" for k in range(39)}, r39: "4"}
    cs.add(_throttle("t0000", {"resourceCounts": {"pod": 9}, "resourceRequests": rr}))
    write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) >= 3 and r39 not in pages[0].dims and r39 not in pages[1].dims
    want, members, reserved = _hold_to_model(cs, [0, 1, 2, 3], [0, 3, 4], [2, 1], None, False, "wide by hand", min_pages=3)
    assert _verdicts_of(want) == ["allow", "allow", "block", "block"] and members == [2, 0]
    whole, admitted = model_admit_gangs(copy.deepcopy(cs), [0, 1, 2, 3], [0, 3, 4], False)
    assert _verdicts_of(whole) == ["allow", "allow", "block", "allow"] and admitted == [False, True]
    (r,) = reserved.values()
    assert r["resourceCounts"] == {"pod": 2} and r["resourceRequests"][r39] == 4 and "memory" in r["resourceRequests"]


# ---- identities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,wide", [GANG_CASES[0], GANG_CASES[7], GANG_CASES[-2], GANG_CASES[-1]])
def test_full_quorum_and_all_required_are_admit_gangs(seed, wide, oracle_mod):
    """min = size without flags, every member required, every member required with min = 1: kt_admit_gangs_launch /
    kt_paged_admit_gangs byte for byte — status matrix, summary words, reserved tables of every page, members > 0 where admitted."""
    assert [w for _, w in (GANG_CASES[0], GANG_CASES[7], GANG_CASES[-2], GANG_CASES[-1])] == [False, False, True, True]
    cs, queue, off = gang_case(seed, wide, oracle_mod)
    queue = np.array(queue, np.int64)
    sizes = np.diff(off)
    pages = cs.build_pages()
    assert len(pages) >= (3 if wide else 1)
    every = np.ones(len(queue), bool)

    def gangs(es, **kw):
        return es[0].admit_gangs(queue, off, **kw) if len(es) == 1 else E.paged_admit_gangs(es, queue, off, **kw)

    def elastic(es, mins, req, **kw):
        if len(es) == 1:
            return es[0].admit_gangs_elastic(queue, off, mins, req, **kw)
        return E.paged_admit_gangs_elastic(es, queue, off, mins, req, **kw)

    for on_equal in (False, True):
        for mins, req in ((sizes, None), (sizes, every), (np.ones(len(sizes), np.int64), every)):
            plain, other = paging.PagedEngine(pages), paging.PagedEngine(pages)
            try:
                for commit in (False, True):
                    st1, sm1, adm = gangs(plain.engines, on_equal=on_equal, commit=commit)
                    st2, sm2, members = elastic(other.engines, mins, req, on_equal=on_equal, commit=commit)
                    np.testing.assert_array_equal(st2, st1)
                    np.testing.assert_array_equal(sm2, sm1)
                    np.testing.assert_array_equal(members > 0, adm != 0)
                    np.testing.assert_array_equal(members[adm != 0], sizes[adm != 0])
                for a, b in zip(other.engines, plain.engines):
                    _same_reserved(a.fetch_reserved(), b.fetch_reserved())
            finally:
                plain.close()
                other.close()


def test_gangs_of_one_pod_are_plain_admission():
    snap, queue = _workload()
    plain, gang = (E.Engine.for_snapshot(snap) for _ in range(2))
    try:
        ones = np.arange(len(queue) + 1)
        for commit in (False, True):
            st1, sm1 = plain.admit(queue, commit=commit)
            st2, sm2, members = gang.admit_gangs_elastic(queue, ones, np.ones(len(queue), np.int64), commit=commit)
            np.testing.assert_array_equal(st2, st1)
            np.testing.assert_array_equal(sm2, sm1)
            np.testing.assert_array_equal(members, (sm1 == 0).astype(np.int64))
        assert members.any() and not members.all()
        _same_reserved(gang.fetch_reserved(), plain.fetch_reserved())
    finally:
        plain.close()
        gang.close()


# ---- validation, slots, degenerate shapes --------------------------------------------------------------------------------------
def _refused(call, code, *words):
    with pytest.raises(E.EngineError) as ex:
        call()
    assert ex.value.code == code, str(ex.value)
    for w in words:
        assert w in str(ex.value), str(ex.value)


def test_refused_rules_leave_the_reserved_amounts_alone():
    """Clause (10), in its order, through the engine call and the paged one: every gang_off defect, a missing quorum array, a quorum
    outside [1, size] (the gang and both numbers are named), a flag byte with another bit (the position is named); behind the
    refused commits the reserved amounts are untouched and nothing is pending."""
    snap, queue = _workload()
    queue = queue[:10]
    eng = E.Engine.for_snapshot(snap)
    L = E.lib()

    def raw(off, mins, flags, paged):
        off, q = np.asarray(off, np.int64), np.ascontiguousarray(queue)
        mp = None if mins is None else np.asarray(mins, np.int64)
        fp = None if flags is None else np.asarray(flags, np.uint8)
        args = (len(q), q.ctypes.data, len(off) - 1, off.ctypes.data, None if mp is None else mp.ctypes.data, None if fp is None else fp.ctypes.data,
                0, E.ADMIT_COMMIT)
        if paged:
            import ctypes as C
            hs = (C.c_void_p * 1)(eng._h)
            rc = L.kt_paged_admit_gangs_elastic(hs, 1, *args, None, None, None)
        else:
            rc = L.kt_admit_gangs_elastic_launch(eng._h, *args, None)
        if rc != E.KT_OK:
            raise E.EngineError(rc, L.kt_last_error(eng._h).decode())

    try:
        before = eng.fetch_reserved()
        for paged in (False, True):
            for off in ([1, 10], [0, 4, 9], [0, 4, 4, 10], [0, 6, 4, 10], [0, 4, 12]):  # the offsets come first: the rule is bad too
                _refused(lambda: raw(off, [99] * (len(off) - 1), [2] * 10, paged), INVALID_ARGUMENT, "gang_off")
            _refused(lambda: raw([0, 4, 4, 10], [1, 1, 1], None, paged), INVALID_ARGUMENT, "gang 1 is empty")
            _refused(lambda: raw([0, 4, 10], None, [2] * 10, paged), INVALID_ARGUMENT, "min_members is NULL")
            _refused(lambda: raw([0, 4, 10], [4, 0], [2] * 10, paged), INVALID_ARGUMENT, "gang 1", " 0 ", "[1, 6]")
            _refused(lambda: raw([0, 4, 10], [5, 6], None, paged), INVALID_ARGUMENT, "gang 0", " 5 ", "[1, 4]")
            _refused(lambda: raw([0, 4, 10], [4, 6], [0, 1, 0, 1, 0, 0, 0, 3, 0, 2], paged), INVALID_ARGUMENT, "position 7")
            _refused(lambda: eng.admit_gangs_elastic_fetch(1), NOT_READY)  # a refused launch leaves nothing to fetch
            _refused(lambda: eng.admit_gangs_fetch(1), NOT_READY)
        _refused(lambda: eng.admit_gangs_elastic(queue, [0, 4, 10], [4, 7], commit=True), INVALID_ARGUMENT, "gang 1")
        _refused(lambda: E.paged_admit_gangs_elastic([eng], queue, [0, 4, 10], [4, 6], np.full(10, 4, np.uint8), commit=True), INVALID_ARGUMENT,
                 "position 0")
        _same_reserved(eng.fetch_reserved(), before)
    finally:
        eng.close()


def test_the_gang_slot_answers_counts_and_bytes():
    """Clause (11): behind an elastic launch the elastic fetch answers the counts and kt_admit_gangs_fetch the bytes, 1 where the
    count is above 0; behind a plain gang launch the elastic fetch is KT_ERR_NOT_READY (no counts were kept) while the bytes are
    there; a plain admission drops the pending result for both."""
    snap, queue = _workload()
    off = np.arange(0, len(queue) + 1, 4)
    assert off[-1] == len(queue)
    mins = np.full(len(off) - 1, 2, np.int64)
    eng = E.Engine.for_snapshot(snap)
    try:
        _refused(lambda: eng.admit_gangs_elastic_fetch(1), NOT_READY)  # no gang launch yet
        n, ng = eng.admit_gangs_elastic_launch(queue, off, mins)
        members = eng.admit_gangs_elastic_fetch(ng)
        flags = eng.admit_gangs_fetch(ng)
        np.testing.assert_array_equal(flags, (members > 0).astype(np.uint8))
        _, summary = eng.check_fetch(n)
        ok = np.add.reduceat((summary == 0).astype(np.int64), off[:-1])
        np.testing.assert_array_equal(members, np.where(ok >= 2, ok, 0))
        assert (members > 0).any() and (members < 4).any(), members  # (counts, not the bytes again)
        np.testing.assert_array_equal(eng.admit_gangs_elastic_fetch(ng), members)  # the slot stays until the next launch
        _refused(lambda: eng.admit_gangs_elastic_fetch(ng + 1), -2)  # KT_ERR_OUT_OF_RANGE
        eng.admit_gangs_launch(queue, off)
        _refused(lambda: eng.admit_gangs_elastic_fetch(ng), NOT_READY, "no counts")
        assert eng.admit_gangs_fetch(ng).shape == (ng,)
        eng.admit_gangs_elastic_launch(queue, off, mins)
        eng.admit(queue)  # a plain launch drops the pending gang result
        _refused(lambda: eng.admit_gangs_elastic_fetch(ng), NOT_READY)
        _refused(lambda: eng.admit_gangs_fetch(ng), NOT_READY)
    finally:
        eng.close()


def test_degenerate_shapes():
    """An engine without throttle rows decides on the host from the summaries, with the same rule; the empty queue is KT_OK."""
    snap = W.generate(W.small(seed=5, n_pods=10, n_thr=0, n_cluster=0))
    eng = E.Engine.for_snapshot(snap)
    try:
        assert eng.throttle_rows() == 0
        rows, off = np.arange(10), [0, 3, 4, 10]
        required = np.zeros(10, bool)
        required[[1, 9]] = True
        _, summary, members = eng.admit_gangs_elastic(rows, off, [2, 1, 6], required, commit=True)
        ok = summary == 0
        want = []
        for g, need in enumerate([2, 1, 6]):
            o = ok[off[g]:off[g + 1]]
            kept = o.sum() >= need and o[required[off[g]:off[g + 1]]].all()
            want.append(int(o.sum()) if kept else 0)
        assert ok.all() and want == [3, 1, 6]
        assert list(members) == want
        assert list(eng.admit_gangs_fetch(3)) == [1, 1, 1]
        st, sm, m = E.paged_admit_gangs_elastic([eng], rows, off, [3, 1, 1])
        assert list(m) == [3, 1, 6]
        status, summary, members = eng.admit_gangs_elastic(rows[:0], [0], [])  # the empty queue
        assert summary.shape == (0,) and members.shape == (0,)
        status, summary, members = E.paged_admit_gangs_elastic([eng], rows[:0], [0], [])
        assert summary.shape == (0,) and members.shape == (0,)
    finally:
        eng.close()
    snap, queue = _workload()
    eng = E.Engine.for_snapshot(snap)
    try:
        status, summary, members = eng.admit_gangs_elastic(queue[:0], [0], [], commit=True)
        assert summary.shape == (0,) and members.shape == (0,)
    finally:
        eng.close()


# ---- the C++ plugin mirror -----------------------------------------------------------------------------------------------------
def test_host_plugin_elastic_gangs():
    """KubeThrottler::AdmitElasticGangs against PreFilter / Reserve / Unreserve on a twin, on a mirror of two pages
    (tests/cpp/host_plugin_elastic_gang_test.cpp)."""
    exe = os.path.join(HOST, "host_plugin_elastic_gang_test")
    subprocess.check_call(["make", "-C", HOST, "host_plugin_elastic_gang_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
