"""The match cache: single-chunk programs keep, per pod row, the matched terms of every word of the pod's namespace list, and the
two-per-CU form of the PreFilter sweep replays that table instead of scanning the selectors again.  (The two-per-CU aggregate
replays it too, from a copy of the planes in the order of its scan view: test_agg_match_cache_gpu.py, and with several planes
test_match_cache_planes_gpu.py.  The cases here read the sweep's counter: the second element of assert_counters.)

Every case runs two engines fed alike — one as it comes, one under KT_NO_MATCH_CACHE=1 — and compares the sweep's summary words of
all rows and the reconcile result on all throttle rows between them, the reconcile on the responsible rows and the summary words
with the oracle, and reads from the counters (full builds of the table, scans served from it) which path ran.
"""
import functools

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from test_aggregate_two_per_cu_gpu import assert_same_result, cfg2_scaled
from test_engine_gpu import _permute_pods, _rows_of, _with_pods, assert_reconcile_equal, responsible_rows

pytestmark = pytest.mark.gpu

NOW = (1767225600, 0)
COUNTER_NS_WORD_VISITS, COUNTER_NS_ROWS = E.COUNTER_NS_WORD_VISITS, E.COUNTER_NS_ROWS


@functools.lru_cache(maxsize=None)  # (once per process and question: the modules that import it share the answers)
def shape_with_planes(lo, hi, preset=2):
    """(throttles, ClusterThrottles) of the configs[2] generator (or another preset's) whose single-chunk program has a longest
    namespace word list of lo..hi words, found by compiling small engines (KT_COUNTER_MATCH_CACHE_PLANES after one sweep) over a
    ladder of shapes."""
    seen = []
    for n_thr, n_cluster in ((200, 100), (300, 150), (400, 200), (500, 400), (600, 500), (700, 640), (800, 740), (900, 840), (1100, 1040)):
        snap = W.generate(cfg2_scaled(640, n_thr=n_thr, n_cluster=n_cluster, preset=preset))
        e = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
        try:
            e.check(n=snap.n_pods, want_status=False)
            planes, chunks = e.match_cache_planes(), e.index_stats()["chunks"]
        finally:
            e.close()
        seen.append((n_thr, n_cluster, planes, chunks))
        if chunks == 1 and lo <= planes <= hi:
            return n_thr, n_cluster
    raise AssertionError(f"no shape of the ladder has {lo}..{hi} planes in one chunk: {seen}")


class Twin:
    """Two engines built by `make` and fed alike: `c` as it comes (the cache on), `u` under KT_NO_MATCH_CACHE=1."""

    def __init__(self, monkeypatch, make):
        monkeypatch.delenv("KT_NO_MATCH_CACHE", raising=False)
        self.c = make()
        monkeypatch.setenv("KT_NO_MATCH_CACHE", "1")
        self.u = make()
        monkeypatch.delenv("KT_NO_MATCH_CACHE", raising=False)
        self.steps = 0

    def both(self, f):
        return f(self.c), f(self.u)

    def close(self):
        self.c.close()
        self.u.close()

    def step(self, snap, oracle_mod, now=NOW, n=None):
        """reconcile (apply) + sweep on both engines: against each other on every row, against the oracle (whose stored status
        then is the reconcile's, as the engines')."""
        n = snap.n_pods if n is None else n
        rows = responsible_rows(snap)
        o = oracle_mod.Oracle(snap)
        want = o.reconcile(now, rows=rows, nthreads=8)
        rc, ru = self.both(lambda e: e.reconcile(now, apply=True))
        assert_same_result(rc, ru, snap.n_thr)
        assert_reconcile_equal(_rows_of(rc, rows, snap.D), want, len(rows))
        snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
        _, sm_w = o.check(on_equal=False, want_status=False, nthreads=8)
        (_, sm_c), (_, sm_u) = self.both(lambda e: e.check(n=n, on_equal=False, want_status=False))
        np.testing.assert_array_equal(sm_c, sm_u, err_msg="summary words: cached against uncached")
        np.testing.assert_array_equal(sm_c, sm_w[:n], err_msg="summary words against the oracle")
        self.steps += 1
        return want, sm_w

    def assert_counters(self, builds, scans):
        got = (self.c.match_cache_builds(), self.c.match_cache_scans())
        assert got == (builds, scans), f"cached engine: (builds, scans) = {got}, expected {(builds, scans)}"
        assert (self.u.match_cache_builds(), self.u.match_cache_scans()) == (0, 0), "KT_NO_MATCH_CACHE=1 built or used a table"


def twin_for(snap, monkeypatch):
    return Twin(monkeypatch, lambda: E.Engine.for_snapshot(snap, E.VARIANT_INDEXED))


# ---- 1. basic parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", [2, 3], ids=["configs2-simple", "configs3-rich"])
def test_basic_parity(preset, oracle_mod, monkeypatch):
    """66 037 pods (a multiple of neither 64 nor 1024; the tiles straddle namespaces) x 48 throttles: one build, and the
    sweep of the step replays the table.  Preset 3: configs[3]'s generator — overrides; its selectors are as simple as configs[2]'s
    (a program with vetoes, whose table kt_build_match_cache<true, 3> builds: the `vetoes` kind of test_match_cache_planes_gpu.py)."""
    snap = W.generate(cfg2_scaled(66_037, preset=preset))
    tw = twin_for(snap, monkeypatch)
    try:
        want, sm_w = tw.step(snap, oracle_mod)
        tw.assert_counters(1, 1)
        assert tw.c.index_stats()["chunks"] == 1
        assert (want.used.count > 0).any() and (sm_w > 1).any(), "nothing matched: the case tests nothing"
    finally:
        tw.close()


# ---- 2. two tiles per wave in the check --------------------------------------------------------------------------------------
def test_more_than_512_workgroups_worth_of_pods(oracle_mod, monkeypatch):
    """525 000 pods: more than 512 workgroups x 16 waves x 64 rows — a wave of the sweep takes a second tile."""
    snap = W.generate(cfg2_scaled(525_000))
    assert snap.n_pods > 512 * 1024
    tw = twin_for(snap, monkeypatch)
    try:
        tw.step(snap, oracle_mod)
        tw.assert_counters(1, 1)
    finally:
        tw.close()


# ---- 3. lists of unequal length ----------------------------------------------------------------------------------------------
def test_lists_of_unequal_length(oracle_mod, monkeypatch):
    """One namespace without any Throttle of its own (its list holds the cluster words only) and pods in a namespace whose row has
    no Namespace object (no ClusterThrottle admits it: the namespaced words only) beside the full lists: the planes past a
    lane's list do not count, in tiles that straddle such namespaces."""
    n_thr, n_cluster = shape_with_planes(2, 4)  # (several words: 48 throttles are one word for everybody)
    snap = W.generate(cfg2_scaled(20_011, n_thr=n_thr, n_cluster=n_cluster))
    T = snap.n_thr
    namespaced = np.nonzero((snap.thr_flags[:T] & S.THR_CLUSTER) == 0)[0]
    bare = int(snap.thr_ns[namespaced[0]])
    snap.thr_flags[:T][(snap.thr_ns[:T] == bare) & ((snap.thr_flags[:T] & S.THR_CLUSTER) == 0)] = 0
    gone = int(snap.thr_ns[[t for t in namespaced if int(snap.thr_ns[t]) != bare][0]])
    snap.ns_valid[gone] = 0
    assert (snap.pod_ns[:snap.n_pods] == bare).any() and (snap.pod_ns[:snap.n_pods] == gone).any()
    tw = twin_for(snap, monkeypatch)
    try:
        tw.step(snap, oracle_mod)
        tw.assert_counters(1, 1)
        stats = tw.c.index_stats()
        print("index:", stats)
        assert stats["chunks"] == 1 and stats["words"] > 1
        assert 2 <= tw.c.match_cache_planes() <= 4, tw.c.match_cache_planes()  # (several planes, and still a cached program)
        assert stats["word_visits_per_namespace"] != int(stats["word_visits_per_namespace"]), "every namespace visits as many words"
    finally:
        tw.close()


# ---- 4. nothing that a step changes rebuilds the table -----------------------------------------------------------------------
@pytest.mark.parametrize("preset", [2, 3], ids=["configs2", "configs3-overrides"])
def test_steps_do_not_rebuild(preset, oracle_mod, monkeypatch):
    """Three rounds of reconcile (apply) + sweep with a stored status set from outside, reserved amounts and (preset 3) instants on
    both sides of an override boundary in between: one build for all of them, every round the oracle's."""
    snap = W.generate(cfg2_scaled(30_001, preset=preset))
    tw = twin_for(snap, monkeypatch)
    try:
        tw.step(snap, oracle_mod)
        rows = responsible_rows(snap)
        T = snap.n_thr
        # a stored status from outside: the counts of a few throttles doubled (what another replica's UpdateStatus might leave)
        some = rows[:4].astype(np.int32)
        snap.thr_used.count[some] *= 2
        snap.thr_used.v[some] *= 2
        allrows = np.arange(T, dtype=np.int32)
        tw.both(lambda e: e.set_status(allrows, snap.thr_used, snap.thr_calc, (snap.thr_flags[:T] & S.THR_CALC_AT_NONZERO) != 0,
                                       snap.thr_thrl_flag[:T], snap.thr_thrl_has[:T], (snap.thr_flags[:T] & S.THR_THROTTLED_POD) != 0,
                                       snap.thr_status_msgs_fp[:T]))
        now2 = NOW
        if preset == 3:  # the next instant at which some override begins or ends: one round before it, one behind
            inst, total = tw.c.override_instants(NOW, (NOW[0] + 400 * 86400, 0), cap=1)
            assert total > 0, "preset 3 has no override boundary ahead"
            now2 = inst[0]
        tw.step(snap, oracle_mod, now=(now2[0] - 1, 0) if preset == 3 else NOW)
        res = S.Amounts(3, snap.D)
        for i in range(3):
            res.set_row(i, {0: 1000 * (i + 1), 1: 1 << 30}, count=i + 1)
            for f in ("v", "present", "count", "has_count"):
                getattr(snap.thr_reserved, f)[rows[i]] = getattr(res, f)[i]
        tw.both(lambda e: e.set_reserved(rows[:3].astype(np.int32), res))
        tw.step(snap, oracle_mod, now=(now2[0] + 1, 0) if preset == 3 else NOW)
        tw.assert_counters(1, 3)
    finally:
        tw.close()


# ---- 5. pod events -----------------------------------------------------------------------------------------------------------
def test_pod_events_refresh_their_rows(oracle_mod, monkeypatch):
    """Upserts that change labels and namespace of existing rows, appended rows, a delete followed by an upsert of the same row,
    a batch that names a row twice: after each, sweep and reconcile equal the oracle and the uncached engine — and no event
    rebuilds the table (the rows are refreshed by the list form of the builder)."""
    base = W.generate(cfg2_scaled(5_000))
    P, n0 = 4_300, 4_000
    state = np.full(P, -1, dtype=np.int64)
    state[:n0] = np.arange(n0)

    def make():
        e = E.Engine(base.D, max(base.L, 1), P, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(_permute_pods(base, np.arange(n0)), rows=np.arange(n0))
        return e

    tw = Twin(monkeypatch, make)

    def sweep():
        n = int(np.nonzero(state >= 0)[0].max()) + 1
        snap = _with_pods(base, state[:n])
        tw.step(snap, oracle_mod, n=n)
        base.thr_used, base.thr_calc = snap.thr_used, snap.thr_calc
        base.thr_flags, base.thr_thrl_flag, base.thr_thrl_has = snap.thr_flags, snap.thr_thrl_flag, snap.thr_thrl_has
        tw.assert_counters(1, tw.steps)

    def upsert(rows, pods):
        rows, pods = np.asarray(rows, dtype=np.int64), np.asarray(pods, dtype=np.int64)
        tw.both(lambda e: e.upsert_pods(_permute_pods(base, pods), rows=rows))
        for r, p in zip(rows, pods):  # (in order: the last entry of a row wins)
            state[r] = p

    try:
        sweep()
        upsert(np.arange(10, 31), np.arange(4_500, 4_521))        # other labels, namespaces, requests in existing rows
        sweep()
        upsert([n0, n0 + 1, n0 + 2], [4_600, 4_601, 4_602])        # three appended rows
        sweep()
        tw.both(lambda e: e.delete_pods(np.array([50], dtype=np.int64)))
        state[50] = -1
        upsert([50], [4_700])                                      # a delete, then an upsert of the same row
        sweep()
        tw.both(lambda e: e.delete_pods(np.array([60, 61], dtype=np.int64)))
        state[[60, 61]] = -1
        sweep()                                                    # deleted rows: nothing to refresh, their words are switched off
        upsert([7, 9, 7], [4_800, 4_801, 4_802])                   # one batch names row 7 twice
        sweep()
    finally:
        tw.close()


# ---- 6. program events -------------------------------------------------------------------------------------------------------
def _retarget_selector(snap, t):
    """Throttle t's first `In` value becomes another value of the same key that some other selector uses: a new selector."""
    op, key, val_off, val = snap.preq.op, snap.preq.key, snap.preq.val_off, snap.preq.val
    g = int(snap.thr_term_off[t])
    for r in range(int(snap.term_preq_off[g]), int(snap.term_preq_off[g + 1])):
        if val_off[r + 1] > val_off[r]:
            mine = int(val[val_off[r]])
            for r2 in range(len(op)):
                if key[r2] == key[r] and val_off[r2 + 1] > val_off[r2] and int(val[val_off[r2]]) != mine:
                    val[val_off[r]] = val[val_off[r2]]
                    return
    raise AssertionError("no other value of the key in any selector")


def test_program_events_rebuild(oracle_mod, monkeypatch):
    """A throttle upsert with a new selector, then a namespace whose labels change: each recompiles the program, each costs one
    build of the table, and the results are right before and after."""
    snap = W.generate(cfg2_scaled(20_011))
    tw = twin_for(snap, monkeypatch)
    try:
        want, _ = tw.step(snap, oracle_mod)
        tw.assert_counters(1, 1)
        compiles = tw.c.compiles()
        t0 = int(responsible_rows(snap)[np.nonzero(want.used.count > 0)[0][0]])  # (a throttle that counts pods now)
        _retarget_selector(snap, t0)
        tw.both(lambda e: e.upsert_throttles(snap.throttle_batch([t0]), rows=np.array([t0], dtype=np.int32)))
        want2, _ = tw.step(snap, oracle_mod)
        assert not np.array_equal(want2.used.count, want.used.count), "the new selector selects the same pods"
        assert tw.c.compiles() == compiles + 1
        tw.assert_counters(2, 2)
        # namespace 3 takes the labels of namespace 4 (same keys, other values: other ClusterThrottles admit it)
        a0, a1, b0, b1 = (int(snap.ns_label_off[k]) for k in (3, 4, 4, 5))
        assert a1 - a0 == b1 - b0 and not np.array_equal(snap.ns_label_pair[a0:a1], snap.ns_label_pair[b0:b1])
        snap.ns_label_pair[a0:a1] = snap.ns_label_pair[b0:b1]
        tw.both(lambda e: e.upsert_namespaces(snap))
        tw.step(snap, oracle_mod)
        assert tw.c.compiles() == compiles + 2
        tw.assert_counters(3, 3)
    finally:
        tw.close()


# ---- 7. ineligible programs --------------------------------------------------------------------------------------------------
def test_lists_of_five_to_eight_words_keep_the_scan(oracle_mod, monkeypatch):
    """A program whose longest namespace list has five to eight words (KT_COUNTER_MATCH_CACHE_PLANES says so) fits the table but
    not the four planes the cached sweep holds in registers: no table is built, no scan is served from one, the results right."""
    n_thr, n_cluster = shape_with_planes(5, 8)
    snap = W.generate(cfg2_scaled(6_007, n_thr=n_thr, n_cluster=n_cluster))
    tw = twin_for(snap, monkeypatch)
    try:
        tw.step(snap, oracle_mod)
        print("index:", tw.c.index_stats(), "planes", tw.c.match_cache_planes())
        assert tw.c.index_stats()["chunks"] == 1 and 5 <= tw.c.match_cache_planes() <= 8, tw.c.match_cache_planes()
        tw.assert_counters(0, 0)
    finally:
        tw.close()


def test_sixteen_dimensions_keep_the_scan(oracle_mod, monkeypatch):
    """A 16-dimension engine on the program of the basic case (one plane): its two-per-CU sweep has no cached instantiation (it
    carried scratch and was never measured to win) — no table, no cached scan, the results right."""
    snap = W.generate(cfg2_scaled(20_011, D=16))
    tw = twin_for(snap, monkeypatch)
    try:
        tw.step(snap, oracle_mod)
        assert tw.c.index_stats()["chunks"] == 1 and 1 <= tw.c.match_cache_planes() <= 4, tw.c.match_cache_planes()
        tw.assert_counters(0, 0)
    finally:
        tw.close()


def test_lists_longer_than_the_planes(oracle_mod, monkeypatch):
    """So many ClusterThrottles that a namespace's word list is longer than kMatchPlanes = 8 (read from the index counters before
    it is relied on): no table, no cached scan, the results right."""
    snap = W.generate(cfg2_scaled(6_007, n_thr=2_300, n_cluster=2_240))
    tw = twin_for(snap, monkeypatch)
    try:
        tw.step(snap, oracle_mod)
        visits = int(E.lib().kt_counter(tw.c._h, COUNTER_NS_WORD_VISITS))
        ns_rows = int(E.lib().kt_counter(tw.c._h, COUNTER_NS_ROWS))
        print("index:", tw.c.index_stats(), "visits", visits, "namespace rows", ns_rows)
        assert ns_rows > 0 and visits >= 9 * ns_rows, "the namespaces do not visit nine words each: the case does not test the cap"
        assert tw.c.match_cache_planes() > 8, tw.c.match_cache_planes()
        tw.assert_counters(0, 0)
    finally:
        tw.close()


def test_multi_chunk_program(oracle_mod, monkeypatch):
    """The configs[4] generator at 20 000 pods x 2 000 throttles: several chunks — the table is for single-chunk programs."""
    c = W.preset(4)
    c.n_pods_total = c.n_pods = 20_000
    c.n_thr, c.n_cluster = 2_000, 1_000
    snap = W.generate(c)
    tw = twin_for(snap, monkeypatch)
    try:
        tw.step(snap, oracle_mod)
        assert tw.c.index_stats()["chunks"] > 1, tw.c.index_stats()
        tw.assert_counters(0, 0)
    finally:
        tw.close()


# ---- 8. paths that do not use the table --------------------------------------------------------------------------------------
def test_other_check_paths_leave_the_table_alone(oracle_mod, monkeypatch):
    """Row-subset checks of 5 and of 300 rows, kt_check of one row and a sweep with the status matrix, once the table exists and
    again directly behind an upsert whose refresh is still pending: right, equal on both engines, and neither a build nor a
    cached scan is counted for them."""
    base = W.generate(cfg2_scaled(9_000))
    n0 = 8_000
    state = np.arange(n0, dtype=np.int64)

    def make():
        e = E.Engine(base.D, max(base.L, 1), n0, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(_permute_pods(base, state), rows=np.arange(n0))
        return e

    tw = Twin(monkeypatch, make)
    rng = np.random.default_rng(5)

    def others(snap):
        o = oracle_mod.Oracle(snap)
        st_w, sm_w = o.check(on_equal=False, nthreads=8)
        for k in (5, 300):
            rows = np.sort(rng.choice(n0, k, replace=False)).astype(np.int64)
            rows[0] = 17  # (the row the upsert below rewrites)
            (st_c, sm_c), (st_u, sm_u) = tw.both(lambda e: e.check(rows=rows, want_status=True))
            np.testing.assert_array_equal(sm_c, sm_w[rows]), np.testing.assert_array_equal(st_c, st_w[rows])
            np.testing.assert_array_equal(sm_u, sm_w[rows]), np.testing.assert_array_equal(st_u, st_w[rows])
            (_, sl_c), (_, sl_u) = tw.both(lambda e: e.check(rows=rows, want_status=False))
            np.testing.assert_array_equal(sl_c, sm_w[rows]), np.testing.assert_array_equal(sl_u, sm_w[rows])
        one = np.array([17], dtype=np.int64)
        (_, s1_c), (_, s1_u) = tw.both(lambda e: e.check_atomic(rows=one, want_status=False))
        np.testing.assert_array_equal(s1_c, sm_w[one]), np.testing.assert_array_equal(s1_u, sm_w[one])
        (st_c, sm_c), (st_u, sm_u) = tw.both(lambda e: e.check(n=n0, want_status=True))
        np.testing.assert_array_equal(st_c, st_w), np.testing.assert_array_equal(sm_c, sm_w)
        np.testing.assert_array_equal(st_u, st_w), np.testing.assert_array_equal(sm_u, sm_w)

    try:
        snap = _with_pods(base, state)
        tw.step(snap, oracle_mod)
        tw.assert_counters(1, 1)
        others(snap)
        tw.assert_counters(1, 1)
        state[17] = 8_500  # another namespace, other labels: the refresh of row 17 waits for the next sweep
        tw.both(lambda e: e.upsert_pods(_permute_pods(base, state[[17]]), rows=np.array([17], dtype=np.int64)))
        snap2 = _with_pods(base, state)
        for f in ("thr_used", "thr_calc", "thr_flags", "thr_thrl_flag", "thr_thrl_has"):
            setattr(snap2, f, getattr(snap, f))
        others(snap2)
        tw.assert_counters(1, 1)
        tw.step(snap2, oracle_mod)
        tw.assert_counters(1, 2)
    finally:
        tw.close()
