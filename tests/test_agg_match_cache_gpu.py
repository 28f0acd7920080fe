"""The aggregate scan replays the match cache: the two-per-CU form of the packed aggregate (kt_aggregate_bitmap_one) reads, per
record of the countable scan view, the pod's planes of the match cache in VIEW order (ScanView::mx) instead of scanning the
selectors.  The planes are written by two launches: the gather behind a view build, and the table's builder, which stores every
word it writes for a row at the row's record too.

Every case runs two engines fed alike — one as it comes, one under KT_NO_MATCH_CACHE_AGG=1 (the aggregate keeps its scan) — and
compares the reconcile result on ALL throttle rows between them and on the responsible rows with the oracle; the counters say
which path ran: KT_COUNTER_MATCH_CACHE_AGG_SCANS (aggregate launches that replayed), _BUILDS (full builds of the table), _SCANS
(sweeps that replayed) and KT_COUNTER_VIEW_BUILDS.  Reconciles run without APPLY: the stored status, and with it the oracle's
answer for an unchanged cluster, stays what it was.
"""
import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from test_aggregate_two_per_cu_gpu import (COUNTABLE, PODS_PER_WG, assert_same_result, big_cfg, cfg2_scaled,  # noqa: F401 (big_cfg: fixture)
                                           countable_rows, trim_countable)
from test_engine_gpu import _permute_pods, _rows_of, _with_pods, assert_reconcile_equal, responsible_rows
from test_match_cache_gpu import _retarget_selector, shape_with_planes

pytestmark = pytest.mark.gpu

NOW = (1767225600, 0)
SWITCH = "KT_NO_MATCH_CACHE_AGG"
PATCH_BATCH_MAX = 65536  # kPatchBatchMax


class AggTwin:
    """Two engines built by `make` and fed alike: `c` as it comes (the aggregate replays where it can), `u` under
    KT_NO_MATCH_CACHE_AGG=1.  `env`: further switches, set for both."""

    def __init__(self, monkeypatch, make, env=()):
        for k in env:
            monkeypatch.setenv(k, "1")
        monkeypatch.delenv(SWITCH, raising=False)
        self.c = make()
        monkeypatch.setenv(SWITCH, "1")
        self.u = make()
        monkeypatch.delenv(SWITCH, raising=False)
        for k in env:
            monkeypatch.delenv(k, raising=False)
        self.reconciles = 0

    def both(self, f):
        return f(self.c), f(self.u)

    def close(self):
        self.c.close()
        self.u.close()

    def check_results(self, snap, oracle_mod, rc, ru, rows=None):
        rows = responsible_rows(snap) if rows is None else rows
        want = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows, nthreads=8)
        assert_same_result(rc, ru, snap.n_thr)
        assert_reconcile_equal(_rows_of(rc, rows, snap.D), want, len(rows))
        return want

    def reconcile(self, snap, oracle_mod):
        rc, ru = self.both(lambda e: e.reconcile(NOW, apply=False))
        self.reconciles += 1
        return self.check_results(snap, oracle_mod, rc, ru)

    def assert_counters(self, builds, agg_scans, sweeps=0):
        got = (self.c.match_cache_builds(), self.c.match_cache_agg_scans(), self.c.match_cache_scans())
        assert got == (builds, agg_scans, sweeps), f"cached engine: (builds, aggregate replays, sweep replays) = {got}, expected {(builds, agg_scans, sweeps)}"
        assert self.u.match_cache_agg_scans() == 0, "KT_NO_MATCH_CACHE_AGG=1 replayed an aggregate"


def twin_for(snap, monkeypatch, variant=E.VARIANT_INDEXED, env=()):
    return AggTwin(monkeypatch, lambda: E.Engine.for_snapshot(snap, variant), env)


# ---- 1. parity, and 8. an engine that only ever reconciles -------------------------------------------------------------------
@pytest.mark.parametrize("preset", [2, 3], ids=["configs2-simple", "configs3-rich"])
def test_parity_reconcile_only(preset, oracle_mod, monkeypatch):
    """66 037 pods x 48 throttles (the last tile is partial; preset 3: vetoes and run masks), three reconciles and never a sweep:
    one build of the table, every aggregate replays, no sweep is counted; the other engine never replays and builds no table."""
    snap = W.generate(cfg2_scaled(66_037, preset=preset))
    tw = twin_for(snap, monkeypatch)
    try:
        for _ in range(3):
            want = tw.reconcile(snap, oracle_mod)
        tw.assert_counters(1, 3, 0)
        assert tw.u.match_cache_builds() == 0, "the uncached aggregate built a table no sweep asked for"
        assert tw.c.index_stats()["chunks"] == 1 and tw.c.aggregate_workgroups() == tw.u.aggregate_workgroups()
        assert (want.used.count > 0).any() and (want.used.v != 0).any(), "nothing matched: the case tests nothing"
    finally:
        tw.close()


# ---- 2. a wave's second tile -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_countable", [512 * PODS_PER_WG, 512 * PODS_PER_WG + 1], ids=["512-workgroups", "second-tile"])
def test_second_tile_of_a_wave(n_countable, big_cfg, oracle_mod, monkeypatch):
    """Exactly 512 workgroups x 1024 records, and one record more: every workgroup then owns 17 tiles and its first wave takes a
    second one."""
    snap = W.generate(W.WorkloadCfg.from_buffer_copy(big_cfg))
    trim_countable(snap, n_countable)
    tw = twin_for(snap, monkeypatch)
    try:
        tw.reconcile(snap, oracle_mod)
        tw.assert_counters(1, 1)
        assert tw.c.aggregate_workgroups() > 256
    finally:
        tw.close()


# ---- 3. empty and tiny views -------------------------------------------------------------------------------------------------
def test_empty_and_tiny_views(oracle_mod, monkeypatch):
    """No countable pod at all (the view has no record: nothing may be read), then ONE pod becomes countable (its record is
    appended: a view of one record, 15 of the workgroup's 16 waves own no tile), then a view built for exactly one."""
    snap = W.generate(cfg2_scaled(3_000))
    keep = countable_rows(snap)[:1]
    trim_countable(snap, 0)
    tw = twin_for(snap, monkeypatch)
    try:
        want = tw.reconcile(snap, oracle_mod)
        assert not (want.used.count > 0).any()
        snap.pod_flags[keep] |= np.uint32(S.POD_SCHEDULED)
        tw.both(lambda e: e.upsert_pods(_permute_pods(snap, keep), rows=keep.astype(np.int64)))
        before = tw.c.match_cache_agg_scans()
        want = tw.reconcile(snap, oracle_mod)
        assert (want.used.count > 0).any(), "the one countable pod matches no throttle"
        assert tw.c.match_cache_agg_scans() == before + 1 and tw.c.match_cache_builds() == 1
    finally:
        tw.close()
    tw = twin_for(snap, monkeypatch)  # (exactly one countable pod from the start)
    try:
        tw.reconcile(snap, oracle_mod)
        tw.assert_counters(1, 1)
    finally:
        tw.close()


# ---- 4. pod events -----------------------------------------------------------------------------------------------------------
def test_pod_events_one_batch_each(oracle_mod, monkeypatch):
    """One batch, then a reconcile, for each: listed pods whose labels and namespace change (same record, new planes), pods that
    become countable (appended records, new positions), pods that stop counting, a delete, a delete followed by an upsert of the
    row, a batch that names a row twice.  Every aggregate replays and the table is built once: the rows are refreshed by the list
    form of the builder, which writes the view's planes through."""
    base = W.generate(cfg2_scaled(5_000))
    flags = base.pod_flags[:base.n_pods]
    src_on = np.nonzero((flags & (COUNTABLE | S.POD_FINISHED)) == COUNTABLE)[0]
    src_off = np.nonzero((flags & (COUNTABLE | S.POD_FINISHED)) == (S.POD_VALID | S.POD_SCHED_MATCH))[0]
    assert len(src_on) > 2_500 and len(src_off) > 40
    P, n0 = 4_300, 4_000
    state = np.full(P, -1, dtype=np.int64)
    state[:n0] = np.arange(n0)
    state[100:110] = src_off[:10]    # rows that hold pods which do not count (no record) ...
    state[200:210] = src_on[-10:]    # ... and rows that hold counted ones
    later_on, later_off = src_on[-40:-10], src_off[10:40]

    def make():
        e = E.Engine(base.D, max(base.L, 1), P, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(_permute_pods(base, state[:n0]), rows=np.arange(n0))
        return e

    tw = AggTwin(monkeypatch, make)
    seen = []

    def reconcile():
        n = int(np.nonzero(state >= 0)[0].max()) + 1
        want = tw.reconcile(_with_pods(base, state[:n]), oracle_mod)
        tw.assert_counters(1, tw.reconciles)
        seen.append(want.used.count.copy())

    def upsert(rows, pods):
        rows, pods = np.asarray(rows, dtype=np.int64), np.asarray(pods, dtype=np.int64)
        tw.both(lambda e: e.upsert_pods(_permute_pods(base, pods), rows=rows))
        for r, p in zip(rows, pods):  # (in order: the last entry of a row wins)
            state[r] = p

    try:
        reconcile()
        views = tw.c.view_builds()
        upsert(np.arange(200, 210), later_on[:10])                  # listed pods: other labels, namespaces, requests
        reconcile()
        upsert(np.arange(100, 105), later_on[10:15])                # pods that become countable: appended records
        reconcile()
        upsert([n0, n0 + 1, n0 + 2], later_on[15:18])               # new rows behind the last one
        reconcile()
        upsert(np.arange(205, 210), later_off[:5])                  # pods that stop counting
        reconcile()
        gone = np.arange(300, 330, dtype=np.int64)
        tw.both(lambda e: e.delete_pods(gone))
        state[gone] = -1
        reconcile()                                                 # a delete
        tw.both(lambda e: e.delete_pods(np.array([50], dtype=np.int64)))
        state[50] = -1
        upsert([50], later_on[18:19])                               # a delete, then an upsert of the same row
        reconcile()
        upsert([7, 105, 7, 105], [later_on[20], later_off[6], later_on[21], later_on[22]])  # rows named twice (105: appended once)
        reconcile()
        assert tw.c.view_builds() == views, "an event rebuilt the view: the write-through was not what kept the planes current"
        assert sum(not np.array_equal(a, b) for a, b in zip(seen, seen[1:])) >= 4, "most events changed no count"
    finally:
        tw.close()


# ---- 5. the table goes void --------------------------------------------------------------------------------------------------
def test_more_pending_rows_than_a_refresh_takes(oracle_mod, monkeypatch):
    """More than kPatchBatchMax upserted rows between two reconciles (two batches): the table is void and is built again, the
    view has outgrown its headroom and is built again — its planes are gathered from the new table."""
    base = W.generate(cfg2_scaled(70_000))
    n = base.n_pods
    state = np.arange(n, dtype=np.int64)
    tw = AggTwin(monkeypatch, lambda: E.Engine.for_snapshot(base, E.VARIANT_INDEXED))
    try:
        tw.reconcile(base, oracle_mod)
        tw.assert_counters(1, 1)
        half = PATCH_BATCH_MAX // 2 + 500
        for lo in (0, half):  # every row takes the pod of the row 1 000 further on
            rows = np.arange(lo, lo + half, dtype=np.int64)
            state[rows] = (rows + 1_000) % n
            batch = _permute_pods(base, state[rows])
            tw.both(lambda e: e.upsert_pods(batch, rows=rows))
        assert 2 * half > PATCH_BATCH_MAX
        tw.reconcile(_with_pods(base, state), oracle_mod)
        tw.assert_counters(2, 2)
    finally:
        tw.close()


# ---- 6. a batch the views cannot take ----------------------------------------------------------------------------------------
def test_unpatchable_batch_rebuilds_view_and_planes(oracle_mod, monkeypatch):
    """A pod with a request above everything the packed plan was proved for: views_patchable refuses the batch, the next reconcile
    builds the view again and gathers its planes from the table, which the same call refreshed first (no second build)."""
    base = W.generate(cfg2_scaled(9_000))
    n0 = 8_000
    src = int(countable_rows(base)[-1])
    assert src >= n0
    c0 = int(base.pod_ctr_off[src])
    base.ctr_present[c0] |= 1
    base.ctr_req[c0, 0] = int(base.ctr_req[:int(base.pod_ctr_off[base.n_pods]), 0].max()) * 2 + 1
    state = np.arange(n0, dtype=np.int64)

    def make():
        e = E.Engine(base.D, max(base.L, 1), n0, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(_permute_pods(base, state), rows=np.arange(n0))
        return e

    tw = AggTwin(monkeypatch, make)
    try:
        tw.reconcile(_with_pods(base, state), oracle_mod)
        views = tw.c.view_builds()
        state[17] = src
        tw.both(lambda e: e.upsert_pods(_permute_pods(base, state[[17]]), rows=np.array([17], dtype=np.int64)))
        tw.reconcile(_with_pods(base, state), oracle_mod)
        assert tw.c.view_builds() == views + 1, "the batch was patched into the view: the case does not test the rebuild"
        tw.assert_counters(1, 2)
    finally:
        tw.close()


# ---- 7. the program changes --------------------------------------------------------------------------------------------------
def test_selector_change_rebuilds_table_and_planes(oracle_mod, monkeypatch):
    """A throttle whose selector changes: a compile, a second build of the table, a new view with planes of the new program."""
    snap = W.generate(cfg2_scaled(20_011))
    tw = twin_for(snap, monkeypatch)
    try:
        want = tw.reconcile(snap, oracle_mod)
        compiles = tw.c.compiles()
        t0 = int(responsible_rows(snap)[np.nonzero(want.used.count > 0)[0][0]])
        _retarget_selector(snap, t0)
        tw.both(lambda e: e.upsert_throttles(snap.throttle_batch([t0]), rows=np.array([t0], dtype=np.int32)))
        want2 = tw.reconcile(snap, oracle_mod)
        assert not np.array_equal(want2.used.count, want.used.count), "the new selector selects the same pods"
        assert tw.c.compiles() == compiles + 1
        tw.assert_counters(2, 2)
    finally:
        tw.close()


# ---- 9. the other entry points -----------------------------------------------------------------------------------------------
def test_aggregate_then_finalize_and_row_subsets(oracle_mod, monkeypatch):
    """kt_aggregate_launch + kt_finalize_launch (the slab reduction is a launch of its own there), and kt_reconcile_rows_launch
    with a subset of the throttle rows: both replay, both right."""
    snap = W.generate(cfg2_scaled(30_001, preset=3))
    tw = twin_for(snap, monkeypatch)

    def two_calls(e):
        e.aggregate_launch()
        e.finalize_launch(NOW, apply=False)
        return e.reconcile_fetch()

    try:
        rc, ru = tw.both(two_calls)
        tw.check_results(snap, oracle_mod, rc, ru)
        tw.assert_counters(1, 1)
        subset = responsible_rows(snap)[::3].astype(np.int32)
        rc, ru = tw.both(lambda e: e.reconcile_rows(NOW, subset, apply=False))
        want = oracle_mod.Oracle(snap).reconcile(NOW, rows=subset, nthreads=8)
        assert_reconcile_equal(_rows_of(rc, subset, snap.D), want, len(subset))
        assert_reconcile_equal(_rows_of(ru, subset, snap.D), want, len(subset))
        tw.assert_counters(1, 2)
    finally:
        tw.close()


# ---- 10. back to the scan ----------------------------------------------------------------------------------------------------
def _multi_chunk():
    c = W.preset(4)
    c.n_pods_total = c.n_pods = 20_000
    c.n_thr, c.n_cluster = 2_000, 1_000
    return c


@pytest.mark.parametrize("case", ["sixteen-dims", "five-to-eight-words", "multi-chunk", "incremental", "KT_AGG_ONE_PER_CU", "KT_NO_MATCH_CACHE"])
def test_shapes_that_keep_the_scan(case, oracle_mod, monkeypatch):
    """Engines whose aggregate does not run the cached form: the counter does not rise, no table is built for the aggregate's
    sake, and the results are right."""
    variant, env = E.VARIANT_INDEXED, ()
    if case == "sixteen-dims":
        cfg = cfg2_scaled(20_011, D=16)
    elif case == "five-to-eight-words":
        n_thr, n_cluster = shape_with_planes(5, 8)
        cfg = cfg2_scaled(6_007, n_thr=n_thr, n_cluster=n_cluster)
    elif case == "multi-chunk":
        cfg = _multi_chunk()
    else:
        cfg = cfg2_scaled(20_011)
        if case == "incremental":
            variant |= E.VARIANT_INCREMENTAL
        else:
            env = (case,)
    snap = W.generate(cfg)
    tw = twin_for(snap, monkeypatch, variant, env)
    try:
        tw.reconcile(snap, oracle_mod)
        tw.reconcile(snap, oracle_mod)
        tw.assert_counters(0, 0)
        if case == "multi-chunk":
            assert tw.c.index_stats()["chunks"] > 1
    finally:
        tw.close()


def test_overflow_pod_sends_a_cached_engine_back_to_the_scan(oracle_mod, monkeypatch):
    """An engine with room for 12 labels per pod over a program of at most 8 keys keeps 8 atom slots and replays.  Then a pod
    arrives that carries nine labels every one of which is an atom of the program (a key twice, with two values some selector
    names): its atoms do not fit its atom row, it is an overflow pod, the two-per-CU form cannot take it — the aggregate scans
    again and the counter stands still."""
    c = cfg2_scaled(8_000)
    c.K, c.V, c.L = 6, 2, 6  # (six keys with two values each: 48 throttles name all twelve pairs; a pod carries six labels)
    base = W.generate(c)
    named = set(int(v) for v in base.preq.val)  # the pairs some positive requirement names
    lo, flags = base.pod_label_off, base.pod_flags[:base.n_pods]
    keys_of = lambda p: base.pod_label_key[lo[p]:lo[p + 1]]
    pairs_of = lambda p: base.pod_label_pair[lo[p]:lo[p + 1]]
    on = [int(p) for p in countable_rows(base) if not flags[p] & S.POD_FINISHED]
    full = [p for p in on if all(int(x) in named for x in pairs_of(p))]
    assert full, "the generator gives no countable pod whose labels are all named by selectors"
    src = full[0]
    need = 9 - int(lo[src + 1] - lo[src])
    extra = []  # (key, pair) of other pods: named pairs the pod does not carry yet
    for p in on:
        for k, x in zip(keys_of(p), pairs_of(p)):
            if int(x) in named and int(x) not in set(int(y) for y in pairs_of(src)) and int(x) not in [e[1] for e in extra]:
                extra.append((int(k), int(x)))
        if len(extra) >= need:
            break
    assert need >= 1 and len(extra) >= need, (need, len(extra))
    extra = extra[:need]
    one = _permute_pods(base, [src])
    b = S.Snapshot(base.D, 12)
    b.alloc_namespaces(0, 0)
    b.alloc_throttles(0, 0, 0)
    nl, nc = int(one.pod_label_off[1]), int(one.pod_ctr_off[1])
    b.alloc_pods(1, nl + need, nc)
    b.pod_ns[0], b.pod_flags[0] = one.pod_ns[0], one.pod_flags[0]
    b.pod_label_key[:nl], b.pod_label_pair[:nl] = one.pod_label_key[:nl], one.pod_label_pair[:nl]
    b.pod_label_key[nl:nl + need], b.pod_label_pair[nl:nl + need] = [e[0] for e in extra], [e[1] for e in extra]
    b.pod_label_off[1] = nl + need
    b.ctr_init[:nc], b.ctr_present[:nc], b.ctr_req[:nc] = one.ctr_init[:nc], one.ctr_present[:nc], one.ctr_req[:nc]
    b.pod_ctr_off[1] = nc
    b.pod_ovh_present[0], b.pod_ovh[0] = one.pod_ovh_present[0], one.pod_ovh[0]

    def make():
        e = E.Engine(base.D, 12, base.n_pods, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(base)
        return e

    tw = AggTwin(monkeypatch, make)
    try:
        tw.reconcile(base, oracle_mod)
        tw.assert_counters(1, 1)
        row = np.array([int(countable_rows(base)[3])], dtype=np.int64)
        tw.both(lambda e: e.upsert_pods(b, rows=row))
        rc, ru = tw.both(lambda e: e.reconcile(NOW, apply=False))
        assert_same_result(rc, ru, base.n_thr)
        assert tw.c.match_cache_agg_scans() == 1, "the aggregate replayed over an overflow pod"
        assert tw.c.aggregate_workgroups() <= 256
    finally:
        tw.close()
