"""The match cache with SEVERAL planes.  Every kernel of the cache addresses plane k as base + k * stride — the table by
pod_capacity, the gather and the builder's write-through into the countable view by cv.cap + 1, the aggregate's replay by cv.cap + 1
again — and the other modules multiply by a k other than 0 in one static case only.  Here every case runs on a single-chunk
program whose longest namespace word list has 2..4 words (shape_with_planes), with the two edits of test_lists_of_unequal_length:
`bare` (a namespace that keeps the cluster words only) and `gone` (no Namespace object: the namespaced words only) beside the
namespaces with both kinds of words — lists of unequal length inside one tile.

Three comparisons, all exact: the cached engine against its uncached twin on ALL rows (Twin: KT_NO_MATCH_CACHE=1, neither scan
replays; AggTwin: KT_NO_MATCH_CACHE_AGG=1, the aggregate keeps its scan), the cached engine against the oracle, and the counters,
which say which path ran.  Reconciles run without APPLY: the stored status (the oracle's, stored once when the shape is made) and
with it the answer of a sweep stays a function of the pods alone.

Kinds: the configs[2] and configs[3] generators — both compile to the SIMPLE form of the index (matchLabels-style terms of one
or two keys: kt_build_match_cache<false, 2>; configs[3] adds overrides, no other selector) — and `vetoes`: configs[2] with every
third second requirement turned into NotIn, which makes the index rich (kt_index.cpp: has_veto) and the builder
kt_build_match_cache<true, 3>.
"""
import functools

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from test_agg_match_cache_gpu import AggTwin
from test_aggregate_two_per_cu_gpu import COUNTABLE, assert_same_result, cfg2_scaled, countable_rows
from test_engine_gpu import _permute_pods, _rows_of, _with_pods, assert_reconcile_equal, responsible_rows
from test_match_cache_gpu import Twin, _retarget_selector, shape_with_planes

pytestmark = pytest.mark.gpu

NOW = (1767225600, 0)
N_PODS = 6_007   # (about 3 800 countable: several 1 024-record workgroups, the last tile partial; 64 namespaces straddle the tiles)
SPARE = 300      # free rows behind the fed ones
KINDS = {"configs2": (2, False), "configs3": (3, False), "vetoes": (2, True)}
FULL, CLUSTER_ONLY, NAMESPACED_ONLY, NO_LIST = 0, 1, 2, 3  # what a namespace's word list holds


class Shape:
    """The snapshot of one kind with its two edited namespaces, and the pods of its populations."""

    def __init__(self, snap, bare, gone):
        self.snap, self.bare, self.gone = snap, bare, gone
        T, n = snap.n_thr, snap.n_pods
        fl = snap.thr_flags[:T]
        namespaced = ((fl & S.THR_VALID) != 0) & ((fl & S.THR_CLUSTER) == 0)
        has = np.zeros(snap.n_ns, dtype=bool)
        has[snap.thr_ns[:T][namespaced]] = True
        obj = snap.ns_valid[:snap.n_ns] != 0
        self.ns_class = np.where(has & obj, FULL, np.where(obj, CLUSTER_ONLY, np.where(has, NAMESPACED_ONLY, NO_LIST)))
        assert self.ns_class[bare] == CLUSTER_ONLY and self.ns_class[gone] == NAMESPACED_ONLY
        ns, pf = snap.pod_ns[:n], snap.pod_flags[:n]
        self.on = (pf & (COUNTABLE | S.POD_FINISHED)) == COUNTABLE                       # pods that count
        self.off = (pf & (COUNTABLE | S.POD_FINISHED)) == (S.POD_VALID | S.POD_SCHED_MATCH)  # valid pods that do not (unscheduled)
        self.in_ns = {"bare": ns == bare, "gone": ns == gone, "full": self.ns_class[ns] == FULL}
        for k, m in self.in_ns.items():  # (a case whose populations are missing must fail, not skip)
            assert (m & self.on).sum() >= 20 and (m & self.off).sum() >= 5, f"too few pods in `{k}`: {(m & self.on).sum()} on, {(m & self.off).sum()} off"

    def pods(self, where, k, salt=0, on=True):
        """k pods of a population (base pod numbers), taken cyclically from position `salt`: `where` in bare / gone / full"""
        pool = np.nonzero(self.in_ns[where] & (self.on if on else self.off))[0]
        return pool[(salt + np.arange(k)) % len(pool)]

    def klass(self, pods):
        """the list class of base pods (by their namespace), -1 for `no pod`"""
        pods = np.asarray(pods)
        return np.where(pods >= 0, self.ns_class[self.snap.pod_ns[np.where(pods >= 0, pods, 0)]], -1)

    @functools.lru_cache(maxsize=None)
    def feed(self, n0):
        return _permute_pods(self.snap, np.arange(n0))


def make_shape(kind, oracle_mod, lo=2, hi=4, D=8, n_pods=N_PODS):
    preset, vetoes = KINDS[kind]
    n_thr, n_cluster = shape_with_planes(lo, hi, preset)
    snap = W.generate(cfg2_scaled(n_pods, n_thr=n_thr, n_cluster=n_cluster, D=D, preset=preset))
    T = snap.n_thr
    namespaced = np.nonzero((snap.thr_flags[:T] & S.THR_CLUSTER) == 0)[0]
    bare = int(snap.thr_ns[namespaced[0]])
    snap.thr_flags[:T][(snap.thr_ns[:T] == bare) & ((snap.thr_flags[:T] & S.THR_CLUSTER) == 0)] = 0
    gone = int(snap.thr_ns[[t for t in namespaced if int(snap.thr_ns[t]) != bare][0]])
    snap.ns_valid[gone] = 0
    if vetoes:  # every third In that is not the first requirement of its term becomes NotIn (pair atoms only: no pod overflows its atom row)
        first = set(int(r) for r in snap.term_preq_off[:-1])
        later = [r for r in range(len(snap.preq.op)) if r not in first and snap.preq.op[r] == S.OP_IN]
        snap.preq.op[later[::3]] = S.OP_NOT_IN
        assert len(later[::3]) >= 10, "hardly a requirement to negate: the program would stay simple"
    rows = responsible_rows(snap)
    want = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows, nthreads=8)
    snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
    return Shape(snap, bare, gone)


@pytest.fixture(scope="module")
def shapes(oracle_mod):
    """kind -> Shape, made once per module.  READ-ONLY: a case that edits a snapshot makes its own (make_shape)."""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = make_shape(kind, oracle_mod)
        return made[kind]
    return get


def counters(e):
    return e.match_cache_builds(), e.match_cache_agg_scans(), e.match_cache_scans()


def assert_multi_plane(e, lo=2, hi=4):
    """What every case claims of its program, read from the engine after its first scan."""
    stats = e.index_stats()
    assert lo <= e.match_cache_planes() <= hi, f"{e.match_cache_planes()} planes"
    assert 2 <= lo and hi <= 4
    assert stats["chunks"] == 1, stats
    assert stats["word_visits_per_namespace"] != int(stats["word_visits_per_namespace"]), "every namespace visits as many words"


def assert_view_planes_are_the_tables(e):
    """Read behind a cached reconcile (nothing pending, the view's planes valid): record j of the countable view holds, in EVERY
    plane, the table's word of the pod row it lists — zeroes past the end of a list included, which no replay would show (a
    replay stops at the length of the lane's own list).  Returns (table, view planes, pod row of every record)."""
    mw, _ = e.match_planes()
    mx, rows = e.match_planes(view=True)
    assert mx.shape[0] == mw.shape[0] == e.match_cache_planes() and mx.shape[1] > 0
    assert len(np.unique(rows)) == len(rows), "a pod row has two records"
    np.testing.assert_array_equal(mx, mw[:, rows], err_msg="planes of the view's records against the table's words of their rows")
    return mw, mx, rows


def reconcile_all(tw, snap, oracle_mod):
    """A reconcile without APPLY on both engines: against each other on every throttle row, against the oracle on the responsible ones."""
    rows = responsible_rows(snap)
    want = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows, nthreads=8)
    rc, ru = tw.both(lambda e: e.reconcile(NOW, apply=False))
    assert_same_result(rc, ru, snap.n_thr)
    assert_reconcile_equal(_rows_of(rc, rows, snap.D), want, len(rows))
    return want


def sweep_all(tw, snap, oracle_mod, n=None):
    """The lean sweep of rows [0, n) on both engines: the summary words of all rows against each other and against the oracle."""
    n = snap.n_pods if n is None else n
    _, sm_w = oracle_mod.Oracle(snap).check(on_equal=False, want_status=False, nthreads=8)
    (_, sm_c), (_, sm_u) = tw.both(lambda e: e.check(n=n, on_equal=False, want_status=False))
    np.testing.assert_array_equal(sm_c, sm_u, err_msg="summary words: cached against uncached")
    np.testing.assert_array_equal(sm_c, sm_w[:n], err_msg="summary words against the oracle")
    return sm_w


def without_pods_of(snap, ns):
    """`snap` with the pods of namespace ns gone (their rows hold no pod)."""
    src = np.arange(snap.n_pods, dtype=np.int64)
    src[snap.pod_ns[:snap.n_pods] == ns] = -1
    return _with_pods(snap, src)


class Rig:
    """A pair of engines with SPARE free rows behind the n0 fed ones, and the book of which base pod every row holds."""

    def __init__(self, shape, twin_cls, monkeypatch, n0=None, spare=SPARE):
        self.shape, self.base = shape, shape.snap
        base = self.base
        self.n0 = base.n_pods if n0 is None else n0
        self.P = self.n0 + spare
        self.state = np.full(self.P, -1, dtype=np.int64)
        self.state[:self.n0] = np.arange(self.n0)
        batch, n0, P = shape.feed(self.n0), self.n0, self.P

        def make():
            e = E.Engine(base.D, max(base.L, 1), P, max(base.n_thr, 1), max(base.n_ns, 1))
            e.upsert_namespaces(base)
            e.upsert_throttles(base)
            e.upsert_pods(batch, rows=np.arange(n0))
            return e

        self.tw = twin_cls(monkeypatch, make)
        self.reconciles = self.sweeps = 0
        self.agg_replays = True  # (False: the aggregate of this shape keeps its scan and the view has no planes)

    def close(self):
        self.tw.close()

    def snap(self):
        n = int(np.nonzero(self.state >= 0)[0].max()) + 1
        return _with_pods(self.base, self.state[:n]), n

    def upsert(self, rows, pods):
        rows, pods = np.asarray(rows, dtype=np.int64), np.asarray(pods, dtype=np.int64)
        batch = _permute_pods(self.base, pods)
        self.tw.both(lambda e: e.upsert_pods(batch, rows=rows))
        for r, p in zip(rows, pods):  # (in order: the last entry of a row wins)
            self.state[r] = p

    def delete(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        self.tw.both(lambda e: e.delete_pods(rows))
        self.state[rows] = -1

    def reconcile(self, oracle_mod):
        snap, _ = self.snap()
        self.reconciles += 1
        want = reconcile_all(self.tw, snap, oracle_mod)
        if self.agg_replays:
            assert_view_planes_are_the_tables(self.tw.c)
        return want

    def sweep(self, oracle_mod):
        snap, n = self.snap()
        self.sweeps += 1
        return sweep_all(self.tw, snap, oracle_mod, n=n)

    def count_holding(self, where, on=True):
        sh = self.shape
        held = np.where(self.state >= 0, self.state, 0)
        return int(((self.state >= 0) & sh.in_ns[where][held] & (sh.on if on else sh.off)[held]).sum())

    def rows_holding(self, where, k, salt=0, on=True, avoid=()):
        """k rows (ascending from position `salt` of the candidates, cyclically) that hold a pod of the population NOW"""
        sh = self.shape
        held = np.where(self.state >= 0, self.state, 0)
        ok = (self.state >= 0) & sh.in_ns[where][held] & (sh.on if on else sh.off)[held]
        ok[np.asarray(list(avoid), dtype=np.int64)] = False
        cand = np.nonzero(ok)[0]
        assert len(cand) >= k, f"{len(cand)} rows hold a pod of `{where}`, {k} wanted"
        return cand[(salt + np.arange(k)) % len(cand)]


def mixed_batch(rig, salt, n_each=24, appended=3):
    """One pod-event batch that crosses the list lengths in every direction — rows of full-list namespaces take pods of `bare` and
    of `gone`, rows of `bare` and of `gone` take pods of full-list namespaces — interleaved so that every 64 entries of the row
    list hold all three classes, and `appended` new rows behind the last one (one pod of each population in turn)."""
    sh = rig.shape
    a = rig.rows_holding("full", 2 * n_each, salt=salt * 131)
    b = rig.rows_holding("bare", n_each // 2, salt=salt * 7)
    g = rig.rows_holding("gone", n_each // 2, salt=salt * 5)
    rows, pods = [], []
    for i in range(n_each):
        rows += [a[2 * i], a[2 * i + 1]]
        pods += [sh.pods("bare", 1, salt + i)[0], sh.pods("gone", 1, salt + i)[0]]
        if i < len(b):
            rows += [b[i], g[i]]
            pods += [sh.pods("full", 1, 3 * salt + 2 * i)[0], sh.pods("full", 1, 3 * salt + 2 * i + 1)[0]]
    hi = int(np.nonzero(rig.state >= 0)[0].max()) + 1
    for i in range(appended):
        rows.append(hi + i)
        pods.append(sh.pods(("bare", "gone", "full")[i % 3], 1, salt + 50 + i)[0])
    assert len(set(rows)) == len(rows) and len(rows) > 64
    assert_tiles_mix_lengths(sh, pods)
    return rows, pods


def assert_tiles_mix_lengths(shape, pods):
    """Every 64-entry tile of a refresh list (more than one entry long) holds pods of at least two list classes."""
    k = shape.klass(pods)
    for lo in range(0, len(k), 64):
        tile = k[lo:lo + 64]
        assert len(tile) < 2 or len(set(tile.tolist())) >= 2, f"the tile at entry {lo} holds one list class only: {set(tile.tolist())}"


# ---- 1. the aggregate's replay, static (and 6., 7.: the same case on other shapes) --------------------------------------------
def static_case(shape, oracle_mod, monkeypatch, agg_replays=True, lo=2, hi=4):
    snap = shape.snap
    tw = AggTwin(monkeypatch, lambda: E.Engine.for_snapshot(snap, E.VARIANT_INDEXED))
    try:
        for _ in range(3):
            want = reconcile_all(tw, snap, oracle_mod)
        assert_multi_plane(tw.c, lo, hi)
        assert counters(tw.c) == (1, 3 if agg_replays else 0, 0), counters(tw.c)
        if agg_replays:
            mw, _, _ = assert_view_planes_are_the_tables(tw.c)
            assert all(mw[k].any() for k in range(mw.shape[0])), "a plane of the table is empty: nothing of it can go wrong"
        assert tw.u.match_cache_agg_scans() == 0, "KT_NO_MATCH_CACHE_AGG=1 replayed an aggregate"
        # the counts draw on the pods of both edited namespaces: without them the oracle counts less somewhere
        for name, ns in (("bare", shape.bare), ("gone", shape.gone)):
            less = oracle_mod.Oracle(without_pods_of(snap, ns)).reconcile(NOW, rows=responsible_rows(snap), nthreads=8)
            assert (less.used.count < want.used.count).any(), f"no throttle counts a pod of `{name}`"
        views = tw.c.view_builds()
        sm_w = sweep_all(tw, snap, oracle_mod)
        assert counters(tw.c) == (1, 3 if agg_replays else 0, 1), counters(tw.c)
        assert tw.c.view_builds() == views
        assert (sm_w > 1).any(), "no pod matches a throttle: the sweep tests nothing"
    finally:
        tw.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_static_aggregate_replay(kind, shapes, oracle_mod, monkeypatch):
    """Three reconciles of the static snapshot and never a sweep: one build (the gather fills 2..4 planes of the view), every
    aggregate replays; throttles count pods of `bare` and of `gone`; then one sweep replays the table without a build."""
    static_case(shapes(kind), oracle_mod, monkeypatch)


# ---- 2. both orders inside a step ----------------------------------------------------------------------------------------------
def orders_case(shape, order, oracle_mod, monkeypatch, agg_replays=True):
    rig = Rig(shape, Twin, monkeypatch)
    rig.agg_replays = agg_replays
    try:
        before = rig.reconcile(oracle_mod)
        assert_multi_plane(rig.tw.c)
        views = rig.tw.c.view_builds()
        rig.upsert(*mixed_batch(rig, salt=1))
        if order == "sweep-reconcile":
            rig.sweep(oracle_mod)
            after = rig.reconcile(oracle_mod)
        elif order == "reconcile-sweep":
            after = rig.reconcile(oracle_mod)
            rig.sweep(oracle_mod)
        elif order == "sweep-batch-reconcile":
            rig.sweep(oracle_mod)
            rig.upsert(*mixed_batch(rig, salt=2))
            after = rig.reconcile(oracle_mod)
        else:
            rig.reconcile(oracle_mod)
            after = rig.reconcile(oracle_mod)
            rig.sweep(oracle_mod)
        assert not np.array_equal(before.used.count, after.used.count), "the batch changed no count"
        assert counters(rig.tw.c) == (1, rig.reconciles if agg_replays else 0, rig.sweeps), (counters(rig.tw.c), rig.reconciles, rig.sweeps)
        assert counters(rig.tw.u) == (0, 0, 0), "KT_NO_MATCH_CACHE=1 built or used a table"
        assert rig.tw.c.view_builds() == views, "an event batch rebuilt the view"
    finally:
        rig.close()


ORDERS = ["sweep-reconcile", "reconcile-sweep", "sweep-batch-reconcile", "reconcile-reconcile-sweep"]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_both_orders_inside_a_step(kind, order, shapes, oracle_mod, monkeypatch):
    """Behind one pod-event batch that crosses the list lengths, the sweep and the reconcile in either order (the first of them
    refreshes the rows and writes the view's planes through, the other finds nothing pending), a second batch between them, two
    reconciles in a row: one build, every scan replays, the view is never rebuilt."""
    orders_case(shapes(kind), order, oracle_mod, monkeypatch)


# ---- 3. namespace moves across list lengths ------------------------------------------------------------------------------------
DIRECTIONS = {"full-to-bare": ("full", "bare"), "full-to-gone": ("full", "gone"), "bare-to-full": ("bare", "full"), "gone-to-full": ("gone", "full")}
LIST_SIZES = (1, 63, 64, 65, 200)


@pytest.mark.parametrize("kind", ["configs2", "vetoes"])
@pytest.mark.parametrize("direction", list(DIRECTIONS))
def test_moves_across_list_lengths(direction, kind, shapes, oracle_mod, monkeypatch):
    """Refresh lists of 1, 63, 64, 65 and 200 rows: every other entry moves a pod across the list lengths in the case's direction,
    the entries between them put a pod of ANOTHER length into a row of a full-list namespace (the lanes of one tile of the list
    form sit in namespaces with lists of different length: its round counter must still be every lane's list position); a second
    batch moves the pods back.  Behind each batch the sweep and the reconcile, in alternating order."""
    shape = shapes(kind)
    src, dst = DIRECTIONS[direction]
    other = {"full": "gone", "bare": "gone", "gone": "bare"}  # a population of another list length (and not `full`)
    rig = Rig(shape, Twin, monkeypatch)
    try:
        rig.reconcile(oracle_mod)
        assert_multi_plane(rig.tw.c)
        views, step = rig.tw.c.view_builds(), 0
        for size in LIST_SIZES:
            n_move = min((size + 1) // 2, rig.count_holding(src))
            movers = rig.rows_holding(src, n_move, salt=size)
            fillers = rig.rows_holding("full", size - n_move, salt=3 * size, avoid=movers)
            is_mover = [(i + 1) * n_move // size > i * n_move // size for i in range(size)]  # (spread evenly over the list)
            rows = np.empty(size, dtype=np.int64)
            rows[is_mover], rows[np.logical_not(is_mover)] = movers, fillers
            original = rig.state[rows].copy()
            for back in (False, True):
                pods = np.empty(size, dtype=np.int64)
                if not back:  # forth: the movers take pods of `dst`
                    pods[is_mover] = shape.pods(dst, n_move, size)
                    pods[np.logical_not(is_mover)] = shape.pods(other[dst], size - n_move, size)
                else:         # back: the movers take the pods they held before
                    pods[is_mover] = original[is_mover]
                    pods[np.logical_not(is_mover)] = shape.pods(other[src], size - n_move, 2 * size + 1)
                assert (shape.klass(pods[is_mover]) != shape.klass(rig.state[movers])).all(), "a mover keeps its list length"
                if size > 1:
                    assert_tiles_mix_lengths(shape, pods)
                rig.upsert(rows, pods)
                if step % 2 == 0:
                    rig.sweep(oracle_mod), rig.reconcile(oracle_mod)
                else:
                    rig.reconcile(oracle_mod), rig.sweep(oracle_mod)
                step += 1
            np.testing.assert_array_equal(rig.state[movers], original[is_mover])
        # the table the list form of the builder kept current, against the one a fresh engine builds from the pods as they are now
        snap, n = rig.snap()
        fresh = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
        try:
            fresh.reconcile(NOW, apply=False)
            np.testing.assert_array_equal(rig.tw.c.match_planes()[0][:, :n], fresh.match_planes()[0], err_msg="refreshed table against a fresh build")
        finally:
            fresh.close()
        assert counters(rig.tw.c) == (1, rig.reconciles, rig.sweeps), (counters(rig.tw.c), rig.reconciles, rig.sweeps)
        assert counters(rig.tw.u) == (0, 0, 0)
        assert rig.tw.c.view_builds() == views, "a move rebuilt the view"
    finally:
        rig.close()


@pytest.mark.parametrize("first", ["sweep", "reconcile"])
def test_row_named_twice_and_row_deleted_before_any_scan(first, shapes, oracle_mod, monkeypatch):
    """One batch names 36 rows twice with pods of namespaces of different list length — the last entry wins, in the table and in
    the view's planes — and one row is upserted and deleted again before any scan: its listed row holds no pod when the refresh
    runs (every plane of it is 0), it counts nowhere and its summary word is that of an empty row."""
    shape = shapes("configs2")
    rig = Rig(shape, Twin, monkeypatch)
    try:
        before = rig.reconcile(oracle_mod)
        assert_multi_plane(rig.tw.c)
        views = rig.tw.c.view_builds()
        a, b = rig.rows_holding("full", 24, salt=11), rig.rows_holding("bare", 12, salt=3)
        once = rig.rows_holding("full", 6, salt=500, avoid=a)
        # rows of full-list namespaces take a pod of another one, then one of `bare` or `gone`; rows of `bare` one of `gone`, then a full list
        twice_rows = np.concatenate([a, b, once, a, b])
        twice_pods = np.concatenate([shape.pods("full", 24, 5), shape.pods("gone", 12, 5), shape.pods("gone", 6, 30),
                                     [shape.pods(("bare", "gone")[i % 2], 1, 5 + i)[0] for i in range(24)], shape.pods("full", 12, 60)])
        k = shape.klass(twice_pods)
        assert (k[:36] != k[42:]).all(), "the two entries of a row have lists of the same class"
        rig.upsert(twice_rows, twice_pods)
        q = int(rig.rows_holding("full", 1, salt=40, avoid=twice_rows)[0])
        rig.upsert([q], shape.pods("gone", 1, 9))
        rig.delete([q])
        assert rig.state[q] == -1
        np.testing.assert_array_equal(rig.state[np.concatenate([a, b])], twice_pods[42:])
        if first == "sweep":
            rig.sweep(oracle_mod)
            after = rig.reconcile(oracle_mod)
        else:
            after = rig.reconcile(oracle_mod)
            rig.sweep(oracle_mod)
        assert not np.array_equal(before.used.count, after.used.count), "the events changed no count"
        assert not rig.tw.c.match_planes()[0][:, q].any(), "the row that holds no pod kept matched terms"
        assert counters(rig.tw.c) == (1, 2, 1), counters(rig.tw.c)
        assert rig.tw.c.view_builds() == views
    finally:
        rig.close()


def test_planes_past_a_short_list_are_zeroed(shapes, oracle_mod, monkeypatch):
    """Rows of full-list namespaces whose records hold matched terms in the LAST plane move to `bare`, in a batch of their own:
    no lane of the refresh tile has a list as long as the table has planes, the builder's rounds end before the last plane and
    its trailing fill is what zeroes it — in the table and, through the row's record, in the view."""
    shape = shapes("configs2")
    rig = Rig(shape, AggTwin, monkeypatch)
    try:
        rig.reconcile(oracle_mod)
        assert_multi_plane(rig.tw.c)
        _, mx, rows = assert_view_planes_are_the_tables(rig.tw.c)
        last = mx.shape[0] - 1
        movers = rows[(mx[last] != 0) & shape.in_ns["full"][rig.state[rows]]][:40]
        assert len(movers) >= 5, "hardly a record with a match in the last plane"
        rig.upsert(movers, shape.pods("bare", len(movers), 3))
        rig.reconcile(oracle_mod)
        mw, mx, rows = assert_view_planes_are_the_tables(rig.tw.c)
        assert not mw[last, movers].any(), "the list of `bare` is as long as the longest one: the case does not test the trailing fill"
        assert np.isin(movers, rows).all()
        assert counters(rig.tw.c) == (1, 2, 0), counters(rig.tw.c)
    finally:
        rig.close()


# ---- 4. records that appear and disappear --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["configs2", "configs3"])
def test_records_appear_and_disappear(kind, shapes, oracle_mod, monkeypatch):
    """Reconciles only (the planes of the view come through the builder's write-through and through nothing else): pods of all
    three populations become countable (records appended behind cv.n), pods stop counting, a row is deleted and upserted again,
    new rows behind the last one — each followed by its own reconcile, one build, never a view build."""
    shape = shapes(kind)
    rig = Rig(shape, AggTwin, monkeypatch)
    seen = []

    def reconcile():
        seen.append(rig.reconcile(oracle_mod).used.count.copy())
        assert counters(rig.tw.c) == (1, rig.reconciles, 0), (counters(rig.tw.c), rig.reconciles)
        assert rig.tw.u.match_cache_agg_scans() == 0

    try:
        reconcile()
        assert_multi_plane(rig.tw.c)
        views = rig.tw.c.view_builds()
        three = ("bare", "gone", "full")
        # rows whose pods do not count (no record) take pods that do: 66 records appended, a tile and a bit of the refresh list
        rows = np.sort(np.concatenate([rig.rows_holding(w, 60 if w == "full" else 5, on=False) for w in three]))
        pods = np.array([shape.pods(three[i % 3], 1, i)[0] for i in range(len(rows))])
        assert len(rows) > 64 and not shape.on[rig.state[rows]].any()
        assert_tiles_mix_lengths(shape, pods)
        rig.upsert(rows, pods)
        reconcile()
        # pods stop counting: rows of every population take unscheduled pods of another
        rows = np.concatenate([rig.rows_holding(w, 12, salt=7) for w in three])
        pods = np.array([shape.pods(three[(i + 1) % 3], 1, i, on=False)[0] for i in range(len(rows))])
        rig.upsert(rows, pods)
        reconcile()
        # a delete, then an upsert of the same rows with pods of another list length
        rows = np.concatenate([rig.rows_holding(w, 3, salt=20) for w in three])
        rig.delete(rows)
        rig.upsert(rows, [shape.pods(three[(i + 2) % 3], 1, 30 + i)[0] for i in range(len(rows))])
        reconcile()
        # new rows behind the last one
        rig.upsert(rig.n0 + np.arange(9), [shape.pods(three[i % 3], 1, 60 + i)[0] for i in range(9)])
        reconcile()
        # a delete alone: the records stay listed and stop counting
        rig.delete(np.concatenate([rig.rows_holding(w, 4, salt=33) for w in three]))
        reconcile()
        assert rig.tw.c.view_builds() == views, "an event rebuilt the view: the write-through was not what kept the planes current"
        assert all(not np.array_equal(a, b) for a, b in zip(seen, seen[1:])), "an event changed no count"
    finally:
        rig.close()


# ---- 5. the gather with several planes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["configs2", "configs3"])
def test_gather_behind_an_unpatchable_batch(kind, oracle_mod, monkeypatch):
    """test_unpatchable_batch_rebuilds_view_and_planes on the multi-plane shape: a request above everything the packed plan was
    proved for — the view is built again and all its planes are gathered from the table, which the same call refreshed first."""
    shape = make_shape(kind, oracle_mod)  # (its own: the request is edited)
    base = shape.snap
    n0 = N_PODS - 200
    src = int(countable_rows(base)[-1])
    assert src >= n0
    c0 = int(base.pod_ctr_off[src])
    base.ctr_present[c0] |= 1
    base.ctr_req[c0, 0] = int(base.ctr_req[:int(base.pod_ctr_off[base.n_pods]), 0].max()) * 2 + 1
    rig = Rig(shape, AggTwin, monkeypatch, n0=n0, spare=0)
    try:
        rig.reconcile(oracle_mod)
        assert_multi_plane(rig.tw.c)
        views = rig.tw.c.view_builds()
        rig.upsert([17], [src])
        rig.reconcile(oracle_mod)
        assert rig.tw.c.view_builds() == views + 1, "the batch was patched into the view: the case does not test the rebuild"
        assert counters(rig.tw.c) == (1, 2, 0), counters(rig.tw.c)
    finally:
        rig.close()


@pytest.mark.parametrize("kind", ["configs2", "configs3"])
def test_gather_when_the_headroom_runs_out(kind, shapes, oracle_mod, monkeypatch):
    """An engine whose pod_capacity is its number of fed rows: the view's headroom is pod_capacity - cv.n, the rows that do not
    count.  ALL of them become countable in one batch — patched in: the view is full to its last record (record cap - 1 of a
    plane of cap + 1 words) and its planes came through the write-through of a 2 200-row refresh list; then one more row is
    upserted: the batch does not fit, the view is built again and gathered, under the table of the first build."""
    shape = shapes(kind)
    rig = Rig(shape, AggTwin, monkeypatch, spare=0)
    try:
        rig.reconcile(oracle_mod)
        assert_multi_plane(rig.tw.c)
        views = rig.tw.c.view_builds()
        countable = countable_rows(shape.snap)  # (row r holds base pod r: the view lists exactly these)
        idle = np.setdiff1d(np.arange(rig.P), countable)
        assert len(idle) == rig.P - len(countable) and len(idle) > 1_000  # = the headroom
        three = ("bare", "gone", "full")
        pods = np.array([shape.pods(three[i % 3], 1, i // 3)[0] for i in range(len(idle))])
        assert_tiles_mix_lengths(shape, pods)
        rig.upsert(idle, pods)
        rig.reconcile(oracle_mod)
        assert rig.tw.c.view_builds() == views, "a batch of exactly the headroom was not patched in"
        assert counters(rig.tw.c) == (1, 2, 0), counters(rig.tw.c)
        rig.upsert(rig.rows_holding("full", 1, salt=5), shape.pods("bare", 1, 77))  # one pod more than the headroom takes
        rig.reconcile(oracle_mod)
        assert rig.tw.c.view_builds() == views + 1, "the view took a batch beyond its headroom"
        assert counters(rig.tw.c) == (1, 3, 0), counters(rig.tw.c)
    finally:
        rig.close()


@pytest.mark.parametrize("kind", ["configs2", "configs3"])
def test_gather_behind_a_selector_change(kind, oracle_mod, monkeypatch):
    """A throttle whose selector changes: compile, a second build of the table, a new view whose planes are gathered from it."""
    shape = make_shape(kind, oracle_mod)  # (its own: the selector is edited)
    snap = shape.snap
    tw = AggTwin(monkeypatch, lambda: E.Engine.for_snapshot(snap, E.VARIANT_INDEXED))
    try:
        want = reconcile_all(tw, snap, oracle_mod)
        assert_multi_plane(tw.c)
        compiles, views = tw.c.compiles(), tw.c.view_builds()
        t0 = int(responsible_rows(snap)[np.nonzero(want.used.count > 0)[0][0]])
        _retarget_selector(snap, t0)
        tw.both(lambda e: e.upsert_throttles(snap.throttle_batch([t0]), rows=np.array([t0], dtype=np.int32)))
        want2 = reconcile_all(tw, snap, oracle_mod)
        assert not np.array_equal(want2.used.count, want.used.count), "the new selector selects the same pods"
        assert tw.c.compiles() == compiles + 1 and tw.c.view_builds() == views + 1
        assert_multi_plane(tw.c)
        assert counters(tw.c) == (2, 2, 0), counters(tw.c)
    finally:
        tw.close()


def test_table_rebuilt_under_a_valid_view(oracle_mod, monkeypatch):
    """The full build's write-through.  It needs a table that goes void (more than kPatchBatchMax = 65 536 rows upserted between
    two scans) under a view that stays valid (every batch fits the headroom that is left) — and the headroom passes 65 536
    records only in a view of more than 2^20 of them (max(65 536, n / 16)): 1.85 million pods, 68 000 of which change their
    namespace in two batches.  One more build, no view build, and the view's planes are the new table's."""
    shape = make_shape("configs2", oracle_mod, n_pods=1_850_000)
    snap = shape.snap
    n = snap.n_pods
    assert len(countable_rows(snap)) > (1 << 20) + 4_096
    tw = AggTwin(monkeypatch, lambda: E.Engine.for_snapshot(snap, E.VARIANT_INDEXED))
    try:
        tw.both(lambda e: e.reconcile(NOW, apply=False))
        assert_multi_plane(tw.c)
        assert counters(tw.c) == (1, 1, 0), counters(tw.c)
        views = tw.c.view_builds()
        rows = np.arange(0, 27 * 68_000, 27, dtype=np.int64)
        assert rows[-1] < n and 34_000 <= 65_536 < len(rows) < len(countable_rows(snap)) // 16
        snap.pod_ns[rows] = snap.pod_ns[(rows + 1_000) % n]  # (in place: the snapshot is this case's own)
        assert len(set(shape.klass(rows[:64]).tolist())) >= 2
        for part in (rows[:34_000], rows[34_000:]):
            batch = _permute_pods(snap, part)
            tw.both(lambda e: e.upsert_pods(batch, rows=part))
        reconcile_all(tw, snap, oracle_mod)
        assert counters(tw.c) == (2, 2, 0), counters(tw.c)
        assert tw.c.view_builds() == views, "the view was rebuilt: its planes were gathered, not written through by the build"
        assert_view_planes_are_the_tables(tw.c)
    finally:
        tw.close()


# ---- 6. fewer than eight dimensions --------------------------------------------------------------------------------------------
# The cached instantiations are chosen by dt_bucket_ix(D) <= 8: engines of fewer dimensions run them too.  What the counters say
# (DESIGN.md §3): the sweep replays at every D; the aggregate replays only where its two-per-CU form runs, and that form needs
# 512 slabs of packed records inside a slab area cut for 256 slabs of PLAIN records of D dimensions (agg_slab_area_bytes) — at
# D = 5 they fit, at D = 1 and D = 3 they do not: the aggregate keeps its one-per-CU scan there and the table is built for the sweep.
AGG_REPLAYS_AT = {1: False, 3: False, 5: True}


@pytest.mark.parametrize("D", [1, 3, 5])
def test_fewer_than_eight_dimensions(D, oracle_mod, monkeypatch):
    shape = make_shape("configs2", oracle_mod, D=D)
    static_case(shape, oracle_mod, monkeypatch, agg_replays=AGG_REPLAYS_AT[D])
    orders_case(shape, "sweep-reconcile", oracle_mod, monkeypatch, agg_replays=AGG_REPLAYS_AT[D])


# ---- 7. exactly kMatchReplay planes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["configs2", "configs3"])
def test_exactly_four_planes(kind, oracle_mod, monkeypatch):
    """The longest list the cached forms take: every plane the replays hold in registers is in use."""
    static_case(make_shape(kind, oracle_mod, lo=4, hi=4), oracle_mod, monkeypatch, lo=4, hi=4)
