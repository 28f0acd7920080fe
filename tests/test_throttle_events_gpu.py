"""Throttle events on a live engine, scan form by scan form.

tests/test_namespace_events_gpu.py feeds an engine created EMPTY by events and moves Namespace objects between full sweeps; here the
Throttle / ClusterThrottle objects move: thresholds, overrides, selectors, kinds, deletes, returns into the freed row, appended rows
(the row count grows, one row stays empty), one row named three times in a batch, throttle and pod events in one gap.  A throttle
event invalidates more derived state than a namespace event — same_selector decides between an upload of the spec tables and a
recompile; a recompile rebuilds the admission sets, the index and its chunks, the atom rows, both scan views and their view-ordered
copies, the match cache planes and the match-code records; thr_rows_hi sets the width of every per-throttle buffer and of the status
matrix — and every sweep (reconcile(apply), the status matrix, the lean sweep, a few-pod PreFilter before and after it) is held to
the oracle on the state the events have reached.  Every comparison is exact.

The refused feeds (section 3) take their malformed batches from tests/throttle_batches.py and from nowhere else: the list that
tests/test_throttle_batch_cpu.py has run through the validation pass alone."""
import copy

import numpy as np
import pytest

import lived_engine as LE
import throttle_batches as TB
from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from test_engine_gpu import _permute_pods, _rows_of, _with_pods, assert_reconcile_equal, responsible_rows
from test_match_cache_gpu import NOW
from test_match_codes_gpu import CodesTwin, Pool, assert_records
from test_namespace_events_gpu import FORMS

pytestmark = pytest.mark.gpu

THR_SIDE = ("n_thr", "thr_flags", "thr_ns", "thr_spec", "thr_calc", "thr_used", "thr_reserved", "thr_thrl_flag", "thr_thrl_has",
            "thr_status_msgs_fp", "thr_spec_msgs_fp", "thr_ovr_off", "ovr_begin_s", "ovr_begin_ns", "ovr_end_s", "ovr_end_ns", "ovr_flags",
            "ovr_thr", "thr_term_off", "term_flags", "term_preq_off", "term_nreq_off", "preq", "nreq")
TERMS = ("thr_term_off", "term_flags", "term_preq_off", "term_nreq_off", "preq", "nreq")
STATUS_BITS = S.THR_CALC_AT_NONZERO | S.THR_THROTTLED_POD


# ---- the throttle table as a value: one one-row batch per row (None: the row holds nothing) ---------------------------------
def thr_table(snap):
    return [snap.throttle_batch([t]) if snap.thr_flags[t] else None for t in range(snap.n_thr)]


def thr_batch(entries, D, L):
    """A throttles-only batch of these entries, in this order (for kt_upsert_throttles)."""
    return LE._gather_throttles([None if e is None else (e, 0) for e in entries], D, L)


def put_thr_table(snap, table):
    """The snapshot's throttle side becomes ``table`` (new arrays: a snapshot that shares the old ones keeps them)."""
    b = thr_batch(table, snap.D, snap.L)
    for f in THR_SIDE:
        setattr(snap, f, getattr(b, f))
    snap._keep = None


def with_terms(entry, terms_of):
    """``entry`` with the selector terms of ``terms_of``"""
    out = copy.deepcopy(entry)
    for f in TERMS:
        setattr(out, f, copy.deepcopy(getattr(terms_of, f)))
    return out


def terms_key(entry):
    n = int(entry.thr_term_off[1])
    pools = tuple(tuple(np.asarray(x).tobytes() for x in LE.paging._pool_arrays(p)) for p in (entry.preq, entry.nreq))
    return (entry.term_flags[:n].tobytes(), entry.term_preq_off[:n + 1].tobytes(), entry.term_nreq_off[:n + 1].tobytes(), pools)


def with_threshold(entry, v=None, count=None):
    out = copy.deepcopy(entry)
    if v is not None:
        out.thr_spec.v[0] = v
    if count is not None:
        out.thr_spec.count[0] = count
    return out


def with_overrides(entry, windows):
    """``entry`` with these overrides in place of its own: [(begin seconds, end seconds, {dim: value}, pods or None)]"""
    out = copy.deepcopy(entry)
    k = len(windows)
    out.thr_ovr_off = np.array([0, k], np.uint32)
    out.ovr_begin_s = np.array([w[0] for w in windows] or [S.ZERO_TIME_S], np.int64)
    out.ovr_end_s = np.array([w[1] for w in windows] or [S.ZERO_TIME_S], np.int64)
    out.ovr_begin_ns = np.zeros(max(k, 1), np.int32)
    out.ovr_end_ns = np.zeros(max(k, 1), np.int32)
    out.ovr_flags = np.zeros(max(k, 1), np.uint8)
    out.ovr_thr = S.Amounts(k, entry.D)
    for i, w in enumerate(windows):
        out.ovr_thr.set_row(i, w[2], w[3])
    return out


def without_status(entry, reserved=None):
    """``entry`` as a fresh object: no stored status, and this reservation ({dim: value}, pods)"""
    out = copy.deepcopy(entry)
    for tab in (out.thr_used, out.thr_calc, out.thr_reserved):
        tab.set_row(0, {})
    out.thr_flags[0] = int(out.thr_flags[0]) & ~STATUS_BITS
    out.thr_thrl_flag[0] = out.thr_thrl_has[0] = 0
    out.thr_status_msgs_fp[0] = 0
    if reserved is not None:
        out.thr_reserved.set_row(0, *reserved)
    return out


def amounts_row(a, t):
    return tuple(np.array(getattr(a, f)[t]) for f in ("v", "present", "count", "has_count"))


def same_row(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. the generated workload, form by form -------------------------------------------------------------------------------
class Cluster:
    """The model of the test: the generated snapshot, the throttle table and the pod rows as the events have left them, and — with
    an engine — the engine fed by the same events.  Without one (``eng is None``) only the oracle's side runs: the script of events,
    the choice of throttles and that every event is non-vacuous can be looked at on a machine without a GPU."""

    def __init__(self, form, oracle_mod, monkeypatch, gpu=True, n0=2400, P=2600):
        budget, dims, variant = FORMS[form]
        if budget:
            monkeypatch.setenv("KT_CHUNK_BUDGET", str(budget))
        self.form, self.o, self.one_chunk, self.incremental = form, oracle_mod, form == "one-chunk", form == "incremental"
        self.base = base = W.generate(W.small(seed=83, n_pods=2600, n_thr=96, n_cluster=48, D=dims))
        self.pool = copy.copy(base)          # (the pods of the generator, whatever the throttle side becomes)
        self.table = thr_table(base)
        put_thr_table(base, self.table)
        self.n_thr0 = base.n_thr
        self.cap = base.n_thr + 8
        self.n0 = n0
        self.state = np.full(P, -1, dtype=np.int64)
        self.state[:n0] = np.arange(n0)
        self.no_object = {r for r in range(base.n_ns) if not base.ns_valid[r]}
        self.seen, self.at, self.last = [], {}, {}
        self.eng = None
        if gpu:
            self.eng = eng = E.Engine(base.D, max(base.L, 1), P, self.cap, max(base.n_ns, 1), -1, variant)
            eng.upsert_namespaces(base)
            eng.upsert_throttles(base)
            eng.upsert_pods(_permute_pods(base, np.arange(n0)), rows=np.arange(n0))

    def close(self):
        if self.eng is not None:
            self.eng.close()

    # -- the state
    def rows_in_use(self):
        return int(np.nonzero(self.state >= 0)[0].max()) + 1

    def snap(self, state=None):
        return _with_pods(self.base, self.state[:self.rows_in_use()] if state is None else state)

    def matches(self, t, state=None):
        """pod rows the oracle says throttle row t affects (on the stored status as it is)"""
        st, _ = self.o.Oracle(self.snap(state)).check(on_equal=False, nthreads=8)
        col = st[:, t]
        return np.nonzero((col != S.NOT_AFFECTED) & (col != S.ERROR))[0]

    # -- events, on the engine and on the table the oracle's snapshots are made from
    def feed(self, rows, entries):
        if self.eng is not None:
            self.eng.upsert_throttles(thr_batch(entries, self.base.D, self.base.L), rows=np.asarray(rows, np.int32))
        for r, x in zip(rows, entries):
            self.table += [None] * (r + 1 - len(self.table))
            self.table[r] = x
        put_thr_table(self.base, self.table)

    def delete(self, rows):
        if self.eng is not None:
            self.eng.delete_throttles(np.asarray(rows, np.int32))
        for r in rows:
            if r < len(self.table):
                self.table[r] = None
        put_thr_table(self.base, self.table)

    def upsert_pods(self, rows, pods):
        rows, pods = np.asarray(rows, np.int64), np.asarray(pods, np.int64)
        if self.eng is not None:
            self.eng.upsert_pods(_permute_pods(self.pool, pods), rows=rows)
        self.state[rows] = pods

    def delete_pods(self, rows):
        rows = np.asarray(rows, np.int64)
        if self.eng is not None:
            self.eng.delete_pods(rows)
        self.state[rows] = -1

    # -- a few-pod PreFilter of up to 8 rows the changed throttle matches (or matched), on the stored status as it is
    def few(self, event, look, served):
        snap = self.snap()
        _, sm_w = self.o.Oracle(snap).check(on_equal=False, want_status=False, nthreads=8)
        live = [int(r) for r in look if r < len(sm_w) and self.state[r] >= 0][:8]
        assert live, f"{event}: no live row the changed throttle matches"
        if self.eng is None:
            return
        rows = np.array(live, np.int64)
        before = self.eng.few_checks_served()
        _, sm = self.eng.check_atomic(rows=rows, on_equal=False, want_status=False)
        np.testing.assert_array_equal(sm, sm_w[rows], err_msg=f"{event}: a PreFilter of rows {live} on the stored status")
        if served:
            assert self.eng.few_checks_served() == before + 1, f"{event}: the few-pod path was not taken"

    # -- the sweep of the namespace file, and what the event may have cost
    def sweep(self, event=None, thr=None, compiles=None, same_views=False, same_tables=False, look=None):
        """``thr``: the changed throttle row(s); ``compiles``: how many the gap costs (None: not asked); same_views / same_tables:
        no view and no match cache table is built either."""
        eng = self.eng
        if event:  # rows the changed throttles match now, rows the caller adds, rows they matched at the last sweep
            changed = [int(t) for t in np.atleast_1d(thr)]
            look = np.concatenate([self.matches(t) for t in changed] + ([] if look is None else [look]) +
                                  [self.last["matches"](t) for t in changed]).astype(np.int64)
            self.few(event, look, served=False)
        n = self.rows_in_use()
        snap = self.snap()
        o = self.o.Oracle(snap)
        rows = responsible_rows(snap)
        want = o.reconcile(NOW, rows=rows)
        if eng is not None:
            got = eng.reconcile(NOW, apply=True)
            assert_reconcile_equal(_rows_of(got, rows, snap.D), want, len(rows))
        snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
        st_w, sm_w = o.check(on_equal=False, nthreads=8)
        if eng is not None:
            st_g, sm_g = eng.check(n=n, on_equal=False, want_status=True)
            np.testing.assert_array_equal(st_g, st_w)
            np.testing.assert_array_equal(sm_g, sm_w)
            _, sm_lean = eng.check(n=n, on_equal=False, want_status=False)
            np.testing.assert_array_equal(sm_lean, sm_w)
            assert st_g.shape == (n, len(self.table)), (st_g.shape, n, len(self.table))
        self.table = thr_table(snap)   # the stored status is the engine's: the next events carry it
        put_thr_table(self.base, self.table)
        by_row = dict(zip((int(r) for r in rows), range(len(rows))))
        prev = self.last
        col = {t: np.nonzero((st_w[:, t] != S.NOT_AFFECTED) & (st_w[:, t] != S.ERROR))[0] for t in range(st_w.shape[1])}
        self.last = {"want": want, "by_row": by_row, "st": st_w, "sm": sm_w, "n": n, "got": got if eng is not None else None,
                     "matches": lambda t: col.get(int(t), np.zeros(0, np.int64)),
                     "throttled": {t: (int(want.thrl_flag[i]), int(want.thrl_pod[i])) for t, i in by_row.items()}}
        self.seen.append(({t: int(want.used.count[i]) for t, i in by_row.items()}, np.array(sm_w[:self.n0])))
        if event:
            (c0, s0), (c1, s1) = self.seen[-2], self.seen[-1]
            assert c0 != c1 or not np.array_equal(s0, s1), f"{event}: neither used.count nor a summary word moves"
        if eng is not None:
            now = {"compiles": eng.compiles(), "views": eng.view_builds(), "tables": eng.match_cache_builds()}
            if event:
                at = self.at
                if compiles is not None:
                    assert now["compiles"] == at["compiles"] + compiles, f"{event}: {now['compiles'] - at['compiles']} compiles in the gap"
                if compiles:
                    assert now["views"] >= at["views"] + 1, f"{event}: no scan view was built behind a recompile"
                    if self.one_chunk:
                        assert now["tables"] == at["tables"] + 1, f"{event}: {now['tables'] - at['tables']} match cache builds"
                if same_views:
                    assert now["views"] == at["views"], f"{event}: {now['views'] - at['views']} view builds"
                if same_tables:
                    assert now["tables"] == at["tables"], f"{event}: {now['tables'] - at['tables']} match cache builds"
                if self.incremental and compiles is not None:  # (as test_engine_gpu.py::test_incremental_event_path asks it)
                    rescanned = "no scan" not in eng.kernel_name(E.KERNEL_AGGREGATE)
                    assert rescanned == (compiles > 0), f"{event}: the aggregate ran {eng.kernel_name(E.KERNEL_AGGREGATE)!r}"
            self.at.update(now)
            if self.one_chunk:
                assert_records(eng, st_w, self.state[:n] >= 0, snap.pod_ns, no_object=self.no_object)
        if event:
            self.few(event, look, served=True)
        return prev


def pick_throttles(c):
    """By the oracle: ``big`` is the responsible throttle with the most counted pods, ``other`` one of the same kind whose terms
    differ (the one with the most counted pods among those), ``small`` a namespaced Throttle that counts pods."""
    counts, _ = c.seen[-1]
    flags = c.base.thr_flags
    order = sorted(counts, key=lambda t: (-counts[t], t))
    # (no override is active at NOW: the calculated threshold is spec.threshold, an edit of it shows)
    plain = lambda t: same_row(amounts_row(c.last["want"].calc, c.last["by_row"][t]), amounts_row(c.base.thr_spec, t))
    big = next(t for t in order if plain(t))
    kind = int(flags[big]) & S.THR_CLUSTER
    other = next(t for t in order[1:] if (int(flags[t]) & S.THR_CLUSTER) == kind and counts[t] > 0 and counts[t] != counts[big]
                 and terms_key(c.table[t]) != terms_key(c.table[big]))
    small = next(t for t in order if t not in (big, other) and not (int(flags[t]) & S.THR_CLUSTER) and counts[t] > 0)
    return big, other, small


def throttle_events(form, oracle_mod, monkeypatch, gpu=True):
    c = Cluster(form, oracle_mod, monkeypatch, gpu)
    eng = c.eng
    try:
        c.sweep()
        if eng is not None:
            if c.one_chunk:
                assert eng.index_stats()["chunks"] == 1 and eng.match_cache_scans() >= 1, "the cached sweep does not run: the case tests nothing"
            elif form == "several-chunks":
                assert eng.index_stats()["chunks"] > 1
            elif form == "sixteen-dims":
                assert eng.packed_words() > 4, eng.packed_words()
        big, other, small = pick_throttles(c)
        n_thr = c.n_thr0
        orig = {t: copy.deepcopy(c.table[t]) for t in (big, other, small)}
        used = lambda t: amounts_row(c.last["want"].used, c.last["by_row"][t])

        # 1. a threshold edit: big's spec.threshold drops below its used (where big is throttled already: rises above it), the
        #    throttled flags flip
        v, _, cnt, _ = used(big)
        was = c.last["throttled"][big]
        edited = (v // 2, int(cnt) // 2) if was == (0, 0) else (v * 2 + 1, int(cnt) * 2 + 1)
        c.feed([big], [with_threshold(c.table[big], *edited)])
        c.sweep("a threshold edit", big, compiles=0, same_views=True, same_tables=True)
        assert c.last["throttled"][big] != was, f"the threshold edit does not flip a throttled flag of row {big}: {was}"

        # 2. an override whose window contains NOW is added to other, then moved so that NOW falls outside
        v, present, cnt, _ = used(other)
        open_ = c.last["throttled"][other] != (0, 0)   # (throttled now: the override opens it; else it closes it)
        amount = {d: int(v[d]) * 4 + 1000 if open_ else int(v[d]) // 2 for d in range(c.base.D) if (int(present) >> d) & 1}
        pods = int(cnt) * 4 + 10 if open_ else int(cnt) // 2
        plain = c.table[other]
        c.feed([other], [with_overrides(plain, [(NOW[0] - 3600, NOW[0] + 3600, amount, pods)])])
        c.sweep("an override whose window contains now", other, compiles=0)
        c.feed([other], [with_overrides(c.table[other], [(NOW[0] + 3600, NOW[0] + 7200, amount, pods)])])
        c.sweep("the override's window moves behind now", other, compiles=0)

        # 3. a selector swap as two one-row batches; 4. undone in ONE batch naming both rows
        c.feed([big], [with_terms(c.table[big], orig[other])])
        c.feed([other], [with_terms(c.table[other], orig[big])])
        c.sweep("a selector swap between two throttles", [big, other], compiles=1)
        c.feed([big, other], [with_terms(c.table[big], orig[big]), with_terms(c.table[other], orig[other])])
        c.sweep("the swap is undone in one batch", [big, other], compiles=1)

        # 5. a kind change: small becomes a ClusterThrottle with the same terms (the KT_THR_CLUSTER bit alone), and changes back
        as_cluster = copy.deepcopy(c.table[small])
        as_cluster.thr_flags[0] |= S.THR_CLUSTER
        c.feed([small], [as_cluster])
        c.sweep("a Throttle becomes a ClusterThrottle", small, compiles=1)
        back = copy.deepcopy(c.table[small])
        back.thr_flags[0] = int(back.thr_flags[0]) & ~S.THR_CLUSTER
        c.feed([small], [back])
        c.sweep("... and a Throttle again", small, compiles=1)

        # 6. delete_throttles([big]): its column is zero for every pod, `used` of the other rows is untouched
        before = {t: used(t) for t in c.last["by_row"] if t != big}
        edited_big = copy.deepcopy(c.table[big])
        c.delete([big])
        prev = c.sweep("delete_throttles of the throttle with the most counted pods", big, compiles=1)
        assert not c.last["st"][:, big][c.last["st"][:, big] != S.ERROR].any() and big not in c.last["by_row"]
        assert all(same_row(used(t), before[t]) for t in before), "`used` of another row moved"
        if eng is not None:
            assert all(same_row(amounts_row(c.last["got"].used, t), amounts_row(prev["got"].used, t)) for t in before)

        # 7. big returns in its own row: stored status zero, a reservation rides in the batch
        reservation = ({0: 7}, 2)
        c.feed([big], [without_status(edited_big, reservation)])
        if eng is not None:
            assert same_row(amounts_row(eng.fetch_reserved(), big), amounts_row(c.base.thr_reserved, big)), "fetch_reserved() right behind the event"
        c.sweep("the deleted throttle returns in its own row with a reservation", big, compiles=1)
        if eng is not None:
            res = amounts_row(eng.fetch_reserved(), big)
            assert int(res[0][0]) == 7 and int(res[2]) == 2 and same_row(res, amounts_row(c.base.thr_reserved, big)), res

        # 8. an append: copies of big and other in rows n_thr and n_thr + 2 in one batch, row n_thr + 1 stays empty
        c.feed([n_thr, n_thr + 2], [copy.deepcopy(c.table[big]), copy.deepcopy(c.table[other])])
        c.sweep("copies of two throttles are appended, one row stays empty between them", [n_thr, n_thr + 2], compiles=1)
        st = c.last["st"]
        assert st.shape[1] == n_thr + 3 and not st[:, n_thr + 1][st[:, n_thr + 1] != S.ERROR].any()
        assert same_row(used(n_thr), used(big)) and same_row(used(n_thr + 2), used(other)), "a copy's `used` is not its original's"
        if eng is not None:
            assert eng.throttle_rows() == n_thr + 3

        # 9. one batch names big's row three times: other's selector, its own with the edited threshold, its own with the original
        was = c.last["throttled"][big]
        cur = c.table[big]
        own = with_threshold(cur, orig[big].thr_spec.v[0].copy(), int(orig[big].thr_spec.count[0]))
        c.feed([big, big, big], [with_terms(cur, orig[other]), copy.deepcopy(cur), own])
        assert c.table[big] is own
        c.sweep("one batch names a row three times: the last entry wins", big, compiles=1)
        assert c.last["throttled"][big] != was, "the original threshold does not flip a throttled flag back"

        # 10. throttle and pod events in one gap: big's selector changes, four pods it now matches are upserted into rows it used to
        #     match, four arrive in new rows, four leave — then ONE sweep
        old_rows = c.last["matches"](big)
        old_rows = old_rows[old_rows < c.n0]
        c.feed([big], [with_terms(c.table[big], orig[other])])
        spare = np.arange(c.n0, 2600)
        fits = spare[np.isin(np.arange(len(spare)), c.matches(big, state=spare))]
        assert len(old_rows) >= 8 and len(fits) >= 8, (len(old_rows), len(fits))
        c.upsert_pods(old_rows[:4], fits[:4])
        c.upsert_pods(np.arange(c.n0, c.n0 + 4), fits[4:8])
        c.delete_pods(old_rows[4:8])
        c.sweep("a selector change, pod upserts, arrivals and deletes in one gap", big, compiles=1, look=np.arange(c.n0, c.n0 + 4))

        # 11. delete_throttles names an appended row, a never-fed row inside the capacity and big's row twice
        c.delete([n_thr, n_thr + 5, big, big])
        c.sweep("delete_throttles of an appended row, a never-fed row and one row twice", [big, n_thr], compiles=1)
        st = c.last["st"]
        assert st.shape[1] == n_thr + 3 and not st[:, [big, n_thr, n_thr + 1]][st[:, [big, n_thr, n_thr + 1]] != S.ERROR].any()
        assert len(c.seen) == 14
        return c.seen
    finally:
        c.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_throttle_events_between_sweeps(form, oracle_mod, monkeypatch):
    """one-chunk: the match cache and the match-code records in both scans (assert_records after every sweep, one table build per
    recompile); several-chunks (KT_CHUNK_BUDGET=5000): both views and the namespace-ordered copies; sixteen-dims: eight packed
    words; incremental: the maintained partials survive threshold and override events and are rescanned once behind everything in
    same_selector's key.  Every event is non-vacuous by the oracle alone; a threshold or override event costs no compile, no view
    and no table; anything in same_selector's key costs exactly one compile per gap."""
    throttle_events(form, oracle_mod, monkeypatch)


# ---- 2. the record headers of the 15 / 16 / 24-match pods ------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return Pool()


def test_throttle_events_rewrite_the_records(pool, oracle_mod, monkeypatch):
    """The hand-made cluster of test_match_codes_gpu.py at 1025 rows, fed by events.  One of the sixteen c-h16-* leaves: the p-h16 /
    r-h16 pods drop from 16 matching ClusterThrottles (header 0xFF: read the planes) to 15 (the largest record); nine of the
    twenty-four c-h24-* leave in one batch: 15 again; one more ClusterThrottle selecting tier=h15 arrives in a fresh row: the h15
    pods go from 15 to 0xFF; the ten come back in one batch and the appended row is deleted in the same gap: the headers of the
    start.  One compile and one table build per gap, in both engines of the twin."""
    base = copy.copy(pool.snap)
    table = thr_table(base)
    put_thr_table(base, table)
    n = 1025
    rows_of = {"h15": (3, 7), "h16": (5, 9), "h24": (64, 66)}   # first and second tile; in ns1 and ns2
    state = pool.rows(n, {r: pool.of(k, i) for k, rs in rows_of.items() for i, r in enumerate(rs)})
    names = [t["metadata"]["name"] for t in pool.cs.throttles]
    assert len(names) == base.n_thr
    h16 = [i for i, x in enumerate(names) if x.startswith("c-h16-")]
    h24 = [i for i, x in enumerate(names) if x.startswith("c-h24-")]
    h15 = [i for i, x in enumerate(names) if x.startswith("c-h15-")]
    assert (len(h15), len(h16), len(h24)) == (15, 16, 24)
    fresh = base.n_thr

    def make():
        e = E.Engine(base.D, max(base.L, 1), n, base.n_thr + 4, max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(_permute_pods(base, state), rows=np.arange(n))
        return e

    tw = CodesTwin(monkeypatch, make)
    builds, compiles = [0], []

    def sweep():
        nonlocal table
        snap = _with_pods(base, state)
        st_w, sm_w = tw.step(snap, oracle_mod)
        table = thr_table(snap)
        put_thr_table(base, table)
        builds[0] += 1
        assert tw.c.match_cache_builds() == builds[0] and tw.u.match_cache_builds() == builds[0], "one table build per recompile"
        compiles.append((tw.c.compiles(), tw.u.compiles()))
        assert compiles[-1] == (compiles[0][0] + builds[0] - 1, compiles[0][1] + builds[0] - 1), f"one compile per gap: {compiles}"
        hdr, _ = assert_records(tw.c, st_w, np.ones(n, dtype=bool), snap.pod_ns)
        return [[int(hdr[r]) for r in rows_of[k]] for k in ("h15", "h16", "h24")]

    def feed(rows, entries):
        tw.both(lambda e: e.upsert_throttles(thr_batch(entries, base.D, base.L), rows=np.asarray(rows, np.int32)))
        for r, x in zip(rows, entries):
            table.extend([None] * (r + 1 - len(table)))
            table[r] = x
        put_thr_table(base, table)

    def delete(rows):
        tw.both(lambda e: e.delete_throttles(np.asarray(rows, np.int32)))
        for r in rows:
            table[r] = None
        put_thr_table(base, table)

    try:
        assert sweep() == [[15, 15], [0xFF, 0xFF], [0xFF, 0xFF]]
        start = [copy.deepcopy(x) for x in table]
        delete(h16[7:8])
        assert sweep() == [[15, 15], [15, 15], [0xFF, 0xFF]]
        delete(h24[3:12])
        assert sweep() == [[15, 15], [15, 15], [15, 15]]
        feed([fresh], [copy.deepcopy(table[h15[0]])])
        assert sweep() == [[0xFF, 0xFF], [15, 15], [15, 15]]
        assert tw.c.throttle_rows() == fresh + 1
        back = h16[7:8] + h24[3:12]
        feed(back, [without_status(start[t]) for t in back])   # everything back in one batch ...
        delete([fresh])                                        # ... and the appended row emptied in the same gap
        assert sweep() == [[15, 15], [0xFF, 0xFF], [0xFF, 0xFF]]
    finally:
        tw.close()


# ---- 3. refused feeds ------------------------------------------------------------------------------------------------------
def test_refused_throttle_feeds_leave_the_engine_as_it_was(oracle_mod, monkeypatch):
    """Every malformed batch of tests/throttle_batches.py (the list the CPU test has run through the validation pass alone), a batch
    whose LAST entry names row `capacity` behind valid entries that would change the throttle with the most counted pods, a delete
    that names that row and row `capacity`, and kt_load_snapshot refused three ways — a pod with L + 1 labels, a throttle whose
    `used` lies beyond 2^60, a snapshot larger than the capacity.  After each: the code and the text, no compile, no view, no table,
    the check that was pending is still fetchable and is the oracle's matrix of the unchanged state (the refusals return before
    anything marks results stale), fetch_reserved() as before; at the end one full sweep equals the oracle with no compile."""
    c = Cluster("one-chunk", oracle_mod, monkeypatch)
    eng = c.eng
    try:
        c.sweep()
        big, other, small = pick_throttles(c)
        n, cap = c.last["n"], c.cap
        st_w, sm_w = c.last["st"], c.last["sm"]
        counters = lambda: (eng.compiles(), eng.view_builds(), eng.match_cache_builds())
        eng.check_launch(n, want_status=True)
        at = counters()
        reserved = LE._amounts(eng.fetch_reserved(), eng.throttle_rows())
        assert c.base.n_ns >= 2

        def refused(what, call, code, text):
            with pytest.raises(E.EngineError) as err:
                call()
            assert err.value.code == code and text in str(err.value), f"{what}: {err.value}"
            assert counters() == at, f"{what}: compiles, view builds, match cache builds {counters()}, {at} before"
            try:   # still pending, and the answer of the unchanged state
                st_g, sm_g = eng.check_fetch(n, want_status=True)
            except E.EngineError as gone:
                raise AssertionError(f"{what}: the check that was pending is not fetchable any more: {gone}")
            np.testing.assert_array_equal(st_g, st_w, err_msg=what)
            np.testing.assert_array_equal(sm_g, sm_w, err_msg=what)
            eng.check_launch(n, want_status=True)
            assert counters() == at, f"{what}: the relaunched check compiled or built something"
            assert LE.same(LE._amounts(eng.fetch_reserved(), eng.throttle_rows()), reserved), f"{what}: fetch_reserved() moved"

        for name in TB.MALFORMED_NAMES:
            batch, rows, code, text = TB.malformed(name, D=c.base.D, rows=(big, other, small), throttle_capacity=cap,
                                                   namespace_capacity=max(c.base.n_ns, 1))
            refused(name, lambda: eng.upsert_throttles(batch, rows=rows), code, text)
        tight = with_threshold(c.table[big], c.table[big].thr_spec.v[0] // 1000, 0)
        refused("a batch whose last entry names row `capacity`",
                lambda: eng.upsert_throttles(thr_batch([tight, with_terms(c.table[other], c.table[big]), c.table[small]], c.base.D, c.base.L),
                                             rows=np.array([big, other, cap], np.int32)), -2, f"throttle row {cap}")
        refused("delete_throttles([big, capacity])", lambda: eng.delete_throttles(np.array([big, cap], np.int32)), -2, f"throttle row {cap}")
        # kt_load_snapshot, refused: the snapshots hold OTHER pods and throttles than the engine (a load that went halfway shows)
        small_world = W.generate(W.small(seed=84, n_pods=300, n_thr=40, n_cluster=20, D=c.base.D))
        wide = copy.copy(small_world)
        for f in ("pod_label_off", "pod_label_key", "pod_label_pair"):
            setattr(wide, f, getattr(wide, f).copy())
        extra = c.base.L + 1 - int(wide.pod_label_off[1] - wide.pod_label_off[0])   # the first pod gets L + 1 labels
        assert extra > 0
        wide.pod_label_key = np.insert(wide.pod_label_key, 0, [1] * extra).astype(np.uint32)
        wide.pod_label_pair = np.insert(wide.pod_label_pair, 0, [1] * extra).astype(np.uint32)
        wide.pod_label_off[1:] += np.uint32(extra)
        wide._keep = None
        refused("load_snapshot: a pod with L + 1 labels", lambda: eng.load_snapshot(wide), -2, f"pod 0 has {c.base.L + 1} labels")
        heavy = copy.copy(small_world)
        heavy.thr_used = small_world.thr_used.copy()
        heavy.thr_used.v[heavy.n_thr - 1, 0] = TB.BEYOND
        heavy.thr_used.present[heavy.n_thr - 1] |= np.uint32(1)
        heavy._keep = None
        refused("load_snapshot: a throttle's used beyond 2^60", lambda: eng.load_snapshot(heavy), -4,
                f"throttle {heavy.n_thr - 1}: status.used / reserved beyond 2^60")
        large = W.generate(W.small(seed=85, n_pods=64, n_thr=c.cap + 1, n_cluster=20, D=c.base.D))
        refused("load_snapshot: more throttles than the capacity", lambda: eng.load_snapshot(large), -2, "larger than the configured capacity")
        # one full sweep: the oracle on the unchanged state, no compile
        st_g, sm_g = eng.check_fetch(n, want_status=True)
        np.testing.assert_array_equal(st_g, st_w)
        before = len(c.seen)
        c.sweep()
        assert len(c.seen) == before + 1 and c.seen[-1][0] == c.seen[-2][0] and np.array_equal(c.seen[-1][1], c.seen[-2][1])
        assert eng.compiles() == at[0], "the sweep behind the refused calls compiled"
    finally:
        c.close()


# ---- 4. pending results across a throttle event ----------------------------------------------------------------------------
def _code(f):
    try:
        f()
    except E.EngineError as err:
        return err.code
    return 0


# what is launched in front of the event: name -> (the battery's keys it answers, the throttle whose append carries the row count of
# the `grow` layout across 1024 and moves them)
PENDING = {"headroom": ([("headroom", LE.CAP, False)], "c-none"),
           "forecast-and-preempt": ([("forecast", False), ("preempt", False, False)], "c-none"),
           "admit_gangs": ([("admit_gangs", False)], "c-y"),
           "check-and-reconcile": ([("check", False)], "c-none")}


@pytest.mark.parametrize("layout", [None, "grow"], ids=["threshold-edit", "append-across-1024"])
@pytest.mark.parametrize("what", list(PENDING))
def test_pending_results_across_a_throttle_event(what, layout, oracle_mod):
    """kt_engine.h: behind an accepted throttle event kt_check_fetch and kt_reconcile_fetch answer KT_ERR_NOT_READY, and a pending
    query result answers the exact state at its launch or KT_ERR_NOT_READY, never anything else.  The engine's result slots do not
    hold all queries at once (a headroom launch drops a pending forecast and preempt result, an admission takes the check slot and
    drops all three), so each group is launched in a life of its own, in front of an event that moves its answer: a threshold edit
    (ns1/t-job drops from 1700m to 100m of cpu in front of the first reconcile; no compile), or — on the layout `grow` of lived_engine.Layout, 1100 rows of capacity, the rows in use ending at 1023 — an
    append that carries the row count across 1024, so that every per-throttle buffer is reallocated behind the pending result.
    "The state at launch" is the battery of the hold in front of the launch: the live engine's bytes, equal to those of a twin
    loaded fresh from the mirror and to the host models.  Behind the event everything is launched again and held the same way."""
    keys, appended = PENDING[what]
    life = LE.Life(oracle_mod, gpu=True, layout=None if layout is None else LE.Layout(layout, "holes"))
    try:
        if layout is None:   # (nothing reconciled yet: PreFilter reads spec.threshold, so a threshold edit alone moves every answer)
            life.hold("start, nothing reconciled yet")
        else:
            LE.start(life)
        at_launch = life.live_held[-1][1]
        # launches and fetches go to the engine itself, in its own numbering: a stretched life translates on the way in and out
        lay = life.layout
        eng, q = (life.eng, life.q) if lay is None else (life.eng.raw, lay.questions(life.q))
        n, m, k, ng = len(q.pods), len(q.cands), len(LE.INSTANTS), len(q.gang_off) - 1
        outcome = {}

        def fetched(name, fetch, key=None, part=slice(None)):
            try:
                got = LE._answer(fetch)
            except E.EngineError as err:   # (_answer records a refusal as a value: not reached)
                raise AssertionError(f"{name}: {err}")
            if isinstance(got[0], str):
                assert got[1] == -5, f"{name}: {got}"
                outcome[name] = "KT_ERR_NOT_READY"
                return
            assert key is not None, f"{name}: fetchable behind a throttle event: {got}"
            assert LE.same(got, tuple(at_launch[key])[part]), f"{name}: neither the answer of the state at launch nor KT_ERR_NOT_READY: {got}"
            outcome[name] = "the answer of the state at launch"

        if what == "headroom":
            eng.headroom_launch(n, q.pods, LE.CAP)
        elif what == "forecast-and-preempt":
            eng.forecast_launch(q.pods, LE.INSTANTS)
            eng.preempt_launch(q.pods, q.cands, NOW)
        elif what == "admit_gangs":
            eng.admit_gangs_launch(q.gang_rows, q.gang_off)
        else:
            eng.reconcile_launch(NOW, apply=False)
            eng.check_launch(n, q.pods, want_status=True)
        if layout is None:
            t, (_, cpu), mirror = life.pl.initial.index("ns1/t-job"), life.pl.dim("cpu"), life.mirror.snaps[0]
            assert mirror.thr_spec.v[t, cpu] == 170 and life.pl.scales[0]["cpu"] == -2
            mirror.thr_spec.v[t, cpu] = 10   # 1700m -> 100m: less than any job pod of ns1 asks for
            compiles = eng.compiles()
            life.eng.upsert_throttles(mirror.throttle_batch([t]), rows=np.array([t], np.int32))
        else:
            assert eng.throttle_rows() == LE.CHUNK, eng.throttle_rows()
            life.upsert_throttles([life.mirror.n_thr], [appended])
        if what == "headroom":
            limiting = (lambda l: l) if lay is None else lay.limiting
            fetched("headroom", lambda: (lambda copies, l: (copies, limiting(l)))(*eng.headroom_fetch(n)), keys[0])
        elif what == "forecast-and-preempt":
            fetched("forecast", lambda: eng.forecast_fetch(n, k), keys[0])
            fetched("preempt", lambda: eng.preempt_fetch(n, m), keys[1])
        elif what == "admit_gangs":
            fetched("admit_gangs: the gang bytes", lambda: eng.admit_gangs_fetch(ng), keys[0], part=slice(2, 3))
            fetched("admit_gangs: the matrix in the check slot", lambda: eng.check_fetch(len(q.gang_rows), want_status=True))
        else:
            fetched("check", lambda: eng.check_fetch(n, want_status=True))
            fetched("reconcile", eng.reconcile_fetch)
        if layout is not None:
            assert eng.throttle_rows() > LE.CHUNK, "the append does not carry the row count across 1024"
        behind = life.hold(f"{what}: everything launched again behind the event")
        assert LE.differences(behind, at_launch, keys) == keys, f"the event does not move {LE.differences(at_launch, behind, keys)} of {keys}"
        if layout is None:
            assert eng.compiles() == compiles, "a threshold edit compiled"
        print("pending across a throttle event:", what, layout, outcome)
    finally:
        life.close()
