"""Namespace events between sweeps, scan form by scan form.

tests/test_queries_after_events_gpu.py follows Namespace events through the admission queries on 40 pods: the few-pod check and the
smallest aggregate.  Here an engine created EMPTY is fed a generated workload of 2 600 pods by events — more than 256 rows, so the
cached sweep runs — and between full sweeps (reconcile(apply), the status matrix and the lean sweep, each against the oracle on the
state the events have reached, as test_engine_gpu.py::test_pod_events_between_sweeps does for pod events) Namespace objects swap
labels, leave and return.  A namespace event marks the program dirty; everything derived has to follow the recompile: the
admission sets cached per throttle, the index and its chunks, the atom rows, both scan views and their view-ordered copies, the
match cache planes and the match-code records, an incremental engine's maintained partials.  Every comparison is exact."""
import copy

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from test_engine_gpu import _permute_pods, _rows_of, _with_pods, assert_reconcile_equal, responsible_rows
from test_match_cache_gpu import NOW
from test_match_codes_gpu import CodesTwin, Pool, assert_records

pytestmark = pytest.mark.gpu


# ---- the namespace table as a value ----------------------------------------------------------------------------------------
def ns_table(snap):
    """[(valid, [(key id, pair id), ...])] per namespace row"""
    return [(int(snap.ns_valid[r]), [(int(snap.ns_label_key[i]), int(snap.ns_label_pair[i]))
                                     for i in range(int(snap.ns_label_off[r]), int(snap.ns_label_off[r + 1]))]) for r in range(snap.n_ns)]


def ns_batch(D, L, entries):
    """A namespaces-only batch of these (valid, labels) entries, in this order (for kt_upsert_namespaces)."""
    b = S.Snapshot(D, L)
    b.alloc_namespaces(len(entries), sum(len(labels) for _, labels in entries))
    b.alloc_pods(0, 0, 0)
    b.alloc_throttles(0, 0, 0)
    n = 0
    for i, (valid, labels) in enumerate(entries):
        b.ns_valid[i] = valid
        for key, pair in labels:
            b.ns_label_key[n], b.ns_label_pair[n] = key, pair
            n += 1
        b.ns_label_off[i + 1] = n
    return b


def put_ns_table(snap, table):
    """The snapshot's namespace side becomes ``table`` (new arrays: a snapshot that shares the old ones keeps them)."""
    b = ns_batch(snap.D, snap.L, table)
    for f in ("ns_valid", "ns_label_off", "ns_label_key", "ns_label_pair"):
        setattr(snap, f, getattr(b, f))
    snap._keep = None


GONE = (0, [])


# ---- 1. the generated workload, form by form -------------------------------------------------------------------------------
FORMS = {"one-chunk": (None, 8, E.VARIANT_INDEXED), "several-chunks": (5000, 8, E.VARIANT_INDEXED),
         "sixteen-dims": (None, 16, E.VARIANT_INDEXED), "incremental": (None, 8, E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)}


@pytest.mark.parametrize("form", list(FORMS))
def test_namespace_events_between_sweeps(form, oracle_mod, monkeypatch):
    """one-chunk: the match cache and the match-code records in both scans (assert_records after every sweep: the records against
    the planes and the oracle's status matrix, the view-ordered copy against the row table; one table build per recompile);
    several-chunks (KT_CHUNK_BUDGET=5000): both views and the namespace-ordered copies; sixteen-dims: eight packed words;
    incremental: only compile_program voids the maintained partials behind a namespace event that no pod event follows.
    Every event is non-vacuous by the oracle alone (used.count or the summary words move), costs one compile, and rebuilds a view."""
    budget, dims, variant = FORMS[form]
    if budget:
        monkeypatch.setenv("KT_CHUNK_BUDGET", str(budget))
    base = W.generate(W.small(seed=83, n_pods=2600, n_thr=96, n_cluster=48, D=dims))
    table = ns_table(base)
    put_ns_table(base, table)
    P, n0 = 2600, 2400
    state = np.full(P, -1, dtype=np.int64)
    state[:n0] = np.arange(n0)
    # the namespace that holds the most counted pods, and one whose labels differ from its
    counted = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED
    running = (base.pod_flags[:n0] & (counted | S.POD_FINISHED)) == counted
    per_ns = np.bincount(base.pod_ns[:n0][running], minlength=base.n_ns)
    big = int(np.argmax(per_ns))
    other = next(r for r in np.argsort(-per_ns) if r != big and table[r][0] and set(table[r][1]) != set(table[big][1]))
    other = int(other)
    one_chunk = form == "one-chunk"
    eng = E.Engine(base.D, max(base.L, 1), P, max(base.n_thr, 1), max(base.n_ns, 1), -1, variant)
    try:
        eng.upsert_namespaces(base)
        eng.upsert_throttles(base)
        eng.upsert_pods(_permute_pods(base, np.arange(n0)), rows=np.arange(n0))
        seen = []      # per sweep: what the oracle says (used.count of the responsible rows, the summary words)
        at = {}

        def sweep(event=None):
            n = int(np.nonzero(state >= 0)[0].max()) + 1
            snap = _with_pods(base, state[:n])
            o = oracle_mod.Oracle(snap)
            rows = responsible_rows(snap)
            want = o.reconcile(NOW, rows=rows)
            got = eng.reconcile(NOW, apply=True)
            assert_reconcile_equal(_rows_of(got, rows, snap.D), want, len(rows))
            snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
            st_w, sm_w = o.check(on_equal=False, nthreads=8)
            st_g, sm_g = eng.check(n=n, on_equal=False, want_status=True)
            np.testing.assert_array_equal(st_g, st_w)
            _, sm_lean = eng.check(n=n, on_equal=False, want_status=False)
            np.testing.assert_array_equal(sm_lean, sm_w)
            for f in ("thr_used", "thr_calc", "thr_flags", "thr_thrl_flag", "thr_thrl_has"):  # the stored status is the engine's
                setattr(base, f, getattr(snap, f))
            seen.append((np.array(want.used.count[:len(rows)]), np.array(sm_w[:n0])))
            now = {"compiles": eng.compiles(), "views": eng.view_builds(), "tables": eng.match_cache_builds()}
            if event:
                (c0, s0), (c1, s1) = seen[-2], seen[-1]
                assert not (np.array_equal(c0, c1) and np.array_equal(s0, s1)), f"{event}: neither used.count nor a summary word moves"
                assert now["compiles"] == at["compiles"] + 1, f"{event}: {now['compiles'] - at['compiles']} compiles in the gap"
                assert now["views"] >= at["views"] + 1, f"{event}: no scan view was built behind a recompile"
                if one_chunk:
                    assert now["tables"] == at["tables"] + 1, f"{event}: {now['tables'] - at['tables']} match cache builds"
            at.update(now)
            if one_chunk:
                assert_records(eng, st_w, state[:n] >= 0, snap.pod_ns, no_object={r for r, x in enumerate(table) if not x[0]})

        def feed(rows, entries):
            """the event on the engine and on the table the oracle's snapshots are made from"""
            eng.upsert_namespaces(ns_batch(base.D, base.L, entries), rows=np.asarray(rows, np.int32))
            for r, x in zip(rows, entries):
                table[r] = x
            put_ns_table(base, table)

        sweep()
        if one_chunk:
            assert eng.index_stats()["chunks"] == 1 and eng.match_cache_scans() >= 1, "the cached sweep does not run: the case tests nothing"
        elif form == "several-chunks":
            assert eng.index_stats()["chunks"] > 1
        elif form == "sixteen-dims":
            assert eng.packed_words() > 4, eng.packed_words()
        mine, theirs = table[big], table[other]
        feed([big], [theirs])                       # a label swap of two namespaces, as two one-row batches with rows=
        feed([other], [mine])
        sweep("a label swap between two namespaces")
        feed([big], [mine])
        feed([other], [theirs])
        sweep("the swap is undone")
        eng.delete_namespaces(np.array([big], np.int32))
        table[big] = GONE
        put_ns_table(base, table)
        sweep("delete_namespaces of the namespace that holds the most counted pods")
        feed([big], [mine])
        sweep("its return")
        eng.delete_namespaces(np.array([big], np.int32))
        table[big] = GONE
        put_ns_table(base, table)
        inside = np.nonzero(base.pod_ns[:n0] == big)[0]
        spare = np.nonzero(base.pod_ns[n0:2600] == big)[0] + n0
        assert len(inside) >= 8 and len(spare) >= 4
        upd, new = inside[:4], np.arange(n0, n0 + 4)  # rows of the namespace take other pods of it, four more arrive, four leave
        state[upd] = spare[:4]
        state[new] = spare[:4][::-1]
        eng.upsert_pods(_permute_pods(base, state[upd]), rows=upd)
        eng.upsert_pods(_permute_pods(base, state[new]), rows=new)
        gone = inside[4:8].astype(np.int64)
        state[gone] = -1
        eng.delete_pods(gone)
        sweep("a delete, then pod upserts and deletes inside that namespace")
        feed([big], [mine])                          # no pod event at all before the next reconcile
        sweep("its return behind the pod events")
        assert len(seen) == 7
    finally:
        eng.close()


# ---- 2. the record headers of the 15 / 16 / 24-match pods ------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return Pool()


def test_namespace_events_rewrite_the_records(pool, oracle_mod, monkeypatch):
    """The hand-made cluster of test_match_codes_gpu.py at 1025 rows, fed by events.  ns1 loses env=prod: its p-h15 / p-h16 / p-h24
    pods drop from 15, 16 and 24 matching ClusterThrottles to none, their record headers from 15, 0xFF and 0xFF to 0, while their
    ns2 siblings keep theirs; ns2 is deleted: its rows answer Error; both return in one batch: the headers of the start."""
    base = copy.copy(pool.snap)
    table = ns_table(base)
    n = 1025
    mine = {3: pool.of("h15"), 5: pool.of("h16"), 64: pool.of("h24")}           # in ns1
    sibling = {7: pool.of("h15", 1), 9: pool.of("h16", 1), 66: pool.of("h24", 1)}  # in ns2
    state = pool.rows(n, {**mine, **sibling})
    assert all(base.pod_ns[p] == 1 for p in mine.values()) and all(base.pod_ns[p] == 2 for p in sibling.values())

    def make():
        e = E.Engine(base.D, max(base.L, 1), n, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(_permute_pods(base, state), rows=np.arange(n))
        return e

    tw = CodesTwin(monkeypatch, make)
    builds = [0]

    def sweep():
        snap = _with_pods(base, state)
        st_w, sm_w = tw.step(snap, oracle_mod)
        for f in ("thr_used", "thr_calc", "thr_flags", "thr_thrl_flag", "thr_thrl_has"):
            setattr(base, f, getattr(snap, f))
        builds[0] += 1
        assert tw.c.match_cache_builds() == builds[0] and tw.u.match_cache_builds() == builds[0], "one table build per recompile"
        hdr, _ = assert_records(tw.c, st_w, np.ones(n, dtype=bool), snap.pod_ns, no_object={r for r, x in enumerate(table) if not x[0]})
        return [int(hdr[r]) for r in mine], [int(hdr[r]) for r in sibling], sm_w

    def feed(rows, entries):
        tw.both(lambda e: e.upsert_namespaces(ns_batch(base.D, base.L, entries), rows=np.asarray(rows, np.int32)))
        for r, x in zip(rows, entries):
            table[r] = x
        put_ns_table(base, table)

    try:
        assert sweep()[:2] == ([15, 0xFF, 0xFF], [15, 0xFF, 0xFF])
        ns1, ns2 = table[1], table[2]
        (env,) = set(table[0][1]) & set(ns1[1]) & set(ns2[1])                   # env=prod: the one pair the three share
        feed([1], [(1, [x for x in ns1[1] if x != env])])
        assert sweep()[:2] == ([0, 0, 0], [15, 0xFF, 0xFF])
        tw.both(lambda e: e.delete_namespaces(np.array([2], np.int32)))
        table[2] = GONE
        put_ns_table(base, table)
        m, s, sm_w = sweep()
        assert m == [0, 0, 0] and all(int(sm_w[r]) & 3 == S.VERDICT_ERROR for r in sibling), (m, s, [int(sm_w[r]) for r in sibling])
        feed([2, 1], [ns2, ns1])
        assert sweep()[:2] == ([15, 0xFF, 0xFF], [15, 0xFF, 0xFF])
    finally:
        tw.close()
