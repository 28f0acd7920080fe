"""Match-code records: the cached PreFilter sweep replays each pod's matched terms from one 16-byte record (a count and up to 15
codes `list position << 6 | bit`, 0xFF for "more than 15: read the planes") instead of the planes of the match cache.

Twin pattern of test_match_cache_gpu.py: two engines fed alike, `c` as it comes (the sweep replays the records) and `u` under
KT_NO_MATCH_CODES=1 (the sweep replays the planes).  Every case compares the summary word of every row and every reconcile field
between the two and with the oracle, and decodes Engine.match_codes() on the host against Engine.match_planes() and the oracle's
status matrix: the bits of a record are bits of the planes, their number is the number of throttles that affect the pod (what the
planes hold after the run rule: a throttle with several matching terms is reported once), ascending, overflow rows carry 0xFF.

The pods come from one small hand-made cluster (a pool of pod kinds); a case places pool pods into rows with _with_pods:
  ordinary pods of three namespaces; a pod nothing matches; a pod of a namespace that has no Throttle of its own and no label a
  ClusterThrottle admits (a word list shorter than the plane count); a pod of a namespace without a Namespace object;
  pods with exactly 15, 16 and 24 matching ClusterThrottles (ClusterThrottles with one selector each per tier);
  pods all of whose terms of a two- and a three-term throttle match.
The aggregate replays the records too, from a copy in the order of its scan view (match_codes(view=True)): every case compares that
copy with the row table through the view's row list; KT_NO_MATCH_CODES_AGG=1 keeps the aggregate on the planes.
"""
import copy

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from kube_throttler_amd.objects import ClusterState
from test_aggregate_two_per_cu_gpu import assert_same_result, cfg2_scaled
from test_check_cached_full_list_gpu import _tight_matches, _tighten
from test_engine_gpu import _permute_pods, _rows_of, _with_pods, assert_reconcile_equal, responsible_rows
from test_match_cache_gpu import NOW, shape_with_planes

pytestmark = pytest.mark.gpu

SWITCH = "KT_NO_MATCH_CODES"
HEAVY = {"h15": 15, "h16": 16, "h24": 24}  # tier label -> ClusterThrottles that select it


# ---- the pool --------------------------------------------------------------------------------------------------------------
def _pod(name, ns, labels, cpu, mem, node=None):
    p = {"kind": "Pod", "metadata": {"name": name, "namespace": ns, "labels": dict(labels)},
         "spec": {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": cpu, "memory": mem}}}]},
         "status": {"phase": "Running" if node else "Pending"}}
    if node:
        p["spec"]["nodeName"] = node
    return p


def _thr(kind, name, terms, threshold, ns=None):
    md = {"name": name}
    if kind == "Throttle":
        md["namespace"] = ns
    sel = []
    for labels in terms:
        t = {"podSelector": {"matchLabels": dict(labels)}}
        if kind == "ClusterThrottle":
            t["namespaceSelector"] = {"matchLabels": {"env": "prod"}}
        sel.append(t)
    return {"kind": kind, "metadata": md, "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": sel}, "threshold": threshold}}


class Pool:
    """The cluster's snapshot and where its pod kinds sit."""

    def __init__(self):
        cs = ClusterState()
        for ns in ("ns0", "ns1", "ns2"):
            cs.add_namespace(ns, {"env": "prod", "kubernetes.io/metadata.name": ns})
        cs.add_namespace("bare", {"env": "dev"})  # no Throttle of its own, no ClusterThrottle admits it
        self.kinds = {}

        def add(kind, pod):
            self.kinds.setdefault(kind, []).append(len(cs.pods))
            cs.add(pod)

        apps, teams = ("job", "web", "db"), ("x", "y")
        for i in range(96):  # ordinary pods: every (namespace, app, team), pending and running, requests of several sizes
            ns, app, team = f"ns{i % 3}", apps[(i // 3) % 3], teams[(i // 9) % 2]
            add("ordinary", _pod(f"o{i}", ns, {"app": app, "team": team}, f"{100 * (1 + i % 7)}m", f"{64 * (1 + i % 5)}Mi", node="n1" if i % 4 == 0 else None))
        add("nomatch", _pod("nomatch", "ns0", {"app": "none"}, "100m", "64Mi"))
        add("bare", _pod("bare", "bare", {"app": "job", "team": "x"}, "100m", "64Mi"))
        add("ghost", _pod("ghost", "ghost", {"app": "job", "team": "x"}, "100m", "64Mi"))  # (no Namespace object: Error)
        for tier in HEAVY:
            add(tier, _pod(f"p-{tier}", "ns1", {"tier": tier}, "200m", "128Mi"))
            add(tier, _pod(f"r-{tier}", "ns2", {"tier": tier}, "300m", "64Mi", node="n2"))
        add("multi", _pod("multi2", "ns0", {"app": "job", "team": "x", "m": "two"}, "100m", "64Mi"))
        add("multi", _pod("multi3", "ns1", {"app": "web", "team": "y", "m": "three", "z": "1"}, "100m", "64Mi", node="n3"))
        # throttles: per namespace and app, with thresholds around what the pods ask (some verdicts need the comparison)
        for n in range(3):
            for app in apps:
                cs.add(_thr("Throttle", f"t-{app}", [{"app": app}], {"resourceRequests": {"cpu": f"{600 + 300 * n}m", "memory": "1Gi"}}, ns=f"ns{n}"))
            cs.add(_thr("Throttle", "t-team", [{"team": "x"}], {"resourceCounts": {"pod": 3 + n}}, ns=f"ns{n}"))
        for app in apps:
            for team in teams:
                cs.add(_thr("ClusterThrottle", f"c-{app}-{team}", [{"app": app, "team": team}], {"resourceRequests": {"cpu": "2"}, "resourceCounts": {"pod": 40}}))
        # throttles of two and three terms that ALL match one pod (and whose terms match ordinary pods one at a time)
        cs.add(_thr("Throttle", "t-two", [{"m": "two"}, {"app": "job", "team": "x"}], {"resourceCounts": {"pod": 100}}, ns="ns0"))
        cs.add(_thr("ClusterThrottle", "c-three", [{"m": "three"}, {"z": "1"}, {"app": "web", "team": "y"}], {"resourceRequests": {"cpu": "50"}}))
        for tier, k in HEAVY.items():
            for j in range(k):
                cs.add(_thr("ClusterThrottle", f"c-{tier}-{j}", [{"tier": tier}], {"resourceRequests": {"cpu": f"{1 + j % 3}"}, "resourceCounts": {"pod": 10 + j}}))
        self.cs = cs
        self.snap = cs.build().snapshot

    def of(self, kind, i=0):
        return self.kinds[kind][i]

    def rows(self, n, special):
        """state[row] = pool pod: ordinary pods in turn, `special` {row: pool pod} on top (rows at or beyond n are dropped)."""
        o = self.kinds["ordinary"]
        state = np.array([o[(7 * r + r // 64) % len(o)] for r in range(n)], dtype=np.int64)
        for r, p in special.items():
            if r < n:
                state[r] = p
        return state


@pytest.fixture(scope="module")
def pool():
    return Pool()


# ---- the twin --------------------------------------------------------------------------------------------------------------
class CodesTwin:
    def __init__(self, monkeypatch, make, env=None):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        monkeypatch.delenv(SWITCH, raising=False)
        self.c = make()
        monkeypatch.setenv(SWITCH, "1")
        self.u = make()
        monkeypatch.delenv(SWITCH, raising=False)
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)

    def both(self, f):
        return f(self.c), f(self.u)

    def close(self):
        self.c.close()
        self.u.close()

    def step(self, snap, oracle_mod, n=None):
        """reconcile (apply) + sweep on both: every reconcile field and every summary word against each other and the oracle.
        Returns the oracle's status matrix of the sweep."""
        n = snap.n_pods if n is None else n
        rows = responsible_rows(snap)
        o = oracle_mod.Oracle(snap)
        want = o.reconcile(NOW, rows=rows, nthreads=8)
        rc, ru = self.both(lambda e: e.reconcile(NOW, apply=True))
        assert_same_result(rc, ru, snap.n_thr)
        assert_reconcile_equal(_rows_of(rc, rows, snap.D), want, len(rows))
        assert_reconcile_equal(_rows_of(ru, rows, snap.D), want, len(rows))
        snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
        st_w, sm_w = o.check(on_equal=False, want_status=True, nthreads=8)
        (_, sm_c), (_, sm_u) = self.both(lambda e: e.check(n=n, on_equal=False, want_status=False))
        np.testing.assert_array_equal(sm_c, sm_u, err_msg="summary words: records against planes")
        np.testing.assert_array_equal(sm_c, sm_w[:n], err_msg="summary words against the oracle")
        return st_w[:n], sm_w[:n]


def decode(rec, rows):
    """rec: uint8[n, 16] -> (header[n], words[4, n] of the codes, ascending[n]); words and order of the listed rows only"""
    n = rec.shape[0]
    hdr = rec[:, 0].astype(np.int64)
    words = np.zeros((4, n), dtype=np.uint64)
    asc = np.ones(n, dtype=bool)
    for r in rows:
        k = 0 if hdr[r] == 0xFF else int(hdr[r])
        assert k <= 15, f"row {r}: header {hdr[r]}"
        codes = [int(c) for c in rec[r, 1:1 + k]]
        asc[r] = all(a < b for a, b in zip(codes, codes[1:]))
        for c in codes:
            words[c >> 6, r] |= np.uint64(1) << np.uint64(c & 63)
        if hdr[r] != 0xFF:
            assert not rec[r, 1 + k:].any(), f"row {r}: bytes behind the last code"
    return hdr, words, asc


def run_rule(x, lo, hi):
    """kt_match_codes.h: match_run_rule, in Python integers"""
    m = (1 << 64) - 1
    return x & ~(((x | hi) - lo) & m) & m


def assert_records(e, st_w, live, ns_of, expect_overflow=(), rows=None, no_object=()):
    """The records of engine e against its planes and the oracle's status matrix st_w[row, throttle] (live[row]: the row holds a
    pod; ns_of[row]: its namespace row; rows: the rows to look at, default all).  The words a record decodes to are EXACTLY the
    planes' words after the run rule (Engine.match_runs: the word and the run masks of a plane for a namespace).  Rows without a
    pod are gated by the pod's state, as the planes': their records are not looked at.  And the view table is the row table
    through `rows`: every record of the countable scan view is the record of the pod row it lists.
    no_object: namespace rows whose Namespace object is gone while Throttles of their own stay.  Their pods answer Error for
    every throttle (the matrix row is all 255 and names no throttle), but the table still lists the terms of those Throttles their
    labels match — the verdict is gated by the namespace, not by the table.  For them the header is held to the planes instead:
    the number of bits the run rule leaves."""
    runs = {}
    rec, none = e.match_codes()
    assert none is None
    mw, _ = e.match_planes()
    n = len(live)
    assert rec.shape == (mw.shape[1], 16) and mw.shape[1] >= n and mw.shape[0] <= 4
    look = [int(r) for r in (np.arange(n) if rows is None else rows) if live[r]]
    hdr, words, asc = decode(rec[:n], look)
    affected = ((st_w != 0) & (st_w != 255)).sum(axis=1)
    for r in look:
        if int(ns_of[r]) in no_object:
            assert (st_w[r] == 255).all(), f"row {r}: its namespace has no object, the oracle does not answer Error"
            bits = 0
            for k in range(mw.shape[0]):
                key = (int(ns_of[r]), k)
                if key not in runs:
                    runs[key] = e.match_runs(*key)
                w, lo, hi = runs[key]
                bits += bin(run_rule(int(mw[k, r]), lo, hi)).count("1") if w >= 0 else 0
            affected[r] = bits
        if affected[r] > 15:
            assert hdr[r] == 0xFF, f"row {r}: {affected[r]} throttles affect the pod, header {hdr[r]}"
            continue
        assert hdr[r] == affected[r], f"row {r}: header {hdr[r]}, {affected[r]} throttles affect the pod"
        assert asc[r], f"row {r}: codes not ascending"
        for k in range(mw.shape[0]):
            key = (int(ns_of[r]), k)
            if key not in runs:
                runs[key] = e.match_runs(*key)
            w, lo, hi = runs[key]
            want = run_rule(int(mw[k, r]), lo, hi) if w >= 0 else 0
            assert int(words[k, r]) == want, f"row {r}, plane {k}: codes {int(words[k, r]):x}, the plane after the run rule {want:x}"
        assert not words[mw.shape[0]:, r].any(), f"row {r}: a code names a plane the table does not have"
    for r in expect_overflow:
        assert hdr[r] == 0xFF and affected[r] > 15, f"row {r}: header {hdr[r]}, {affected[r]} affected"
    recv, vrows = e.match_codes(view=True)
    assert len(vrows) > 0 and len(np.unique(vrows)) == len(vrows), "a pod row has two records"
    np.testing.assert_array_equal(recv, rec[vrows], err_msg="records of the view against the table's records of their rows")
    return hdr, affected


def make_for(snap):
    return lambda: E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)


def counters(e):
    return e.match_cache_builds(), e.match_cache_scans()


# ---- 1. row counts, the pod kinds, 15 / 16 / 24 matches --------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 257, 321, 1025, 2049])
def test_row_counts_and_overflow_rows(n, pool, oracle_mod, monkeypatch):
    """63 / 64 / 65 rows: a partial tile and a second tile of the TABLE — a sweep of up to 256 rows takes the few-pod form of the
    check, which reads no table: the reconcile's aggregate builds it, the records are decoded, the sweep counter stays 0.  257 and
    321: the smallest cached sweeps, a tile of one row; 1025 and 2049: a second and a third workgroup.  (A wave's second tile:
    test_a_waves_second_tile.)  Row 3: exactly 15 matches (the largest record), row 5: 16 (header 0xFF) in the same tile as
    ordinary pods, the 24-match pod in the tile after it where there is one (else in tile 0), with a second 15-match pod beside
    it; nothing-matches, short-list and no-Namespace pods."""
    nxt = 64 if n > 64 else 40
    special = {3: pool.of("h15"), 5: pool.of("h16"), 9: pool.of("nomatch"), 11: pool.of("bare"), 13: pool.of("ghost"), 17: pool.of("multi", 0),
               19: pool.of("multi", 1), nxt: pool.of("h24"), nxt + 1 if nxt + 1 < n else 41: pool.of("h15", 1),
               130: pool.of("multi", 0), 131: pool.of("multi", 1)}  # (tile 0 falls back to the planes: these two in a tile that replays codes)
    for r, p in ((n - 1, pool.of("h16", 1)), (1000, pool.of("h24", 1)), (1024, pool.of("h15")), (2047, pool.of("h16")), (2048, pool.of("h24"))):
        special.setdefault(r, p)  # (the last row, the rows around the workgroups' boundaries; an earlier entry of a row stays)
    state = pool.rows(n, special)
    snap = _with_pods(pool.snap, state)
    tw = CodesTwin(monkeypatch, make_for(snap))
    try:
        st_w, sm_w = tw.step(snap, oracle_mod)
        scans = 1 if n > 256 else 0
        assert counters(tw.c) == (1, scans) and counters(tw.u) == (1, scans), (counters(tw.c), counters(tw.u))
        assert tw.c.index_stats()["chunks"] == 1 and 1 <= tw.c.match_cache_planes() <= 4
        assert tw.c.match_cache_agg_scans() == 1 and tw.u.match_cache_agg_scans() == 1, "the aggregate did not replay"
        over = [r for r in range(n) if state[r] in pool.kinds["h16"] + pool.kinds["h24"]]
        assert 5 in over and nxt in over and (len(over) >= 3 or n == 65)
        hdr, affected = assert_records(tw.c, st_w, np.ones(n, dtype=bool), snap.pod_ns, expect_overflow=over)
        assert_records(tw.u, st_w, np.ones(n, dtype=bool), snap.pod_ns)  # (the records are kept under the switch too: one library, both sides)
        assert affected[3] == 15 and hdr[3] == 15, (affected[3], hdr[3])
        assert affected[5] == 16 and affected[nxt] == 24, (affected[5], affected[nxt])
        assert affected[9] == 0 and hdr[9] == 0 and sm_w[9] == 0
        assert affected[11] == 0 and hdr[11] == 0, "the pod of the namespace nothing serves"
        assert sm_w[13] == 2, "the pod without a Namespace object is an Error"
        # all terms of the two- and three-term throttles match these pods: reported once, so fewer codes than plane bits
        mw, _ = tw.c.match_planes()
        for r in (17, 19) + ((130, 131) if n > 131 else ()):
            bits = sum(bin(int(mw[k, r])).count("1") for k in range(mw.shape[0]))
            assert hdr[r] == affected[r] < bits, f"row {r}: {hdr[r]} codes, {bits} plane bits, {affected[r]} throttles"
        assert (sm_w > 1).any(), "nobody is throttled: the case tests nothing"
    finally:
        tw.close()


# ---- 2. the tight-match list runs full inside the code loop ----------------------------------------------------------------
def test_more_than_64_tight_matches_in_one_tile(pool, oracle_mod, monkeypatch):
    """Tile 0 holds 64 copies of the pods with the most provably tight matches (test_check_cached_full_list_gpu.py counts them the
    same way): the list passes 64 entries and drains in the middle of the loop over the codes."""
    def tightened(state):  # (thresholds of its own: the pool's are shared)
        s = _with_pods(pool.snap, state)
        s.thr_spec = copy.deepcopy(s.thr_spec)
        _tighten(s, oracle_mod)
        return s

    n = 300
    state = pool.rows(n, {})
    score = _tight_matches(tightened(state), oracle_mod).sum(axis=1)
    top = np.argsort(-score, kind="stable")[:8]
    state[:64] = state[top[np.arange(64) % 8]]
    snap = tightened(state)
    listed = int(_tight_matches(snap, oracle_mod)[:64].sum())
    assert listed > 64, f"only {listed} provably tight matches in tile 0: the list does not run full"
    tw = CodesTwin(monkeypatch, make_for(snap))
    try:
        st_w, _ = tw.step(snap, oracle_mod)
        assert counters(tw.c) == (1, 1)
        assert_records(tw.c, st_w, np.ones(n, dtype=bool), snap.pod_ns)
    finally:
        tw.close()


def test_a_waves_second_tile(oracle_mod, monkeypatch):
    """512 x 1024 + 65 pods of the configs[2] generator: more tiles than the sweep has waves — the first waves take a second tile,
    the last of them a partial one (the records of the first, the 8 192nd and the last tiles are decoded)."""
    snap = W.generate(cfg2_scaled(512 * 1024 + 65))
    n = snap.n_pods
    assert n == 512 * 1024 + 65
    tw = CodesTwin(monkeypatch, make_for(snap))
    try:
        st_w, _ = tw.step(snap, oracle_mod)
        assert counters(tw.c) == (1, 1) and counters(tw.u) == (1, 1)
        live = (snap.pod_flags[:n] & 1) != 0
        assert_records(tw.c, st_w, live, snap.pod_ns, rows=np.concatenate([np.arange(128), np.arange(512 * 1024 - 64, n)]))
    finally:
        tw.close()


# ---- 3. pod events ---------------------------------------------------------------------------------------------------------
def test_pod_events_rewrite_their_records(pool, oracle_mod, monkeypatch):
    """Upserts that change a row's labels (an ordinary row becomes a 16-match row and back, a 15-match row appears), a delete, a
    batch that names a row twice, a pending pod that becomes a running one and back (in and out of the countable view): after each,
    both engines equal the oracle, the records equal a fresh decode against planes and status matrix — and nothing rebuilds the table."""
    base = pool.snap
    P, n0 = 400, 300
    state = np.full(P, -1, dtype=np.int64)
    state[:n0] = pool.rows(n0, {3: pool.of("h15")})

    def make():
        e = E.Engine(base.D, max(base.L, 1), P, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(_permute_pods(base, state[:n0]), rows=np.arange(n0))
        return e

    tw = CodesTwin(monkeypatch, make)
    steps = [0]

    def sweep():
        n = int(np.nonzero(state >= 0)[0].max()) + 1
        snap = _with_pods(base, state[:n])
        st_w, _ = tw.step(snap, oracle_mod, n=n)
        for f in ("thr_used", "thr_calc", "thr_flags", "thr_thrl_flag", "thr_thrl_has"):
            setattr(base, f, getattr(snap, f))
        steps[0] += 1
        assert counters(tw.c) == (1, steps[0]) and counters(tw.u) == (1, steps[0]), (counters(tw.c), counters(tw.u), steps[0])
        return assert_records(tw.c, st_w, state[:n] >= 0, snap.pod_ns)

    def upsert(rows, pods):
        rows, pods = np.asarray(rows, dtype=np.int64), np.asarray(pods, dtype=np.int64)
        tw.both(lambda e: e.upsert_pods(_permute_pods(base, pods), rows=rows))
        for r, p in zip(rows, pods):
            state[r] = p

    try:
        hdr, _ = sweep()
        assert hdr[3] == 15
        upsert([10, 70], [pool.of("h16"), pool.of("h15", 1)])              # other labels in existing rows: an overflow row appears
        hdr, _ = sweep()
        assert hdr[10] == 0xFF and hdr[70] == 15
        upsert([10, n0], [pool.of("ordinary", 5), pool.of("h24")])         # ... and goes; an appended row in a new tile
        hdr, _ = sweep()
        assert hdr[10] != 0xFF and hdr[n0] == 0xFF
        tw.both(lambda e: e.delete_pods(np.array([70], dtype=np.int64)))   # a delete: the record stays behind, the row is off
        state[70] = -1
        sweep()
        upsert([7, 9, 7], [pool.of("h15"), pool.of("nomatch"), pool.of("multi", 0)])  # one batch names row 7 twice: the last wins
        hdr, aff = sweep()
        assert hdr[7] == aff[7] and hdr[9] == 0
        pend, run = pool.of("h15"), pool.of("h15", 1)                      # pending -> running -> pending: in and out of the view
        upsert([20], [pend])
        sweep()
        upsert([20], [run])
        sweep()
        upsert([20], [pend])
        sweep()
    finally:
        tw.close()


# ---- 3b. the aggregate's switch --------------------------------------------------------------------------------------------
def test_aggregate_switch_keeps_the_planes_there(pool, oracle_mod, monkeypatch):
    """KT_NO_MATCH_CODES_AGG=1 on both engines of the twin: the sweep replays codes (on `c`), the aggregate replays planes on both,
    KT_COUNTER_MATCH_CACHE_AGG_SCANS still counts, the results are the oracle's."""
    n = 1025
    state = pool.rows(n, {3: pool.of("h15"), 5: pool.of("h16"), 64: pool.of("h24"), 130: pool.of("multi", 0), 131: pool.of("multi", 1)})
    snap = _with_pods(pool.snap, state)
    tw = CodesTwin(monkeypatch, make_for(snap), env={"KT_NO_MATCH_CODES_AGG": "1"})
    try:
        st_w, _ = tw.step(snap, oracle_mod)
        assert counters(tw.c) == (1, 1) and counters(tw.u) == (1, 1)
        assert tw.c.match_cache_agg_scans() == 1 and tw.u.match_cache_agg_scans() == 1
        assert_records(tw.c, st_w, np.ones(n, dtype=bool), snap.pod_ns, expect_overflow=[5, 64])
    finally:
        tw.close()


# ---- 4. programs without records -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["five-to-eight-planes", "multi-chunk"])
def test_programs_without_records(case, oracle_mod, monkeypatch):
    """A program whose lists have five to eight words, and one of several chunks: no records are used (none can be read), and
    the results equal the twin's and the oracle's."""
    if case == "multi-chunk":
        c = W.preset(4)
        c.n_pods_total = c.n_pods = 6_000
        c.n_thr, c.n_cluster = 2_000, 1_000
        snap = W.generate(c)
    else:
        n_thr, n_cluster = shape_with_planes(5, 8)
        snap = W.generate(cfg2_scaled(6_007, n_thr=n_thr, n_cluster=n_cluster))
    tw = CodesTwin(monkeypatch, make_for(snap))
    try:
        tw.step(snap, oracle_mod)
        if case == "multi-chunk":
            assert tw.c.index_stats()["chunks"] > 1
        else:
            assert 5 <= tw.c.match_cache_planes() <= 8
        assert tw.c.match_cache_scans() == 0
        with pytest.raises(E.EngineError):
            tw.c.match_codes()
    finally:
        tw.close()


# ---- 5. the generated workload: records of longer lists --------------------------------------------------------------------
def test_generated_workload_with_several_planes(oracle_mod, monkeypatch):
    """The configs[2] generator at a shape with two to four planes, 4 099 pods: codes name every list position, and rows with more
    than seven codes exist (the second half of the record)."""
    n_thr, n_cluster = shape_with_planes(2, 4)
    snap = W.generate(cfg2_scaled(4_099, n_thr=n_thr, n_cluster=n_cluster))
    tw = CodesTwin(monkeypatch, make_for(snap))
    try:
        st_w, _ = tw.step(snap, oracle_mod)
        assert counters(tw.c) == (1, 1)
        live = (snap.pod_flags[:snap.n_pods] & 1) != 0
        hdr, _ = assert_records(tw.c, st_w, live, snap.pod_ns)
        rec, _ = tw.c.match_codes()
        used = hdr[live & (hdr != 0xFF)]
        print("codes per row: max", used.max(), "mean", used.mean(), "planes", tw.c.match_cache_planes())
        assert (rec[:snap.n_pods][live & (hdr != 0xFF) & (hdr > 0), 1:] >> 6).max() >= 1, "no code names a list position behind the first"
    finally:
        tw.close()
