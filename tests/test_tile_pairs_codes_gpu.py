"""Tile pairs of the cached PreFilter sweep on the match-code form (kt_check_bitmap_cached<PL, true>): a wave walks its tiles two at
a time — both 24-byte records requested as one batch, replayed one after the other into ONE tight-match list whose entries name
their tile (`slot << 26 | lane << 20 | term`), drained once per pair; what a lane settled waits in cnt[slot][lane].

Twin pattern of test_match_codes_gpu.py: two engines fed alike, `c` as it comes (pairs) and `u` under KT_NO_TILE_PAIRS_CHECK=1
(singles, the same library).  Every case compares the summary word of every row and every reconcile field between the two and with
the oracle.

The sweep's grid is min(ceil(n / 1024), 512) workgroups of 16 waves, tiles strided over the waves: wave g of the grid owns tiles
g, g + 8 192, g + 16 384 ... — a wave owns a second tile only when n > 524 288, and only then does the launch take the pair form
(an instantiation of its own; the switch is an argument of it), so every case here has at least that many rows.
The pair of wave g is (tile g, tile g + 8 192) = rows 64 g + [0, 64) and 524 288 + 64 g + [0, 64): `row_a(g, lane)`, `row_b(g, lane)`.

The pods of the one-plane cases come from the hand-made pool of test_match_codes_gpu.py (ordinary pods of three namespaces, pods
with 15 / 16 / 24 matching ClusterThrottles — 16 and 24 overflow the record: header 0xFF, that tile falls back to the planes —, a
pod of a namespace without a Namespace object), placed by a vectorised form of _with_pods (the helper's Python loop over a million
rows takes a minute; `fast_with_pods` is checked against it on a few hundred rows).  The four-plane cases take the configs[2]
generator at the shape shape_with_planes(4, 4) finds.

Which form a launch took is not visible in any counter; under KT_DEBUG_LDS=1 the launch says `pairs=0/1` on stderr (and the LDS of
the form: the pair form has a second row of counters per wave), and test_debug_line_names_the_form reads that line in a child process.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from test_aggregate_two_per_cu_gpu import assert_same_result, cfg2_scaled
from test_check_cached_full_list_gpu import _tight_matches, _tighten
from test_engine_gpu import _permute_pods, _rows_of, _with_pods, assert_reconcile_equal, responsible_rows
from test_match_cache_gpu import NOW, shape_with_planes
from test_match_codes_gpu import Pool

pytestmark = pytest.mark.gpu

SWITCH = "KT_NO_TILE_PAIRS_CHECK"
WAVES = 512 * 16      # waves of the sweep's largest grid
B0 = WAVES * 64       # 524 288: the first row of every wave's second tile
POD_FIELDS = ("pod_ns", "pod_flags", "pod_label_off", "pod_label_key", "pod_label_pair", "pod_ctr_off", "ctr_init", "ctr_present", "ctr_req",
              "pod_ovh_present", "pod_ovh")


def row_a(g, lane=0):
    return 64 * g + lane


def row_b(g, lane=0):
    return B0 + 64 * g + lane


# ---- pods by the million -----------------------------------------------------------------------------------------------------
def fast_permute_pods(snap, rows):
    """_permute_pods without its loop over the rows: a pods-only batch holding snap's pods in the order given by rows."""
    rows = np.asarray(rows, dtype=np.int64)
    b = S.Snapshot(snap.D, snap.L)
    b.alloc_namespaces(0, 0)
    b.alloc_throttles(0, 0, 0)

    def spans(off):  # (destination offsets, source index of every destination element)
        off = off.astype(np.int64)
        ln = off[rows + 1] - off[rows]
        dst = np.concatenate([[0], np.cumsum(ln)])
        return dst, np.repeat(off[rows] - dst[:-1], ln) + np.arange(dst[-1])

    l_dst, l_src = spans(snap.pod_label_off)
    c_dst, c_src = spans(snap.pod_ctr_off)
    n = len(rows)
    b.alloc_pods(n, int(l_dst[-1]), int(c_dst[-1]))
    b.pod_ns[:n], b.pod_flags[:n] = snap.pod_ns[rows], snap.pod_flags[rows]
    b.pod_label_off[:] = l_dst
    b.pod_label_key[:len(l_src)], b.pod_label_pair[:len(l_src)] = snap.pod_label_key[l_src], snap.pod_label_pair[l_src]
    b.pod_ctr_off[:] = c_dst
    b.ctr_init[:len(c_src)], b.ctr_present[:len(c_src)], b.ctr_req[:len(c_src)] = snap.ctr_init[c_src], snap.ctr_present[c_src], snap.ctr_req[c_src]
    b.pod_ovh_present[:n], b.pod_ovh[:n] = snap.pod_ovh_present[rows], snap.pod_ovh[rows]
    return b


def fast_with_pods(base, src_rows):
    """_with_pods over fast_permute_pods: a copy of `base` whose pod row r holds base's pod src_rows[r] (-1: row deleted)."""
    src_rows = np.asarray(src_rows)
    pods = fast_permute_pods(base, np.where(src_rows >= 0, src_rows, 0))
    out = copy.copy(base)
    out.n_pods = pods.n_pods
    for f in POD_FIELDS:
        setattr(out, f, getattr(pods, f))
    out.pod_flags = out.pod_flags.copy()
    out.pod_flags[:len(src_rows)][src_rows < 0] = 0
    return out


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    state = p.rows(300, {3: p.of("h16"), 5: p.of("ghost"), 64: p.of("h24"), 70: p.of("bare")})
    state[100:110] = -1
    slow, fast = _with_pods(p.snap, state), fast_with_pods(p.snap, state)
    assert slow.n_pods == fast.n_pods
    for f in POD_FIELDS:
        np.testing.assert_array_equal(getattr(fast, f), getattr(slow, f), err_msg=f"fast_with_pods: {f}")
    return p


@pytest.fixture(scope="module")
def four_planes():
    return shape_with_planes(4, 4)


# ---- the twin ----------------------------------------------------------------------------------------------------------------
class PairsTwin:
    def __init__(self, monkeypatch, make):
        monkeypatch.delenv(SWITCH, raising=False)
        self.c = make()
        monkeypatch.setenv(SWITCH, "1")
        self.u = make()
        monkeypatch.delenv(SWITCH, raising=False)

    def both(self, f):
        return f(self.c), f(self.u)

    def close(self):
        self.c.close()
        self.u.close()

    def step(self, snap, oracle_mod, n=None, want_status=False):
        """reconcile (apply) + sweep on both: every reconcile field and every summary word against each other and the oracle.
        Returns the oracle's (status matrix or None, summary words) of the sweep."""
        n = snap.n_pods if n is None else n
        rows = responsible_rows(snap)
        o = oracle_mod.Oracle(snap)
        want = o.reconcile(NOW, rows=rows, nthreads=8)
        rc, ru = self.both(lambda e: e.reconcile(NOW, apply=True))
        assert_same_result(rc, ru, snap.n_thr)
        assert_reconcile_equal(_rows_of(rc, rows, snap.D), want, len(rows))
        assert_reconcile_equal(_rows_of(ru, rows, snap.D), want, len(rows))
        snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
        st_w, sm_w = o.check(on_equal=False, want_status=want_status, nthreads=8)
        (_, sm_c), (_, sm_u) = self.both(lambda e: e.check(n=n, on_equal=False, want_status=False))
        np.testing.assert_array_equal(sm_c, sm_u, err_msg="summary words: tile pairs against single tiles")
        np.testing.assert_array_equal(sm_c, sm_w[:n], err_msg="summary words against the oracle")
        assert self.c.match_cache_scans() == self.u.match_cache_scans() >= 1, "the sweep did not replay the table"
        return (st_w[:n] if st_w is not None else None), sm_w[:n]


def make_for(snap):
    return lambda: E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)


def headers(e, rows):
    rec, _ = e.match_codes()
    return rec[np.asarray(rows), 0]


ROW_COUNTS = [B0, B0 + 1, B0 + 65, 2 * B0, 2 * B0 + 1]


# ---- 1. row counts, one plane: overflow records and verdict bits on either side of a pair ------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_one_plane(n, pool, oracle_mod, monkeypatch):
    """524 288: no wave owns two tiles (the launch keeps the single form: the pair path stays idle).  524 289: exactly one pair — wave 0's —, whose second
    tile has one valid lane.  524 288 + 65: wave 0's pair is full, wave 1's second tile has one lane.  1 048 576: every wave
    exactly one pair.  1 048 577: wave 0 has a pair and then a single tile of one lane.
    What sits where (second-tile rows exist as far as n reaches; the row of wave 0's and wave 1's second tile is its lane 0, so
    that the smallest shapes have it):
      wave 0: 16 matches in the FIRST tile only, a 15-match pod (the largest record) beside it and in the second tile;
      wave 1: 16 / 24 matches in the SECOND tile only (lane 0 and lane 5);
      wave 2: 16 matches in the first AND 24 in the second tile: both fall back to the planes;
      wave 3: the pod of a namespace without a Namespace object (Error) in the first tile, wave 4: in the second, wave 5: in both;
      wave 6: a first tile all of whose rows are deleted, wave 7: such a second tile; wave 8: both, with one live lane in each;
      the last row: a 24-match pod."""
    special = {row_a(0, 3): pool.of("h16"), row_a(0, 4): pool.of("h15"), row_b(0, 0): pool.of("h15", 1),
               row_b(1, 0): pool.of("h16", 1), row_b(1, 5): pool.of("h24"),
               row_a(2, 7): pool.of("h16"), row_b(2, 9): pool.of("h24", 1),
               row_a(3, 1): pool.of("ghost"), row_b(4, 2): pool.of("ghost"), row_a(5, 63): pool.of("ghost"), row_b(5, 0): pool.of("ghost"),
               n - 1: pool.of("h24")}
    state = pool.rows(n, special)
    for lo in (row_a(6), row_b(7), row_a(8), row_b(8)):
        state[lo:lo + 64] = -1  # (a slice past n is empty)
    for r in (row_a(8, 11), row_b(8, 13)):
        if r < n:
            state[r] = pool.of("ordinary", 3)
    snap = fast_with_pods(pool.snap, state)
    assert snap.n_pods == n
    tw = PairsTwin(monkeypatch, make_for(snap))
    try:
        _, sm_w = tw.step(snap, oracle_mod)
        assert tw.c.index_stats()["chunks"] == 1
        over = [r for r in (row_a(0, 3), row_b(1, 0), row_b(1, 5), row_a(2, 7), row_b(2, 9), n - 1) if r < n and state[r] >= 0]
        assert (headers(tw.c, over) == 0xFF).all(), "the 16- and 24-match pods do not overflow their records"
        assert (headers(tw.c, [r for r in (row_a(0, 4), row_b(0, 0)) if r < n and r != n - 1]) == 15).all()
        for r in (row_a(3, 1), row_b(4, 2), row_a(5, 63), row_b(5, 0)):
            if r < n and r != n - 1:
                assert sm_w[r] == 2, f"row {r}: the pod without a Namespace object is an Error"
        for lo in (row_a(6), row_b(7)):
            assert not sm_w[lo:min(lo + 64, n)].any(), "deleted rows carry a verdict"
        assert (sm_w > 2).any(), "nobody is throttled: the case tests nothing"
    finally:
        tw.close()


# ---- 2. row counts, four planes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_four_planes(n, four_planes, oracle_mod, monkeypatch):
    """The same row counts on the configs[2] generator at a shape with four planes: codes name all four list positions."""
    n_thr, n_cluster = four_planes
    snap = W.generate(cfg2_scaled(n, n_thr=n_thr, n_cluster=n_cluster))
    assert snap.n_pods == n
    tw = PairsTwin(monkeypatch, make_for(snap))
    try:
        _, sm_w = tw.step(snap, oracle_mod)
        assert tw.c.index_stats()["chunks"] == 1 and tw.c.match_cache_planes() == 4
        assert (sm_w > 2).any(), "nobody is throttled: the case tests nothing"
    finally:
        tw.close()


# ---- 3. the list: one list per pair ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["first-tile-alone", "full-during-second"])
def test_the_list_runs_full_inside_a_pair(case, pool, oracle_mod, monkeypatch):
    """524 288 + 64 rows: wave 0 owns the one pair.  Tight matches are counted on the host as test_check_cached_full_list_gpu.py
    counts them (a lower bound of what the wave lists).
      first-tile-alone  : more than 64 provably tight matches in the pair's first tile: the list drains in the middle of the
                          first replay, with slot-0 entries only, and the second tile lists again behind it;
      full-during-second: at most 64 in the first tile (the wave's list holds ALL matches of tight throttles there, provable or
                          not: the first tile is kept to a few of the densest pods so that the bound of 64 holds for every match
                          of theirs), the rest in the second — the lean mid-replay drain sees entries of both slots."""
    n = B0 + 64

    def tightened(state):  # (thresholds of its own: the pool's are shared)
        s = fast_with_pods(pool.snap, state)
        s.thr_spec = copy.deepcopy(s.thr_spec)
        _tighten(s, oracle_mod)
        return s

    state = pool.rows(n, {})
    probe = pool.rows(4096, {})
    score = _tight_matches(tightened(probe), oracle_mod).sum(axis=1)
    top = probe[np.argsort(-score, kind="stable")[:8]]
    dense = top[np.arange(64) % 8]
    if case == "first-tile-alone":
        state[:64] = dense
    else:
        state[:64] = pool.of("nomatch")
        state[:6] = top[:6]
        state[B0:B0 + 64] = dense
    snap = tightened(state)
    tm = _tight_matches(snap, oracle_mod)
    in_a, in_b = int(tm[:64].sum()), int(tm[B0:B0 + 64].sum())
    if case == "first-tile-alone":
        assert in_a > 64, f"only {in_a} provably tight matches in the first tile: the list does not run full there"
    else:
        # every match of the six dense pods, tight or not, is at most 6 x 15 codes; what the wave lists of them is bounded by the
        # matches of throttles that are tight for SOME pod — count those, not only the provable ones
        st, _ = oracle_mod.Oracle(snap).check(rows=np.arange(64, dtype=np.int64), on_equal=False, want_status=True, nthreads=8)
        all_a = int(((st != 0) & (st != 255)).sum())
        assert in_a >= 1 and all_a <= 64, f"{all_a} matches in the first tile: the list may drain before the second replay"
        assert in_a + in_b > 64, f"{in_a} + {in_b} provably tight matches: the list does not run full during the second replay"
    tw = PairsTwin(monkeypatch, make_for(snap))
    try:
        _, sm_w = tw.step(snap, oracle_mod)
        assert (sm_w[:64] > 2).any(), "no pod of the first tile is throttled by anything: the case is not what it says"
    finally:
        tw.close()


# ---- 4. pod events in a pair's second tile -----------------------------------------------------------------------------------
def test_pod_events_in_a_second_tile(pool, oracle_mod, monkeypatch):
    """An upsert (an ordinary row becomes a 16-match row: an overflow record appears; another becomes a 15-match row) and a delete
    in wave 0's second tile between two steps: the write-through of the codes reaches the sweep's next replay, no table rebuild."""
    base = copy.copy(pool.snap)  # (the stored status of the steps stays this test's)
    n = B0 + 64
    P = n + 64
    state = pool.rows(n, {row_b(0, 1): pool.of("h15")})

    def make():
        e = E.Engine(base.D, max(base.L, 1), P, max(base.n_thr, 1), max(base.n_ns, 1))
        e.upsert_namespaces(base)
        e.upsert_throttles(base)
        e.upsert_pods(fast_permute_pods(base, state), rows=np.arange(n))
        return e

    tw = PairsTwin(monkeypatch, make)
    try:
        def sweep():
            snap = fast_with_pods(base, state)
            tw.step(snap, oracle_mod, n=n)
            for f in ("thr_used", "thr_calc", "thr_flags", "thr_thrl_flag", "thr_thrl_has"):
                setattr(base, f, getattr(snap, f))
            assert tw.c.match_cache_builds() == 1 and tw.u.match_cache_builds() == 1, "a pod event rebuilt the table"

        sweep()
        assert headers(tw.c, [row_b(0, 1)])[0] == 15
        rows = np.array([row_b(0, 7), row_b(0, 40), row_a(0, 2)], dtype=np.int64)
        pods = np.array([pool.of("h16"), pool.of("h15", 1), pool.of("multi", 0)], dtype=np.int64)
        tw.both(lambda e: e.upsert_pods(_permute_pods(base, pods), rows=rows))
        state[rows] = pods
        tw.both(lambda e: e.delete_pods(np.array([row_b(0, 20)], dtype=np.int64)))
        state[row_b(0, 20)] = -1
        sweep()
        assert headers(tw.c, [row_b(0, 7)])[0] == 0xFF and headers(tw.c, [row_b(0, 40)])[0] == 15
        tw.both(lambda e: e.upsert_pods(_permute_pods(base, np.array([pool.of("ordinary", 5)])), rows=np.array([row_b(0, 7)], dtype=np.int64)))
        state[row_b(0, 7)] = pool.of("ordinary", 5)
        sweep()
        assert headers(tw.c, [row_b(0, 7)])[0] != 0xFF
    finally:
        tw.close()


# ---- 5. the launch's debug line ----------------------------------------------------------------------------------------------
_CHILD = """
import os, sys
sys.path[:0] = %r
import numpy as np
from kube_throttler_amd import engine as E
from kube_throttler_amd import workload as W
from test_aggregate_two_per_cu_gpu import cfg2_scaled
for n, sw in ((524288, None), (524289, None), (524289, "1")):
    snap = W.generate(cfg2_scaled(n))
    os.environ.pop("KT_NO_TILE_PAIRS_CHECK", None)
    if sw:
        os.environ["KT_NO_TILE_PAIRS_CHECK"] = sw
    e = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    e.check(n=snap.n_pods, on_equal=False, want_status=False)
    e.close()
"""


def test_debug_line_names_the_form():
    """KT_DEBUG_LDS=1: the cached sweep's line says pairs=0 at 524 288 rows (no wave owns a second tile: the single form, the smaller
    LDS), pairs=1 at 524 289 as the engine comes and pairs=0 there under the switch — the same form, by its LDS."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, KT_DEBUG_LDS="1")
    env.pop(SWITCH, None)
    r = subprocess.run([sys.executable, "-c", _CHILD % ([os.path.dirname(here), here],)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("kt_check_bitmap_cached:")]
    assert len(lines) == 3 and all("match codes" in ln for ln in lines), r.stderr[-2000:]
    assert [ln.rstrip()[-7:] for ln in lines] == ["pairs=0", "pairs=1", "pairs=0"], lines
    lds = [int(ln.split("lds=")[1].split()[0]) for ln in lines]
    assert lds[1] == lds[2] == lds[0] + 16 * 64 * 8, lines
