"""The cached PreFilter sweep (kt_check_bitmap_cached) with a tight-match list that runs FULL inside one tile.  A wave lists the
matches whose verdict needs the comparison of the pod's requests with thr[] / head[] — 128 entries — and drains the list on the spot
as soon as it holds more than 64, through a lean form of the drain (one dimension at a time, the pod's non-zero mask read again
from its meta word).  The workload's own mix has four or five such matches per tile, so no other test gets there.

The case: thresholds that leave every throttle a headroom of about a median request (most matches then need the comparison), and
in tile 0 copies of the eight pods that match most of those throttles.  The list is per wave and no engine counter sees it, so the
count is computed here, as a lower bound: a throttle that gives one matched pod `not throttled` and another `insufficient` or
`exceeds` can only have compared their requests — it is tight, and each of its matches is listed.  Twin of engines as in
test_match_cache_gpu.py (one as it comes, one under KT_NO_MATCH_CACHE=1): reconcile with APPLY, full sweep, every summary word
against the oracle's and the twin's, KT_COUNTER_MATCH_CACHE_SCANS rises.
"""
import numpy as np
import pytest

from kube_throttler_amd import workload as W
from test_aggregate_two_per_cu_gpu import cfg2_scaled
from test_engine_gpu import _with_pods, responsible_rows
from test_match_cache_gpu import NOW, twin_for

pytestmark = pytest.mark.gpu

N_PODS = 20_011  # (a multiple of neither 64 nor 1024)


def _tighten(snap, oracle_mod):
    """Every threshold = what the throttle's pods use + what is reserved + a request that pods really carry (per dimension, the
    median of the non-zero ones among the first 4 096 containers): 1 <= headroom < the largest request."""
    rows = responsible_rows(snap)
    used = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows, nthreads=8).used
    req = snap.ctr_req[:min(int(snap.pod_ctr_off[snap.n_pods]), 4096)]
    typical = [int(np.median(req[:, d][req[:, d] > 0])) if (req[:, d] > 0).any() else 1 for d in range(snap.D)]
    for i, t in enumerate(rows):
        for d in range(snap.D):
            if (int(snap.thr_spec.present[t]) >> d) & 1:
                snap.thr_spec.v[t, d] = int(used.v[i, d]) + int(snap.thr_reserved.v[t, d]) + typical[d]


def _tight_matches(snap, oracle_mod):
    """matched[pod, throttle] restricted to the provably tight throttles, with the oracle's reconcile applied to the snapshot's
    stored status (as the step under test will apply it again: same pods, same result)."""
    s = snap
    rows = responsible_rows(s)
    o = oracle_mod.Oracle(s)
    want = o.reconcile(NOW, rows=rows, nthreads=8)
    s.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
    st, _ = o.check(rows=np.arange(s.n_pods, dtype=np.int64), on_equal=False, want_status=True, nthreads=8)
    tight = (st == 1).any(axis=0) & ((st == 3) | (st == 4)).any(axis=0)
    return ((st != 0) & (st != 255))[:, tight]


def test_more_than_64_tight_matches_in_one_tile(oracle_mod, monkeypatch):
    base = W.generate(cfg2_scaled(N_PODS))
    _tighten(base, oracle_mod)
    score = _tight_matches(base, oracle_mod).sum(axis=1)
    top = np.argsort(-score, kind="stable")[:8]
    state = np.arange(N_PODS, dtype=np.int64)
    state[:64] = top[np.arange(64) % 8]
    snap = _with_pods(base, state)
    _tighten(snap, oracle_mod)  # (again: tile 0's new pods moved what the throttles use)
    listed = int(_tight_matches(snap, oracle_mod)[:64].sum())
    assert listed > 64, f"only {listed} provably tight matches in tile 0: the list does not run full"
    tw = twin_for(snap, monkeypatch)
    try:
        _, sm_w = tw.step(snap, oracle_mod)
        tw.assert_counters(1, 1)
        assert tw.c.index_stats()["chunks"] == 1
        assert (sm_w[:64] > 1).any(), "no pod of tile 0 is throttled by anything: the case is not what it says"
    finally:
        tw.close()
