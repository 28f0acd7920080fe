"""The two-per-CU form of the packed aggregate scan (kt_aggregate_bitmap_one) and the reductions over up to 512 slabs.

Slabs 256..511 only exist when more than 256 workgroups launch: a workgroup takes 1024 listed pods (aggregate_blocks), so the
cases here list more than 262 144 countable pods.  Every case compares a reconcile with the oracle on the responsible throttles
and, field by field on ALL throttle rows, with the same engine kept at one workgroup per CU (KT_AGG_ONE_PER_CU=1); the engine's
workgroup counter says which form ran.
"""
import numpy as np
import pytest

from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from kube_throttler_amd import workload as W
from test_engine_gpu import _permute_pods, _rows_of, assert_reconcile_equal, responsible_rows

pytestmark = pytest.mark.gpu

NOW = (1767225600, 0)
PODS_PER_WG = 1024  # kBlockIx: what aggregate_blocks gives a workgroup
COUNTABLE = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED


def cfg2_scaled(n_pods, n_thr=48, n_cluster=24, D=8, seed=None, preset=2):
    """BASELINE configs[2]'s generator settings (8 labels per pod, D = 8, single-term selectors), scaled down — or those of
    another preset (configs[3]: selectors of several terms with matchExpressions)."""
    c = W.preset(preset)
    c.n_pods_total = c.n_pods = n_pods
    c.n_thr, c.n_cluster, c.D = n_thr, n_cluster, D
    if seed is not None:
        c.seed = seed
    return c


def countable_rows(snap):
    return np.nonzero((snap.pod_flags[:snap.n_pods] & COUNTABLE) == COUNTABLE)[0]


def trim_countable(snap, n):
    """Leave exactly n countable pods: the surplus ones are unscheduled (shouldCountIn false: the view no longer lists them)."""
    rows = countable_rows(snap)
    assert len(rows) >= n, (len(rows), n)
    snap.pod_flags[rows[n:]] &= ~np.uint32(S.POD_SCHEDULED)
    assert len(countable_rows(snap)) == n


def expected_workgroups(n, max_wg):
    """launch_aggregate_indexed: ceil(n / 1024) workgroups, capped, then exactly those that own a tile of the contiguous ranges"""
    tiles = (n + 63) // 64
    nb = min(max(1, (n + PODS_PER_WG - 1) // PODS_PER_WG), max_wg)
    tpb = (tiles + nb - 1) // nb
    return (tiles + tpb - 1) // tpb


ALL_FIELDS = ("calc_updated", "thrl_flag", "thrl_has", "thrl_pod", "error")


def assert_same_result(a, b, T):
    for name in ALL_FIELDS:
        np.testing.assert_array_equal(getattr(a, name)[:T], getattr(b, name)[:T], err_msg=name)
    for tab in ("used", "calc"):
        for f in ("v", "present", "count", "has_count"):
            np.testing.assert_array_equal(getattr(getattr(a, tab), f)[:T], getattr(getattr(b, tab), f)[:T], err_msg=f"{tab}.{f}")


def reconcile_both_forms(snap, oracle_mod, monkeypatch):
    """One engine as it comes and one kept at one workgroup per CU reconcile the snapshot: both against the oracle, and against
    each other on every throttle row.  Returns (workgroups of the first, workgroups of the second, the oracle's result)."""
    rows = responsible_rows(snap)
    results, counters = {}, {}
    for mode in ("two", "one"):
        if mode == "one":
            monkeypatch.setenv("KT_AGG_ONE_PER_CU", "1")
        else:
            monkeypatch.delenv("KT_AGG_ONE_PER_CU", raising=False)
        eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
        try:
            results[mode] = [eng.reconcile(NOW, apply=False)]
            counters[mode] = [eng.aggregate_workgroups()]
            assert eng.kernel_name(E.KERNEL_AGGREGATE) == "kt_aggregate_bitmap_packed", eng.kernel_name(E.KERNEL_AGGREGATE)
        finally:
            eng.close()
    monkeypatch.delenv("KT_AGG_ONE_PER_CU", raising=False)
    want = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows, nthreads=8)
    for mode in ("two", "one"):
        assert_reconcile_equal(_rows_of(results[mode][0], rows, snap.D), want, len(rows))
    assert_same_result(results["two"][0], results["one"][0], snap.n_thr)
    assert counters["one"][0] <= 256, counters
    return counters["two"][0], counters["one"][0], want


def test_configs2_throttles_on_300k_counted_pods(oracle_mod, monkeypatch):
    """About 300k counted pods x 48 throttles of the configs[2] generator, D = 8, 8 labels: more than 256 workgroups ran, and
    the sums over slabs 256.. are the oracle's."""
    snap = W.generate(cfg2_scaled(500_000))
    n = len(countable_rows(snap))
    assert n > 256 * PODS_PER_WG, n
    two, one, want = reconcile_both_forms(snap, oracle_mod, monkeypatch)
    print(f"countable pods {n}: workgroups {two} (two per CU), {one} (one per CU)")
    assert two > 256 and two == expected_workgroups(n, 512), (two, n)
    assert one == expected_workgroups(n, 256)
    assert (want.used.count > 0).any() and (want.used.v != 0).any()


@pytest.fixture(scope="module")
def big_cfg():
    return cfg2_scaled(920_000)


@pytest.mark.parametrize("n_countable", [256 * PODS_PER_WG, 256 * PODS_PER_WG + 1, 512 * PODS_PER_WG, 512 * PODS_PER_WG + 1],
                         ids=["256-workgroups", "257-workgroups", "512-workgroups", "capped-grid"])
def test_boundary_workgroup_counts(n_countable, big_cfg, oracle_mod, monkeypatch):
    """Exactly 256, 257 and 512 workgroups' worth of countable pods, and one pod more than 512 workgroups take at 1024 pods each:
    the grid is capped and every workgroup scans one tile more."""
    cfg = W.WorkloadCfg.from_buffer_copy(big_cfg)
    if n_countable <= 257 * PODS_PER_WG:  # (the small cases need no 920k pods)
        cfg.n_pods_total = cfg.n_pods = 460_000
    snap = W.generate(cfg)
    trim_countable(snap, n_countable)
    two, one, _ = reconcile_both_forms(snap, oracle_mod, monkeypatch)
    print(f"countable pods {n_countable}: workgroups {two} (two per CU), {one} (one per CU)")
    assert two == expected_workgroups(n_countable, 512), two
    if n_countable == 256 * PODS_PER_WG:
        assert two == 256
    elif n_countable == 256 * PODS_PER_WG + 1:
        assert two == 257
    elif n_countable == 512 * PODS_PER_WG:
        assert two == 512
    else:
        assert 256 < two <= 512


def test_nine_bit_headroom_does_not_pack(oracle_mod, monkeypatch):
    """A request so large that its field takes 56 bits at one workgroup per CU — 8 bits of headroom: it packs — and would take
    56 at two per CU as well, where 9 bits of headroom leave 55: the launch stays one per CU and the sums are right.
    (Field width = bit length of value x pods per workgroup; the view holds the listed pods + 65 536 records of headroom, a
    workgroup ceil(tiles / workgroups) + 16 tiles of 64.)"""
    snap = W.generate(cfg2_scaled(500_000))
    rows = countable_rows(snap)
    n = len(rows)
    assert n > 256 * PODS_PER_WG

    def slab_pods(max_wg):
        cap = n + max(65536, n // 16)
        tiles = (cap + 63) // 64
        blocks = min((cap + PODS_PER_WG - 1) // PODS_PER_WG, max_wg)
        return ((tiles + blocks - 1) // blocks + 16) * 64

    p1, p2 = slab_pods(256), slab_pods(512)
    value = ((1 << 55) + p2 - 1) // p2 + 1  # the smallest values whose sum over a two-per-CU workgroup's pods needs 56 bits
    value |= 1                              # (odd: no common trailing zeros to shift out)
    assert (value * p2).bit_length() == 56 and (value * p1).bit_length() == 56, (value, p1, p2)
    for r in rows[5::n // 2000]:  # two thousand pods over the list (their total, 2^55, stays below the 2^60 the engine sums exactly)
        c = int(snap.pod_ctr_off[int(r)])
        snap.ctr_present[c] |= 1
        snap.ctr_req[c, 0] = value
    two, one, want = reconcile_both_forms(snap, oracle_mod, monkeypatch)
    print(f"countable pods {n}, value {value}: workgroups {two} / {one}")
    assert two <= 256, two
    assert (want.used.v[:, 0] >= value).any()


def test_unmatched_throttle_and_zero_valued_key(oracle_mod, monkeypatch):
    """The key-mask unit of the records over 512 slabs: a Throttle whose namespace holds no counted pod (every slab's record of
    it stays zero), and a resource name that pods only ever carry with the value 0 (it has no field: `used` lists it because
    the OR of the zero-key masks says so)."""
    snap = W.generate(cfg2_scaled(500_000))
    n_ctr = int(snap.pod_ctr_off[snap.n_pods])
    snap.ctr_req[:n_ctr, 7] = 0
    snap.pod_ovh[:snap.n_pods, 7] = 0
    rows = countable_rows(snap)
    for r in rows[::1000]:  # a few hundred pods over the whole list (slabs below and above 256) carry key 7 with the value 0
        snap.ctr_present[int(snap.pod_ctr_off[int(r)])] |= 1 << 7
    thr = responsible_rows(snap)
    namespaced = [int(t) for t in thr if not (snap.thr_flags[t] & S.THR_CLUSTER)]
    t0 = namespaced[0]
    snap.pod_flags[:snap.n_pods][snap.pod_ns[:snap.n_pods] == snap.thr_ns[t0]] &= ~np.uint32(S.POD_SCHEDULED)
    assert len(countable_rows(snap)) > 256 * PODS_PER_WG
    two, one, want = reconcile_both_forms(snap, oracle_mod, monkeypatch)
    assert two > 256, two
    i0 = int(np.nonzero(thr == t0)[0][0])
    assert want.used.count[i0] == 0 and not want.used.v[i0].any()
    assert (want.used.v[:, 7] == 0).all() and ((want.used.present >> 7) & 1).any(), "no throttle lists the zero-valued key"


def test_reconciles_in_a_row_and_after_an_upsert(oracle_mod, monkeypatch):
    """Two reconciles in a row on one engine (consumed partials, a fresh slab epoch), then a pod that becomes countable (its
    record is appended to the scan view) and a third reconcile: all three the oracle's, in both forms."""
    snap = W.generate(cfg2_scaled(500_000))
    rows_t = responsible_rows(snap)
    want = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows_t, nthreads=8)
    flags = snap.pod_flags[:snap.n_pods]
    unsched = np.nonzero((flags & (COUNTABLE | S.POD_FINISHED)) == (S.POD_VALID | S.POD_SCHED_MATCH))[0][:3]
    assert len(unsched) == 3
    got = {}
    for mode in ("two", "one"):
        if mode == "one":
            monkeypatch.setenv("KT_AGG_ONE_PER_CU", "1")
        snap.pod_flags[unsched] &= ~np.uint32(S.POD_SCHEDULED)
        eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
        try:
            r1 = eng.reconcile(NOW, apply=False)
            wg1 = eng.aggregate_workgroups()
            r2 = eng.reconcile(NOW, apply=False)
            assert_reconcile_equal(_rows_of(r1, rows_t, snap.D), want, len(rows_t))
            assert_same_result(r1, r2, snap.n_thr)
            snap.pod_flags[unsched] |= np.uint32(S.POD_SCHEDULED)
            eng.upsert_pods(_permute_pods(snap, unsched), rows=unsched.astype(np.int64))
            r3 = eng.reconcile(NOW, apply=False)
            got[mode] = (r3, wg1, eng.aggregate_workgroups())
        finally:
            eng.close()
    monkeypatch.delenv("KT_AGG_ONE_PER_CU", raising=False)
    want3 = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows_t, nthreads=8)
    for mode in ("two", "one"):
        assert_reconcile_equal(_rows_of(got[mode][0], rows_t, snap.D), want3, len(rows_t))
    assert_same_result(got["two"][0], got["one"][0], snap.n_thr)
    assert not np.array_equal(want3.used.count, want.used.count), "the upsert changed nothing"
    assert got["two"][1] > 256 and got["two"][2] > 256, got["two"][1:]
    assert got["one"][1] <= 256 and got["one"][2] <= 256, got["one"][1:]


def test_configs3_selectors_run_the_rich_instantiation(oracle_mod, monkeypatch):
    """Throttles of the configs[3] generator (several terms per selector, matchExpressions: the `rich` instantiation of the
    form, vetoes and `has_adj` run masks) over more than 256 workgroups' worth of countable pods."""
    snap = W.generate(cfg2_scaled(500_000, preset=3))
    n = len(countable_rows(snap))
    assert n > 256 * PODS_PER_WG, n
    two, one, want = reconcile_both_forms(snap, oracle_mod, monkeypatch)
    print(f"configs[3] selectors, countable pods {n}: workgroups {two} (two per CU), {one} (one per CU)")
    assert two > 256 and two == expected_workgroups(n, 512), (two, n)
    assert one == expected_workgroups(n, 256)
    assert (want.used.count > 0).any() and (want.used.v != 0).any()


def test_sixteen_dimensions(oracle_mod, monkeypatch):
    """D = 16, more than 256 workgroups' worth of countable pods.  Sixteen populated dimensions do not pack into the three words
    the two-per-CU form takes (a field holds the sum of a workgroup's ~1000 pods, >= 10 bits, under 9 bits of headroom: 16 x 19
    bits > 192), so the engine keeps its plan of more than three words and the launch stays one per CU — the same plan, the same
    grid and the same results as the engine that is kept there by the switch."""
    snap = W.generate(cfg2_scaled(500_000, D=16))
    n = len(countable_rows(snap))
    assert n > 256 * PODS_PER_WG, n
    assert all((snap.ctr_req[:int(snap.pod_ctr_off[snap.n_pods]), d] != 0).any() for d in range(16)), "a dimension nobody requests"
    rows = responsible_rows(snap)
    res = {}
    for mode in ("two", "one"):
        if mode == "one":
            monkeypatch.setenv("KT_AGG_ONE_PER_CU", "1")
        eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
        try:
            res[mode] = (eng.reconcile(NOW, apply=False), eng.aggregate_workgroups(), eng.packed_words())
        finally:
            eng.close()
    monkeypatch.delenv("KT_AGG_ONE_PER_CU", raising=False)
    want = oracle_mod.Oracle(snap).reconcile(NOW, rows=rows, nthreads=8)
    print(f"D = 16, countable pods {n}: workgroups {res['two'][1]} / {res['one'][1]}, packed words {res['two'][2]} / {res['one'][2]}")
    for mode in ("two", "one"):
        assert_reconcile_equal(_rows_of(res[mode][0], rows, snap.D), want, len(rows))
    assert_same_result(res["two"][0], res["one"][0], snap.n_thr)
    assert res["one"][2] > 3, res["one"][2]
    assert res["two"][2] == res["one"][2], (res["two"][2], res["one"][2])
    assert res["two"][1] == res["one"][1] == expected_workgroups(n, 256), (res["two"][1], res["one"][1])
