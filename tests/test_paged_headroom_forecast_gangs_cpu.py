"""The paged gang headroom forecast (kt_paged_headroom_forecast_gangs), pinned on the CPU.

``paging.paged_headroom_forecast_gangs_of`` — what kt_kernels_headroom_forecast_gangs_paged.hip computes per lane: per page
CalculateThreshold at the lane's instant, ONE "differs" fact over all pages, then per (throttle, page) pair the search over the
copies against that page's reserved row plus j x what one copy reserves there, the pod count on page 0 only — is held to the
operational reference of tests/paged_headroom_forecast_gangs_reference.py: per instant a copy of every page reconciled with the
OR-ed bytes, then ``cap`` consecutive copies of the gang walked member by member over per-page oracle checks and admits.  Random
clusters over 20 to 40 resource names with loosened thresholds and directed cases with their answers written out.
tests/test_paged_headroom_forecast_gangs_gpu.py holds the kernel to the same reference."""
import pytest

import forecast_reference as FR
import headroom_forecast_gangs_reference as HFGR
import paged_headroom_forecast_gangs_reference as R
import paged_headroom_forecast_reference as PHFR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

NOW, CAP, DCAP = R.NOW, R.CAP, R.DIRECTED_CAP


@pytest.mark.parametrize("seed,factor", R.CASES)
def test_the_model_equals_the_reference_on_wide_clusters(seed, factor, oracle_mod):
    snaps, gangs, want = R.wide_reference(seed, factor, oracle_mod)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for on_equal in (False, True):
        for g, (copies, limiting, blocker, _) in zip(gangs, want[on_equal]):
            for need in (1, 2):
                got = paging.paged_headroom_forecast_gangs_of(snaps, g, FR.INSTANTS, CAP, need, on_equal, ctx=ctx)
                assert got == (R.first_of(copies, need), copies, limiting, blocker), f"seed {seed} on_equal={on_equal} gang {g} want={need}"


def test_the_cases_are_not_vacuous(oracle_mod):
    """Conditions on the inputs, on the reference side alone: a weak generator cannot hide a failure.  Observed over R.CASES at
    CAP, both on_equal values together (the counts the search that chose R.CASES reported):
    24 gangs x 2 x 37 instants = 1776 cells, 853 with 0 copies and 473 at cap;
      1. 441 cells with 0 < copies < cap of a gang of at least two members;
      2. 16 rows with at least three distinct values;
      3. 651 cells whose blocker is not the gang's first member;
      4. 109 cells that differ from the minimum over the pages' own single-engine references;
      5. 14 rows whose first is strictly between 0 and NONE at want = 2;
      6. 669 cells whose limiting row is not-throttled in page 0's own check: the deciding name lies on another page."""
    between = three = later = not_the_minimum = first_inside = off_page_0 = cells = 0
    shapes = []
    for seed, factor in R.CASES:
        snaps, gangs, want = R.wide_reference(seed, factor, oracle_mod)
        shapes.append([s.D for s in snaps])
        own = R.own_states(snaps, oracle_mod, FR.INSTANTS)
        for eq in (False, True):
            for g, (copies, limiting, blocker, off) in zip(gangs, want[eq]):
                cells += len(copies)
                if len(g) >= 2:
                    between += sum(0 < c < CAP for c in copies)                                   # 1
                three += len(set(copies)) >= 3                                                    # 2
                later += sum(b > 0 for b in blocker)                                              # 3
                pages = R.min_of_pages(snaps, oracle_mod, g, FR.INSTANTS, CAP, eq, states=own)
                not_the_minimum += sum(a != b for a, b in zip(copies, pages))                     # 4
                first_inside += R.first_of(copies, 2) > 0                                         # 5
                off_page_0 += sum(off)                                                            # 6
    seen = (f"{cells} cells: between (gangs of >= 2) {between}, rows with >= 3 values {three}, blocker behind the first member {later}, "
            f"not the minimum of the pages {not_the_minimum}, first inside at want = 2 {first_inside}, decided off page 0 {off_page_0}; "
            f"pages {shapes}")
    assert between >= 1 and three >= 1 and later >= 1 and not_the_minimum >= 1 and first_inside >= 1 and off_page_0 >= 1, seen
    assert set(R.GPU_CASES) <= set(R.CASES) and 1 <= len(R.GPU_CASES) <= 4


# ---- directed cases, with their answers written out ----
@pytest.mark.parametrize("name", sorted(R.DIRECTED))
def test_directed_cases_shared_with_the_gpu_suite(name, oracle_mod):
    snaps, members, inst, ref = R.directed_reference(name, oracle_mod)
    assert len(snaps) == 2
    for on_equal in (False, True):
        copies, limiting, blocker = (list(x) for x in R.DIRECTED[name][1][on_equal])
        assert ref[on_equal] == (copies, limiting, blocker), f"{name} on_equal={on_equal}: the reference"
        for need in (1, 2):
            assert paging.paged_headroom_forecast_gangs_of(snaps, members, inst, DCAP, need, on_equal) == (
                R.first_of(copies, need), copies, limiting, blocker), f"{name} on_equal={on_equal} want={need}: the model"


def test_directed_the_pages_own_answers_do_not_combine(oracle_mod):
    """In "another-page-replaces-the-threshold" page 0 on its own never sees a reason to replace inside a window: it reads spec
    there, and outside its calculated threshold, which is spec — the minimum over the pages' own answers misses the 4."""
    snaps, members, inst, ref = R.directed_reference("another-page-replaces-the-threshold", oracle_mod)
    assert ref[False][0] == [2, 2, 4, 4, 4, 4, 2, 2, 2, 2]
    assert R.min_of_pages(snaps, oracle_mod, members, inst, DCAP) == [2] * 10


# ---- the identities of the header, on the model ----
@pytest.mark.parametrize("name", sorted(HFGR.DIRECTED))
def test_one_page_is_headroom_forecast_gangs_of_on_the_directed_cases(name):
    """(P1)"""
    snap, members, inst = HFGR.DIRECTED[name]()
    for on_equal in (False, True):
        for need in (1, 2):
            assert (paging.paged_headroom_forecast_gangs_of([snap], members, inst, HFGR.CAP, need, on_equal)
                    == paging.headroom_forecast_gangs_of(snap, members, inst, HFGR.CAP, need, on_equal)), name


@pytest.mark.parametrize("seed", [1, 3])  # (clusters whose reference copies take at least three values)
def test_one_page_is_headroom_forecast_gangs_of(seed, oracle_mod):
    """(P1)"""
    snap, gangs, inst, _ = HFGR.cluster_case(seed, oracle_mod)
    for on_equal in (False, True):
        for g in gangs:
            assert (paging.paged_headroom_forecast_gangs_of([snap], g, inst, HFGR.CAP, 2, on_equal)
                    == paging.headroom_forecast_gangs_of(snap, g, inst, HFGR.CAP, 2, on_equal)), f"seed {seed} gang {g}"


@pytest.mark.parametrize("seed,factor", PHFR.CASES[:3])
def test_a_gang_of_one_is_the_paged_headroom_forecast(seed, factor, oracle_mod):
    """(G1)"""
    snaps, pods = PHFR.wide_case(seed, factor, oracle_mod)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for on_equal in (False, True):
        for p in pods:
            first, copies, limiting = paging.paged_headroom_forecast_of(snaps, p, FR.INSTANTS, CAP, 2, on_equal, ctx=ctx)
            got = paging.paged_headroom_forecast_gangs_of(snaps, [p], FR.INSTANTS, CAP, 2, on_equal, ctx=ctx)
            assert got[:3] == (first, copies, limiting), f"seed {seed} pod{p}"
            assert got[3] == [0 if c < CAP else -1 for c in copies]


@pytest.mark.parametrize("seed,factor", R.CASES)
def test_cap_one_is_the_paged_gang_forecast(seed, factor, oracle_mod):
    """(G2)"""
    snaps, gangs = R.wide_case(seed, factor, oracle_mod)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for on_equal in (False, True):
        for g in gangs:
            f_first, verdicts, blockers = paging.paged_forecast_gangs_of(snaps, g, FR.INSTANTS, on_equal, ctx=ctx)
            first, copies, _, blocker = paging.paged_headroom_forecast_gangs_of(snaps, g, FR.INSTANTS, 1, 1, on_equal, ctx=ctx)
            assert copies == [1 if v == S.VERDICT_ALLOW else 0 for v in verdicts]
            assert (first, blocker) == (f_first, blockers)
