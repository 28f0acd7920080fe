"""The paged gang forecast without a GPU: ``paging.paged_forecast_gangs_of`` (the closed form of kt_paged_forecast_gangs on page
snapshots) against the operational reference of tests/paged_forecast_gangs_reference.py — per instant a copy of every page, the
oracle's reconcile with the bytes OR-ed over the pages, the members admitted in order over every page — on random wide clusters and
on directed cases whose answers are derived by hand; the identities that tie the call to its neighbours; and the C-ABI symbol."""
import ctypes as C
import os
import subprocess

import pytest

import forecast_gangs_reference as FGR
import forecast_reference as FR
import paged_forecast_gangs_reference as R
import paged_preempt_gangs_reference as PPGR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kube_throttler_amd", "csrc")
NOW = FR.NOW
A, B, ERR = R.A, R.B, R.ERR


def test_some_last_page_is_narrow_and_some_cluster_has_three_pages(oracle_mod):
    shapes = [[s.D for s in R.wide_reference(seed, factor, oracle_mod)[0]] for seed, factor in R.CASES]
    assert all(20 <= sum(sh) <= 40 for sh in shapes), shapes
    assert any(sh[-1] < S.KT_MAX_DIMS for sh in shapes) and any(len(sh) == 3 for sh in shapes) and any(len(sh) == 2 for sh in shapes), shapes
    sizes = {len(g) for seed, factor in R.CASES for g in R.wide_reference(seed, factor, oracle_mod)[1]}
    assert sizes >= {1, 2, 3, 4}, sizes


@pytest.mark.parametrize("seed,factor", R.CASES)
@pytest.mark.parametrize("on_equal", [False, True])
def test_closed_form_equals_the_reference_on_wide_clusters(seed, factor, on_equal, oracle_mod):
    snaps, gangs, want, _ = R.wide_reference(seed, factor, oracle_mod)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for g, ref in zip(gangs, want[on_equal]):
        assert paging.paged_forecast_gangs_of(snaps, g, FR.INSTANTS, on_equal, ctx=ctx) == ref, f"seed {seed} gang {g} on_equal={on_equal}"


def test_the_cached_walk_is_first_blocked(oracle_mod):
    """The reference copies the reconciled pages of an instant per gang instead of reconciling again: the same answer as
    ``paged_preempt_gangs_reference.first_blocked`` itself."""
    for name in ("reservation-on-the-second-page", "error-member", "count-judged-once"):
        snaps, members, inst, want = R.directed_reference(name, oracle_mod)
        for eq in (False, True):
            literal = [PPGR.first_blocked(snaps, oracle_mod, members, [], now=t, on_equal=eq) for t in inst]
            assert [-1 if b is None else b for b in literal] == want[eq][2], name


def non_vacuity_counts(oracle_mod):
    """Gang rows (a gang under one on_equal) per class, from the reference alone: (a) differs from the AND of the members' own
    paged forecasts, (b) differs from the pages' own gang forecasts combined, (c) first > 0, (d) first == -1 with no Error, (e)
    Error, (f) at some instant a page other than 0 decides the blocker: page 0 alone names a later one or none."""
    n = dict(a=0, b=0, c=0, d=0, e=0, f=0)
    for seed, factor in R.CASES:
        snaps, gangs, want, _ = R.wide_reference(seed, factor, oracle_mod)
        own = R.own_states(snaps, oracle_mod, FR.INSTANTS)
        for eq in (False, True):
            for g, (first, ver, blk) in zip(gangs, want[eq]):
                if ERR in ver:
                    n["e"] += 1
                else:
                    n["a"] += ver != R.members_and(snaps, oracle_mod, g, FR.INSTANTS, eq)
                    n["d"] += first == -1
                n["b"] += ver != R.pages_combined(snaps, oracle_mod, g, FR.INSTANTS, eq, states=own)
                n["c"] += first > 0
                page0 = FGR.reference(snaps[0], oracle_mod, g, FR.INSTANTS, eq, states=own[0])[2]
                n["f"] += any(b >= 0 and (q == -1 or q > b) for b, q in zip(blk, page0))
    return n


def test_the_cases_are_not_vacuous(oracle_mod):
    n = non_vacuity_counts(oracle_mod)
    print("non-vacuity counts over", R.CASES, ":", n)
    assert all(v >= 3 for v in n.values()), n


@pytest.mark.parametrize("name", sorted(R.DIRECTED))
def test_the_directed_answers(name, oracle_mod):
    """The hand-derived answer: the reference gives it, and the closed form gives it."""
    snaps, members, inst, want = R.directed_reference(name, oracle_mod)
    assert len(snaps) == 2
    for eq, answer in R.DIRECTED[name][1].items():
        assert want[eq] == answer, f"{name} on_equal={eq}: the reference says {want[eq]}"
        assert paging.paged_forecast_gangs_of(snaps, members, inst, eq) == answer, f"{name} on_equal={eq}: the closed form"


def test_directed_what_the_existing_calls_cannot_say(oracle_mod):
    snaps, members, inst, want = R.directed_reference("reservation-on-the-second-page", oracle_mod)
    assert R.members_and(snaps, oracle_mod, members, inst) == [A] * len(inst)  # each member alone passes everywhere
    assert want[False][1] == R._row(A, B)
    snaps, members, inst, want = R.directed_reference("another-page-replaces-the-threshold", oracle_mod)
    assert FGR.reference(snaps[0], oracle_mod, members, inst)[1] == [B] * len(inst)  # page 0's own gang forecast: blocked throughout
    assert paging.forecast_gangs_of(snaps[0], members, inst)[1] == [B] * len(inst)
    assert R.pages_combined(snaps, oracle_mod, members, inst) == [B] * len(inst) and want[False][0] == 2
    snaps, members, inst, want = R.directed_reference("blocker-is-the-minimum-over-pages-per-instant", oracle_mod)
    assert len(set(want[False][2])) == 3  # the blockers differ per instant
    snaps, members, inst, _ = R.directed_reference("stored-on-one-page-calculated-at-on-page-0", oracle_mod)
    assert [bool(int(s.thr_flags[0]) & S.THR_CALC_AT_NONZERO) for s in snaps] == [True, False]


# ---- identities on the closed form ----
@pytest.mark.parametrize("seed", [1, 4, 5])
def test_one_page_is_forecast_gangs_of(seed, oracle_mod):
    snap, gangs, _, _ = FGR.cluster_reference(seed, oracle_mod)
    for on_equal in (False, True):
        for g in gangs:
            assert paging.paged_forecast_gangs_of([snap], g, FR.INSTANTS, on_equal) == paging.forecast_gangs_of(snap, g, FR.INSTANTS, on_equal)
    for name, make in FGR.DIRECTED.items():
        snap, members, inst = make()
        for on_equal in (False, True):
            assert paging.paged_forecast_gangs_of([snap], members, inst, on_equal) == paging.forecast_gangs_of(snap, members, inst, on_equal), name


@pytest.mark.parametrize("seed,factor", R.CASES[:3])
def test_a_gang_of_one_is_paged_forecast_of(seed, factor, oracle_mod):
    snaps, _, _, _ = R.wide_reference(seed, factor, oracle_mod)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for on_equal in (False, True):
        for p in FR.forecast_pods(seed, snaps[0], n_pods=6):
            first, verdicts = paging.paged_forecast_of(snaps, p, FR.INSTANTS, on_equal, ctx=ctx)
            assert paging.paged_forecast_gangs_of(snaps, [p], FR.INSTANTS, on_equal, ctx=ctx) == \
                (first, verdicts, [-1 if v == A else 0 for v in verdicts]), f"seed {seed} pod{p}"


def test_a_single_instant_is_paged_preempt_gangs_of_without_candidates(oracle_mod):
    cases = [PPGR.DIRECTED[name][0]()[:2] for name in sorted(PPGR.DIRECTED)]
    for seed, factor in R.CASES[:3]:
        snaps, gangs, _, _ = R.wide_reference(seed, factor, oracle_mod)
        cases += [(snaps, g) for g in gangs]
    for snaps, members in cases:
        for on_equal in (False, True):
            prefix, _, blocker = paging.paged_preempt_gangs_of(snaps, members, [], NOW, on_equal)
            first, _, blockers = paging.paged_forecast_gangs_of(snaps, members, [NOW], on_equal)
            assert (first == 0) == (prefix == 0) and blockers[0] == blocker, (members, on_equal)


# ---- the C-ABI ----
PROGRAM = r'''
#include "kt_engine.h"
typedef int32_t (*paged_forecast_gangs_fn)(kt_engine* const*, int32_t, int64_t, const int64_t*, int64_t, const int64_t*, int64_t, const int64_t*,
                                           const int32_t*, int32_t, int64_t*, uint8_t*, int64_t*);
int main(void) {
  paged_forecast_gangs_fn f = kt_paged_forecast_gangs;
  /* no page set is refused before anything else is looked at */
  return f(0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0) == KT_ERR_INVALID_ARGUMENT ? 0 : 2;
}
'''


def test_abi_symbol_signature_and_binding(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    assert hasattr(lib, "kt_paged_forecast_gangs") and "kt_paged_forecast_gangs" in E.EXPORTS
    src = tmp_path / "paged_forecast_gangs_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "paged_forecast_gangs_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert E.lib().kt_paged_forecast_gangs.argtypes == [C.POINTER(p), i32, i64, p, i64, p, i64, p, p, i32, p, p, p]
    assert callable(E.paged_forecast_gangs) and callable(paging.PagedEngine.forecast_gangs) and callable(paging.paged_forecast_gangs_of)
