"""The paged admission forecast (kt_paged_forecast), pinned on the CPU.

``paging.paged_forecast_of`` — the closed form kt_kernels_forecast_paged.hip computes per lane: per page CalculateThreshold at the
lane's instant, ONE "differs" fact over all pages (status.calculatedThreshold is compared and replaced as a whole), the count
part once and every page's name part of the four steps — is held to the reference of tests/paged_forecast_reference.py: per
instant a copy of every page, the oracle's reconcile per page, the OR of the calc_updated / error bytes, the oracle's check per
page, combined.  Random clusters over 20 to 40 resource names (odd seeds with a stored status written back, even seeds never
reconciled) and directed cases with their answers written out.  tests/test_paged_forecast_gpu.py holds the kernel to the same
reference."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import forecast_reference as FR
import paged_forecast_reference as PFR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kube_throttler_amd", "csrc")
NOW = PFR.NOW
A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK

# Chosen on the CPU so that the REFERENCE meets the bounds of test_the_cases_cover_every_outcome (seeds divisible by 4 hold pods of
# a namespace without object, seed 10 selectors that do not convert).  Observed over these seeds with on_equal = False: 84 cases,
# first = 0: 23, first >= 1: 22, none: 39, at least two flips: 32, a later page decides: 36, the whole-threshold rule decides: 9.
SEEDS = [3, 7, 8, 10, 14, 19, 29, 32, 34, 46, 51, 52, 57, 58]


@functools.lru_cache(maxsize=None)
def paged_case(seed, oracle_mod):
    """(page snapshots, pod rows, {on_equal: reference verdicts [pods][instants]}) — computed once, never modified."""
    snaps, pods = PFR.wide_case(seed, oracle_mod)
    assert 2 <= len(snaps) <= 3 and 20 <= sum(s.D for s in snaps) <= 40
    want = {eq: PFR.reference_verdicts(snaps, oracle_mod, pods, FR.INSTANTS, eq) for eq in (False, True)}
    return snaps, pods, want


def test_some_last_page_is_narrow_and_some_cluster_has_three_pages(oracle_mod):
    shapes = [[s.D for s in paged_case(seed, oracle_mod)[0]] for seed in SEEDS]
    assert any(sh[-1] < S.KT_MAX_DIMS for sh in shapes) and any(len(sh) == 3 for sh in shapes) and any(len(sh) == 2 for sh in shapes), shapes


@pytest.mark.parametrize("seed", SEEDS)
def test_closed_form_equals_the_reference_on_wide_clusters(seed, oracle_mod):
    snaps, pods, want = paged_case(seed, oracle_mod)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for on_equal in (False, True):
        firsts = FR.first_of(want[on_equal])
        for i, p in enumerate(pods):
            first, verdicts = paging.paged_forecast_of(snaps, p, FR.INSTANTS, on_equal, ctx=ctx)
            assert verdicts == want[on_equal][i].tolist(), f"seed {seed} on_equal={on_equal} pod{p}"
            assert first == firsts[i], f"seed {seed} on_equal={on_equal} pod{p}: {first} != {firsts[i]}"


@pytest.mark.parametrize("seed", [1, 4, 5])
def test_one_page_is_forecast_of(seed, oracle_mod):
    from test_forecast_cpu import forecast_case
    snap, pods, _ = forecast_case(seed, oracle_mod)
    for on_equal in (False, True):
        for p in pods:
            assert paging.paged_forecast_of([snap], p, FR.INSTANTS, on_equal) == paging.forecast_of(snap, p, FR.INSTANTS, on_equal), f"seed {seed} pod{p}"
    for name, make in FR.DIRECTED.items():
        snap, p, inst = make()
        assert paging.paged_forecast_of([snap], p, inst) == paging.forecast_of(snap, p, inst), name


@pytest.mark.parametrize("seed", SEEDS)
def test_every_page_gives_the_same_instants(seed, oracle_mod):
    snaps, _, _ = paged_case(seed, oracle_mod)
    lists = [paging.override_instants_of(s, NOW, FR.BEYOND) for s in snaps]
    assert lists[0] and all(got == lists[0] for got in lists[1:])


def test_the_cases_cover_every_outcome(oracle_mod):
    """Conditions on the inputs, on the reference side alone: a weak generator cannot hide a failure."""
    rows, page0, ored = [], [], []
    for seed in SEEDS:
        snaps, pods, want = paged_case(seed, oracle_mod)
        for eq in (False, True):
            own = PFR.own_rows(snaps, oracle_mod, pods, FR.INSTANTS, eq)
            rows += list(want[eq])
            page0 += list(own[0])
            ored += list(PFR.or_of_pages(own))
    firsts = FR.first_of(rows)
    zero, later, none = sum(k == 0 for k in firsts), sum(k >= 1 for k in firsts), sum(k == -1 for k in firsts)
    twice = sum(FR.flips(row) >= 2 for row in rows)
    later_page = sum(bool((a != b).any()) for a, b in zip(rows, page0))  # the joint row is not page 0's own row
    whole = sum(bool((a != b).any()) for a, b in zip(rows, ored))        # ... and not the OR of the pages' own rows
    shares = (f"{len(rows)} cases, first = 0: {zero}, first >= 1: {later}, none: {none}, flips >= 2: {twice}, a later page decides: "
              f"{later_page}, the whole-threshold rule decides: {whole}")
    assert 10 * zero >= len(rows), shares
    assert 10 * later >= len(rows), shares
    assert 10 * none >= len(rows), shares
    assert 10 * twice >= len(rows), shares
    assert 10 * later_page >= len(rows), shares
    assert whole >= 1, shares


# ---- directed cases, with their answers written out ----
def _joint(snaps, oracle_mod, p, instants, answer, on_equal=False):
    want = PFR.reference_verdicts(snaps, oracle_mod, [p], instants, on_equal)[0].tolist()
    assert (FR.first_of([want])[0], want) == answer
    assert paging.paged_forecast_of(snaps, p, instants, on_equal) == answer


@pytest.mark.parametrize("name", sorted(PFR.DIRECTED))
def test_directed_cases_shared_with_the_gpu_suite(name, oracle_mod):
    snaps, p, instants, answer = PFR.DIRECTED[name]()
    assert len(snaps) == 2
    _joint(snaps, oracle_mod, p, instants, answer)


def test_directed_the_pages_own_answers_do_not_combine(oracle_mod):
    snaps, p, instants, answer = PFR.DIRECTED["later-page-replaces-the-threshold"]()
    assert answer == (0, [A, A, A, B, B])
    own = PFR.own_rows(snaps, oracle_mod, [p], instants)
    assert [o[0].tolist() for o in own] == [[B] * 5, [A] * 5]  # page 0 keeps spec {cpu: 1} throughout, page 1 never stops the pod
    assert [paging.forecast_of(s, p, instants)[1] for s in snaps] == [[B] * 5, [A] * 5]
    assert PFR.or_of_pages(own)[0].tolist() == [B] * 5
    # the replacing page holds nothing the pod requests: still page 1 decides which threshold page 0 reads
    snaps, p, instants, answer = PFR.DIRECTED["replacing-page-holds-nothing-the-pod-asks"]()
    assert answer == (0, [A, A, A, B, B])
    assert int(snaps[1].pod_flags[p]) & S.POD_VALID and not any(int(v) for v in paging.pod_requests(snaps[1], p).values())


def test_directed_stored_status_on_every_page_and_count_judged_once(oracle_mod):
    snaps, p, instants, answer = PFR.DIRECTED["error-throttle-stopping-name-on-page-1"]()
    assert answer == (-1, [B] * 5)
    assert paging.forecast_of(snaps[0], p, instants) == (0, [A] * 5)  # page 0 alone: cpu 6 under the stored spec 100
    snaps, p, instants, answer = PFR.DIRECTED["count-only-override"]()
    assert answer == (2, [B, B, A, A, A, A, B, B, B])


def flags_disagree(oracle_mod, both):
    """The whole-threshold cluster reconciled at NOW with the OR-ed bytes, the status applied to page 1 alone (``both``: to both
    pages): between a paged reconcile that applies and the host's write-back the pages' calculatedAt flags may disagree."""
    snaps, p, instants, _ = PFR.DIRECTED["later-page-replaces-the-threshold"]()
    rows = PR.responsible_rows(snaps[0])
    results = [oracle_mod.Oracle(s).reconcile(NOW, rows=rows) for s in snaps]
    updated = np.zeros(len(rows), np.uint8)
    for r in results:
        updated |= (np.asarray(r.calc_updated[:len(rows)]) != 0).astype(np.uint8)
    assert updated.tolist() == [1] and [int(r.calc_updated[0]) for r in results] == [0, 1]
    for k, (s, r) in enumerate(zip(snaps, results)):
        if both or k == 1:
            s.apply_status(r.used, r.calc, updated, r.thrl_flag, r.thrl_has, r.thrl_pod, r.error, rows=rows)
    return snaps, p, instants


def test_directed_calculated_at_flags_disagree(oracle_mod):
    answer = (0, [A, A, A, B, B])  # the stored {r19: 5} is read until the override ends, then replaced by spec {cpu: 1}
    snaps, p, instants = flags_disagree(oracle_mod, both=True)
    assert [bool(int(s.thr_flags[0]) & S.THR_CALC_AT_NONZERO) for s in snaps] == [True, True]
    _joint(snaps, oracle_mod, p, instants, answer)
    snaps, p, instants = flags_disagree(oracle_mod, both=False)
    assert [bool(int(s.thr_flags[0]) & S.THR_CALC_AT_NONZERO) for s in snaps] == [False, True]
    assert paging.paged_forecast_of(snaps, p, instants) == answer


# ---- the C-ABI ----
PROGRAM = r'''
#include "kt_engine.h"
typedef int32_t (*paged_forecast_fn)(kt_engine* const*, int32_t, int64_t, const int64_t*, int64_t, const int64_t*, const int32_t*, int32_t,
                                     int64_t*, uint8_t*);
int main(void) {
  paged_forecast_fn f = kt_paged_forecast;
  /* no page set is refused before anything else is looked at */
  return f(0, 0, 0, 0, 1, 0, 0, 0, 0, 0) == KT_ERR_INVALID_ARGUMENT ? 0 : 2;
}
'''


def test_abi_symbol_signature_and_binding(tmp_path):
    E.build()
    lib = C.CDLL(E.LIB_PATH)
    assert hasattr(lib, "kt_paged_forecast") and "kt_paged_forecast" in E.EXPORTS
    src = tmp_path / "paged_forecast_abi.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "paged_forecast_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include", str(src), f"-L{CSRC}",
                           "-lkt_engine", f"-Wl,-rpath,{CSRC}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert E.lib().kt_paged_forecast.argtypes == [C.POINTER(p), i32, i64, p, i64, p, p, i32, p, p]
    assert callable(E.paged_forecast) and callable(paging.PagedEngine.forecast) and callable(paging.PagedEngine.override_instants)
