"""The headroom forecast (kt_headroom_forecast_launch), pinned on the CPU.

``paging.headroom_forecast_of`` — the closed form kt_kernels_headroom_forecast.hip computes per lane: ``forecast_of``'s threshold
at the lane's instant, ``headroom_of``'s term per amount, the lexicographic minimum of (copies, throttle row) — is held to the
reference of tests/headroom_forecast_reference.py: per instant a copy of the snapshot, the oracle's reconcile, the oracle's admit
of ``[pod] * cap``.  The random clusters and the shared directed cases are those of the forecast (tests/forecast_reference.py);
tests/test_headroom_forecast_gpu.py holds the kernel to the same reference."""
import functools

import pytest

import forecast_reference as FR
import headroom_forecast_reference as HR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_forecast_cpu import forecast_case

CAP = HR.CAP
# test_forecast_cpu.SEEDS as they stand: checked on the CPU, the REFERENCE meets the bounds of test_the_cases_cover_every_outcome
# below with them.  Observed over these seeds, both on_equal values together: 256 (pod, on_equal) rows, copies 0 at every
# instant: 113 (44 %), cap at some instant: 105 (41 %), strictly between 0 and cap at some instant: 53 (21 %), at least two
# distinct values: 109 (43 %), a limiting row that changes between instants: 109 (43 %).
SEEDS = [1, 3, 4, 5, 8, 10, 14, 19, 20, 23, 36, 37, 46, 49, 56, 60]


@functools.lru_cache(maxsize=None)
def headroom_forecast_case(seed, oracle_mod):
    """(snapshot, pod rows, {on_equal: (copies, limiting) [pods][instants]}) — computed once, never modified."""
    snap, pods, _ = forecast_case(seed, oracle_mod)
    states = [FR.state_at(snap, oracle_mod, t) for t in FR.INSTANTS]
    want = {eq: HR.reference(snap, oracle_mod, pods, FR.INSTANTS, CAP, eq, states=states) for eq in (False, True)}
    return snap, pods, want


def _both(snap, oracle_mod, p, instants, on_equal=False, cap=CAP, want=1):
    copies, limiting = HR.reference(snap, oracle_mod, [p], instants, cap, on_equal)
    got = paging.headroom_forecast_of(snap, p, instants, cap, want, on_equal)
    assert got[1] == copies[0].tolist(), (got[1], copies[0].tolist())
    assert got[2] == limiting[0].tolist(), (got[2], limiting[0].tolist())
    assert got[0] == HR.first_of(copies, want)[0]
    return got


@pytest.mark.parametrize("seed", SEEDS)
def test_closed_form_equals_reconcile_admit_per_instant(seed, oracle_mod):
    snap, pods, want = headroom_forecast_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, FR.NOW)
    for on_equal in (False, True):
        copies, limiting = want[on_equal]
        for w in (1, CAP):
            firsts = HR.first_of(copies, w)
            for i, p in enumerate(pods):
                got = paging.headroom_forecast_of(snap, p, FR.INSTANTS, CAP, w, on_equal, ctx=ctx)
                assert got[1] == copies[i].tolist(), f"seed {seed} on_equal={on_equal} pod{p}"
                assert got[2] == limiting[i].tolist(), f"seed {seed} on_equal={on_equal} pod{p}"
                assert got[0] == firsts[i], f"seed {seed} on_equal={on_equal} pod{p} want={w}"


def test_the_cases_cover_every_outcome(oracle_mod):
    """Conditions on the inputs, on the reference side alone: a weak generator cannot hide a failure."""
    rows = []
    for seed in SEEDS:
        for eq in (False, True):
            copies, limiting = headroom_forecast_case(seed, oracle_mod)[2][eq]
            rows += list(zip(copies.tolist(), limiting.tolist()))
    never = sum(all(c == 0 for c in cs) for cs, _ in rows)
    full = sum(any(c == CAP for c in cs) for cs, _ in rows)
    between = sum(any(0 < c < CAP for c in cs) for cs, _ in rows)
    distinct = sum(len(set(cs)) >= 2 for cs, _ in rows)
    moves = sum(len(set(ls)) >= 2 for _, ls in rows)
    shares = f"{len(rows)} rows, never: {never}, cap somewhere: {full}, between: {between}, two values: {distinct}, limiting changes: {moves}"
    print(shares)
    for share in (never, full, between, distinct, moves):
        assert 10 * share >= len(rows), shares


@pytest.mark.parametrize("seed", SEEDS)
def test_cap_one_is_the_forecast(seed, oracle_mod):
    """(I1): with cap == want == 1 a copy is admitted exactly where the forecast's verdict is Success."""
    snap, pods, verdicts = forecast_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, FR.NOW)
    for on_equal in (False, True):
        firsts = FR.first_of(verdicts[on_equal])
        for i, p in enumerate(pods):
            first, copies, limiting = paging.headroom_forecast_of(snap, p, FR.INSTANTS, 1, 1, on_equal, ctx=ctx)
            assert copies == [int(v == S.VERDICT_ALLOW) for v in verdicts[on_equal][i]], f"seed {seed} on_equal={on_equal} pod{p}"
            assert first == firsts[i]
            assert all(l == -1 for l, v in zip(limiting, verdicts[on_equal][i]) if v != S.VERDICT_BLOCK)
            assert all(l >= 0 for l, v in zip(limiting, verdicts[on_equal][i]) if v == S.VERDICT_BLOCK)


@pytest.mark.parametrize("name", sorted(FR.DIRECTED))
def test_directed_cases_of_the_forecast(name, oracle_mod):
    snap, p, instants = FR.DIRECTED[name]()
    for on_equal in (False, True):
        _both(snap, oracle_mod, p, instants, on_equal)


@pytest.mark.parametrize("name", sorted(HR.DIRECTED))
def test_directed_cases_shared_with_the_gpu_suite(name, oracle_mod):
    snap, p, instants = HR.DIRECTED[name]()
    for on_equal in (False, True):
        for want in (1, 2, CAP):
            _both(snap, oracle_mod, p, instants, on_equal, want=want)


def test_directed_count_override_raises_the_copies(oracle_mod):
    # EDGE = T0, T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, T3, T4; two pods run: count 2 admits nobody, count 5 three copies
    snap, p, inst = HR.DIRECTED["count-2-to-5"]()
    assert _both(snap, oracle_mod, p, inst) == (2, [0, 0, 3, 3, 3, 3, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0])
    assert _both(snap, oracle_mod, p, inst, want=3)[0] == 2
    assert _both(snap, oracle_mod, p, inst, want=4)[0] == -1


def test_directed_tie_reports_the_lower_row(oracle_mod):
    snap, p, inst = HR.DIRECTED["tie-lower-row-limits"]()
    assert _both(snap, oracle_mod, p, inst) == (0, [1, 1, 2, 2, 2, 2, 1, 1, 1], [1, 1, 0, 0, 0, 0, 1, 1, 1])


def test_directed_special_pods(oracle_mod):
    snap, p, inst = FR.DIRECTED["no-throttle-affects-the-pod"]()
    assert _both(snap, oracle_mod, p, inst) == (0, [CAP] * 9, [-1] * 9)
    snap, p, inst = FR.DIRECTED["pod-in-a-namespace-without-object"]()
    assert _both(snap, oracle_mod, p, inst) == (-1, [0] * 9, [-1] * 9)
    snap.pod_flags[0] = 0  # an invalid row
    assert _both(snap, oracle_mod, 0, inst) == (-1, [0] * 9, [-1] * 9)
    assert paging.headroom_forecast_of(snap, 99, inst, CAP) == (-1, [0] * 9, [-1] * 9)


def test_the_largest_cap_against_a_threshold_of_two_to_the_62():
    """Closed form only (no queue of 2^31 pods can be walked).  used = 2 x 4 = 8, the pod asks 2^32, the override's threshold is
    2^62 + 8: without on_equal copy j passes while 8 + (j + 1) 2^32 <= 2^62 + 8, 2^30 copies; with on_equal the inequality is
    strict, 2^30 - 1 copies.  Outside the window the spec's 10 is below the request: step 1, no copy."""
    cap = 2**31 - 1
    snap = FR.timed(FR._run({0: 10}, ask=2**32), 0, [(FR.T1, FR.T2, {0: 2**62 + 8}, None)])
    window = [0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert paging.headroom_forecast_of(snap, 0, FR.EDGE, cap, 2**30) == (2, [2**30 * w for w in window], [0] * 9)
    assert paging.headroom_forecast_of(snap, 0, FR.EDGE, cap, 2**30, on_equal=True) == (-1, [(2**30 - 1) * w for w in window], [0] * 9)
    # ... and a request of 1: 2^62 units of room admit every one of the 2^31 - 1 copies
    snap = FR.timed(FR._run({0: 10}, ask=1, each=5), 0, [(FR.T1, FR.T2, {0: 2**62}, None)])
    assert paging.headroom_forecast_of(snap, 0, FR.EDGE, cap, cap) == (2, [cap * w for w in window], [-1 if w else 0 for w in window])
