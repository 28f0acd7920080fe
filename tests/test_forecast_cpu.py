"""The admission forecast (kt_forecast_launch), pinned on the CPU.

``paging.forecast_of`` — the closed form kt_kernels_forecast.hip computes per lane: CalculateThreshold at the lane's instant
(first active override wins per name and for the count), replaced only where it differs from the stored calculatedThreshold, read
by the check iff calculatedAt was non-zero or it is replaced, throttled from a fresh aggregate, the four CheckThrottledFor steps —
is held to the reference of tests/forecast_reference.py: per instant a copy of the snapshot, the oracle's reconcile, the oracle's
check.  Random manifest clusters of up to 60 pods x 12 throttles with overrides on most throttles (odd seeds with a stored status
written back by a reconcile, even seeds with the status of a cluster nobody has reconciled yet) and directed cases.
tests/test_forecast_gpu.py holds the kernel to the same reference."""
import functools

import numpy as np
import pytest

import forecast_reference as FR
import preempt_reference as PR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_paged_admit_cpu import write_status

# Chosen on the CPU so that the REFERENCE meets the bounds of test_the_cases_cover_every_outcome (seeds divisible by 4 hold pods
# of a namespace without object, seeds divisible by 5 selectors that do not convert).  Observed over these seeds, both on_equal
# values together: 256 cases, first = 0: 82 (32 %), first >= 1: 61 (24 %), none: 113 (44 %), at least two flips: 79 (31 %).
SEEDS = [1, 3, 4, 5, 8, 10, 14, 19, 20, 23, 36, 37, 46, 49, 56, 60]


@functools.lru_cache(maxsize=None)
def forecast_case(seed, oracle_mod):
    """(snapshot, pod rows, {on_equal: reference verdicts [pods][instants]}) — computed once, never modified."""
    cs = FR.forecast_cluster(seed)
    if seed % 2:
        write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1
    snap = pages[0].snapshot
    assert snap.n_pods <= 60 and snap.n_thr <= 12
    pods = FR.forecast_pods(seed, snap)
    states = [FR.state_at(snap, oracle_mod, t) for t in FR.INSTANTS]
    want = {eq: FR.reference_verdicts(snap, oracle_mod, pods, FR.INSTANTS, eq, states=states) for eq in (False, True)}
    return snap, pods, want


@pytest.mark.parametrize("seed", SEEDS)
def test_forecast_of_equals_reconcile_check_per_instant(seed, oracle_mod):
    snap, pods, want = forecast_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, FR.NOW)
    for on_equal in (False, True):
        firsts = FR.first_of(want[on_equal])
        for i, p in enumerate(pods):
            first, verdicts = paging.forecast_of(snap, p, FR.INSTANTS, on_equal, ctx=ctx)
            assert verdicts == want[on_equal][i].tolist(), f"seed {seed} on_equal={on_equal} pod{p}"
            assert first == firsts[i], f"seed {seed} on_equal={on_equal} pod{p}: {first} != {firsts[i]}"


def test_the_cases_cover_every_outcome(oracle_mod):
    """Conditions on the inputs, on the reference side alone: a weak generator cannot hide a failure."""
    rows = [row for seed in SEEDS for eq in (False, True) for row in forecast_case(seed, oracle_mod)[2][eq]]
    firsts = FR.first_of(rows)
    zero, later, none = sum(k == 0 for k in firsts), sum(k >= 1 for k in firsts), sum(k == -1 for k in firsts)
    twice = sum(FR.flips(row) >= 2 for row in rows)
    shares = f"{len(rows)} cases, first = 0: {zero}, first >= 1: {later}, none: {none}, flips >= 2: {twice}"
    assert 10 * zero >= len(rows), shares
    assert 10 * later >= len(rows), shares
    assert 10 * none >= len(rows), shares
    assert 10 * twice >= len(rows), shares


@pytest.mark.parametrize("seed", SEEDS)
def test_override_instants_of_misses_no_change(seed, oracle_mod):
    """Brute force: CalculateThreshold through the oracle at consecutive candidate instants — where the calculated threshold of
    some responsible throttle differs between t - 1 ns and t, t must be listed; and the list is sorted, distinct and inside
    (from, until]."""
    snap, _, _ = forecast_case(seed, oracle_mod)
    rows = PR.responsible_rows(snap)
    lo, hi = FR.NOW, FR.BEYOND
    got = paging.override_instants_of(snap, lo, hi)
    assert got == sorted(set(got)) and all(lo < t <= hi for t in got)
    blank = PR.copy_snapshot(snap)  # (no stored threshold: every reconcile reports the one it computes)
    for t in rows:
        blank.thr_calc.set_row(int(t), {}, None)
        blank.thr_flags[t] &= ~np.uint32(S.THR_CALC_AT_NONZERO)
        blank.thr_status_msgs_fp[t] = 0
    o = oracle_mod.Oracle(blank)

    def threshold_at(t):
        r = o.reconcile(t, rows=rows)
        return r.calc.v[:len(rows)].tolist(), r.calc.present[:len(rows)].tolist(), r.calc.count[:len(rows)].tolist(), \
            r.calc.has_count[:len(rows)].tolist()
    candidates = [t for t in FR.instants_under_test() if lo < t <= hi]
    changes = [t for t in candidates if threshold_at(FR.shift(t, -1)) != threshold_at(t)]
    assert set(changes) <= set(got), f"seed {seed}: a threshold changes at {sorted(set(changes) - set(got))}, which is not listed"
    # ... and a half-open window drops exactly the instants outside it
    mid = FR.BOUNDARIES[5]
    assert paging.override_instants_of(snap, lo, mid) == [t for t in got if t <= mid]
    assert paging.override_instants_of(snap, mid, hi) == [t for t in got if t > mid]


def test_override_instants_of_end_is_end_plus_one_ns():
    snap = FR.timed(FR._run({0: 10}), 0, [(FR.T1, FR.T2, {0: 100}, None), (None, (FR.T3[0], 999_999_999), {0: 1}, None),
                                           (FR.T4, None, {0: 1}, None, S.OVR_PARSE_ERROR | FR.BEGIN_PARSED)])
    assert paging.override_instants_of(snap, FR.T0, FR.BEYOND) == [FR.T1, FR.shift(FR.T2, 1), (FR.T3[0] + 1, 0)]
    assert paging.override_instants_of(snap, FR.T1, FR.T2) == []  # (from, until]: T1 itself is outside, T2 + 1 ns beyond
    snap.thr_flags[0] &= ~np.uint32(S.THR_RESPONSIBLE)
    assert paging.override_instants_of(snap, FR.T0, FR.BEYOND) == []


# ---- directed cases on snapshots built by hand (forecast_reference.DIRECTED) ----
def _both(snap, oracle_mod, p, instants, on_equal=False):
    want = FR.reference_verdicts(snap, oracle_mod, [p], instants, on_equal)[0].tolist()
    first, verdicts = paging.forecast_of(snap, p, instants, on_equal)
    assert verdicts == want, (verdicts, want)
    assert first == FR.first_of([want])[0]
    return first, verdicts


@pytest.mark.parametrize("name", sorted(FR.DIRECTED))
def test_directed_cases_shared_with_the_gpu_suite(name, oracle_mod):
    snap, p, instants = FR.DIRECTED[name]()
    for on_equal in (False, True):
        _both(snap, oracle_mod, p, instants, on_equal)


def test_directed_inclusive_begin_and_end(oracle_mod):
    A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK
    # EDGE = T0, T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, T3, T4
    snap, p, inst = FR.DIRECTED["window-opens-inclusive"]()
    assert _both(snap, oracle_mod, p, inst) == (2, [B, B, A, A, A, A, B, B, B])  # passes at `end`, fails at end + 1 ns
    snap, p, inst = FR.DIRECTED["window-closes-inclusive"]()
    assert _both(snap, oracle_mod, p, inst) == (0, [A, A, B, B, B, B, A, A, A])
    snap, p, inst = FR.DIRECTED["begin-equals-end"]()
    assert _both(snap, oracle_mod, p, inst) == (5, [B, B, B, B, B, A, B, B, B])


def test_directed_merge_of_overlapping_overrides(oracle_mod):
    A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK
    snap, p, inst = FR.DIRECTED["overlap-first-wins-second-supplies-count"]()
    # T1 .. T2 - 1: only the first (passes); T2 .. T3: both — name 0 from the first, the count 2 from the second (2 pods run:
    # blocked); T3 + 1 .. T4: only the second (cpu 5 < used 8: blocked); beyond: spec
    assert _both(snap, oracle_mod, p, inst) == (2, [B, B, A, A, A, B, B, B, B, B, B])
    snap, p, inst = FR.DIRECTED["overlap-first-wins-per-name"]()
    assert _both(snap, oracle_mod, p, inst) == (2, [B, B, A, A, A, A, B, B, B, B])
    snap, p, inst = FR.DIRECTED["override-omits-the-name"]()
    assert _both(snap, oracle_mod, p, inst) == (2, [B, B, A, A, A, A, B, B, B])


def test_directed_which_threshold_the_check_reads(oracle_mod):
    A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK
    snap, p, inst = FR.DIRECTED["unreconciled-empty-override-keeps-spec"]()
    assert _both(snap, oracle_mod, p, inst) == (-1, [B] * 9)  # the empty override is never read: nothing replaces, spec stays
    snap, p, inst = FR.DIRECTED["unreconciled-equal-to-empty-stored"]()
    assert _both(snap, oracle_mod, p, inst) == (0, [A] * 9)
    snap, p, inst = FR.DIRECTED["error-throttle-active-override"]()
    assert _both(snap, oracle_mod, p, inst) == (0, [A] * 9)  # the stored status, at every instant
    snap, p, inst = FR.DIRECTED["parse-error-override"]()
    assert _both(snap, oracle_mod, p, inst) == (-1, [B] * 9)


def test_directed_exceeds_and_errors(oracle_mod):
    A, B, E = S.VERDICT_ALLOW, S.VERDICT_BLOCK, S.VERDICT_ERROR
    snap, p, inst = FR.DIRECTED["override-below-the-request"]()
    assert _both(snap, oracle_mod, p, inst) == (0, [A, A, B, B, B, B, A, A, A])
    snap, p, inst = FR.DIRECTED["never-passes"]()
    assert _both(snap, oracle_mod, p, inst) == (-1, [B] * 9)
    snap, p, inst = FR.DIRECTED["no-throttle-affects-the-pod"]()
    assert _both(snap, oracle_mod, p, inst) == (0, [A] * 9)
    snap, p, inst = FR.DIRECTED["pod-in-a-namespace-without-object"]()
    assert _both(snap, oracle_mod, p, inst) == (-1, [E] * 9)
    snap.pod_flags[0] = 0  # an invalid row
    assert paging.forecast_of(snap, 0, inst) == (-1, [E] * 9)
    assert paging.forecast_of(snap, 99, inst) == (-1, [E] * 9)


@pytest.mark.parametrize("cluster", [False, True])
def test_directed_on_equal_at_exact_equality(cluster, oracle_mod):
    A, B = S.VERDICT_ALLOW, S.VERDICT_BLOCK
    snap, p, inst = FR.DIRECTED["equality-clusterthrottle" if cluster else "equality-throttle"]()
    # spec 10 = used 8 + 2: step 4 passes only without on_equal; the override 8 = used: step 3, a Throttle's is always on-equal
    assert _both(snap, oracle_mod, p, inst, True) == (-1, [B] * 9)
    # without on_equal the spec passes; inside the window used 8 >= the override's 8: throttled (IsThrottled(used, true)), step 2
    assert _both(snap, oracle_mod, p, inst, False) == (0, [A, A, B, B, B, B, A, A, A])
    snap, p, inst = FR.DIRECTED["equality-step3-clusterthrottle" if cluster else "equality-step3-throttle"]()
    window = [A, A, B, B, B, B, A, A, A]
    assert _both(snap, oracle_mod, p, inst, True) == (0, window)
    assert _both(snap, oracle_mod, p, inst, False) == (0, [A] * 9 if cluster else window)


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_single_instant_agrees_with_preempt_prefix_zero(name, oracle_mod):
    """With inst = [now], first == 0 exactly where the preemption query at `now` reports prefix 0."""
    snap, p, cands = PR.DIRECTED[name]()
    for on_equal in (False, True):
        k = PR.reference_prefix(snap, oracle_mod, p, cands, PR.NOW, on_equal)
        first, _ = _both(snap, oracle_mod, p, [PR.NOW], on_equal)
        assert (first == 0) == (k == 0), (first, k)
