"""The gang forecast (kt_forecast_gangs_launch), pinned on the CPU.

``paging.forecast_gangs_of`` — the closed form kt_kernels_forecast_gangs.hip computes per lane: the threshold of
``paging.forecast_of`` at the lane's instant, met by the members in order under the reserved prefix — is held to the reference of
tests/forecast_gangs_reference.py: per instant a copy of the snapshot, the oracle's reconcile, the oracle's in-order admission of
the members.  Generator A couples the members through one throttle whose levels sit where their sums land; generator B draws gangs
on the manifest clusters of tests/test_forecast_cpu.py (error selectors, pods of a namespace without object, several throttles
and names).  tests/test_forecast_gangs_gpu.py holds the kernel to the same reference."""
import pytest

import forecast_gangs_reference as FG
import forecast_reference as FR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_forecast_cpu import SEEDS


def _same(got, want, what):
    first, verdicts, blockers = got
    assert [int(v) for v in verdicts] == want[1], f"{what}: verdicts {list(verdicts)} != {want[1]}"
    assert [int(b) for b in blockers] == want[2], f"{what}: blockers {list(blockers)} != {want[2]}"
    assert int(first) == want[0], f"{what}: first {first} != {want[0]}"


@pytest.mark.parametrize("seed", FG.STAIR_SEEDS)
def test_generator_a_equals_reconcile_admit_per_instant(seed, oracle_mod):
    snap, members, inst, want, _ = FG.stair_reference(seed, oracle_mod)
    ctx = paging.preempt_context(snap, FR.NOW)
    for on_equal in (False, True):
        _same(paging.forecast_gangs_of(snap, members, inst, on_equal, ctx=ctx), want[on_equal], f"seed {seed} on_equal={on_equal}")


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_b_equals_reconcile_admit_per_instant(seed, oracle_mod):
    snap, gangs, want, _ = FG.cluster_reference(seed, oracle_mod)
    ctx = paging.preempt_context(snap, FR.NOW)
    for on_equal in (False, True):
        for g, members in enumerate(gangs):
            _same(paging.forecast_gangs_of(snap, members, FR.INSTANTS, on_equal, ctx=ctx), want[on_equal][g],
                  f"seed {seed} on_equal={on_equal} gang {members}")


@pytest.mark.parametrize("name", sorted(FG.DIRECTED))
def test_directed_cases_shared_with_the_gpu_suite(name, oracle_mod):
    snap, members, inst = FG.DIRECTED[name]()
    for on_equal in (False, True):
        _same(paging.forecast_gangs_of(snap, members, inst, on_equal), FG.reference(snap, oracle_mod, members, inst, on_equal),
              f"{name} on_equal={on_equal}")


def _tenth(count, total, share=10):
    return 100 * count >= share * total


def test_the_cases_cover_every_outcome(oracle_mod):
    """Conditions on the inputs, on the reference side alone: a weak generator cannot hide a failure."""
    rows, differs, moves = [], 0, 0
    for seed in FG.STAIR_SEEDS:
        _, _, _, want, alone = FG.stair_reference(seed, oracle_mod)
        for eq in (False, True):
            first, verdicts, blockers = want[eq]
            rows.append((first, verdicts))
            differs += verdicts != alone[eq]
            moves += len({b for b in blockers if b >= 0}) >= 2
    n = len(rows)
    assert n == 120
    zero, later, none = sum(f == 0 for f, _ in rows), sum(f >= 1 for f, _ in rows), sum(f == -1 for f, _ in rows)
    twice = sum(FR.flips(v) >= 2 for _, v in rows)
    shares = f"{n} cases, first = 0: {zero}, first >= 1: {later}, none: {none}, flips >= 2: {twice}, differs: {differs}, blocker moves: {moves}"
    print(shares)
    assert _tenth(zero, n) and _tenth(later, n) and _tenth(none, n) and _tenth(twice, n), shares
    assert _tenth(differs, n, 20), shares
    assert _tenth(moves, n, 15), shares


def test_the_cluster_cases_cover_every_outcome(oracle_mod):
    rows, errors = [], 0
    for seed in SEEDS:
        _, gangs, want, bad = FG.cluster_reference(seed, oracle_mod)
        for eq in (False, True):
            rows += [(first, verdicts) for first, verdicts, _ in want[eq]]
            errors += sum(bad)
    n = len(rows)
    assert n == 128
    zero, later, none = sum(f == 0 for f, _ in rows), sum(f >= 1 for f, _ in rows), sum(f == -1 for f, _ in rows)
    twice = sum(FR.flips(v) >= 2 for _, v in rows)
    shares = f"{n} cases, first = 0: {zero}, first >= 1: {later}, none: {none}, flips >= 2: {twice}, an Error member: {errors}"
    print(shares)
    assert _tenth(zero, n) and _tenth(later, n) and _tenth(none, n) and _tenth(twice, n) and _tenth(errors, n), shares


def test_directed_the_example_and_its_neighbours(oracle_mod):
    A, B, E = S.VERDICT_ALLOW, S.VERDICT_BLOCK, S.VERDICT_ERROR
    window = [B, B, A, A, A, A, B, B, B]  # EDGE = T0, T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, T3, T4
    snap, members, inst = FG.DIRECTED["each-alone-passes-the-gang-only-in-the-window"]()
    assert paging.forecast_gangs_of(snap, members, inst) == (2, window, [-1 if v == A else 1 for v in window])
    for p in members:  # each member alone passes at every instant
        assert paging.forecast_of(snap, p, inst) == (0, [A] * 9)
    snap, members, inst = FG.DIRECTED["the-same-on-a-pod-count"]()
    assert paging.forecast_gangs_of(snap, members, inst) == (2, window, [-1 if v == A else 1 for v in window])
    snap, members, inst = FG.DIRECTED["member-order-big-small"]()
    assert paging.forecast_gangs_of(snap, members, inst)[:2] == (7, [B] * 7 + [A, A, B])
    snap, members, inst = FG.DIRECTED["member-order-small-big"]()
    assert paging.forecast_gangs_of(snap, members, inst)[:2] == (0, [A] * 10)
    snap, members, inst = FG.DIRECTED["the-blocker-moves-with-the-instant"]()
    assert paging.forecast_gangs_of(snap, members, inst) == (7, [B] * 7 + [A, B], [1, 1, 2, 1, 1, 0, 1, -1, 1])
    snap, members, inst = FG.DIRECTED["member-without-namespace-object-last"]()
    assert paging.forecast_gangs_of(snap, members, inst) == (-1, [E] * 9, [2, 2, 1, 1, 1, 1, 2, 2, 2])
    snap, members, inst = FG.DIRECTED["invalid-member-row-first"]()
    assert paging.forecast_gangs_of(snap, members, inst) == (-1, [E] * 9, [0] * 9)
    snap, members, inst = FG.DIRECTED["error-throttle-stops-the-second-member-only"]()
    assert paging.forecast_gangs_of(snap, members, inst) == (-1, [B] * 9, [1] * 9)
    assert paging.forecast_gangs_of(snap, [99], inst) == (-1, [E] * 9, [0] * 9)  # a row outside the snapshot


@pytest.mark.parametrize("name", sorted(FR.DIRECTED))
def test_a_gang_of_one_is_the_plain_forecast(name):
    snap, p, inst = FR.DIRECTED[name]()
    for on_equal in (False, True):
        first, verdicts = paging.forecast_of(snap, p, inst, on_equal)
        assert paging.forecast_gangs_of(snap, [p], inst, on_equal) == (first, verdicts, [-1 if v == S.VERDICT_ALLOW else 0 for v in verdicts])
