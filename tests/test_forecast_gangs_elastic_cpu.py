"""The elastic gang forecast (kt_forecast_gangs_elastic_launch), pinned on the CPU: the reference of
tests/forecast_gangs_elastic_reference.py (per instant a copy of the snapshot, the oracle's reconcile, the oracle's in-order
admission, then the rule) is held to the identities of the header against the references of its neighbours, to the hand-derived
answers of the directed cases, and to floors that show the generators' cases reach what a throttle-major judge gets wrong.
tests/test_forecast_gangs_elastic_gpu.py holds the kernel to the same reference."""
import pytest

import forecast_gangs_elastic_reference as FE
import forecast_gangs_reference as FG
import forecast_reference as FR
from kube_throttler_amd import snapshot as S
from test_forecast_cpu import SEEDS

A, B, ERR = S.VERDICT_ALLOW, S.VERDICT_BLOCK, S.VERDICT_ERROR


def _whole(ref, size, want):
    """(E1): first, verdicts and blockers are the gang forecast's, the count is the size exactly where the verdict is Success."""
    first, verdicts, counts, blockers = ref
    assert (first, verdicts, blockers) == want
    assert [c == size for c in counts] == [v == A for v in verdicts]


@pytest.mark.parametrize("seed", FG.STAIR_SEEDS)
def test_e1_generator_a(seed, oracle_mod):
    snap, members, inst, want, _ = FG.stair_reference(seed, oracle_mod)
    n = len(members)
    for eq in (False, True):
        _whole(FE.reference(snap, oracle_mod, members, n, None, inst, eq), n, want[eq])
        _whole(FE.reference(snap, oracle_mod, members, 1, [True] * n, inst, eq), n, want[eq])


@pytest.mark.parametrize("seed", SEEDS)
def test_e1_generator_b(seed, oracle_mod):
    snap, gangs, want, _ = FG.cluster_reference(seed, oracle_mod)
    for eq in (False, True):
        for g, members in enumerate(gangs):
            n = len(members)
            _whole(FE.reference(snap, oracle_mod, members, n, None, FR.INSTANTS, eq), n, want[eq][g])
            _whole(FE.reference(snap, oracle_mod, members, 1 + seed % n, [True] * n, FR.INSTANTS, eq), n, want[eq][g])


@pytest.mark.parametrize("name", sorted(FG.DIRECTED))
def test_e1_directed(name, oracle_mod):
    snap, members, inst = FG.DIRECTED[name]()
    n = len(members)
    for eq in (False, True):
        _whole(FE.reference(snap, oracle_mod, members, n, None, inst, eq), n, FG.reference(snap, oracle_mod, members, inst, eq))


@pytest.mark.parametrize("name", sorted(FR.DIRECTED))
def test_e2_a_gang_of_one_is_the_plain_forecast(name, oracle_mod):
    snap, p, inst = FR.DIRECTED[name]()
    for eq in (False, True):
        verdicts = [int(v) for v in FR.reference_verdicts(snap, oracle_mod, [p], inst, eq)[0]]
        first, got, counts, blockers = FE.reference(snap, oracle_mod, [p], 1, None, inst, eq)
        assert (first, got) == (FR.first_of([verdicts])[0], verdicts)
        assert counts == [int(v == A) for v in verdicts] and blockers == [-1 if v == A else 0 for v in verdicts]


@pytest.mark.parametrize("build", [FE.failed_member_reserves_nowhere, FE.failed_member_reserves_nowhere_on_a_count])
def test_a_failed_member_reserves_on_no_throttle(build, oracle_mod):
    """The case a throttle-major judge fails: m0 fails on A and therefore does not weigh on B, where m1 then passes."""
    snap = build()
    ok = FE.successes(snap, oracle_mod, [0, 1, 2], FE.EDGE)
    assert ok == [[True, False, False] if k in FE.WINDOW else [False, True, False] for k in range(len(FE.EDGE))]
    for name, (members, quorum, required, want) in FE.NOWHERE.items():
        assert FE.reference(snap, oracle_mod, members, quorum, required, FE.EDGE) == want, name
    # the whole gang never fits, and the all-or-nothing forecast blames the first member outside the window
    assert FG.reference(snap, oracle_mod, [0, 1, 2], FE.EDGE) == (-1, [B] * 9, FE._by_window(1, 0))


def test_directed_answers_derived_by_hand(oracle_mod):
    def ref(name):
        snap, members, quorum, required, inst = FE.DIRECTED[name]()
        return FE.reference(snap, oracle_mod, members, quorum, required, inst)

    in_w = FE._by_window  # (inside the window T1 .. T2, outside)
    # the Error member never succeeds; the two valid members ask 1 each under 10 (one runs), inside the window under 2
    assert ref("required-error-member-first") == (-1, [ERR] * 9, in_w(1, 2), [0] * 9)
    assert ref("required-error-member-last") == (-1, [ERR] * 9, in_w(1, 2), [2] * 9)
    assert ref("required-invalid-member-last") == (-1, [ERR] * 9, in_w(1, 2), [2] * 9)
    assert ref("error-member-not-required-quorum-2") == (0, in_w(B, A), in_w(1, 2), in_w(0, -1))
    assert ref("error-member-not-required-quorum-1") == (0, [A] * 9, in_w(1, 2), [-1] * 9)
    assert ref("quorum-out-of-reach-by-the-error-member") == (-1, [ERR] * 9, in_w(1, 2), in_w(1, 2))
    assert ref("quorum-out-of-reach-by-the-invalid-member") == (-1, [ERR] * 9, in_w(1, 2), [0] * 9)
    assert ref("gang-no-throttle-affects") == (0, [A] * 9, [2] * 9, [-1] * 9)
    # the middle member is required and no throttle affects it; 4 + 3 + 3 > 8 stops the third outside the window, 10 admits it
    assert ref("member-no-throttle-affects") == (0, [A] * 9, in_w(3, 2), [-1] * 9)
    # used 4 under 8, 10 between T3 and T4: [5, -2] — the first fails outside (9 > 8), the second always passes
    assert ref("member-order-big-small") == (0, [A] * 10, [1] * 7 + [2, 2, 1], [-1] * 10)
    assert ref("member-order-small-big") == (0, [A] * 10, [2] * 10, [-1] * 10)
    # three members of 3, the third required, quorum 2: spec 5 admits one, 7 (at T1) two, 2 (at T2) none, 9 (at T3) all three —
    # and a member behind one that failed is still evaluated: it fails where the first two took the room
    assert ref("the-blocker-moves-with-the-instant") == (7, [B] * 7 + [A, B], [1, 1, 2, 1, 1, 0, 1, 3, 1], [2] * 7 + [-1, 2])
    assert ref("error-throttle-keeps-its-stored-status") == (0, [A] * 9, [1] * 9, [-1] * 9)
    assert ref("stored-reserved-amounts") == (2, in_w(A, B), in_w(2, 0), in_w(-1, 0))


@pytest.mark.parametrize("name", sorted(FE.DIRECTED))
def test_directed_cases_are_well_formed(name, oracle_mod):
    snap, members, quorum, required, inst = FE.DIRECTED[name]()
    for eq in (False, True):
        first, verdicts, counts, blockers = FE.reference(snap, oracle_mod, members, quorum, required, inst, eq)
        assert len(verdicts) == len(counts) == len(blockers) == len(inst)
        assert all((b == -1) == (v == A) and -1 <= b < len(members) for v, b in zip(verdicts, blockers))
        assert all(0 <= c <= len(members) for c in counts)
        assert (ERR in verdicts) == (set(verdicts) == {ERR})


def _behind(ok):
    """A member succeeds BEHIND one that failed."""
    return any(x and not all(ok[:j]) for j, x in enumerate(ok))


def _tally(cases):
    """cases: (size, quorum, (first, verdicts, counts, blockers), success lists, the whole gang's first) per gang, at
    on_equal=False -> (cells admitted with fewer than all members, cells where the quorum is reached but the gang is refused for a
    required member, cells in which a member succeeds behind one that failed, gangs whose first instant differs from the whole
    gang's, gangs that are Error throughout)."""
    partial = required_out = behind = differs = errors = 0
    for size, quorum, (first, verdicts, counts, _), ok, whole_first in cases:
        partial += sum(v == A and c < size for v, c in zip(verdicts, counts))
        required_out += sum(v == B and c >= quorum for v, c in zip(verdicts, counts))
        behind += sum(_behind(o) for o in ok)
        differs += first != whole_first
        errors += set(verdicts) == {ERR}
    return partial, required_out, behind, differs, errors


def test_the_stair_cases_reach_what_all_or_nothing_cannot(oracle_mod):
    """Floors on the REFERENCE alone, at about half of what the cases give (124 / 58 / 164 / 12)."""
    cases = []
    for seed in FG.STAIR_SEEDS:
        _, members, _, quorum, _, want, ok = FE.stair_reference(seed, oracle_mod)
        cases.append((len(members), quorum, want[False], ok[False], FG.stair_reference(seed, oracle_mod)[3][False][0]))
    partial, required_out, behind, differs, _ = _tally(cases)
    print(f"stairs: partial {partial}, quorum reached but a required member out {required_out}, behind a failure {behind}, first differs {differs}")
    assert partial >= 60 and required_out >= 25 and behind >= 80 and differs >= 6


def test_the_cluster_cases_reach_what_all_or_nothing_cannot(oracle_mod):
    """Floors on the REFERENCE alone, at about half of what the cases give (164 / 135 / 489 / 9 / 11)."""
    cases = []
    for seed in SEEDS:
        _, gangs, quorums, _, want, ok = FE.cluster_reference(seed, oracle_mod)
        whole = FG.cluster_reference(seed, oracle_mod)[2][False]
        cases += [(len(m), quorums[g], want[False][g], ok[False][g], whole[g][0]) for g, m in enumerate(gangs)]
    partial, required_out, behind, differs, errors = _tally(cases)
    print(f"clusters: partial {partial}, quorum reached but a required member out {required_out}, behind a failure {behind}, "
          f"first differs {differs}, Error throughout {errors}")
    assert partial >= 80 and required_out >= 60 and behind >= 240 and differs >= 4 and errors >= 5
