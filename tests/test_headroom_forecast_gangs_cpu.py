"""The gang headroom forecast (kt_headroom_forecast_gangs_launch), pinned on the CPU.

``paging.headroom_forecast_gangs_of`` — the restatement of what kt_kernels_headroom_forecast_gangs.hip computes per lane:
``forecast_gangs_of``'s threshold and throttled flags at the lane's instant, ``headroom_gangs_of``'s A_t, range and judge per
candidate copy, a bisection per instant, the lexicographic minimum of (copies, first stopped member, throttle row) — is held to
the reference of tests/headroom_forecast_gangs_reference.py: per instant a copy of the snapshot, the oracle's reconcile, the
oracle's admit of ``members * cap``.  The random cases are the gang forecast's two generators with loosened thresholds, cases with
a negative request left out (the call refuses such an engine: tests/test_headroom_forecast_gangs_gpu.py).  That file holds the
kernel to the same reference."""
import pytest

import forecast_gangs_reference as FG
import forecast_reference as FR
import headroom_forecast_gangs_reference as HG
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

# Chosen on the reference alone (test_the_cases_cover_every_outcome): HG.STAIR_SEEDS = 0 .. 39, HG.CLUSTER_SEEDS = the odd and even
# seeds [1, 3, 4, 5, 8, 10, 14, 19, 20, 23] of the forecast tests, thresholds times HG.FACTOR = 6, CAP = 12.  Observed with them,
# both on_equal values together: 50 cases, 160 gangs, 3920 (gang, instant) cells — copies 0: 2340 (60 %), strictly between: 976
# (25 %), cap: 604 (15 %); gangs whose copies change between two instants: 75 (47 %); blocked cells 3316, blocker behind the
# gang's first member: 817 (25 %); gangs with an Error or invalid member: 26.
CAP = HG.CAP
WANT = 2


def test_random_cases_equal_reconcile_and_gang_admit_per_instant(oracle_mod):
    cases = HG.random_cases(oracle_mod)
    assert len(cases) >= 40
    for name, snap, gangs, inst, want in cases:
        ctx = paging.preempt_context(snap, inst[0])
        for on_equal in (False, True):
            for members, w in zip(gangs, want[on_equal]):
                got = paging.headroom_forecast_gangs_of(snap, members, inst, CAP, WANT, on_equal, ctx=ctx)
                assert got == w, f"{name} on_equal={on_equal} gang {members}: {got} != {w}"
                for k in (1, CAP):
                    assert paging.headroom_forecast_gangs_of(snap, members, inst, CAP, k, on_equal, ctx=ctx)[0] == HG.first_of(w[1], k)


@pytest.mark.parametrize("name", sorted(HG.DIRECTED))
def test_directed(name, oracle_mod):
    snap, members, inst = HG.DIRECTED[name]()
    for on_equal in (False, True):
        for cap, want in ((16, 1), (16, 2), (1, 1)):
            w = HG.reference(snap, oracle_mod, members, inst, cap, want, on_equal)
            assert paging.headroom_forecast_gangs_of(snap, members, inst, cap, want, on_equal) == w, f"{name} on_equal={on_equal} cap={cap}"


def test_directed_numbers_written_out(oracle_mod):
    ref = lambda name, cap=16, eq=False: HG.reference(*HG.DIRECTED[name]()[:1], oracle_mod, *HG.DIRECTED[name]()[1:], cap, 1, eq)
    # used 4, the members ask 3 + 3: spec 9 -> 0 copies, the second member stopped; 16 -> 2 copies, the first member of the third
    first, copies, limiting, blocker = ref("second-member-stopped-by-what-the-first-reserved")
    assert (first, copies, blocker) == (2, [0, 0, 2, 2, 2, 2, 0, 0, 0], [1, 1, 0, 0, 0, 0, 1, 1, 1]) and limiting == [0] * 9
    # on_equal: 4 + 6 * 2 = 16 is reached by the second member of copy 1
    assert ref("second-member-stopped-by-what-the-first-reserved", eq=True)[1:] == ([0, 0, 1, 1, 1, 1, 0, 0, 0], [0] * 9, [1] * 9)
    # three members of 3: spec 5 stops the second, 7 the third, 2 the first, 9 nobody in copy 0 (and the first of copy 1)
    assert ref("the-blocker-moves-with-the-instant")[1:] == ([0] * 7 + [1, 0], [0] * 9, [1, 1, 2, 1, 1, 0, 1, 0, 1])
    # the Error member last: the blocker moves in front of it inside the window, where limiting names the throttle
    first, copies, limiting, blocker = ref("member-without-namespace-object-last")
    assert (first, copies) == (-1, [0] * 9) and blocker == [2, 2, 1, 1, 1, 1, 2, 2, 2] and limiting == [-1, -1, 0, 0, 0, 0, -1, -1, -1]
    assert ref("invalid-member-row-last")[2:] == (limiting, blocker)
    assert ref("gang-no-throttle-affects", cap=7) == (0, [7] * 9, [-1] * 9, [-1] * 9)
    # the stored status (spec cpu 10, nothing used) at every instant: the first member (6) reserves, the second is stopped
    assert ref("error-throttle-stops-the-second-member-only") == (-1, [0] * 9, [0] * 9, [1] * 9)


def test_a_gang_of_one_is_headroom_forecast_of(oracle_mod):
    """(G1) on the model: first, copies and limiting of ``headroom_forecast_of``; the blocker is the pod itself where copies < cap."""
    for name, snap, gangs, inst, _ in HG.random_cases(oracle_mod):
        ctx = paging.preempt_context(snap, inst[0])
        for on_equal in (False, True):
            for p in sorted({p for g in gangs for p in g}):
                first, copies, limiting, blocker = paging.headroom_forecast_gangs_of(snap, [p], inst, CAP, WANT, on_equal, ctx=ctx)
                assert (first, copies, limiting) == paging.headroom_forecast_of(snap, p, inst, CAP, WANT, on_equal, ctx=ctx), f"{name} pod{p}"
                assert blocker == [0 if c < CAP else -1 for c in copies], f"{name} pod{p}"


def test_cap_one_is_the_gang_forecast(oracle_mod):
    """(G2) on the model: with cap == want == 1 a copy is admitted exactly where the gang forecast's verdict is Success, and first
    and blocker are the gang forecast's."""
    for name, snap, gangs, inst, _ in HG.random_cases(oracle_mod):
        ctx = paging.preempt_context(snap, inst[0])
        for on_equal in (False, True):
            for members in gangs:
                f_first, verdicts, f_blocker = paging.forecast_gangs_of(snap, members, inst, on_equal, ctx=ctx)
                first, copies, _, blocker = paging.headroom_forecast_gangs_of(snap, members, inst, 1, 1, on_equal, ctx=ctx)
                assert copies == [1 if v == S.VERDICT_ALLOW else 0 for v in verdicts], f"{name} gang {members}"
                assert (first, blocker) == (f_first, f_blocker), f"{name} gang {members}"
    for name in sorted(FG.DIRECTED):  # the directed cases of the gang forecast, its own reference in the place of the model
        snap, members, inst = FG.DIRECTED[name]()
        if HG.has_negative_request(snap):
            continue
        for on_equal in (False, True):
            f_first, verdicts, f_blocker = FG.reference(snap, oracle_mod, members, inst, on_equal)
            first, copies, _, blocker = paging.headroom_forecast_gangs_of(snap, members, inst, 1, 1, on_equal)
            assert copies == [1 if v == S.VERDICT_ALLOW else 0 for v in verdicts] and (first, blocker) == (f_first, f_blocker), name


def test_the_cases_cover_every_outcome(oracle_mod):
    """Conditions on the random cases at CAP, on the reference side alone, both on_equal values together: a weak generator cannot
    hide a failure."""
    cells = at_zero = between = at_cap = gangs = changes = blocked = behind = error_gangs = stored = 0
    for name, snap, gs, inst, want in HG.random_cases(oracle_mod):
        stored += any(t["error"] for t in paging.preempt_context(snap, inst[0])["thr"])
        for on_equal in (False, True):
            for members, (_, copies, limiting, blocker) in zip(gs, want[on_equal]):
                gangs += 1
                changes += len(set(copies)) >= 2
                error_gangs += set(copies) == {0} and any(l == -1 and b >= 0 for l, b in zip(limiting, blocker))
                for c, b in zip(copies, blocker):
                    cells += 1
                    at_zero += c == 0
                    between += 0 < c < CAP
                    at_cap += c == CAP
                    blocked += c < CAP
                    behind += c < CAP and b > 0
    shares = (f"{cells} cells, at 0: {at_zero}, between: {between}, at the cap: {at_cap}; {gangs} gangs, copies change: {changes}, an Error "
              f"member: {error_gangs}; blocked cells {blocked}, blocker behind the first member: {behind}; cases with a stored-status "
              f"throttle: {stored}")
    print(shares)
    assert 10 * at_zero >= cells and 10 * between >= cells and 10 * at_cap >= cells, shares
    assert 10 * changes >= gangs and 10 * behind >= blocked, shares
    assert error_gangs >= 1 and stored >= 1, shares
