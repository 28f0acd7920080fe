"""The elastic gang preemption query (kt_preempt_gangs_elastic_launch), pinned on the CPU.

``paging.preempt_gangs_elastic_of`` — the member-major walk kt_kernels_preempt_gangs_elastic.hip computes: a state per throttle of
the union that every candidate moves on, the members in order on it, a failed member reserving nowhere — is held to the reference
of tests/preempt_gangs_elastic_reference.py: delete the prefix, reconcile with the oracle, admit the gang in order with the oracle,
apply the rule, for every k; and the reprieve as its definition.  The clusters, gangs and seeds are those of
tests/test_preempt_gangs_cpu.py under ``forecast_gangs_elastic_reference.seeded_rule``.  tests/test_preempt_gangs_elastic_gpu.py
holds the kernel to the same reference."""
import pytest

import preempt_gangs_elastic_reference as ER
import preempt_gangs_reference as GR
import preempt_reference as PR
from kube_throttler_amd import paging
from test_preempt_cpu import SEEDS

A, B = ER.A, ER.B


def held_to_the_reference(snap, members, quorum, required, cands, want, ctx=None):
    for eq in (False, True):
        w = want[eq]
        got = paging.preempt_gangs_elastic_of(snap, members, quorum, required, cands, PR.NOW, eq, ctx=ctx)
        assert got == (w.prefix, w.victims, w.members, w.blocker), (members, quorum, required, cands, eq, got, w)
        got = paging.preempt_gangs_elastic_of(snap, members, quorum, required, cands, PR.NOW, eq, ctx=ctx, reprieve=True)
        assert got == (w.prefix, w.reprieved, w.reprieved_members, w.blocker), (members, quorum, required, cands, eq, got, w)


@pytest.mark.parametrize("seed", SEEDS)
def test_preempt_gangs_elastic_of_equals_delete_reconcile_walk(seed, oracle_mod):
    snap, ruled, want, _ = ER.seeded_reference(seed, oracle_mod)
    ctx = paging.preempt_context(snap, PR.NOW)
    for (ms, cands, quorum, required), w in zip(ruled, want):
        held_to_the_reference(snap, ms, quorum, required, cands, w, ctx)


def test_the_seeded_cases_reach_what_the_rule_is_for(oracle_mod):
    """Floors on the reference side alone, over SEEDS at on_equal=False: the elastic prefix differs from the whole gang's and admits
    a partial gang, a k behind the prefix fails again (the verdict is not monotone), the reprieve shrinks the mask and changes how
    many members are in."""
    total = differs = partial = fails_behind = shrinks = count_moves = 0
    for seed in SEEDS:
        _, ruled, want, whole = ER.seeded_reference(seed, oracle_mod)
        for (ms, _, _, _), w, wh in zip(ruled, want, whole):
            w = w[False]
            total += 1
            differs += w.prefix != wh[False]
            partial += w.prefix >= 0 and w.prefix != wh[False] and w.members < len(ms)
            fails_behind += w.prefix >= 0 and any(v != A for v in w.verdicts[w.prefix:])
            shrinks += sum(w.reprieved) < sum(w.victims)
            count_moves += w.reprieved_members != w.members
    shares = (f"{total} cases, prefix differs from the whole gang's: {differs}, a partial gang at it: {partial}, a failing k behind the "
              f"prefix: {fails_behind}, shrinking reprieves: {shrinks}, reprieves that change the member count: {count_moves}")
    print(shares)
    assert total == 64, shares
    assert differs >= 16, shares
    assert partial >= 16, shares
    assert fails_behind >= 1, shares
    assert shrinks >= 14, shares
    assert count_moves >= 2, shares


@pytest.mark.parametrize("seed", SEEDS[::2])
def test_p1_the_whole_gang_is_the_gang_query(seed, oracle_mod):
    """(P1) on the reference: quorum = size, or every member required, is kt_preempt_gangs_launch's prefix; the blocker is equal
    where every member is valid and no Error."""
    from test_preempt_gangs_cpu import gang_case
    snap, cases, whole, _ = gang_case(seed, oracle_mod)
    for case, (ms, cands) in enumerate(cases):
        for quorum, required in ((len(ms), None), (1, [True] * len(ms))):
            want = ER.reference(snap, oracle_mod, ms, quorum, required, cands)
            for eq in (False, True):
                k, b = whole[eq][case]
                assert want[eq].prefix == k, (seed, case, eq)
                if k >= 0:
                    assert want[eq].members == len(ms)
                if GR.members_ok(snap, oracle_mod, ms):
                    assert want[eq].blocker == b, (seed, case, eq)
                model = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, eq)
                assert want[eq].victims == model[1], (seed, case, eq)
                assert want[eq].reprieved == paging.preempt_gangs_of(snap, ms, cands, PR.NOW, eq, reprieve=True)[1], (seed, case, eq)
            held_to_the_reference(snap, ms, quorum, required, cands, want)


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_p2_a_gang_of_one_is_the_single_query(name, oracle_mod):
    snap, p, cands = PR.DIRECTED[name]()
    want = ER.reference(snap, oracle_mod, [p], 1, None, cands)
    for eq in (False, True):
        assert want[eq].prefix == PR.reference_prefix(snap, oracle_mod, p, cands, PR.NOW, eq), (name, eq)
        assert (want[eq].prefix, want[eq].victims) == paging.preempt_of(snap, p, cands, PR.NOW, eq), (name, eq)
        assert want[eq].reprieved == paging.preempt_of(snap, p, cands, PR.NOW, eq, reprieve=True)[1], (name, eq)
    held_to_the_reference(snap, [p], 1, None, cands, want)


@pytest.mark.parametrize("name", sorted(ER.HAND))
def test_hand_derived_cases(name, oracle_mod):
    _, _, _, _, table, verdicts = ER.HAND[name]
    snap, ms, quorum, required, cands = ER.hand_case(name)
    want = ER.reference(snap, oracle_mod, ms, quorum, required, cands)
    for eq in (False, True):
        w = want[eq]
        assert (w.prefix, w.victims, w.members, w.blocker, w.reprieved, w.reprieved_members) == table[eq], (name, eq, w)
        if verdicts is not None:
            assert w.verdicts == verdicts[eq], (name, eq, w.verdicts)
    held_to_the_reference(snap, ms, quorum, required, cands, want)


def test_hand_derived_facts(oracle_mod):
    """What the three cases are for, said once more in the words of the issue."""
    w = ER.reference(ER.hand_case("more-victims-shut-the-required-member-out")[0], oracle_mod, [0, 1], 1, [False, True], [2, 3, 4])
    assert w[False].counts == [0, 1, 1, 1] and w[False].verdicts[3] == B  # the longest prefix fails again
    snap, ms, cands = ER.hand_case("more-victims-shut-the-required-member-out")[0], [0, 1], [2, 3, 4]
    assert GR.reference(snap, oracle_mod, ms, cands)[0] == GR.NONE  # the whole gang never fits (8 + 4 > 10)
    snap = ER.hand_case("reprieve-changes-who-is-in")[0]
    assert GR.reference(snap, oracle_mod, [0, 1], [2, 3])[0] == 2


@pytest.mark.parametrize("name", sorted(ER.CARRIED))
def test_carried_directed_cases(name, oracle_mod):
    snap, ms, quorum, required, cands = ER.CARRIED[name]()
    want = ER.reference(snap, oracle_mod, ms, quorum, required, cands)
    held_to_the_reference(snap, ms, quorum, required, cands, want)


def test_what_the_carried_cases_answer(oracle_mod):
    ref = lambda name: ER.reference(*(lambda s, ms, q, r, c: (s, oracle_mod, ms, q, r, c))(*ER.CARRIED[name]()))
    # an Error or invalid member that is not required: the other member decides; required: out of reach, the count is S_0's
    for kind in ("error", "invalid"):
        w = ref(kind + "-member-not-required")[False]
        assert (w.prefix, w.members, w.blocker) == (1, 1, 0), (kind, w)  # (4 + 4 + 4 > 10: one victim has to go)
        w = ref(kind + "-member-required")[False]
        assert (w.prefix, w.victims, w.members, w.blocker) == (ER.NONE, [0, 0], 0, 1), (kind, w)
    w = ref("quorum-out-of-reach")[False]
    assert (w.prefix, w.members, w.blocker) == (ER.NONE, 0, 0) and set(w.verdicts) == {ER.ERR}, w
    # the error throttle keeps its stored status: the pod passes as things stand
    assert ref("error-throttle-keeps-its-stored-status")[False].prefix == 0
    # stored reserved amounts: one member of the two fits a victim earlier than both
    w = ref("stored-reserved-amounts")
    assert (w[False].prefix, w[True].prefix) < (2, 3) and ref("stored-reserved-amounts-both-required")[False].prefix == 2
    # the first member's zero-valued reservation makes the name present: the second never fits behind it, alone it would
    w = ref("zero-reservation-makes-present")[False]
    assert (w.prefix, w.members) == (0, 1)
    assert ref("zero-reservation-makes-present-second-required")[False].prefix == ER.NONE
    assert ref("zero-reservation-last")[False].prefix == 0
    w = ref("presence-through-one-victim")[False]
    assert (w.prefix, w.victims, w.reprieved) == (2, [1, 1], [0, 1])  # (the throttle matches both; only pod 1 carries the name)
    # the error candidate cuts the list: one victim is not enough, the second is out of reach
    assert ref("error-candidate-cuts")[False].prefix == ER.NONE
    w = ref("three-members-too-large-together")[False]
    assert (w.prefix, w.members) == (1, 1), w  # (used 8: one victim lets the first member in, 4 + 4 + 4 stops the second)
    w = ref("member-exceeds-threshold")[False]
    assert (w.prefix, w.members, w.blocker) == (0, 1, -1), w  # (the member that asks 11 is optional)
