"""Elastic gang admission (kt_admit_gangs_elastic_launch / kt_paged_admit_gangs_elastic), pinned on the CPU.

The reference is built from ``model_admit`` of tests/test_paged_admit_cpu.py the way ``model_admit_gangs`` of
tests/test_gang_admit_cpu.py is: the members of a gang go through the per-pod step one after the other, all of them also behind one
that failed; the gang stays iff at least ``min_members[g]`` verdicts are ``allow`` and every required member's is; otherwise the
reserved amounts go back to the copy taken before the gang.  A kept gang keeps what its allowed members reserved: the others never
reserved.

Pinned here: with ``min = size`` and no flags, and with every member required at any ``min``, it is ``model_admit_gangs``; with gangs
of one pod it is the C oracle's ``kto_admit``; and the rules tests/test_gang_admit_elastic_gpu.py draws over ``GANG_CASES`` hold enough
kept partial gangs, gangs rolled back for a required member, rolled-back gangs with members that had reserved, and verdicts that
depend on a kept partial gang, that an implementation with another rule cannot pass them."""
import copy
import random

import pytest

from test_gang_admit_cpu import GANG_CASES, ONE_PAGE_SEEDS, _oracle_admit, gang_case, model_admit_gangs
from test_paged_admit_cpu import admission_case, model_admit, reserved_totals


def model_admit_gangs_elastic(cs, queue, gang_off, min_members, required, on_equal):
    """The reference: ([(verdict, {throttle: status})] per queue position, [members that stay] per gang, 0 rolled back);
    ``required`` per queue position or None; ``cs.reserved`` ends as the committed totals."""
    out, members = [], []
    for g in range(len(gang_off) - 1):
        i0, i1 = gang_off[g], gang_off[g + 1]
        before = copy.deepcopy(cs.reserved)
        res = model_admit(cs, queue[i0:i1], on_equal)
        ok = [v == "allow" for v, _ in res]
        kept = sum(ok) >= min_members[g] and all(o for k, o in enumerate(ok) if required is not None and required[i0 + k])
        if not kept:
            cs.reserved = before
        out += res
        members.append(sum(ok) if kept else 0)
    return out, members


def elastic_rule(seed, gang_off):
    """The seeded rule of the GPU parity tests: per gang a quorum in [1, size], then per member required with probability 1/4."""
    r = random.Random(2000 + seed)
    min_members, required = [], []
    for g in range(len(gang_off) - 1):
        size = gang_off[g + 1] - gang_off[g]
        min_members.append(r.randint(1, size))
        required += [r.random() < 0.25 for _ in range(size)]
    return min_members, required


def elastic_case(seed, wide, oracle_mod):
    cs, queue, off = gang_case(seed, wide, oracle_mod)
    return (cs, queue, off) + elastic_rule(seed, off)


# ---- pin 1: identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,wide", GANG_CASES)
def test_full_quorum_and_all_required_are_all_or_nothing(seed, wide, oracle_mod):
    cs, queue, off = gang_case(seed, wide, oracle_mod)
    sizes = [off[g + 1] - off[g] for g in range(len(off) - 1)]
    some_min = elastic_rule(seed, off)[0]
    for on_equal in (False, True):
        plain = copy.deepcopy(cs)
        want, admitted = model_admit_gangs(plain, queue, off, on_equal)
        for label, mins, req in (("min = size", sizes, None), ("all required", sizes, [True] * len(queue)),
                                 ("all required, min = 1", [1] * len(sizes), [True] * len(queue)),
                                 ("all required, any min", some_min, [True] * len(queue))):
            work = copy.deepcopy(cs)
            got, members = model_admit_gangs_elastic(work, queue, off, mins, req, on_equal)
            where = f"seed {seed} wide={wide} on_equal={on_equal} {label}"
            assert got == want, where
            assert [m > 0 for m in members] == admitted, where
            assert [m for m in members if m] == [s for s, a in zip(sizes, admitted) if a], where
            assert reserved_totals(work) == reserved_totals(plain), where


@pytest.mark.parametrize("seed", ONE_PAGE_SEEDS)
def test_gangs_of_one_pod_are_kto_admit(seed, oracle_mod):
    cs, queue = admission_case(seed, oracle_mod, wide=False, factor=10)
    for on_equal in (False, True):
        verdicts, rows, totals = _oracle_admit(cs, queue, on_equal, oracle_mod)
        work = copy.deepcopy(cs)
        want, members = model_admit_gangs_elastic(work, queue, list(range(len(queue) + 1)), [1] * len(queue), None, on_equal)
        assert [v for v, _ in want] == verdicts, f"seed {seed} on_equal={on_equal}"
        assert [st for _, st in want] == rows, f"seed {seed} on_equal={on_equal}"
        assert members == [1 if v == "allow" else 0 for v in verdicts]
        got = reserved_totals(work)
        for nn, a in totals.items():
            assert got.get(nn, {}) == a, f"seed {seed}: reserved of {nn}"


# ---- pin 2: the cases are not vacuous ----------------------------------------------------------------------------------------
def test_the_gpu_cases_need_the_elastic_rule(oracle_mod):
    """The floors that keep tests/test_gang_admit_elastic_gpu.py honest, over its cases and seeded rules at on_equal=False: the
    reference alone shows gangs kept with fewer members than their size, gangs that reach their quorum but are rolled back for a
    required member, rolled-back gangs in which some member had reserved, and queue positions whose verdict and status row differ
    from all-or-nothing admission of the same queue (they depend on a kept partial gang)."""
    partial = partial_wide = required_out = required_out_wide = rolled_back_with_admitted = differs = 0
    for seed, wide in GANG_CASES:
        cs, queue, off, mins, req = elastic_case(seed, wide, oracle_mod)
        want, members = model_admit_gangs_elastic(copy.deepcopy(cs), queue, off, mins, req, False)
        whole, _ = model_admit_gangs(copy.deepcopy(cs), queue, off, False)
        for g, m in enumerate(members):
            ok = [v == "allow" for v, _ in want[off[g]:off[g + 1]]]
            if 0 < m < len(ok):
                partial += 1
                partial_wide += wide
            if m == 0 and sum(ok) >= mins[g]:  # the quorum is there: only a required member can have failed
                assert any(r and not o for r, o in zip(req[off[g]:off[g + 1]], ok))
                required_out += 1
                required_out_wide += wide
            if m == 0 and any(ok):
                rolled_back_with_admitted += 1
        differs += sum(1 for a, b in zip(want, whole) if a != b)
    print(f"kept with fewer members than their size: {partial} ({partial_wide} wide), quorum reached but rolled back for a required "
          f"member: {required_out} ({required_out_wide} wide), rolled back with a member that had reserved: {rolled_back_with_admitted}, "
          f"positions that differ from all-or-nothing admission: {differs}")
    assert partial >= 8 and partial_wide >= 2
    assert required_out >= 4 and required_out_wide >= 2
    assert rolled_back_with_admitted >= 10
    assert differs >= 3
