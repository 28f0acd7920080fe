"""The gang preemption query (kt_preempt_gangs_launch), pinned on the CPU.

``paging.preempt_gangs_of`` — the closed form kt_kernels_preempt_gangs.hip computes: `used` lowered by a prefix sum over the
candidates, `reserved` raised by a prefix sum over the members, the four CheckThrottledFor steps for every (member, throttle,
amount) at every prefix length — is held to the reference of tests/preempt_gangs_reference.py: delete the prefix, reconcile with
the oracle, admit the gang in order with the oracle, for every k.  The clusters and seeds are those of tests/test_preempt_cpu.py.
tests/test_preempt_gangs_gpu.py holds the kernel to the same reference."""
import functools

import pytest

import preempt_gangs_reference as GR
import preempt_reference as PR
from kube_throttler_amd import paging
from test_paged_admit_cpu import write_status
from test_preempt_cpu import SEEDS


@functools.lru_cache(maxsize=None)
def gang_case(seed, oracle_mod):
    """(snapshot, [(members, candidates)], {on_equal: [(reference prefix, blocker) per case]},
    {on_equal: [[reference prefix of each member alone] per case]}) — computed once, never modified."""
    cs = PR.preempt_cluster(seed)
    if seed % 2:
        write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1
    snap = pages[0].snapshot
    cases = GR.gang_cases(seed, snap)
    want = {eq: [GR.reference(snap, oracle_mod, ms, cands, PR.NOW, eq) for ms, cands in cases] for eq in (False, True)}
    alone = {eq: [[PR.reference_prefix(snap, oracle_mod, p, cands, PR.NOW, eq) for p in ms] for ms, cands in cases] for eq in (False, True)}
    return snap, cases, want, alone


@pytest.mark.parametrize("seed", SEEDS)
def test_preempt_gangs_of_equals_delete_reconcile_admit(seed, oracle_mod):
    snap, cases, want, _ = gang_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, PR.NOW)
    for on_equal in (False, True):
        for (ms, cands), (k, b) in zip(cases, want[on_equal]):
            prefix, victims, blocker = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, on_equal, ctx=ctx)
            assert (prefix, blocker) == (k, b), f"seed {seed} on_equal={on_equal} gang {ms} over {cands}: {(prefix, blocker)} != {(k, b)}"
            GR.check_victims(snap, oracle_mod, ms, cands, prefix, victims, PR.NOW, on_equal)


def test_the_cases_cover_every_outcome(oracle_mod):
    """Conditions on the inputs, on the reference side alone: a weak generator cannot hide a failure — and the maximum of the
    members' own prefixes must be the wrong answer often enough."""
    deep = none = zero = above = none_passable = total = 0
    for seed in SEEDS:
        _, cases, want, alone = gang_case(seed, oracle_mod)
        for eq in (False, True):
            for (k, _), singles in zip(want[eq], alone[eq]):
                total += 1
                deep += k >= 2
                none += k == -1
                zero += k == 0
                passable = all(s >= 0 for s in singles)
                above += passable and k > max(singles)
                none_passable += passable and k == -1
    shares = f"{total} cases, k* >= 2: {deep}, -1: {none}, 0: {zero}, above the members' maximum: {above}, NONE although passable alone: {none_passable}"
    assert total == 128, shares
    assert deep >= 32, shares
    assert none >= 13, shares
    assert zero >= 8, shares
    assert above >= 10, shares
    assert none_passable >= 2, shares


@pytest.mark.parametrize("name", sorted(GR.DIRECTED))
def test_directed_cases_shared_with_the_gpu_suite(name, oracle_mod):
    build, want, singles = GR.DIRECTED[name]
    snap, ms, cands = build()
    for i, on_equal in enumerate((False, True)):
        k, b = GR.reference(snap, oracle_mod, ms, cands, PR.NOW, on_equal)
        assert k == want[i], f"{name} on_equal={on_equal}: the reference says {k}, the table {want[i]}"
        prefix, victims, blocker = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, on_equal)
        assert (prefix, blocker) == (k, b), (name, on_equal, prefix, blocker, k, b)
        GR.check_victims(snap, oracle_mod, ms, cands, prefix, victims, PR.NOW, on_equal)
        if singles is not None and singles[i] is not None:
            assert [PR.reference_prefix(snap, oracle_mod, p, cands, PR.NOW, on_equal) for p in ms] == singles[i], (name, on_equal)
            assert [paging.preempt_of(snap, p, cands, PR.NOW, on_equal)[0] for p in ms] == singles[i], (name, on_equal)


def test_only_the_reserved_case_is_met_by_the_members_maximum(oracle_mod):
    """A max-over-members implementation fails the directed table: where the members' own prefixes are stated, the gang's prefix
    is above their maximum (or NONE) unless the table's prefix is 0."""
    for name, (build, want, singles) in GR.DIRECTED.items():
        if singles is None or singles[0] is None or want[0] == 0:
            continue
        assert want[0] == GR.NONE or want[0] > max(singles[0]), name


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_a_gang_of_one_is_the_single_query(name):
    snap, p, cands = PR.DIRECTED[name]()
    for on_equal in (False, True):
        prefix, victims = paging.preempt_of(snap, p, cands, PR.NOW, on_equal)
        got = paging.preempt_gangs_of(snap, [p], cands, PR.NOW, on_equal)
        assert got[:2] == (prefix, victims), (name, on_equal)
        assert got[2] == (-1 if prefix == 0 else 0), (name, on_equal)
