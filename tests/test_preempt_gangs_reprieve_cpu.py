"""The gang reprieve pass (kt_preempt_gangs_reprieve_launch), pinned on the CPU.

``paging.preempt_gangs_of(..., reprieve=True)`` — the closed form kt_kernels_preempt_gangs_reprieve.hip computes: per reconciled
throttle of the union the `used` of the current state, a victim put back where every throttle that matches it still admits the
members in order under the reserved prefix — is held to the reference of tests/preempt_gangs_reprieve_reference.py: the walk on
delete + oracle reconcile + oracle in-order admission.  The clusters, gangs and seeds are those of tests/test_preempt_gangs_cpu.py.
tests/test_preempt_gangs_reprieve_gpu.py holds the kernel to the same reference."""
import functools

import pytest

import preempt_gangs_reference as GR
import preempt_gangs_reprieve_reference as GRR
import preempt_reference as PR
import reprieve_reference as RR
from kube_throttler_amd import paging
from test_preempt_cpu import SEEDS
from test_preempt_gangs_cpu import gang_case


@functools.lru_cache(maxsize=None)
def gang_reprieve_case(seed, oracle_mod):
    """(snapshot, [(members, candidates)], {on_equal: [(prefix, blocker)]}, {on_equal: [reference reprieved victims]}) — computed
    once, never modified."""
    snap, cases, want, _ = gang_case(seed, oracle_mod)
    walked = {eq: [GRR.reference_reprieve(snap, oracle_mod, ms, cands, k, PR.NOW, eq) for (ms, cands), (k, _) in zip(cases, want[eq])]
              for eq in (False, True)}
    return snap, cases, want, walked


def _all(seed, oracle_mod):
    """(snapshot, members, candidates, on_equal, prefix, blocker, prefix mask, reprieved victims of the model) per case."""
    snap, cases, want, _ = gang_reprieve_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, PR.NOW)
    for eq in (False, True):
        for (ms, cands), (k, b) in zip(cases, want[eq]):
            plain = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, eq, ctx=ctx)
            got = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, eq, ctx=ctx, reprieve=True)
            assert (got[0], got[2]) == (plain[0], plain[2]) == (k, b)
            yield snap, ms, cands, eq, k, b, plain[1], got[1]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_model_equals_the_walk_on_delete_reconcile_admit(seed, oracle_mod):
    _, cases, _, walked = gang_reprieve_case(seed, oracle_mod)
    i = {False: 0, True: 0}
    for snap, ms, cands, eq, k, b, mask, v in _all(seed, oracle_mod):
        assert v == walked[eq][i[eq]], f"seed {seed} on_equal={eq} gang {ms} over {cands}: prefix {k}"
        i[eq] += 1


def test_the_default_is_unchanged(oracle_mod):
    snap, cases, _, _ = gang_case(SEEDS[0], oracle_mod)
    for ms, cands in cases:
        assert paging.preempt_gangs_of(snap, ms, cands, PR.NOW) == paging.preempt_gangs_of(snap, ms, cands, PR.NOW, reprieve=False)


def test_properties_of_every_case_with_a_positive_prefix(oracle_mod):
    positive = shrunk = 0
    for seed in SEEDS:
        for snap, ms, cands, eq, k, b, mask, v in _all(seed, oracle_mod):
            if k <= 0:
                assert not any(v)
                continue
            positive += 1
            shrunk += sum(v) < sum(mask)
            assert all(m or not r for m, r in zip(mask, v)), "not a subset of the prefix mask"
            GR.check_victims(snap, oracle_mod, ms, cands, k, v, PR.NOW, eq)  # deleting exactly the reprieved set admits the gang
            last = max(j for j in range(k) if mask[j])
            assert v[last] == 1, "the last masked position is never reprieved: the prefix is the shortest"
    assert positive >= 40 and shrunk >= 20, (positive, shrunk)


def test_without_negative_requests_the_set_is_minimal(oracle_mod):
    """Putting any ONE remaining victim back makes the gang fail."""
    seen = 0
    for seed in SEEDS:
        for snap, ms, cands, eq, k, b, mask, v in _all(seed, oracle_mod):
            if k <= 0 or RR.has_negative_requests(snap, list(ms) + list(cands)):
                continue
            left = [c for c, bit in zip(cands, v) if bit]
            for c in left:
                assert GR.first_blocked(snap, oracle_mod, ms, [x for x in left if x != c], PR.NOW, eq) is not None, \
                    f"seed {seed} gang {ms}: {c} could come back"
            seen += 1
    assert seen >= 15, seen


@pytest.mark.parametrize("name", sorted(GRR.DIRECTED))
def test_directed_table(name, oracle_mod):
    build, prefixes, victims = GRR.DIRECTED[name]
    snap, ms, cands = build()
    for i, eq in enumerate((False, True)):
        k, v, b = GRR.reference(snap, oracle_mod, ms, cands, PR.NOW, eq)
        assert (k, v) == (prefixes[i], victims[i]), f"{name} on_equal={eq}: the reference says {(k, v)}, the table {(prefixes[i], victims[i])}"
        assert paging.preempt_gangs_of(snap, ms, cands, PR.NOW, eq, reprieve=True) == (k, v, b), (name, eq)
        plain = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, eq)
        assert plain[0] == k and all(m or not r for m, r in zip(plain[1], v))
        GR.check_victims(snap, oracle_mod, ms, cands, k, v, PR.NOW, eq)


def test_the_members_own_reprieved_sets_do_not_compose(oracle_mod):
    build, prefixes, victims = GRR.DIRECTED["reserved-prefix-keeps-victims"]
    snap, ms, cands = build()
    for i, eq in enumerate((False, True)):
        singles = [paging.preempt_of(snap, p, cands, PR.NOW, eq, reprieve=True) for p in ms]
        assert singles == [(1, [1, 0, 0, 0])] * 2
        assert [RR.reference(snap, oracle_mod, p, cands, PR.NOW, eq) for p in ms] == singles
        union = [int(any(s[1][j] for s in singles)) for j in range(len(cands))]
        gang = paging.preempt_gangs_of(snap, ms, cands, PR.NOW, eq, reprieve=True)
        assert gang[1] == victims[i] != union
        # the union of the members' sets does not admit the gang
        assert GR.first_blocked(snap, oracle_mod, ms, [c for c, bit in zip(cands, union) if bit], PR.NOW, eq) is not None


@pytest.mark.parametrize("name", sorted(set(RR.DIRECTED) | set(PR.DIRECTED)))
def test_a_gang_of_one_is_the_single_reprieve(name):
    snap, p, cands = (RR.DIRECTED.get(name) or PR.DIRECTED[name])()
    for eq in (False, True):
        prefix, victims = paging.preempt_of(snap, p, cands, PR.NOW, eq, reprieve=True)
        assert paging.preempt_gangs_of(snap, [p], cands, PR.NOW, eq, reprieve=True)[:2] == (prefix, victims), (name, eq)


def test_gangs_of_one_on_the_random_clusters(oracle_mod):
    for seed in SEEDS[::4]:
        snap, cases, _, _ = gang_case(seed, oracle_mod)
        ctx = paging.preempt_context(snap, PR.NOW)
        for ms, cands in cases:
            for eq in (False, True):
                assert paging.preempt_gangs_of(snap, ms[:1], cands, PR.NOW, eq, ctx=ctx, reprieve=True)[:2] == \
                    paging.preempt_of(snap, ms[0], cands, PR.NOW, eq, ctx=ctx, reprieve=True)
