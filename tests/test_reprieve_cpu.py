"""The reprieve pass (kt_preempt_reprieve_launch), pinned on the CPU.

``paging.preempt_of(reprieve=True)`` — the walk on the sums of ``preempt_context``, what kt_kernels_reprieve.hip computes per
list entry — is held to the reference of tests/reprieve_reference.py: the walk on delete + oracle reconcile + oracle check.
The random manifest clusters are those of tests/test_preempt_cpu.py (same seeds, both on_equal values); the directed cases are
``preempt_reference.DIRECTED`` and ``reprieve_reference.DIRECTED``.  tests/test_reprieve_gpu.py holds the kernel to the same
reference."""
import functools

import pytest

import preempt_reference as PR
import reprieve_reference as RR
from kube_throttler_amd import paging
from test_preempt_cpu import SEEDS, preempt_case


@functools.lru_cache(maxsize=None)
def reprieve_case(seed, oracle_mod):
    """(snapshot, cases, {on_equal: [reference prefix]}, {on_equal: [reference reprieved victims]}) — computed once, never modified."""
    snap, cases, want = preempt_case(seed, oracle_mod)
    walked = {eq: [RR.reference_reprieve(snap, oracle_mod, p, cands, k, PR.NOW, eq) for (p, cands), k in zip(cases, want[eq])]
              for eq in (False, True)}
    return snap, cases, want, walked


@pytest.mark.parametrize("seed", SEEDS)
def test_preempt_of_reprieve_equals_the_walk_on_the_oracle(seed, oracle_mod):
    snap, cases, want, walked = reprieve_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, PR.NOW)
    for on_equal in (False, True):
        for (p, cands), k, v in zip(cases, want[on_equal], walked[on_equal]):
            prefix, victims = paging.preempt_of(snap, p, cands, PR.NOW, on_equal, ctx=ctx, reprieve=True)
            assert prefix == k and victims == v, f"seed {seed} on_equal={on_equal} pod{p} over {cands}: {prefix}, {victims} != {k}, {v}"
            # the default is today's call
            assert paging.preempt_of(snap, p, cands, PR.NOW, on_equal, ctx=ctx) == paging.preempt_of(snap, p, cands, PR.NOW, on_equal, ctx=ctx,
                                                                                                     reprieve=False)


def _masks(seed, oracle_mod):
    """[(snapshot, p, cands, on_equal, prefix, prefix mask, reprieved)] of one seed; the prefix mask is ``preempt_of``'s, which
    tests/test_preempt_cpu.py holds to the reference."""
    snap, cases, want, walked = reprieve_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, PR.NOW)
    return [(snap, p, cands, eq, k, paging.preempt_of(snap, p, cands, PR.NOW, eq, ctx=ctx)[1], v)
            for eq in (False, True) for (p, cands), k, v in zip(cases, want[eq], walked[eq])]


def test_the_walk_has_something_to_reprieve(oracle_mod):
    """A condition on the inputs, on the reference side alone: in at least a tenth of all cases the reprieved set is strictly
    smaller than the prefix mask (observed: 30 of 192)."""
    rows = [r for seed in SEEDS for r in _masks(seed, oracle_mod)]
    smaller = sum(sum(v) < sum(mask) for *_, mask, v in rows)
    for *_, mask, v in rows:
        assert all(b <= a for a, b in zip(mask, v))  # the walk only ever takes victims out of the mask
    assert 10 * smaller >= len(rows), f"{smaller} of {len(rows)} cases reprieve somebody"


def test_the_last_masked_candidate_is_never_reprieved(oracle_mod):
    for seed in SEEDS:
        for snap, p, cands, eq, k, mask, v in _masks(seed, oracle_mod):
            if k > 0:
                assert mask[k - 1] == 1 and v[k - 1] == 1, f"seed {seed} on_equal={eq} pod{p}: prefix {k}, mask {mask}, reprieved {v}"


def test_without_negative_requests_the_set_is_minimal(oracle_mod):
    """Putting any ONE remaining victim back makes the preemptor fail."""
    seen = 0
    for seed in SEEDS:
        for snap, p, cands, eq, k, mask, v in _masks(seed, oracle_mod):
            if k <= 0 or RR.has_negative_requests(snap, [p] + list(cands)):
                continue
            left = [c for c, b in zip(cands, v) if b]
            assert PR.passes_without(snap, oracle_mod, p, left, PR.NOW, eq)
            for c in left:
                assert not PR.passes_without(snap, oracle_mod, p, [x for x in left if x != c], PR.NOW, eq), f"seed {seed} pod{p}: {c} could come back"
            seen += 1
    assert seen >= 30, seen  # (a third of the 192 cases have a prefix of two or more)


# ---- directed cases ----
def _both(snap, oracle_mod, p, cands, on_equal=False):
    k, v = RR.reference(snap, oracle_mod, p, cands, PR.NOW, on_equal)
    got = paging.preempt_of(snap, p, cands, PR.NOW, on_equal, reprieve=True)
    assert got == (k, v), (got, k, v)
    return got


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_directed_cases_of_the_prefix_query(name, oracle_mod):
    snap, p, cands = PR.DIRECTED[name]()
    for on_equal in (False, True):
        _both(snap, oracle_mod, p, cands, on_equal)


@pytest.mark.parametrize("name", sorted(RR.DIRECTED))
def test_directed_cases_of_the_reprieve_pass(name, oracle_mod):
    snap, p, cands = RR.DIRECTED[name]()
    for on_equal in (False, True):
        _both(snap, oracle_mod, p, cands, on_equal)


def test_directed_cases_are_not_vacuous(oracle_mod):
    def ref(name, eq=False):
        snap, p, cands = RR.DIRECTED[name]()
        return _both(snap, oracle_mod, p, cands, eq)

    assert ref("one-one-six") == (3, [0, 0, 1])
    assert ref("two-throttles-two-victims") == (4, [0, 0, 1, 1])  # list order: small-a, small-b, big-a, big-b
    assert ref("victim-of-two-throttles") == (3, [0, 0, 1])
    assert ref("zero-valued-name-comes-back") == (2, [0, 1])  # pod 2 (memory only) comes back, pod 1 would bring cpu = 0 back
    assert ref("pod-count-alone") == (2, [1, 1, 0, 0])
    assert ref("negative-request-candidate") == (2, [0, 1, 0])
    assert ref("error-throttle-beside-a-reconciled-one") == (3, [0, 0, 1])
    assert ref("error-throttle-override-active")[0] == 0 and ref("error-candidate-cuts") == (-1, [0] * 5)
    assert ref("error-candidate-behind-the-prefix") == (2, [0, 1, 0, 0])
    assert ref("equality-throttle", False) == (1, [1, 0, 0]) and ref("equality-throttle", True) == (2, [0, 1, 0])
    assert ref("equality-clusterthrottle", False) == (1, [1, 0, 0]) and ref("equality-clusterthrottle", True) == (2, [0, 1, 0])
    assert ref("equality-step3-clusterthrottle", False) != ref("equality-step3-clusterthrottle", True)


@pytest.mark.parametrize("m", [5, 66])
def test_the_shapes_of_the_gpu_suite_do_what_they_say(m, oracle_mod):
    snap, p, cands = RR.big_last(m)
    assert _both(snap, oracle_mod, p, cands) == (m - 1, [0] * (m - 2) + [1, 0])
    assert _both(snap, oracle_mod, p, cands, True) == (m - 1, [1] + [0] * (m - 3) + [1, 0])


def test_wide_lists_reprieve_across_names(oracle_mod):
    snap, pre, cands = RR.wide(5, 24, D=3)
    k, v = _both(snap, oracle_mod, pre[0], cands)
    assert k >= 4 and 2 <= sum(v) < sum(paging.preempt_of(snap, pre[0], cands, PR.NOW)[1])
