"""The preemption query (kt_preempt_launch), pinned on the CPU.

``paging.preempt_of`` — the closed form kt_kernels_preempt.hip computes per lane: prefix sums of the candidates' amounts taken
off a fresh aggregate, exact presence from contributor counts, the four CheckThrottledFor steps at every prefix length — is held
to the reference of tests/preempt_reference.py: delete the prefix, reconcile with the oracle, check with the oracle, for every k.
Random manifest clusters of up to 60 pods x 12 throttles (odd seeds with a stored status written back by a reconcile, even
seeds with the status of a cluster nobody has reconciled yet: stale against a fresh reconcile) and directed cases.
tests/test_preempt_gpu.py holds the kernel to the same reference."""
import functools

import numpy as np
import pytest

import preempt_reference as PR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_paged_admit_cpu import write_status

# Chosen on the CPU so that the REFERENCE meets the bounds of test_the_cases_cover_every_outcome (seeds divisible by 4 hold pods
# of a namespace without object, seeds divisible by 5 selectors that do not convert).  Observed over these seeds, both on_equal
# values together: 192 cases, k* >= 2: 67 (35 %), -1: 87 (45 %), 0: 37 (19 %).
SEEDS = [1, 3, 7, 11, 15, 18, 19, 21, 22, 23, 30, 31, 36, 40, 41, 47]


@functools.lru_cache(maxsize=None)
def preempt_case(seed, oracle_mod):
    """(snapshot, [(preemptor, candidates)], {on_equal: [reference prefix per case]}) — computed once, never modified."""
    cs = PR.preempt_cluster(seed)
    if seed % 2:
        write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1
    snap = pages[0].snapshot
    assert snap.n_pods <= 60 and snap.n_thr <= 12
    cases = PR.preempt_cases(seed, snap)
    want = {eq: [PR.reference_prefix(snap, oracle_mod, p, cands, PR.NOW, eq) for p, cands in cases] for eq in (False, True)}
    return snap, cases, want


@pytest.mark.parametrize("seed", SEEDS)
def test_preempt_of_equals_delete_reconcile_check(seed, oracle_mod):
    snap, cases, want = preempt_case(seed, oracle_mod)
    ctx = paging.preempt_context(snap, PR.NOW)
    for on_equal in (False, True):
        for (p, cands), k in zip(cases, want[on_equal]):
            prefix, victims = paging.preempt_of(snap, p, cands, PR.NOW, on_equal, ctx=ctx)
            assert prefix == k, f"seed {seed} on_equal={on_equal} pod{p} over {cands}: {prefix} != {k}"
            PR.check_victims(snap, oracle_mod, p, cands, prefix, victims, PR.NOW, on_equal)


def test_the_cases_cover_every_outcome(oracle_mod):
    """Conditions on the inputs, on the reference side alone: a weak generator cannot hide a failure."""
    ks = [k for seed in SEEDS for eq in (False, True) for k in preempt_case(seed, oracle_mod)[2][eq]]
    deep, none, zero = sum(k >= 2 for k in ks), sum(k == -1 for k in ks), sum(k == 0 for k in ks)
    shares = f"{len(ks)} cases, k* >= 2: {deep}, -1: {none}, 0: {zero}"
    assert 3 * deep >= len(ks), shares
    assert 10 * none >= len(ks), shares
    assert 10 * zero >= len(ks), shares


# ---- directed cases on snapshots built by hand (preempt_reference.tiny) ----
tiny, PENDING = PR.tiny, PR.PENDING


def _both(snap, oracle_mod, p, cands, on_equal=False):
    k = PR.reference_prefix(snap, oracle_mod, p, cands, PR.NOW, on_equal)
    prefix, victims = paging.preempt_of(snap, p, cands, PR.NOW, on_equal)
    assert prefix == k, (prefix, k)
    PR.check_victims(snap, oracle_mod, p, cands, prefix, victims, PR.NOW, on_equal)
    return prefix, victims


def test_directed_prefix_and_mask(oracle_mod):
    # cpu threshold 10: running 4 + 4 + 4, the pending pod asks 3 -> one victim is not enough (8 + 3 > 10), two are
    flags = [PENDING, PR.COUNTED, PR.COUNTED, PR.COUNTED]
    snap = tiny([{0: 3}, {0: 4}, {0: 4}, {0: 4}], {0: 10}, flags=flags)
    assert _both(snap, oracle_mod, 0, [1, 2, 3]) == (2, [1, 1, 0])
    assert _both(snap, oracle_mod, 0, [1])[0] == -1  # candidates exhausted
    assert _both(snap, oracle_mod, 0, [])[0] == -1   # n_cand == 0, blocked
    # pending / finished candidates contribute nothing and are never victims
    flags = [PENDING, PENDING, PR.COUNTED, PR.COUNTED | S.POD_FINISHED, PR.COUNTED, PR.COUNTED]
    snap = tiny([{0: 3}, {0: 4}, {0: 4}, {0: 4}, {0: 4}, {0: 4}], {0: 10}, flags=flags)
    assert _both(snap, oracle_mod, 0, [1, 2, 3, 4, 5]) == (4, [0, 1, 0, 1, 0])


def test_directed_exceeds_and_already_passing(oracle_mod):
    flags = [PENDING, PR.COUNTED, PR.COUNTED]
    assert _both(tiny([{0: 11}, {0: 4}, {0: 4}], {0: 10}, flags=flags), oracle_mod, 0, [1, 2])[0] == -1  # pod-requests-exceeds-threshold
    assert _both(tiny([{0: 1}, {0: 4}, {0: 4}], {0: 10}, flags=flags), oracle_mod, 0, [1, 2]) == (0, [0, 0])


def test_directed_presence_disappears(oracle_mod):
    # threshold memory 0, and the name is in `used` only through pod 1 (value 0): step 3 (0 >= 0 on a Throttle) holds while the
    # name is present and not once its one contributor is gone — the sums alone cannot tell
    flags = [PENDING, PR.COUNTED, PR.COUNTED]
    snap = tiny([{1: 0, 0: 1}, {1: 0}, {0: 1}], {1: 0, 0: 100}, flags=flags)
    assert _both(snap, oracle_mod, 0, [2, 1]) == (0, [0, 0])  # (the pod does not REQUEST memory: value 0)
    snap = tiny([{0: 1}, {0: 0}, {0: 0}], {0: 1}, flags=flags)  # cpu in `used` through two zero-valued contributors
    _both(snap, oracle_mod, 0, [1, 2])


def test_directed_count_only_threshold_and_last_counted_pod(oracle_mod):
    flags = [PENDING, PR.COUNTED, PR.COUNTED]
    snap = tiny([{0: 1}, {0: 1}, {0: 1}], {}, count=2, flags=flags)
    assert _both(snap, oracle_mod, 0, [1, 2]) == (1, [1, 0])
    snap = tiny([{0: 1}, {0: 1}, {0: 1}], {}, count=1, flags=flags)  # count threshold 1: only with nobody counted (count absent)
    assert _both(snap, oracle_mod, 0, [1, 2]) == (2, [1, 1])


@pytest.mark.parametrize("cluster", [False, True])
def test_directed_on_equal_at_exact_equality(cluster, oracle_mod):
    # used 8 + pod 2 = threshold 10 exactly: step 4 passes only without on_equal; used 10 = threshold: step 3 of a Throttle is
    # always on-equal, a ClusterThrottle's follows the caller
    flags = [PENDING, PR.COUNTED, PR.COUNTED, PR.COUNTED]
    snap = tiny([{0: 2}, {0: 2}, {0: 4}, {0: 4}], {0: 10}, cluster=cluster, flags=flags)
    assert _both(snap, oracle_mod, 0, [1, 2, 3], False)[0] == 1
    assert _both(snap, oracle_mod, 0, [1, 2, 3], True)[0] == 2
    snap = tiny([{0: 0, 1: 1}, {0: 5}, {0: 5}], {0: 10, 1: 5}, cluster=cluster, flags=flags[:3])
    _both(snap, oracle_mod, 0, [1, 2], False)
    _both(snap, oracle_mod, 0, [1, 2], True)


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_directed_cases_shared_with_the_gpu_suite(name, oracle_mod):
    snap, p, cands = PR.DIRECTED[name]()
    for on_equal in (False, True):
        _both(snap, oracle_mod, p, cands, on_equal)
