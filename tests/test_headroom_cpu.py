"""Headroom (kt_headroom_launch / kt_paged_headroom), pinned on the CPU.

``headroom(pod, cap, on_equal)`` is DEFINED by the admission walk: the number of leading Success verdicts a dry-run admission of
the queue ``[pod] * cap`` returns.  Both references of that walk add the pod's amount once per queue position when a row
repeats, so they are the reference for this number as they stand: ``model_admit`` of tests/test_paged_admit_cpu.py (manifest
level, any number of resource names) and the C oracle's ``kto_admit`` (at most 16 names).  ``limiting`` is the lowest throttle
row whose status is not ``not-throttled`` in the row PreFilter returns for the first copy that is not admitted.

Pinned here: ``paging.headroom_of`` — the closed form over the page bundles' snapshots that kt_kernels_headroom.hip computes per
lane — equals the walk; the walk's Success verdicts form a prefix (the definition is sound); and the cases hold enough probes
strictly between 0 and the cap, at 0 and at the cap that an implementation of one branch alone cannot pass them.
tests/test_headroom_gpu.py holds the kernel to the same reference."""
import copy
import functools

import numpy as np
import pytest

from kube_throttler_amd import paging
from test_paged_admit_cpu import PAGED_SEEDS, admission_case, model_admit

CAP = 24
FACTOR = 10  # test_paged_admit_cpu.loosen: thresholds a few pods deep
FEW_NAME_SEEDS = list(range(8))
HEADROOM_CASES = [(s, False) for s in FEW_NAME_SEEDS] + [(s, True) for s in PAGED_SEEDS]  # (seed, wide)


def headroom_by_walk(cs, thr_names, i, on_equal, cap=CAP):
    """The reference: (copies, limiting throttle row or -1, the walk's verdicts) of pod ``i`` by model_admit over [i] * cap."""
    res = model_admit(copy.deepcopy(cs), [i] * cap, on_equal)
    verdicts = [v for v, _ in res]
    copies = next((k for k, v in enumerate(verdicts) if v != "allow"), cap)
    limiting = -1
    if copies < cap and verdicts[copies] != "error":
        blocked = [t for t, nn in enumerate(thr_names) if res[copies][1].get(nn, "not-throttled") != "not-throttled"]
        limiting = min(blocked)
    return copies, limiting, verdicts


@functools.lru_cache(maxsize=None)
def headroom_case(seed, wide, oracle_mod):
    """(cs, pages, queue, {on_equal: {pod: (copies, limiting, verdicts)}}) — every pod of the cluster is probed: the queue
    pods and the pods PreFilter answers with an error.  Computed once, shared by the tests, never modified."""
    cs, queue = admission_case(seed, oracle_mod, wide=wide, factor=FACTOR)
    pages = cs.build_pages()
    want = {eq: {i: headroom_by_walk(cs, pages[0].thr_names, i, eq) for i in range(len(cs.pods))} for eq in (False, True)}
    return cs, pages, queue, want


@pytest.mark.parametrize("seed,wide", HEADROOM_CASES)
def test_headroom_of_equals_the_admission_walk(seed, wide, oracle_mod):
    cs, pages, queue, want = headroom_case(seed, wide, oracle_mod)
    assert (len(pages) >= 3) if wide else (len(pages) == 1)
    for on_equal in (False, True):
        for i in range(len(cs.pods)):
            copies, limiting, _ = want[on_equal][i]
            got = paging.headroom_of(pages, i, CAP, on_equal)
            assert got == (copies, limiting), f"seed {seed} wide={wide} on_equal={on_equal} pod{i}: {got} != {(copies, limiting)}"


@pytest.mark.parametrize("seed", FEW_NAME_SEEDS)
def test_headroom_of_equals_kto_admit_with_few_names(seed, oracle_mod):
    cs, pages, queue, _ = headroom_case(seed, False, oracle_mod)
    o = oracle_mod.Oracle(pages[0].snapshot)
    for on_equal in (False, True):
        for p in queue:
            _, summary, _ = o.admit(rows=np.full(CAP, p, np.int64), on_equal=on_equal)
            copies = next((k for k in range(CAP) if summary[k] != 0), CAP)
            assert paging.headroom_of(pages, p, CAP, on_equal)[0] == copies, f"seed {seed} on_equal={on_equal} pod{p}"


def test_success_verdicts_form_a_prefix(oracle_mod):
    """The definition is sound: behind the first copy that is not admitted, no copy is."""
    for seed, wide in HEADROOM_CASES:
        cs, pages, queue, want = headroom_case(seed, wide, oracle_mod)
        for on_equal in (False, True):
            for i, (copies, _, verdicts) in want[on_equal].items():
                assert all(v == "allow" for v in verdicts[:copies]) and all(v != "allow" for v in verdicts[copies:]), \
                    f"seed {seed} wide={wide} on_equal={on_equal} pod{i}: {verdicts}"


def _distribution(cases, oracle_mod):
    between = at_zero = at_cap = 0
    for seed, wide in cases:
        cs, pages, queue, want = headroom_case(seed, wide, oracle_mod)
        for on_equal in (False, True):
            for p in queue:
                c = want[on_equal][p][0]
                between += 0 < c < CAP
                at_zero += c == 0
                at_cap += c == CAP
    return between, at_zero, at_cap


def test_the_probes_cover_every_branch(oracle_mod):
    """On the reference alone, over both on_equal values together: conditions on the cases, not measurements."""
    between, at_zero, at_cap = _distribution([c for c in HEADROOM_CASES if not c[1]], oracle_mod)
    assert between >= 30, (between, at_zero, at_cap)
    between, at_zero, at_cap = _distribution([c for c in HEADROOM_CASES if c[1]], oracle_mod)
    assert between >= 5 and at_zero >= 20 and at_cap >= 20, (between, at_zero, at_cap)
