"""Gang admission (kt_admit_gangs_launch / kt_paged_admit_gangs), pinned on the CPU.

The reference is built from ``model_admit`` and ``reserve`` of tests/test_paged_admit_cpu.py: the queue is cut into consecutive
gangs; the members of a gang go through the per-pod step (Model.check against ``cs.reserved``, Reserve on allow) one after the
other, all of them also behind one that failed; when any verdict is not ``allow`` the reserved amounts go back to the copy taken
before the gang (every member that reserved gets Unreserve: plugin.go:240-257 -> reservedResourceAmounts.removePod,
reserved_resource_amounts.go:79-90, the totals recomputed over the remaining pods, :148-156).

Pinned here: size-1 gangs and a gang of pods that are all allowed are the C oracle's ``kto_admit``; and the cases
tests/test_gang_admit_gpu.py runs hold enough rolled-back gangs with admitted members, admitted gangs of several pods, and
pods whose verdict depends on a rollback, that an implementation without the rollback cannot pass them."""
import copy
import random

import numpy as np
import pytest

from kube_throttler_amd import snapshot as S
from test_paged_admit_cpu import PAGED_SEEDS, VERDICT_NAME, admission_case, model_admit, reserved_totals, row_of

ONE_PAGE_SEEDS = list(range(24))  # TM.random_cluster: at most 16 resource names
FACTOR = 10                       # test_paged_admit_cpu.loosen: queues where some pods pass and later ones are blocked
MAX_GANG = 5
# the cases of the GPU parity tests: (seed, wide)
GANG_CASES = [(s, False) for s in ONE_PAGE_SEEDS] + [(s, True) for s in PAGED_SEEDS]


def gang_cut(seed, n, max_size=MAX_GANG):
    """Offsets [n_gangs + 1] of consecutive gangs of 1..max_size pods over a queue of n."""
    r = random.Random(1000 + seed)
    off = [0]
    while off[-1] < n:
        off.append(min(n, off[-1] + r.randint(1, max_size)))
    return off


def model_admit_gangs(cs, queue, gang_off, on_equal):
    """The reference: ([(verdict, {throttle: status})] per queue position, [admitted] per gang); ``cs.reserved`` ends as the
    committed totals."""
    out, admitted = [], []
    for g in range(len(gang_off) - 1):
        before = copy.deepcopy(cs.reserved)
        res = model_admit(cs, queue[gang_off[g]:gang_off[g + 1]], on_equal)
        ok = all(v == "allow" for v, _ in res)
        if not ok:
            cs.reserved = before
        out += res
        admitted.append(ok)
    return out, admitted


def gang_case(seed, wide, oracle_mod):
    cs, queue = admission_case(seed, oracle_mod, wide=wide, factor=FACTOR)
    return cs, queue, gang_cut(seed, len(queue))


def _oracle_admit(cs, queue, on_equal, oracle_mod):
    pages = cs.build_pages()
    assert len(pages) == 1
    b = pages[0]
    status, summary, reserved = oracle_mod.Oracle(b.snapshot).admit(rows=np.array(queue, np.int64), on_equal=on_equal)
    verdicts = [VERDICT_NAME[int(S.VERDICT_ERROR if w == 2 else S.VERDICT_BLOCK if w & 1 else S.VERDICT_ALLOW)] for w in summary]
    rows = [row_of(status[k], b.thr_names) for k in range(len(queue))]
    totals = {nn: b.amount_to_dict(reserved, t) for t, nn in enumerate(b.thr_names)}
    return verdicts, rows, totals


@pytest.mark.parametrize("seed", ONE_PAGE_SEEDS)
def test_gangs_of_one_pod_are_kto_admit(seed, oracle_mod):
    cs, queue = admission_case(seed, oracle_mod, wide=False, factor=FACTOR)
    for on_equal in (False, True):
        verdicts, rows, totals = _oracle_admit(cs, queue, on_equal, oracle_mod)
        work = copy.deepcopy(cs)
        want, admitted = model_admit_gangs(work, queue, list(range(len(queue) + 1)), on_equal)
        assert [v for v, _ in want] == verdicts, f"seed {seed} on_equal={on_equal}"
        assert [st for _, st in want] == rows, f"seed {seed} on_equal={on_equal}"
        assert admitted == [v == "allow" for v in verdicts]
        got = reserved_totals(work)
        for nn, a in totals.items():
            assert got.get(nn, {}) == a, f"seed {seed}: reserved of {nn}"


@pytest.mark.parametrize("seed", ONE_PAGE_SEEDS)
def test_one_gang_of_allowed_pods_is_kto_admit(seed, oracle_mod):
    cs, queue = admission_case(seed, oracle_mod, wide=False, factor=FACTOR)
    for on_equal in (False, True):
        plain = model_admit(copy.deepcopy(cs), queue, on_equal)
        allowed = [i for i, (v, _) in zip(queue, plain) if v == "allow"]  # admitted in order: each stays allowed without the others
        verdicts, rows, totals = _oracle_admit(cs, allowed, on_equal, oracle_mod)
        assert all(v == "allow" for v in verdicts)
        work = copy.deepcopy(cs)
        want, admitted = model_admit_gangs(work, allowed, [0, len(allowed)] if allowed else [0], on_equal)
        assert [v for v, _ in want] == verdicts and [st for _, st in want] == rows, f"seed {seed} on_equal={on_equal}"
        assert admitted == ([True] if allowed else [])
        got = reserved_totals(work)
        for nn, a in totals.items():
            assert got.get(nn, {}) == a, f"seed {seed}: reserved of {nn}"


def test_the_gpu_cases_need_the_rollback(oracle_mod):
    """The cap that keeps tests/test_gang_admit_gpu.py honest: over its seeds and gang cuts the reference alone shows rolled-back
    gangs that had reserved, admitted gangs of several pods, and pods that are admitted only because an earlier gang was
    rolled back (their verdict differs from plain admission of the same queue)."""
    rolled_back_with_admitted = admitted_multi = differs = 0
    for seed, wide in GANG_CASES:
        cs, queue, off = gang_case(seed, wide, oracle_mod)
        for on_equal in (False, True):
            want, admitted = model_admit_gangs(copy.deepcopy(cs), queue, off, on_equal)
            plain = model_admit(copy.deepcopy(cs), queue, on_equal)
            for g, ok in enumerate(admitted):
                members = want[off[g]:off[g + 1]]
                if not ok and any(v == "allow" for v, _ in members):
                    rolled_back_with_admitted += 1
                if ok and len(members) >= 2:
                    admitted_multi += 1
            differs += sum(1 for (v, _), (pv, _) in zip(want, plain) if v != pv)
    print(f"rolled back with an admitted member: {rolled_back_with_admitted}, admitted gangs of >= 2: {admitted_multi}, "
          f"verdicts that differ from plain admission: {differs}")
    assert rolled_back_with_admitted >= 5
    assert admitted_multi >= 5
    assert differs >= 3
