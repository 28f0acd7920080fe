"""Gang headroom (kt_headroom_gangs_launch), pinned on the CPU.

The reference is the admission walk (tests/headroom_gangs_reference.py): the leading complete copies of the C oracle's admit of
``members * cap``.  Pinned here: ``paging.headroom_gangs_of`` — the restatement of what kt_kernels_headroom_gangs.hip computes
(per throttle A_t, the capped range, the 64-ary search, the lexicographic minimum) — equals the walk in copies, limiting throttle
and blocker on the one-page seeds of tests/test_headroom_cpu.py and tests/test_gang_admit_cpu.py, gangs cut by ``gang_cut``; the
admitted copies form a prefix; a gang of one is ``paging.headroom_of``; and the cases hold enough answers at 0, strictly between
and at the cap that one branch alone cannot pass.  tests/test_headroom_gangs_gpu.py holds the kernel to the same reference."""
import copy
import functools
import random

import pytest

from headroom_gangs_reference import headroom_gangs_by_model, headroom_gangs_by_oracle, oracle_walk
from kube_throttler_amd import paging
from test_gang_admit_cpu import ONE_PAGE_SEEDS, gang_cut, model_admit_gangs
from test_headroom_cpu import FEW_NAME_SEEDS
from test_paged_admit_cpu import admission_case

CAP = 24
FACTOR = 40  # test_paged_admit_cpu.loosen: thresholds a few GANGS deep (chosen on the reference: see the distribution test)
SEEDS = sorted(set(FEW_NAME_SEEDS) | set(ONE_PAGE_SEEDS))


@functools.lru_cache(maxsize=None)
def gangs_case(seed, oracle_mod):
    """(cs, page bundle, [members], {on_equal: [(copies, limiting, blocker)]}) — the gangs: the queue of admission_case (no
    pod PreFilter answers with an error) cut by gang_cut, then every pod of the cluster, those error pods included, shuffled
    and cut again.  Computed once, shared by the tests, never modified."""
    cs, queue = admission_case(seed, oracle_mod, wide=False, factor=FACTOR)
    pages = cs.build_pages()
    assert len(pages) == 1
    everyone = list(range(len(cs.pods)))
    random.Random(77 + seed).shuffle(everyone)
    gangs = []
    for rows, cut in ((queue, gang_cut(seed, len(queue))), (everyone, gang_cut(seed + 500, len(everyone)))):
        gangs += [rows[cut[g]:cut[g + 1]] for g in range(len(cut) - 1)]
    o = oracle_mod.Oracle(pages[0].snapshot)
    want = {eq: [headroom_gangs_by_oracle(o, m, CAP, eq) for m in gangs] for eq in (False, True)}
    return cs, pages[0], gangs, want


@pytest.mark.parametrize("seed", SEEDS)
def test_headroom_gangs_of_equals_the_walk(seed, oracle_mod):
    cs, page, gangs, want = gangs_case(seed, oracle_mod)
    for on_equal in (False, True):
        for k, members in enumerate(gangs):
            got = paging.headroom_gangs_of(page.snapshot, members, CAP, on_equal)
            assert got == want[on_equal][k], f"seed {seed} on_equal={on_equal} gang {members}: {got} != {want[on_equal][k]}"


@pytest.mark.parametrize("seed", SEEDS[:4])
def test_the_oracle_walk_is_the_manifest_walk(seed, oracle_mod):
    cs, page, gangs, want = gangs_case(seed, oracle_mod)
    for on_equal in (False, True):
        for k, members in enumerate(gangs[:6]):
            assert headroom_gangs_by_model(cs, page.thr_names, members, CAP, on_equal) == want[on_equal][k], f"seed {seed} gang {members}"


def test_admitted_copies_form_a_prefix(oracle_mod):
    """The definition is sound: every copy in front of the answer is admitted in full, and no copy behind it is."""
    for seed in SEEDS:
        cs, page, gangs, want = gangs_case(seed, oracle_mod)
        o = oracle_mod.Oracle(page.snapshot)
        for on_equal in (False, True):
            for k, members in enumerate(gangs):
                g, copies = len(members), want[on_equal][k][0]
                _, codes = oracle_walk(o, members, CAP, on_equal)
                whole = [all(c == 0 for c in codes[j * g:(j + 1) * g]) for j in range(CAP)]
                assert whole == [True] * copies + [False] * (CAP - copies), f"seed {seed} on_equal={on_equal} gang {members}: {whole}"


@pytest.mark.parametrize("seed", SEEDS[:3])
def test_the_answer_is_the_gang_admission_of_the_copies(seed, oracle_mod):
    """... and with the rollback of the manifest-level gang admission: the admitted bytes of `cap` copies are that prefix."""
    cs, page, gangs, want = gangs_case(seed, oracle_mod)
    for on_equal in (False, True):
        for k, members in enumerate(gangs[:5]):
            g = len(members)
            _, admitted = model_admit_gangs(copy.deepcopy(cs), list(members) * CAP, [j * g for j in range(CAP + 1)], on_equal)
            copies = want[on_equal][k][0]
            assert admitted == [True] * copies + [False] * (CAP - copies), f"seed {seed} on_equal={on_equal} gang {members}"


@pytest.mark.parametrize("seed", SEEDS)
def test_a_gang_of_one_is_headroom_of(seed, oracle_mod):
    cs, page, gangs, want = gangs_case(seed, oracle_mod)
    for on_equal in (False, True):
        for p in range(len(cs.pods)):
            copies, limiting, _ = paging.headroom_gangs_of(page.snapshot, [p], CAP, on_equal)
            assert (copies, limiting) == paging.headroom_of([page], p, CAP, on_equal), f"seed {seed} on_equal={on_equal} pod{p}"


def test_the_mirror_scenario_on_the_model_alone(oracle_mod):
    """What the expectations of tests/cpp/host_plugin_headroom_gang_test.cpp rest on, without the mirror and without a GPU: the
    restatement's answers on the driver's scenario written as manifests, held to the manifest walk."""
    from test_host_headroom_gang_gpu import scenario
    from test_paged_admit_cpu import write_status
    cs = scenario()
    write_status(cs, oracle_mod)
    page = cs.build_pages()[0]
    rows = {p["metadata"]["name"]: i for i, p in enumerate(cs.pods)}
    ask = lambda members, cap: paging.headroom_gangs_of(page.snapshot, [rows[m] for m in members], cap)
    jobs, few = page.thr_names.index("ns1/jobs"), page.thr_names.index("ns1/few")
    assert ask(["launcher", "w1", "w2"], 10) == (2, jobs, 2) and ask(["w2", "w1", "launcher"], 10) == (2, jobs, 2)
    assert ask(["w1", "w2"], 10) == (3, few, 1) and ask(["launcher", "w1", "w2"], 2) == (2, -1, -1)
    assert ask(["launcher"], 50) == (10, jobs, 0) == paging.headroom_of([page], rows["launcher"], 50) + (0,)
    assert ask(["launcher", "ghost", "huge"], 10) == (0, -1, 1) and ask(["huge", "ghost"], 10) == (0, jobs, 0)
    for members, cap in ((["launcher", "w1", "w2"], 10), (["w1", "w2"], 10), (["launcher", "free"], 50), (["launcher", "ghost", "huge"], 10)):
        assert ask(members, cap) == headroom_gangs_by_model(cs, page.thr_names, [rows[m] for m in members], cap, False), members


def test_the_cases_cover_every_branch(oracle_mod):
    """On the reference alone, over both on_equal values together: conditions on the cases, not measurements."""
    between = at_zero = at_cap = multi_between = error_gangs = blocker_behind_first = 0
    for seed in SEEDS:
        cs, page, gangs, want = gangs_case(seed, oracle_mod)
        for on_equal in (False, True):
            for members, (copies, limiting, blocker) in zip(gangs, want[on_equal]):
                between += 0 < copies < CAP
                multi_between += 0 < copies < CAP and len(members) >= 2
                at_zero += copies == 0
                at_cap += copies == CAP
                error_gangs += copies == 0 and blocker >= 0 and limiting == -1
                blocker_behind_first += blocker > 0
    print(f"between {between} (gangs of >= 2: {multi_between}), at 0: {at_zero}, at the cap: {at_cap}, stopped by an Error member: "
          f"{error_gangs}, blocker behind the first member: {blocker_behind_first}")
    assert between >= 60 and multi_between >= 40
    assert at_zero >= 60 and at_cap >= 60
    assert error_gangs >= 10 and blocker_behind_first >= 40
