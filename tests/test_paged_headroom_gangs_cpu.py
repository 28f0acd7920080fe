"""Gang headroom over pages (kt_paged_headroom_gangs), pinned on the CPU.

Pinned here: ``paging.paged_headroom_gangs_of`` — the restatement of what kt_kernels_headroom_gangs_paged.hip computes (every
(throttle, page) pair a throttle of its own: that page's A_t, the range cut at the running minimum and at int64's end, the
64-ary search, the lexicographic minimum; the pod count on page 0 only).

The main yardstick are the one-page cases of tests/test_headroom_gangs_cpu.py with the cluster rebuilt as pages of one and of two
names: splitting the names over pages changes nothing in the semantics, so the answer must be the C oracle's one-page admission
walk that module computes.  Their distribution (>= 60 answers strictly between, >= 60 at 0, >= 60 at the cap) is pinned there; here
it is pinned that page 0 alone does not decide them.  The wide clusters (three pages of 16 / 16 / 8 names) are held to the
manifest walk; they cover three pages, the widest bucket and the Error rule, hardly the search: nearly all their answers are 0
or the cap.  Identity I3 — the paged answer is the minimum over the pages' own single-engine answers of (copies, blocker or the
gang size, limiting or +inf) — holds where every page carries the same count part, as ``build_pages`` produces it.
tests/test_paged_headroom_gangs_gpu.py holds the kernel to the same references."""
import functools
import random

import pytest

from headroom_gangs_reference import headroom_gangs_by_model
from kube_throttler_amd import paging
from test_gang_admit_cpu import gang_cut
from test_headroom_gangs_cpu import CAP, FACTOR, SEEDS, gangs_case
from test_paged_admit_cpu import PAGED_SEEDS, admission_case

SPLITS = (1, 2)
INF = float("inf")


@functools.lru_cache(maxsize=None)
def split_case(seed, max_dims, oracle_mod):
    """(page bundles of at most ``max_dims`` names, [members], {on_equal: [(copies, limiting, blocker)]}) — gangs_case's cluster
    cut into pages; the expected answers are gangs_case's own: the one-page walk.  Computed once, shared, never modified."""
    cs, _, gangs, want = gangs_case(seed, oracle_mod)
    return cs.build_pages(max_dims=max_dims), gangs, want


@functools.lru_cache(maxsize=None)
def wide_case(seed, oracle_mod):
    """(cs, page bundles, [members]) of a cluster with more than 32 resource names, gangs cut as gangs_case cuts them."""
    cs, queue = admission_case(seed, oracle_mod, wide=True, factor=FACTOR)
    pages = cs.build_pages()
    assert len(pages) == 3
    everyone = list(range(len(cs.pods)))
    random.Random(77 + seed).shuffle(everyone)
    gangs = []
    for rows, cut in ((queue, gang_cut(seed, len(queue))), (everyone, gang_cut(seed + 500, len(everyone)))):
        gangs += [rows[cut[g]:cut[g + 1]] for g in range(len(cut) - 1)]
    return cs, pages, gangs


@functools.lru_cache(maxsize=None)
def wide_want(seed, oracle_mod):
    cs, pages, gangs = wide_case(seed, oracle_mod)
    return {eq: [headroom_gangs_by_model(cs, pages[0].thr_names, m, CAP, eq) for m in gangs] for eq in (False, True)}


def by_identity_3(snaps, members, cap, on_equal):
    """I3: the minimum over the pages' own single-engine answers of (copies, blocker or the gang size, limiting or +inf), mapped
    back to (cap, -1, -1) at the cap; also the page the minimum comes from first."""
    keys = []
    for s in snaps:
        copies, limiting, blocker = paging.headroom_gangs_of(s, members, cap, on_equal)
        keys.append((copies, len(members) if blocker < 0 else blocker, INF if limiting < 0 else limiting))
    copies, blocker, limiting = min(keys)
    answer = (cap, -1, -1) if copies >= cap else (copies, -1 if limiting == INF else limiting, blocker)
    return answer, keys.index(min(keys))


@pytest.mark.parametrize("max_dims", SPLITS)
@pytest.mark.parametrize("seed", SEEDS)
def test_split_pages_equal_the_one_page_walk(seed, max_dims, oracle_mod):
    pages, gangs, want = split_case(seed, max_dims, oracle_mod)
    snaps = [b.snapshot for b in pages]
    for on_equal in (False, True):
        for k, members in enumerate(gangs):
            got = paging.paged_headroom_gangs_of(snaps, members, CAP, on_equal)
            assert got == want[on_equal][k], f"seed {seed} max_dims={max_dims} on_equal={on_equal} gang {members}: {got} != {want[on_equal][k]}"


@pytest.mark.parametrize("seed", SEEDS[:6])
def test_one_snapshot_is_headroom_gangs_of(seed, oracle_mod):
    cs, page, gangs, want = gangs_case(seed, oracle_mod)
    for on_equal in (False, True):
        for members in gangs:
            assert paging.paged_headroom_gangs_of([page.snapshot], members, CAP, on_equal) == paging.headroom_gangs_of(page.snapshot, members, CAP, on_equal)


@pytest.mark.parametrize("max_dims", SPLITS)
def test_page_zero_alone_cannot_pass(max_dims, oracle_mod):
    """Conditions on the inputs, on the references alone: a kernel that reads page 0 only gets these wrong."""
    differs = between_later = 0
    for seed in SEEDS:
        pages, gangs, want = split_case(seed, max_dims, oracle_mod)
        for on_equal in (False, True):
            for members, answer in zip(gangs, want[on_equal]):
                own = paging.headroom_gangs_of(pages[0].snapshot, members, CAP, on_equal)
                differs += own != answer
                between_later += own != answer and 0 < answer[0] < CAP
    print(f"max_dims={max_dims}: page 0's own answer differs in {differs} cases, {between_later} of them strictly between 0 and the cap")
    assert differs >= (40 if max_dims == 1 else 20)
    assert between_later >= (20 if max_dims == 1 else 8)


@pytest.mark.parametrize("max_dims", SPLITS)
@pytest.mark.parametrize("seed", SEEDS)
def test_identity_3_on_the_split_pages(seed, max_dims, oracle_mod):
    pages, gangs, want = split_case(seed, max_dims, oracle_mod)
    snaps = [b.snapshot for b in pages]
    for on_equal in (False, True):
        for k, members in enumerate(gangs):
            assert by_identity_3(snaps, members, CAP, on_equal)[0] == want[on_equal][k], f"seed {seed} max_dims={max_dims} gang {members}"


@pytest.mark.parametrize("seed", PAGED_SEEDS)
def test_wide_clusters_equal_the_manifest_walk(seed, oracle_mod):
    cs, pages, gangs = wide_case(seed, oracle_mod)
    want = wide_want(seed, oracle_mod)
    snaps = [b.snapshot for b in pages]
    assert [s.D for s in snaps] == [16, 16, 8]
    for on_equal in (False, True):
        for k, members in enumerate(gangs):
            got = paging.paged_headroom_gangs_of(snaps, members, CAP, on_equal)
            assert got == want[on_equal][k], f"seed {seed} on_equal={on_equal} gang {members}: {got} != {want[on_equal][k]}"
            assert by_identity_3(snaps, members, CAP, on_equal)[0][0] == want[on_equal][k][0]  # (in copies)


def test_what_the_wide_clusters_cover(oracle_mod):
    """Know what these are: three pages, the widest bucket, the Error rule and later pages that decide — not the search."""
    at_zero = at_cap = error_gangs = later = total = 0
    for seed in PAGED_SEEDS:
        cs, pages, gangs = wide_case(seed, oracle_mod)
        want = wide_want(seed, oracle_mod)
        snaps = [b.snapshot for b in pages]
        for on_equal in (False, True):
            for members, (copies, limiting, blocker) in zip(gangs, want[on_equal]):
                total += 1
                at_zero += copies == 0
                at_cap += copies == CAP
                error_gangs += copies == 0 and blocker >= 0 and limiting == -1
                later += copies < CAP and paging.headroom_gangs_of(snaps[0], members, CAP, on_equal)[0] != copies
    print(f"{total} answers: {at_zero} at 0, {at_cap} at the cap, {error_gangs} stopped by an Error member, {later} decided by a page >= 1")
    assert at_zero >= 40 and at_cap >= 8 and error_gangs >= 4 and later >= 10


@pytest.mark.parametrize("seed", SEEDS)
def test_a_gang_of_one_is_headroom_of(seed, oracle_mod):
    for max_dims in SPLITS:
        pages, gangs, want = split_case(seed, max_dims, oracle_mod)
        snaps = [b.snapshot for b in pages]
        for on_equal in (False, True):
            for p in range(snaps[0].n_pods):
                copies, limiting, _ = paging.paged_headroom_gangs_of(snaps, [p], CAP, on_equal)
                assert (copies, limiting) == paging.headroom_of(pages, p, CAP, on_equal), f"seed {seed} max_dims={max_dims} on_equal={on_equal} pod{p}"
