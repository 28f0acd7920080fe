"""kt_paged_headroom_gangs on the GPU (csrc/kt_kernels_headroom_gangs_paged.hip): how many copies of a whole gang the throttles
admit over pages of resource names — copies, limiting throttle and blocker compared bit for bit, for both isThrottledOnEqual values.

References: on the generated clusters the one-page admission walk of the C oracle (the names split over pages of one) and the
manifest walk (the wide clusters), as tests/test_paged_headroom_gangs_cpu.py computes them; on the hand-built pages (the same
count part on every page) identity I3 over the oracle's admission walk per page — the minimum over the pages of (copies, blocker
or the gang size, limiting or +inf) — plus ``paging.paged_headroom_gangs_of``; where the cap is too large to walk, the value by
hand.  The identities: one page returns the single engine's bytes (I1), a gang of one is kt_paged_headroom (I2), the copies are
the leading complete copies of a dry kt_paged_admit (I4).  The shapes are the smallest at which the kernel can still go wrong: one
case per DT instantiation beside a narrow page, a gang beyond one member block, a deciding throttle in the second chunk of the
affected-throttle list, more gangs than the grid has workgroups, the 64-ary search at the edges of its rounds with the deciding
amount on page 1, the running minimum across the pages of one throttle, the int64 range cut per page, presence on a later page,
the blocker as the minimum over pages, a tie between rows the affected-throttle list does not hold in order (on one engine too),
a page that is skipped, refusals and what the call leaves pending."""
import numpy as np
import pytest

import paged_preempt_reference as PPR
import preempt_reference as PR
from headroom_gangs_reference import headroom_gangs_by_oracle
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from test_headroom_gangs_cpu import CAP, SEEDS, gangs_case
from test_paged_admit_cpu import PAGED_SEEDS
from test_paged_headroom_gangs_cpu import split_case, wide_case, wide_want

pytestmark = pytest.mark.gpu
MAXCAP = E.HEADROOM_MAX_CAP
P = PR.PENDING
INF = float("inf")


def _engines(snaps, **kw):
    return [E.Engine.for_snapshot(s, **kw) for s in snaps]


def _close(engs):
    for e in engs:
        e.close()


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def _queue(gangs):
    rows = [int(p) for g in gangs for p in g]
    off = np.cumsum([0] + [len(g) for g in gangs]).astype(np.int64)
    return rows, off


def launch_all(engs, gangs, cap, on_equal=False):
    """All gangs in ONE call -> per gang (copies, limiting, blocker as a position inside the gang)."""
    rows, off = _queue(gangs)
    copies, limiting, blocker = E.paged_headroom_gangs(engs, rows, off, cap, on_equal)
    assert copies.dtype == np.int64 and limiting.dtype == np.int32 and blocker.dtype == np.int64
    assert copies.shape == limiting.shape == blocker.shape == (len(gangs),)
    out = []
    for g in range(len(gangs)):
        b = int(blocker[g])
        assert b == -1 or off[g] <= b < off[g + 1], (g, b)
        out.append((int(copies[g]), int(limiting[g]), b if b < 0 else b - int(off[g])))
    return out


def by_identity_3(snaps, oracle_mod, members, cap, on_equal):
    """I3 over the oracle's admission walk of ``members * cap`` on every page of its own (the count part is the same in every page)."""
    keys = []
    for s in snaps:
        copies, limiting, blocker = headroom_gangs_by_oracle(oracle_mod.Oracle(s), members, cap, on_equal)
        keys.append((copies, len(members) if blocker < 0 else blocker, INF if limiting < 0 else limiting))
    copies, blocker, limiting = min(keys)
    return (cap, -1, -1) if copies >= cap else (copies, -1 if limiting == INF else limiting, blocker)


def held_to_everything(snaps, oracle_mod, gangs, cap, on_equal=False, walk=True):
    """The engines against paging.paged_headroom_gangs_of and (``walk``) against I3 over the oracle's walks per page."""
    engs = _engines(snaps)
    try:
        got = launch_all(engs, gangs, cap, on_equal)
    finally:
        _close(engs)
    for g, members in enumerate(gangs):
        assert got[g] == paging.paged_headroom_gangs_of(snaps, members, cap, on_equal), f"gang {g} {members} cap={cap} on_equal={on_equal}"
        if walk:
            ref = by_identity_3(snaps, oracle_mod, members, cap, on_equal)
            assert got[g] == ref, f"gang {g} {members} cap={cap} on_equal={on_equal}: {got[g]} != {ref}"
    return got


def _same_bytes(x, y):
    return all(a.tobytes() == b.tobytes() and a.shape == b.shape and a.dtype == b.dtype for a, b in zip(x, y))


# ---- the generated clusters of the CPU pin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS[:10])
def test_split_clusters(seed, oracle_mod):
    """The one-page clusters as pages of one name each, all gangs in ONE call: the answer is the one-page walk's."""
    pages, gangs, want = split_case(seed, 1, oracle_mod)
    engs = _engines([b.snapshot for b in pages])
    try:
        for on_equal in (False, True):
            assert launch_all(engs, gangs, CAP, on_equal) == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        _close(engs)


@pytest.mark.parametrize("seed", PAGED_SEEDS[:2])
def test_wide_clusters(seed, oracle_mod):
    """Three pages of 16 / 16 / 8 names against the manifest walk."""
    cs, pages, gangs = wide_case(seed, oracle_mod)
    want = wide_want(seed, oracle_mod)
    engs = _engines([b.snapshot for b in pages])
    try:
        for on_equal in (False, True):
            assert launch_all(engs, gangs, CAP, on_equal) == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        _close(engs)


# ---- identities ------------------------------------------------------------------------------------------------------------
def _directed_single_engine_shapes():
    """The directed shapes of tests/test_headroom_gangs_gpu.py: (snapshot, gangs, cap)."""
    from test_headroom_gangs_gpu import BIG, _two_namespaces, _two_rows
    out = []
    for D in (1, 8, 16):
        d = D - 1
        other = {x: 2 for x in range(D) if x != d}
        a, b = dict(other), dict(other)
        a[d], b[d] = 3, 4
        snap = PR.tiny([a, b], {d: 30, **({0: 1000} if D > 1 else {})}, flags=[P, P], D=D)
        snap.thr_used.set_row(0, {d: 2}, 1)
        out.append((snap, [[0, 1]], CAP))
    n = 70
    for count in (50, 1000):
        out.append((PR.tiny([{0: 1}] * n, {}, count=count, flags=[P] * n, pod_ns=[1 if i == 66 else 0 for i in range(n)]), [list(range(n))], 3))
    out.append((PR.tiny([{0: 1}] * n, {}, count=3 * n + 65, flags=[P] * n), [list(range(n))], 6))
    for counts in ((2 * 5000 + 1, 2 * 40 + 1), (2 * 40 + 1, 2 * 5000 + 1), (2 * 70, 2 * 3)):
        out.append((_two_rows(*counts), [[0, 1], [1, 0], [0]], MAXCAP))
    for cluster in (False, True):
        out.append((PR.tiny([{0: 2}, {0: 2}], {0: 4}, flags=[P, P], cluster=cluster), [[0, 1], [0]], CAP))
        out.append((PR.tiny([{0: 0, 1: 1}, {0: 5}], {0: 5, 1: 100}, flags=[P, P], cluster=cluster), [[0, 1], [1, 0]], CAP))
    out.append((PR.tiny([{1: BIG}] * 3, {1: 8 * BIG}, flags=[P] * 3), [[0, 1, 2]], MAXCAP))
    out.append((PR.tiny([{1: BIG}] * 3, {1: (1 << 63) - 1}, flags=[P] * 3), [[0, 1, 2]], MAXCAP))
    out.append((_two_namespaces(), [[0, 1], [1, 0], [0, 3, 2], [0, 2, 3], [2]], CAP))
    return out


def test_one_page_returns_the_single_engine_bytes_directed():
    """I1: with one page all three outputs are byte for byte kt_headroom_gangs_launch + kt_headroom_gangs_fetch's."""
    for snap, gangs, cap in _directed_single_engine_shapes():
        rows, off = _queue(gangs)
        eng = E.Engine.for_snapshot(snap)
        try:
            for on_equal in (False, True):
                single = eng.headroom_gangs(rows, off, cap=cap, on_equal=on_equal)
                assert _same_bytes(E.paged_headroom_gangs([eng], rows, off, cap, on_equal), single), (gangs, cap, on_equal)
        finally:
            eng.close()


@pytest.mark.parametrize("seed", SEEDS[:2])
def test_one_page_returns_the_single_engine_bytes_on_clusters(seed, oracle_mod):
    cs, page, gangs, want = gangs_case(seed, oracle_mod)
    rows, off = _queue(gangs)
    eng = E.Engine.for_snapshot(page.snapshot)
    try:
        for on_equal in (False, True):
            single = eng.headroom_gangs(rows, off, cap=CAP, on_equal=on_equal)
            assert _same_bytes(E.paged_headroom_gangs([eng], rows, off, CAP, on_equal), single)
            assert launch_all([eng], gangs, CAP, on_equal) == want[on_equal]
    finally:
        eng.close()


def test_a_gang_of_one_is_kt_paged_headroom(oracle_mod):
    """I2: copies and limiting, byte for byte."""
    pages, gangs, want = split_case(SEEDS[1], 1, oracle_mod)
    n = pages[0].snapshot.n_pods
    engs = _engines([b.snapshot for b in pages])
    try:
        for on_equal in (False, True):
            for cap in (CAP, MAXCAP):
                copies, limiting = E.paged_headroom(engs, np.arange(n), cap, on_equal)
                gcopies, glimiting, gblocker = E.paged_headroom_gangs(engs, np.arange(n), np.arange(n + 1), cap, on_equal)
                assert gcopies.tobytes() == copies.tobytes() and glimiting.tobytes() == limiting.tobytes(), (on_equal, cap)
                assert gblocker.tolist() == [-1 if c == cap else i for i, c in enumerate(copies)]
    finally:
        _close(engs)


def test_the_copies_are_those_of_a_dry_paged_admission(oracle_mod):
    """I4 with cap 6: the leading complete copies of a dry kt_paged_admit of members * cap."""
    cap = 6
    pages, gangs, want = split_case(SEEDS[2], 1, oracle_mod)
    engs = _engines([b.snapshot for b in pages])
    try:
        for on_equal in (False, True):
            got = launch_all(engs, gangs, cap, on_equal)
            for g, members in enumerate(gangs):
                _, summary = E.paged_admit(engs, list(members) * cap, on_equal=on_equal)
                ok = [all(int(w) == 0 for w in summary[j * len(members):(j + 1) * len(members)]) for j in range(cap)]
                assert got[g][0] == next((j for j in range(cap) if not ok[j]), cap), f"gang {members} on_equal={on_equal}"
    finally:
        _close(engs)


# ---- one case per instantiation, member blocks, list chunks, the grid -------------------------------------------------------
@pytest.mark.parametrize("where", ["wide", "narrow"])
@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, where, oracle_mod):
    """The widest page has D names, the narrow one 3 (1 with D = 1): the DT bucket of the widest page serves both.  The deciding
    name sits on page 1 — the LAST name of the wide page, or the last name of the narrow one; the others are requested and
    reserved but no threshold stops them.  3 + 4 per copy against 30 with 2 used: copies 0 .. 3 pass (2 + 28 = 30), on_equal
    stops the second member of copy 3."""
    Dn = 1 if D == 1 else 3

    def page(width, deciding):
        d = width - 1
        a, b = {x: 2 for x in range(width)}, {x: 2 for x in range(width)}
        if not deciding:
            return PR.tiny([a, b], {}, flags=[P, P], D=width)
        a[d], b[d] = 3, 4
        snap = PR.tiny([a, b], {d: 30, **({0: 1000} if width > 1 else {})}, flags=[P, P], D=width)
        snap.thr_used.set_row(0, {d: 2}, 1)
        return snap

    snaps = [page(Dn, False), page(D, True)] if where == "wide" else [page(D, False), page(Dn, True)]
    for on_equal in (False, True):
        got, = held_to_everything(snaps, oracle_mod, [[0, 1]], CAP, on_equal)
        assert got == ((3, 0, 1) if on_equal else (4, 0, 0))


def test_seventy_members_a_name_of_page_one(oracle_mod):
    """The member loop beyond one block of 64: 70 members ask 1 each of a page-1 name against 3 x 70 + 65 — member 65 of copy 3."""
    n = 70
    snaps = PPR.pages_of([[{0: 2}] * n, [{0: 1}] * n], [{}, {0: 3 * n + 65}], [P] * n)
    got, = held_to_everything(snaps, oracle_mod, [list(range(n))], 6)
    assert got == (3, 0, 65)


def test_seventy_members_an_error_member_in_the_second_block(oracle_mod):
    """The member whose namespace has no object sits at position 66; with 50 of a page-1 name member 50 is stopped in front of
    it (50 reserved + 1 > 50), with 1000 the Error member is the blocker and nobody is limiting."""
    n = 70
    for th, want in ((50, (0, 0, 50)), (1000, (0, -1, 66))):
        snaps = PPR.pages_of([[{0: 2}] * n, [{0: 1}] * n], [{}, {0: th}], [P] * n, pod_ns=[1 if i == 66 else 0 for i in range(n)])
        got, = held_to_everything(snaps, oracle_mod, [list(range(n))], 3)
        assert got == want


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect both members — more than one chunk of the LDS list holds; only the last row stops a copy, on page 1."""
    T = 1030
    snaps = PPR.pages_of([[{0: 1}, {0: 1}], [{0: 3}, {0: 3}]], [{}, {0: 20}], [P, P], T=T, row=T - 1)
    for snap in snaps:
        for t in range(T - 1):
            snap.thr_ns[t] = 0
            snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    assert len(paging.affected_throttles(snaps[0], 0)[1]) == T
    got, = held_to_everything(snaps, oracle_mod, [[0, 1]], 9)
    assert got == (3, T - 1, 0)  # 18 + 3 > 20


def test_more_gangs_than_the_grid_has_workgroups(oracle_mod):
    """2050 two-member gangs in one call: the grid strides beyond 2048.  Pods are shared between the gangs; both pages decide."""
    snaps = PPR.pages_of([[{0: a} for a in (1, 2, 3, 4, 5, 3)], [{0: a} for a in (5, 1, 4, 2, 3, 1)]], [{0: 40}, {0: 37}], [P] * 6, counts=[21, 21])
    pairs = [[i, j] for i in range(6) for j in range(6) if i != j]
    want = {tuple(g): by_identity_3(snaps, oracle_mod, g, 16, False) for g in pairs}
    own = {tuple(g): headroom_gangs_by_oracle(oracle_mod.Oracle(snaps[0]), g, 16, False) for g in pairs}
    for g in pairs:
        assert paging.paged_headroom_gangs_of(snaps, g, 16) == want[tuple(g)]
    assert len({w[0] for w in want.values()}) >= 3  # the gangs differ in their answers
    assert sum(own[k] != want[k] for k in want) >= 5 and sum(own[k] == want[k] for k in want) >= 5  # ... and in the page that decides
    gangs = [pairs[(7 * k) % len(pairs)] for k in range(2050)]
    engs = _engines(snaps)
    try:
        got = launch_all(engs, gangs, 16)
    finally:
        _close(engs)
    for k, g in enumerate(gangs):
        assert got[k] == want[tuple(g)], f"gang {k} {g}"


# ---- the search, with the deciding amount on page 1 and page 0 unbounded ----------------------------------------------------
ANSWERS = [0, 1, 63, 64, 65, 4095, 4096, 4097]
WALKED_CAPS = [1, 63, 64, 65, 4095, 4096, 4097]


def _by_hand(H, cap, on_equal):
    """Two members asking 1 each of a name against a threshold of 2 H + 1, nothing used or reserved: the member that meets r
    reserved passes iff r + 1 <= 2 H + 1 (on_equal: <), so copies 0 .. H - 1 pass whole; in copy H the second member is stopped
    (r = 2 H + 1), with on_equal the first one already (r + 1 = 2 H + 1)."""
    return (cap, -1, -1) if H >= cap else (H, 0, 0 if on_equal else 1)


def _searched(H):
    return PPR.pages_of([[{0: 7}, {0: 7}], [{0: 1}, {0: 1}]], [{}, {0: 2 * H + 1}], [P, P])


@pytest.mark.parametrize("H", ANSWERS)
def test_the_search_at_the_edges_of_its_rounds(H, oracle_mod):
    snaps = _searched(H)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            for cap in WALKED_CAPS + [MAXCAP]:
                got, = launch_all(engs, [[0, 1]], cap, on_equal)
                assert got == _by_hand(H, cap, on_equal), f"H={H} cap={cap} on_equal={on_equal}"
                assert got == paging.paged_headroom_gangs_of(snaps, [0, 1], cap, on_equal)
            for cap in (c for c in WALKED_CAPS if c in (1, H - 1, H, H + 1, 4097)):  # the walk: at the cap, around the answer
                assert _by_hand(H, cap, on_equal) == by_identity_3(snaps, oracle_mod, [0, 1], cap, on_equal), f"H={H} cap={cap}"
    finally:
        _close(engs)


@pytest.mark.parametrize("H", [MAXCAP - 1, MAXCAP, MAXCAP + 1, 1 << 40])
def test_the_search_next_to_the_largest_cap(H):
    """The answer next to, at and beyond cap = 2^31 - 1 (by hand: see _by_hand)."""
    snaps = _searched(H)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            got, = launch_all(engs, [[0, 1]], MAXCAP, on_equal)
            assert got == _by_hand(H, MAXCAP, on_equal) == paging.paged_headroom_gangs_of(snaps, [0, 1], MAXCAP, on_equal)
    finally:
        _close(engs)


@pytest.mark.parametrize("amounts", [(2 * 5000 + 1, 2 * 40 + 1), (2 * 40 + 1, 2 * 5000 + 1)])
def test_the_running_minimum_across_the_pages_of_one_throttle(amounts, oracle_mod):
    """A page-0 amount at 5000 (three rounds) then a page-1 amount of the SAME throttle at 40 (one round below the running
    minimum); the other way round page 1 passes at the running minimum and costs one walk."""
    snaps = PPR.pages_of([[{0: 1}, {0: 1}], [{0: 1}, {0: 1}]], [{0: amounts[0]}, {0: amounts[1]}], [P, P])
    got, = held_to_everything(snaps, oracle_mod, [[0, 1]], 6000)
    assert got == (40, 0, 1)
    got, = held_to_everything(snaps, oracle_mod, [[0, 1]], MAXCAP, walk=False)
    assert got == (40, 0, 1)


@pytest.mark.parametrize("lower_row_on", [0, 1])
def test_two_throttles_whose_deciding_amounts_sit_on_different_pages(lower_row_on, oracle_mod):
    """Row 0 names its amount (at 5000) on one page, row 1 (at 40) on the other: row 1 is limiting either way."""
    snaps = PPR.pages_of([[{0: 1}, {0: 1}], [{0: 1}, {0: 1}]], [{}, {}], [P, P], T=2, row=1)
    for k, snap in enumerate(snaps):
        snap.thr_spec.set_row(0, {0: 2 * 5000 + 1} if k == lower_row_on else {}, None)
        snap.thr_spec.set_row(1, {0: 2 * 40 + 1} if k != lower_row_on else {}, None)
    got, = held_to_everything(snaps, oracle_mod, [[0, 1]], 6000)
    assert got == (40, 1, 1)
    got, = held_to_everything(snaps, oracle_mod, [[0, 1]], MAXCAP, walk=False)
    assert got == (40, 1, 1)


# ---- the range cut per page --------------------------------------------------------------------------------------------------
BIG = 1 << 59


def test_large_requests_on_a_named_amount_of_page_one(oracle_mod):
    """Three members asking 2^59 each of a page-1 name against 2^62 = 8 x 2^59: the member that meets r x 2^59 reserved passes iff
    r + 1 <= 8 (on_equal: <).  Copies 0 and 1 pass; in copy 2 (r = 6, 7, 8) the third member is stopped, with on_equal the
    second.  Against a threshold at int64's end (16 x 2^59 - 1) copies 0 .. 4 pass and the candidates end at copy 5."""
    snaps = PPR.pages_of([[{0: 1}] * 3, [{1: BIG}] * 3], [{}, {1: 8 * BIG}], [P] * 3, D=2)
    for cap, walk in ((2, True), (MAXCAP, False)):
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], cap, False, walk)[0] == ((2, 0, 2) if cap > 2 else (2, -1, -1))
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], cap, True, walk)[0] == ((2, 0, 1) if cap > 2 else (2, -1, -1))
    snaps = PPR.pages_of([[{0: 1}] * 3, [{1: BIG}] * 3], [{}, {1: (1 << 63) - 1}], [P] * 3, D=2)
    for on_equal in (False, True):
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], MAXCAP, on_equal, walk=False)[0] == (5, 0, 0)


def test_large_requests_on_a_page_one_name_the_threshold_does_not_name(oracle_mod):
    """The threshold of page 1 names name 0 alone: nothing of name 1 is compared or multiplied, every copy passes."""
    snaps = PPR.pages_of([[{0: 1}] * 3, [{1: BIG}] * 3], [{}, {0: 7}], [P] * 3, D=2)
    assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], 4)[0] == (4, -1, -1)  # the walk: 12 x 2^59 stays inside int64
    for on_equal in (False, True):
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], MAXCAP, on_equal, walk=False)[0] == (MAXCAP, -1, -1)


# ---- presence on a later page ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster", [False, True])
def test_a_name_the_gang_brings_in_on_page_one(cluster, oracle_mod):
    """Name 0 of page 1 is neither used nor reserved: the first member of copy 0 meets no step 3, everyone behind it does.
    2 + 2 per copy against 4: copy 0 fills the threshold exactly and passes; the first member of copy 1 meets reserved =
    threshold.  With on_equal step 4 stops the second member of copy 0 already."""
    snaps = PPR.pages_of([[{0: 1}, {0: 1}], [{0: 2}, {0: 2}]], [{}, {0: 4}], [P, P], cluster=cluster)
    got = {eq: held_to_everything(snaps, oracle_mod, [[0, 1]], CAP, eq)[0] for eq in (False, True)}
    assert got[False] == (1, 0, 0) and got[True] == (0, 0, 1)
    alone = {eq: held_to_everything(snaps, oracle_mod, [[0]], CAP, eq)[0] for eq in (False, True)}
    assert alone[False] == (2, 0, 0) and alone[True] == (1, 0, 0)


@pytest.mark.parametrize("cluster", [False, True])
def test_a_member_that_carries_a_page_one_name_with_value_zero(cluster, oracle_mod):
    """The first member carries name 0 of page 1 with value 0: no request (it passes every step), but its Reserve makes the name
    present there."""
    snaps = PPR.pages_of([[{0: 1}, {0: 1}], [{0: 0, 1: 1}, {0: 5}]], [{}, {0: 5, 1: 100}], [P, P], D=2, cluster=cluster)
    for members in ([0, 1], [1, 0]):
        for on_equal in (False, True):
            held_to_everything(snaps, oracle_mod, [members], CAP, on_equal)
    assert held_to_everything(snaps, oracle_mod, [[0, 1]], CAP)[0] == (1, 0, 1)


# ---- the blocker as the minimum over pages -----------------------------------------------------------------------------------
# asks 1, 1, 5 against 13: copy 0 passes (7); in copy 1 the members meet 7, 8, 9 reserved and the third is stopped (9 + 5 > 13).
# asks 2, 2, 1 against 8: copy 0 passes (5); in copy 1 the members meet 5, 7 and the second is stopped (7 + 2 > 8).
STOPS_THIRD, STOPS_SECOND = ([{0: 1}, {0: 1}, {0: 5}], {0: 13}), ([{0: 2}, {0: 2}, {0: 1}], {0: 8})


@pytest.mark.parametrize("order", [(STOPS_THIRD, STOPS_SECOND), (STOPS_SECOND, STOPS_THIRD)])
def test_the_blocker_is_the_minimum_over_the_pages(order, oracle_mod):
    """At the same copy one page stops member 2 and the other member 1 of the same throttle: the blocker is member 1."""
    snaps = PPR.pages_of([order[0][0], order[1][0]], [order[0][1], order[1][1]], [P] * 3)
    for on_equal in (False, True):
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], CAP, on_equal)[0] == (1, 0, 1)


@pytest.mark.parametrize("row_of_second,want", [(1, (1, 1, 1)), (0, (1, 0, 1))])
def test_two_throttles_with_the_same_copies_stop_different_members_on_different_pages(row_of_second, want, oracle_mod):
    """Page 0 stops member 2 through one row, page 1 member 1 through the other, both in copy 1: the lower (first, t) wins —
    the earlier member, whichever row stops it."""
    snaps = PPR.pages_of([STOPS_THIRD[0], STOPS_SECOND[0]], [{}, {}], [P] * 3, T=2, row=1)
    snaps[0].thr_spec.set_row(0, {}, None), snaps[1].thr_spec.set_row(0, {}, None)
    snaps[0].thr_spec.set_row(1 - row_of_second, STOPS_THIRD[1], None)
    snaps[1].thr_spec.set_row(row_of_second, STOPS_SECOND[1], None)
    for on_equal in (False, True):
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], CAP, on_equal)[0] == want


@pytest.mark.parametrize("paged", [False, True])
def test_a_tie_between_rows_the_list_does_not_hold_in_order(paged, oracle_mod):
    """Rows 3 and 17 stop the same member of the same copy.  The affected-throttle list is filled round by round over the lanes
    (16 rows per lane): it holds rows 0, 17, 3 in that order — the limiting row is still the lowest, 3.  On one engine, and
    with row 17 deciding on page 0 and row 3 on page 1."""
    T = 20
    snaps = PPR.pages_of([STOPS_SECOND[0], STOPS_SECOND[0]], [{}, {}], [P] * 3, T=T, row=17)
    for k, snap in enumerate(snaps):
        snap.thr_ns[3] = 0
        snap.thr_spec.set_row(3, STOPS_SECOND[1] if k == 1 else {}, None)
        snap.thr_spec.set_row(17, STOPS_SECOND[1] if k == 0 else {}, None)
    if not paged:
        snaps = [snaps[0]]
        snaps[0].thr_spec.set_row(3, STOPS_SECOND[1], None)
    assert paging.affected_throttles(snaps[0], 0)[1] == [0, 3, 17]
    for on_equal in (False, True):
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], CAP, on_equal)[0] == (1, 3, 1)
    if not paged:  # ... and the single-engine call, byte for byte
        eng = E.Engine.for_snapshot(snaps[0])
        try:
            single = eng.headroom_gangs([0, 1, 2], [0, 3], cap=CAP)
            assert (int(single[0][0]), int(single[1][0]), int(single[2][0])) == (1, 3, 1)
            assert _same_bytes(E.paged_headroom_gangs([eng], [0, 1, 2], [0, 3], CAP), single)
        finally:
            eng.close()


# ---- the count, a page that is skipped ---------------------------------------------------------------------------------------
def test_the_count_is_judged_once(oracle_mod):
    """A pod-count threshold alone with names on two pages under no threshold: the answer of the one-page count case."""
    H = 3
    snaps = PPR.pages_of([[{0: 1}] * 2, [{0: 2}] * 2], [{}, {}], [P, P], counts=[2 * H + 1, 2 * H + 1])
    for on_equal in (False, True):
        assert held_to_everything(snaps, oracle_mod, [[0, 1]], CAP, on_equal)[0] == _by_hand(H, CAP, on_equal)
        assert held_to_everything(snaps, oracle_mod, [[0, 1]], MAXCAP, on_equal, walk=False)[0] == _by_hand(H, MAXCAP, on_equal)


@pytest.mark.parametrize("last,want", [(8, (1, 0, 1)), (100, (1, 0, 2))])
def test_a_page_that_is_skipped(last, want, oracle_mod):
    """A middle page none of whose names any member requests (its threshold of 0 would stop whoever asked) between two pages that
    decide."""
    snaps = PPR.pages_of([STOPS_THIRD[0], [{}, {}, {}], STOPS_SECOND[0]], [STOPS_THIRD[1], {0: 0}, {0: last}], [P] * 3)
    for on_equal in (False, True):
        assert held_to_everything(snaps, oracle_mod, [[0, 1, 2]], CAP, on_equal)[0] == want


# ---- refusals and what the call leaves pending -------------------------------------------------------------------------------
def test_refusals_and_the_slots_of_page_zero(oracle_mod):
    snaps = PPR.pages_of([[{0: 1}, {0: 1}], [{0: 1}, {0: 1}]], [{0: 2 * 5 + 1}, {0: 2 * 3 + 1}], [P, P])
    members, want = [0, 1], (3, 0, 1)
    rows, off = np.array(members, np.int64), np.array([0, 2], np.int64)
    engs = _engines(snaps)
    other_T = E.Engine.for_snapshot(PR.tiny([{0: 1}, {0: 1}], {0: 7}, flags=[P, P], T=2, row=1))
    neg = E.Engine.for_snapshot(PR.tiny([{0: 1}, {0: -1}], {0: 5}, flags=[P, P]))
    wide = E.Engine.for_snapshot(snaps[1])
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    hg = lambda r, o, cap=CAP, pages=None: E.paged_headroom_gangs(pages or engs, r, o, cap)
    try:
        res_before = [e.fetch_reserved() for e in engs]

        def raw(n=2, r=rows, ng=1, o=off, cap=CAP):
            ptr = lambda a: None if a is None else a.ctypes.data
            return L.kt_paged_headroom_gangs(hs, 2, n, ptr(r), ng, ptr(o), 0, cap, None, None, None)

        def every_refusal():
            assert raw(n=-1) == -1 and raw(ng=-1) == -1 and raw(r=None) == -1
            # every gang_off defect kt_admit_gangs_launch refuses
            assert raw(o=None) == -1
            assert _code(lambda: hg(members, [1, 2])) == -1     # gang_off[0] != 0
            assert _code(lambda: hg(members, [0, 0, 2])) == -1  # an empty gang
            assert _code(lambda: hg(members, [0, 2, 1])) == -1  # descending
            assert _code(lambda: hg(members, [0, 1])) == -1     # gang_off[n_gangs] != n
            assert _code(lambda: hg(members, [0, 3])) == -1
            assert raw(ng=0) == -1                              # no gangs for a queue of 2
            assert _code(lambda: hg([], [0, 0])) == -1          # n == 0 with n_gangs == 1
            assert _code(lambda: hg([0, 1, 0], [0, 3])) == -1   # a pod twice within ONE gang
            assert _code(lambda: hg([0, 99], [0, 2])) == -2     # a pod row outside a page's capacity
            assert _code(lambda: hg([-1], [0, 1])) == -2
            for cap in (0, -3, 1 << 31):
                assert _code(lambda: hg(members, [0, 2], cap)) == -1, cap
            # the page set
            assert _code(lambda: hg(members, [0, 2], pages=[engs[0], other_T])) == -1  # different throttle-row counts
            assert _code(lambda: hg(members, [0, 2], pages=[engs[0], engs[0]])) == -1  # an engine named twice
            # per page: a negative request fed to page 1 only, sums in two blocks on page 1 only
            assert _code(lambda: hg([0], [0, 1], pages=[engs[0], neg])) == -7          # KT_ERR_UNSUPPORTED
            msg = L.kt_last_error(neg._h).decode()
            assert "negative" in msg and "page 1" in msg
            assert _code(lambda: hg(members, [0, 2], pages=[engs[0], wide])) == -7
            assert "page 1" in L.kt_last_error(wide._h).decode()

        wide.set_wide_sums(1)
        wide.reconcile(PR.NOW, apply=False)
        every_refusal()
        # a refused call touches no slot of page 0: a pending check and a pending gang headroom result are still fetchable
        engs[0].check_launch(2, rows)
        every_refusal()
        engs[0].check_fetch(2)
        engs[0].headroom_gangs_launch(members, [0, 2], cap=CAP)
        every_refusal()
        single = engs[0].headroom_gangs_fetch(1)
        assert (int(single[0][0]), int(single[1][0]), int(single[2][0])) == paging.headroom_gangs_of(snaps[0], members, CAP)
        # a pod may be in several gangs
        assert launch_all(engs, [[0, 1], [1, 0], [0]], CAP) == [want, want, paging.paged_headroom_gangs_of(snaps, [0], CAP)]
        # the results have been handed out: no headroom result of either kind is pending on page 0
        assert _code(lambda: engs[0].headroom_fetch(1)) == -5 and _code(lambda: engs[0].headroom_gangs_fetch(1)) == -5
        # ... whatever was pending before
        engs[0].headroom_gangs_launch(members, [0, 2], cap=CAP)
        assert launch_all(engs, [members], CAP) == [want]
        assert _code(lambda: engs[0].headroom_gangs_fetch(1)) == -5
        engs[0].headroom_launch(2, rows, cap=CAP)
        assert launch_all(engs, [members], CAP) == [want]
        assert _code(lambda: engs[0].headroom_fetch(2)) == -5
        # a pending kt_check_launch of page 0 is gone; page 1's is not touched
        engs[0].check_launch(2, rows)
        engs[1].check_launch(2, rows)
        assert launch_all(engs, [members], CAP) == [want]
        assert _code(lambda: engs[0].check_fetch(2)) == -5
        engs[1].check_fetch(2)
        # nullable outputs
        copies, none, nothing = E.paged_headroom_gangs(engs, members, [0, 2], CAP, want_limiting=False, want_blocker=False)
        assert none is None and nothing is None and int(copies[0]) == want[0]
        assert raw() == 0
        # n == 0 with n_gangs == 0: KT_OK, nothing launched
        assert [x.tolist() for x in E.paged_headroom_gangs(engs, [], [0], CAP)] == [[], [], []]
        assert raw(n=0, r=None, ng=0, o=None) == 0
        # a dry run: the reserved amounts of no page have changed
        for before, e in zip(res_before, engs):
            after = e.fetch_reserved()
            for f in ("v", "present", "count", "has_count"):
                assert getattr(before, f).tobytes() == getattr(after, f).tobytes()
        assert launch_all(engs, [members], CAP) == [want]
    finally:
        _close(engs + [other_T, neg, wide])


def test_matrix_bytes_beyond_two_gib_are_refused():
    """n x throttle_rows > 2^31: pod 0, valid, as so many gangs of one — nothing but the matrix rule can answer -2."""
    T = 1030
    engs = _engines(PPR.pages_of([[{0: 3}], [{0: 3}]], [{0: 20}, {0: 20}], [P], T=T, row=T - 1))
    try:
        big = 2**31 // T + 1
        assert _code(lambda: E.paged_headroom_gangs(engs, np.zeros(big, np.int64), np.arange(big + 1), 4)) == -2
        assert "throttle_rows" in E.lib().kt_last_error(engs[0]._h).decode()
    finally:
        _close(engs)
