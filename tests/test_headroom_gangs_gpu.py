"""The gang headroom on the GPU: Engine.headroom_gangs (kt_headroom_gangs_launch / kt_headroom_gangs_fetch,
csrc/kt_kernels_headroom_gangs.hip) against the walk of tests/headroom_gangs_reference.py (the C oracle's admit of
``members * cap``) and ``paging.headroom_gangs_of`` — copies, limiting throttle and blocker compared bit for bit, for both
on_equal.  The shapes are the smallest at which the kernel can still go wrong: one case per DT instantiation (D = 1, 8, 16), a
gang beyond one member block, a deciding throttle in the second chunk of the affected-throttle list, more gangs than the grid
has workgroups, the 64-ary search at the edges of its rounds and at cap = 2^31 - 1 (expectations derived by hand: a walk of 2^31
copies is not a reference), presence, values next to int64's end, ties between throttles, refusals and the check slot."""
import copy

import numpy as np
import pytest

import preempt_reference as PR
from headroom_gangs_reference import headroom_gangs_by_oracle
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_headroom_gangs_cpu import CAP, SEEDS, gangs_case

pytestmark = pytest.mark.gpu
MAXCAP = E.HEADROOM_MAX_CAP
P = PR.PENDING


def _queue(gangs):
    rows = [int(p) for g in gangs for p in g]
    off = np.cumsum([0] + [len(g) for g in gangs]).astype(np.int64)
    return rows, off


def launch_all(eng, gangs, cap, on_equal=False):
    """All gangs in ONE launch -> per gang (copies, limiting, blocker as a position inside the gang)."""
    rows, off = _queue(gangs)
    copies, limiting, blocker = eng.headroom_gangs(rows, off, cap=cap, on_equal=on_equal)
    assert copies.dtype == np.int64 and limiting.dtype == np.int32 and blocker.dtype == np.int64
    assert copies.shape == limiting.shape == blocker.shape == (len(gangs),)
    out = []
    for g in range(len(gangs)):
        b = int(blocker[g])
        assert b == -1 or off[g] <= b < off[g + 1], (g, b)
        out.append((int(copies[g]), int(limiting[g]), b if b < 0 else b - int(off[g])))
    return out


def held_to_everything(snap, oracle_mod, gangs, cap, on_equal=False, walk=True):
    """The engine against paging.headroom_gangs_of and (``walk``) against the oracle's admission of members * cap."""
    eng = E.Engine.for_snapshot(snap)
    try:
        got = launch_all(eng, gangs, cap, on_equal)
    finally:
        eng.close()
    o = oracle_mod.Oracle(snap) if walk else None
    for g, members in enumerate(gangs):
        assert got[g] == paging.headroom_gangs_of(snap, members, cap, on_equal), f"gang {g} {members} cap={cap} on_equal={on_equal}"
        if walk:
            ref = headroom_gangs_by_oracle(o, members, cap, on_equal)
            assert got[g] == ref, f"gang {g} {members} cap={cap} on_equal={on_equal}: {got[g]} != {ref}"
    return got


# ---- the generated clusters of the CPU pin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS[:10])
def test_generated_clusters(seed, oracle_mod):
    cs, page, gangs, want = gangs_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(page.snapshot)
    try:
        for on_equal in (False, True):
            assert launch_all(eng, gangs, CAP, on_equal) == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        eng.close()


# ---- one case per instantiation, member blocks, list chunks, the grid -------------------------------------------------------
@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    """The deciding name is the last one; the others are requested and reserved but no threshold stops them.  3 + 4 per copy
    against 30 with 2 used: copies 0 .. 3 pass (2 + 28 = 30), on_equal stops the second member of copy 3."""
    d = D - 1
    other = {x: 2 for x in range(D) if x != d}
    a, b = dict(other), dict(other)
    a[d], b[d] = 3, 4
    snap = PR.tiny([a, b], {d: 30, **({0: 1000} if D > 1 else {})}, flags=[P, P], D=D)
    snap.thr_used.set_row(0, {d: 2}, 1)
    for on_equal in (False, True):
        got, = held_to_everything(snap, oracle_mod, [[0, 1]], CAP, on_equal)
        assert got == ((3, 0, 1) if on_equal else (4, 0, 0))


def test_seventy_members_an_error_member_in_the_second_block(oracle_mod):
    """The member ballot strides 64: the member whose namespace has no object sits at position 66; with a count threshold of
    50 member 50 is stopped in front of it, with 1000 the Error member is the blocker and nobody is limiting."""
    n = 70
    for count, want in ((50, (0, 0, 50)), (1000, (0, -1, 66))):
        snap = PR.tiny([{0: 1}] * n, {}, count=count, flags=[P] * n, pod_ns=[1 if i == 66 else 0 for i in range(n)])
        got, = held_to_everything(snap, oracle_mod, [list(range(n))], 3)
        assert got == want


def test_seventy_members_a_count_threshold(oracle_mod):
    n = 70
    snap = PR.tiny([{0: 1}] * n, {}, count=3 * n + 65, flags=[P] * n)
    got, = held_to_everything(snap, oracle_mod, [list(range(n))], 6)
    assert got == (3, 0, 65)


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect both members — more than one chunk of the LDS list holds; only the last row stops a copy."""
    T = 1030
    snap = PR.tiny([{0: 3}, {0: 3}], {0: 20}, flags=[P, P], T=T, row=T - 1)
    for t in range(T - 1):
        snap.thr_ns[t] = 0
        snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    assert len(paging.affected_throttles(snap, 0)[1]) == T
    got, = held_to_everything(snap, oracle_mod, [[0, 1]], 9)
    assert got == (3, T - 1, 0)  # 18 + 3 > 20


def test_more_gangs_than_the_grid_has_workgroups(oracle_mod):
    """2050 two-member gangs in one launch: the grid strides beyond 2048.  Pods are shared between the gangs."""
    asks = [1, 2, 3, 4, 5, 3]
    snap = PR.tiny([{0: a} for a in asks], {0: 40}, count=21, flags=[P] * 6)
    pairs = [[i, j] for i in range(6) for j in range(6) if i != j]
    o = oracle_mod.Oracle(snap)
    want = {tuple(g): headroom_gangs_by_oracle(o, g, 16, False) for g in pairs}
    for g in pairs:
        assert paging.headroom_gangs_of(snap, g, 16) == want[tuple(g)]
    assert len({w[0] for w in want.values()}) >= 3  # the gangs differ in their answers
    gangs = [pairs[(7 * k) % len(pairs)] for k in range(2050)]
    eng = E.Engine.for_snapshot(snap)
    try:
        got = launch_all(eng, gangs, 16)
    finally:
        eng.close()
    for k, g in enumerate(gangs):
        assert got[k] == want[tuple(g)], f"gang {k} {g}"


# ---- the search --------------------------------------------------------------------------------------------------------------
ANSWERS = [0, 1, 63, 64, 65, 4095, 4096, 4097]
WALKED_CAPS = [1, 63, 64, 65, 4095, 4096, 4097]


def _by_hand(H, cap, on_equal):
    """Two members against a pod-count threshold of 2 H + 1, nothing used or reserved: the member that meets r reserved pods
    passes iff r + 1 <= 2 H + 1 (on_equal: <), so copies 0 .. H - 1 pass whole; in copy H the second member is stopped (r =
    2 H + 1), with on_equal the first one already (r + 1 = 2 H + 1)."""
    return (cap, -1, -1) if H >= cap else (H, 0, 0 if on_equal else 1)


@pytest.mark.parametrize("H", ANSWERS)
def test_the_search_at_the_edges_of_its_rounds(H, oracle_mod):
    snap = PR.tiny([{0: 1}, {0: 1}], {}, count=2 * H + 1, flags=[P, P])
    o = oracle_mod.Oracle(snap)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            for cap in WALKED_CAPS + [MAXCAP]:
                got, = launch_all(eng, [[0, 1]], cap, on_equal)
                assert got == _by_hand(H, cap, on_equal), f"H={H} cap={cap} on_equal={on_equal}"
                assert got == paging.headroom_gangs_of(snap, [0, 1], cap, on_equal)
            for cap in (c for c in WALKED_CAPS if c in (1, H - 1, H, H + 1, 4097)):  # the walk: at the cap, around the answer
                assert _by_hand(H, cap, on_equal) == headroom_gangs_by_oracle(o, [0, 1], cap, on_equal), f"H={H} cap={cap}"
    finally:
        eng.close()


@pytest.mark.parametrize("H", [MAXCAP - 1, MAXCAP, MAXCAP + 1, 1 << 40])
def test_the_search_next_to_the_largest_cap(H):
    """The answer next to, at and beyond cap = 2^31 - 1 (by hand: see _by_hand)."""
    snap = PR.tiny([{0: 1}, {0: 1}], {}, count=2 * H + 1, flags=[P, P])
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            got, = launch_all(eng, [[0, 1]], MAXCAP, on_equal)
            assert got == _by_hand(H, MAXCAP, on_equal) == paging.headroom_gangs_of(snap, [0, 1], MAXCAP, on_equal)
    finally:
        eng.close()


def _two_rows(count0, count1):
    """Two throttle rows that both affect the two members, each with a pod-count threshold of its own."""
    snap = PR.tiny([{0: 1}, {0: 1}], {}, count=count1, flags=[P, P], T=2, row=1)
    snap.thr_spec.set_row(0, {}, count0)
    return snap


@pytest.mark.parametrize("counts,want", [((2 * 5000 + 1, 2 * 40 + 1), (40, 1, 1)), ((2 * 40 + 1, 2 * 5000 + 1), (40, 0, 1)),
                                         ((2 * 5000 + 1, 2 * 64 + 1), (64, 1, 1)), ((2 * 70, 2 * 3), (3, 1, 0))])
def test_a_second_throttle_narrows_the_running_minimum(counts, want, oracle_mod):
    """Behind a first throttle at 5000 (three rounds) the second one decides below 64 (one round); the other way round the
    second passes at the running minimum and costs one walk."""
    snap = _two_rows(*counts)
    got, = held_to_everything(snap, oracle_mod, [[0, 1]], 6000)
    assert got == want
    got, = held_to_everything(snap, oracle_mod, [[0, 1]], MAXCAP, walk=False)
    assert got == want


# ---- presence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster", [False, True])
def test_a_name_the_gang_brings_in(cluster, oracle_mod):
    """Name 0 is neither used nor reserved: the first member of copy 0 meets no step 3, everyone behind it does (the name is
    present from then on).  2 + 2 per copy against 4: copy 0 fills the threshold exactly and passes; the first member of copy 1
    meets reserved = threshold — a Throttle's step 3 stops it as `active`, a ClusterThrottle's step 4 as `insufficient`.  With
    on_equal step 4 stops the second member of copy 0 already."""
    snap = PR.tiny([{0: 2}, {0: 2}], {0: 4}, flags=[P, P], cluster=cluster)
    got = {eq: held_to_everything(snap, oracle_mod, [[0, 1]], CAP, eq)[0] for eq in (False, True)}
    assert got[False] == (1, 0, 0) and got[True] == (0, 0, 1)
    alone = {eq: held_to_everything(snap, oracle_mod, [[0]], CAP, eq)[0] for eq in (False, True)}
    assert alone[False] == (2, 0, 0) and alone[True] == (1, 0, 0)


@pytest.mark.parametrize("cluster", [False, True])
def test_a_member_that_carries_a_name_with_value_zero(cluster, oracle_mod):
    """The first member carries name 0 with value 0: no request (it passes every step), but its Reserve makes the name present."""
    snap = PR.tiny([{0: 0, 1: 1}, {0: 5}], {0: 5, 1: 100}, flags=[P, P], cluster=cluster)
    for members in ([0, 1], [1, 0]):
        for on_equal in (False, True):
            held_to_everything(snap, oracle_mod, [members], CAP, on_equal)
    assert held_to_everything(snap, oracle_mod, [[0, 1]], CAP)[0] == (1, 0, 1)


# ---- values next to int64's end ----------------------------------------------------------------------------------------------
BIG = 1 << 59


def test_large_requests_on_a_name_the_threshold_does_not_name(oracle_mod):
    """3 x 2^59 per copy on name 1; the threshold names name 0 alone: nothing of name 1 is compared, every copy passes."""
    snap = PR.tiny([{1: BIG}] * 3, {0: 7}, flags=[P] * 3)
    assert held_to_everything(snap, oracle_mod, [[0, 1, 2]], 4)[0] == (4, -1, -1)  # the walk: 12 x 2^59 stays inside int64
    for on_equal in (False, True):
        assert held_to_everything(snap, oracle_mod, [[0, 1, 2]], MAXCAP, on_equal, walk=False)[0] == (MAXCAP, -1, -1)


def test_large_requests_on_a_named_amount(oracle_mod):
    """The same requests against 2^62 = 8 x 2^59 on name 1: the member that meets r x 2^59 reserved passes iff r + 1 <= 8
    (on_equal: <).  Copies 0 and 1 pass; in copy 2 (r = 6, 7, 8) the third member is stopped, with on_equal the second."""
    snap = PR.tiny([{1: BIG}] * 3, {1: 8 * BIG}, flags=[P] * 3)
    for cap, walk in ((2, True), (MAXCAP, False)):
        assert held_to_everything(snap, oracle_mod, [[0, 1, 2]], cap, False, walk)[0] == ((2, 0, 2) if cap > 2 else (2, -1, -1))
        assert held_to_everything(snap, oracle_mod, [[0, 1, 2]], cap, True, walk)[0] == ((2, 0, 1) if cap > 2 else (2, -1, -1))
    snap = PR.tiny([{1: BIG}] * 3, {1: (1 << 63) - 1}, flags=[P] * 3)  # a threshold at int64's end: 16 x 2^59 - 1
    for on_equal in (False, True):
        assert held_to_everything(snap, oracle_mod, [[0, 1, 2]], MAXCAP, on_equal, walk=False)[0] == (5, 0, 0)


# ---- blocker and limiting ----------------------------------------------------------------------------------------------------
def _two_namespaces():
    """Row 0: a Throttle of namespace 0 on name 0; row 1: a Throttle of namespace 2 on name 1.  Pod 0 lives in namespace 0,
    pod 1 in namespace 2, pod 2 in namespace 1 (no Namespace object: its PreFilter is an Error), pod 3 in namespace 0 asking
    more than the threshold."""
    snap = PR.tiny([{0: 3}, {1: 3}, {0: 1}, {0: 9}], {1: 5}, flags=[P] * 4, T=2, row=1, pod_ns=[0, 2, 1, 0])
    snap.thr_ns[1] = 2
    snap.thr_spec.set_row(0, {0: 5}, None)
    return snap


def test_two_throttles_with_the_same_copies_stop_different_members(oracle_mod):
    snap = _two_namespaces()
    for on_equal in (False, True):
        assert held_to_everything(snap, oracle_mod, [[0, 1]], CAP, on_equal)[0] == (1, 0, 0)
        assert held_to_everything(snap, oracle_mod, [[1, 0]], CAP, on_equal)[0] == (1, 1, 0)  # the order of the members decides


def test_an_error_member_behind_a_member_a_throttle_stops(oracle_mod):
    snap = _two_namespaces()
    assert held_to_everything(snap, oracle_mod, [[0, 3, 2]], CAP)[0] == (0, 0, 1)   # 9 > 5: pod 3 is stopped in front of the Error
    assert held_to_everything(snap, oracle_mod, [[0, 2, 3]], CAP)[0] == (0, -1, 1)  # the Error member comes first
    assert held_to_everything(snap, oracle_mod, [[2]], CAP)[0] == (0, -1, 0)
    snap.pod_flags[1] = 0                                                           # an invalid row
    assert held_to_everything(snap, oracle_mod, [[0, 1]], CAP, walk=False)[0] == (0, -1, 1)


def test_a_gang_no_throttle_affects(oracle_mod):
    snap = PR.tiny([{0: 3}, {0: 3}], {0: 1}, flags=[P, P], pod_ns=[2, 2])
    snap.thr_ns[0] = 0
    assert held_to_everything(snap, oracle_mod, [[0, 1]], 7)[0] == (7, -1, -1)


# ---- a gang of one is the plain headroom -------------------------------------------------------------------------------------
def test_a_gang_of_one_is_kt_headroom_on_its_directed_shapes(oracle_mod):
    from test_headroom_gpu import DIRECTED, _cluster
    from test_paged_admit_cpu import write_status
    for case in sorted(DIRECTED):
        for kind in ("Throttle", "ClusterThrottle"):
            threshold, pods = DIRECTED[case]
            cs = _cluster(kind, copy.deepcopy(threshold), copy.deepcopy(pods))
            write_status(cs, oracle_mod)
            pages = cs.build_pages()
            n = len(cs.pods)
            eng = E.Engine.for_snapshot(pages[0].snapshot)
            try:
                for on_equal in (False, True):
                    for cap in (CAP, MAXCAP):
                        copies, limiting = eng.headroom(np.arange(n), cap=cap, on_equal=on_equal)
                        gcopies, glimiting, gblocker = eng.headroom_gangs(np.arange(n), np.arange(n + 1), cap=cap, on_equal=on_equal)
                        assert gcopies.tobytes() == copies.tobytes() and glimiting.tobytes() == limiting.tobytes(), f"{case} {kind} {on_equal}"
                        assert gblocker.tolist() == [-1 if c == cap else i for i, c in enumerate(copies)]
            finally:
                eng.close()


# ---- refusals and the check slot ---------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def test_refusals_and_the_check_slot(oracle_mod):
    snap = _two_rows(2 * 5 + 1, 2 * 3 + 1)
    members = [0, 1]
    want = (3, 1, 1)
    eng = E.Engine.for_snapshot(snap)
    neg = E.Engine.for_snapshot(PR.tiny([{0: 1}, {0: -1}], {0: 5}, flags=[P, P]))
    L = E.lib()
    rows, off = np.array(members, np.int64), np.array([0, 2], np.int64)
    hg = lambda r, o, cap=CAP: eng.headroom_gangs(r, o, cap=cap)
    try:
        assert _code(lambda: eng.headroom_gangs_fetch(1)) == -5  # KT_ERR_NOT_READY: no launch yet
        res_before = eng.fetch_reserved()
        status_before = [eng.check(rows=rows, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = [x.copy() for eq in (False, True) for x in eng.headroom(rows, cap=MAXCAP, on_equal=eq)]

        def raw(n=2, r=rows, ng=1, o=off, cap=CAP):
            ptr = lambda a: None if a is None else a.ctypes.data
            return L.kt_headroom_gangs_launch(eng._h, n, ptr(r), ng, ptr(o), 0, cap, None)

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
            assert _code(lambda: hg([0, 99], [0, 2])) == -2     # a pod row outside the capacity
            assert _code(lambda: hg([-1], [0, 1])) == -2
            for cap in (0, -3, 1 << 31):
                assert _code(lambda: hg(members, [0, 2], cap)) == -1, cap

        every_refusal()
        wide = E.Engine.for_snapshot(snap)
        try:  # sums in two blocks, as kt_headroom_launch refuses them
            wide.set_wide_sums(1)
            wide.reconcile(PR.NOW, apply=False)
            assert _code(lambda: wide.headroom_gangs(members, [0, 2], cap=CAP)) == -7  # KT_ERR_UNSUPPORTED
            assert _code(lambda: wide.headroom(rows, cap=CAP)) == -7
        finally:
            wide.close()
        assert _code(lambda: eng.headroom_gangs_fetch(1)) == -5  # a refused launch leaves nothing to fetch
        # an engine that has been fed ONE negative request: the search rests on monotonicity; the plain headroom serves it
        assert _code(lambda: neg.headroom_gangs([0], [0, 1], cap=CAP)) == -7
        assert "negative" in L.kt_last_error(neg._h).decode()
        assert neg.headroom([0, 1], cap=CAP)[0].shape == (2,)
        # a pod may be in several gangs
        assert launch_all(eng, [[0, 1], [1, 0], [0]], CAP) == [want, want, paging.headroom_gangs_of(snap, [0], CAP)]
        # the one pending headroom result is shared: the kind of the last launch decides which fetch may read it
        eng.headroom_gangs_launch(members, [0, 2], cap=CAP)
        assert _code(lambda: eng.headroom_fetch(1)) == -5
        got = eng.headroom_gangs_fetch(1)
        assert (int(got[0][0]), int(got[1][0]), int(got[2][0])) == want
        assert _code(lambda: eng.headroom_gangs_fetch(2)) == -2  # more gangs than the launch had
        eng.headroom_launch(2, rows, cap=CAP)
        assert _code(lambda: eng.headroom_gangs_fetch(1)) == -5
        assert eng.headroom_fetch(2)[0].shape == (2,)
        # nullable outputs
        eng.headroom_gangs_launch(members, [0, 2], cap=CAP)
        copies, none, nothing = eng.headroom_gangs_fetch(1, want_limiting=False, want_blocker=False)
        assert none is None and nothing is None and int(copies[0]) == want[0]
        assert L.kt_headroom_gangs_fetch(eng._h, 1, None, None, None) == 0
        # n == 0 with n_gangs == 0: KT_OK, nothing launched
        eng.headroom_gangs_launch([], [0], cap=CAP)
        assert eng.headroom_gangs_fetch(0)[0].tolist() == []
        assert _code(lambda: eng.headroom_fetch(0)) == -5
        # the check slot: the launch drops a pending check, a later user of the slot drops the launch
        eng.check_launch(2, rows)
        eng.headroom_gangs_launch(members, [0, 2], cap=CAP)
        assert _code(lambda: eng.check_fetch(2)) == -5
        eng.check_launch(2, rows, want_status=True)
        assert _code(lambda: eng.headroom_gangs_fetch(1)) == -5
        eng.check_fetch(2, True)
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        res_after = eng.fetch_reserved()
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
        status_after = [eng.check(rows=rows, on_equal=eq)[0] for eq in (False, True)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(status_before, status_after))
        room_after = [x for eq in (False, True) for x in eng.headroom(rows, cap=MAXCAP, on_equal=eq)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, room_after))
    finally:
        eng.close()
        neg.close()


def test_matrix_bytes_beyond_two_gib_are_refused():
    """n x throttle_rows > 2^31: pod 0, valid, as so many gangs of one — nothing but the matrix rule can answer -2."""
    T = 1030
    eng = E.Engine.for_snapshot(PR.tiny([{0: 3}], {0: 20}, flags=[P], T=T, row=T - 1))
    try:
        big = 2**31 // T + 1
        assert _code(lambda: eng.headroom_gangs(np.zeros(big, np.int64), np.arange(big + 1), cap=4)) == -2
        assert "throttle_rows" in E.lib().kt_last_error(eng._h).decode()
    finally:
        eng.close()
