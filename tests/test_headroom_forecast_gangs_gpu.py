"""The gang headroom forecast on the GPU: Engine.headroom_forecast_gangs (kt_headroom_forecast_gangs_launch /
kt_headroom_forecast_gangs_fetch, csrc/kt_kernels_headroom_forecast_gangs.hip) against the reference of
tests/headroom_forecast_gangs_reference.py (per instant: a copy of the snapshot, the oracle's reconcile, the oracle's admit of
members * cap) and ``paging.headroom_forecast_gangs_of``; first, copies, limiting and blocker compared bit for bit.  The shapes
are the smallest at which the kernel can still go wrong: instant blocks of 64 with the per-position triple and the ballot across
them, lanes of one block whose searches end at different depths, the largest cap with the lane-own mask of A_t and the int64
cut-off, deciding throttles in the second chunk of the affected-throttle list and in an order the list does not keep, one case
per DT instantiation (D = 1, 8, 16), a member ballot of two blocks, more gangs than the grid has workgroups."""
import os
import subprocess

import numpy as np
import pytest

import forecast_reference as FR
import headroom_forecast_gangs_reference as HG
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

pytestmark = pytest.mark.gpu
NOW = FR.NOW
CAP = HG.CAP
MAXCAP = E.HEADROOM_MAX_CAP
INT64_MAX = (1 << 63) - 1
P, C = PR.PENDING, PR.COUNTED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch(eng, gangs, inst, cap, want=1, on_equal=False):
    """All gangs in ONE launch -> (first [n_gangs], copies, limiting, blocker [n_gangs][m]) as lists."""
    rows, off = HG.queue_of(gangs)
    first, copies, limiting, blocker = eng.headroom_forecast_gangs(rows, off, inst, cap=cap, want=want, on_equal=on_equal)
    assert first.dtype == np.int64 and copies.dtype == np.int64 and limiting.dtype == np.int32 and blocker.dtype == np.int64
    assert first.shape == (len(gangs),) and copies.shape == limiting.shape == blocker.shape == (len(gangs), len(inst))
    for g in range(len(gangs)):
        assert all(b == -1 or off[g] <= b < off[g + 1] for b in blocker[g].tolist()), (g, blocker[g].tolist())
    return first.tolist(), copies.tolist(), limiting.tolist(), blocker.tolist()


def by_model(snap, gangs, inst, cap, want=1, on_equal=False):
    ctx = paging.preempt_context(snap, inst[0])
    _, off = HG.queue_of(gangs)
    out = [paging.headroom_forecast_gangs_of(snap, g, inst, cap, want, on_equal, ctx=ctx) for g in gangs]
    return ([r[0] for r in out], [r[1] for r in out], [r[2] for r in out],
            [[b + off[i] if b >= 0 else -1 for b in r[3]] for i, r in enumerate(out)])


def held_to_everything(snap, oracle_mod, gangs, inst, cap=16, want=1, on_equal=False, walk=True):
    """The engine against paging.headroom_forecast_gangs_of and (``walk``) against the oracle's reconcile and admission."""
    eng = E.Engine.for_snapshot(snap)
    try:
        got = launch(eng, gangs, inst, cap, want, on_equal)
    finally:
        eng.close()
    assert got == by_model(snap, gangs, inst, cap, want, on_equal), f"cap={cap} want={want} on_equal={on_equal}"
    if walk:
        ref = HG.expected(snap, oracle_mod, gangs, inst, cap, want, on_equal)
        assert got == tuple(ref), f"cap={cap} want={want} on_equal={on_equal}: {got} != {ref}"
    return got


# ---- the random cases of the CPU pin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(5))
def test_random_cases(part, oracle_mod):
    cases = HG.random_cases(oracle_mod)[part::5]
    assert cases
    for name, snap, gangs, inst, want in cases:
        _, off = HG.queue_of(gangs)
        eng = E.Engine.for_snapshot(snap)
        try:
            for on_equal in (False, True):
                first, copies, limiting, blocker = launch(eng, gangs, inst, CAP, 2, on_equal)
                for g, w in enumerate(want[on_equal]):
                    got = (first[g], copies[g], limiting[g], [b - off[g] if b >= 0 else -1 for b in blocker[g]])
                    assert got == w, f"{name} on_equal={on_equal} gang {gangs[g]}: {got} != {w}"
        finally:
            eng.close()


@pytest.mark.parametrize("name", sorted(HG.DIRECTED))
def test_directed(name, oracle_mod):
    """Among them: a zero-valued name that brings presence, an Error member and an invalid member with an earlier member stopped
    inside the window only, a gang no throttle affects, a stored-status throttle that binds at every instant."""
    snap, members, inst = HG.DIRECTED[name]()
    for on_equal in (False, True):
        held_to_everything(snap, oracle_mod, [members], inst, 16, 2, on_equal)


# ---- instant blocks --------------------------------------------------------------------------------------------------------
def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


@pytest.mark.parametrize("m,lo,hi", [(1, 0, 0), (1, None, None), (63, 62, 62), (64, 63, 63), (65, 64, 64), (65, 63, 64), (130, 64, 100),
                                     (130, 100, 128), (130, 128, 129), (130, 129, 129), (130, None, None), (130, 0, 129)])
def test_instant_blocks_the_triple_and_the_ballot(m, lo, hi, oracle_mod):
    """Rows 0 and 1 both select the two members; used 4, they ask 3 each.  Row 0's cpu 17 admits 2 copies throughout (4 + 12 <= 17)
    and stops the first member of the third.  Row 1's cpu 9 admits none: the second member is stopped by what the first reserved
    (4 + 3 + 3 > 9); its override 30 (4 copies) is active over positions lo .. hi of the m instants: there row 0 decides."""
    inst = _seconds(m)
    ovr = [(inst[lo], inst[hi], {0: 30}, None)] if lo is not None else [(FR.shift(inst[-1], 1), None, {0: 30}, None)]
    snap = PR.tiny([{0: 3}, {0: 3}, {0: 4}], {0: 9}, flags=[P, P, C], T=2, row=1)
    snap.thr_spec.set_row(0, {0: 17}, None)
    FR.timed(snap, 1, ovr)
    inside = [lo is not None and lo <= k <= hi for k in range(m)]
    for want in (1, 2):
        first, copies, limiting, blocker = held_to_everything(snap, oracle_mod, [[0, 1]], inst, want=want)
        assert first == [lo if lo is not None else -1]
        assert copies[0] == [2 if x else 0 for x in inside]
        assert limiting[0] == [0 if x else 1 for x in inside]
        assert blocker[0] == [0 if x else 1 for x in inside]


# ---- lanes whose searches end at different depths in one block ----------------------------------------------------------------
DEPTHS = [0, 1, 2, 63, 64, 65, 1000, None]  # copies per window; None: all `cap`
USED, ASKS = 5, (3, 4)


def _depths_cluster(exact):
    """One throttle, one override window per entry of DEPTHS: threshold USED + 7 H (+ 3 unless ``exact``) — the gang asks 3 + 4
    per copy.  Between the windows spec's USED + 7 x 5 + 3 holds: 5 copies.  -> (snapshot, instants, the threshold at each)"""
    A = sum(ASKS)
    spec = USED + A * 5 + 3
    snap = PR.tiny([{0: ASKS[0]}, {0: ASKS[1]}, {0: USED}], {0: spec}, flags=[P, P, C])
    ovr, inst, ths = [], [NOW], [spec]
    for i, H in enumerate(DEPTHS):
        begin, end = (NOW[0] + 100 * (i + 1), 0), (NOW[0] + 100 * (i + 1) + 50, 0)
        th = USED + A * (H if H is not None else 1 << 21) + (0 if exact else 3)
        ovr.append((begin, end, {0: th}, None))
        inst += [begin, FR.shift(end, 1)]
        ths += [th, spec]
    return FR.timed(snap, 0, ovr), inst, ths


@pytest.mark.parametrize("exact", [False, True])
def test_lanes_of_one_block_search_to_different_depths(exact, oracle_mod):
    """The lane-own bisection: the instants of ONE block admit 0, 1, 2, 63, 64, 65, 1000 and cap = 2^20 copies.  Expected by
    arithmetic: floor((threshold - used) / A) copies, one fewer with on_equal on exact division; the copy that is refused stops
    at its first member, or at its second where the first still fits below the threshold.  The oracle walks cap = 16 only."""
    cap, A = 1 << 20, sum(ASKS)
    snap, inst, ths = _depths_cluster(exact)
    assert len(inst) <= 64
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            w_copies, w_blocker = [], []
            for th in ths:
                room = th - USED - (1 if on_equal else 0)  # copy j passes iff USED + (j + 1) A <= room
                h = min(cap, max(room, 0) // A)
                s = USED + A * h  # what the first member of copy h meets: `used` is present, a Throttle's step 3 is on-equal
                stops_first = s >= th or (s + ASKS[0] >= th if on_equal else s + ASKS[0] > th)
                w_copies.append(h)
                w_blocker.append(-1 if h == cap else 0 if stops_first else 1)
            assert sorted(set(w_copies)) == sorted({5, cap} | ({max(H - 1, 0) for H in DEPTHS[:-1]} if exact and on_equal else set(DEPTHS[:-1])))
            for want in (1, 64, cap):
                first, copies, limiting, blocker = launch(eng, [[0, 1]], inst, cap, want, on_equal)
                assert copies[0] == w_copies, f"exact={exact} on_equal={on_equal}"
                assert blocker[0] == w_blocker and limiting[0] == [-1 if b < 0 else 0 for b in w_blocker]
                assert first == [HG.first_of(w_copies, want)]
            assert (first, copies, limiting, blocker) == by_model(snap, [[0, 1]], inst, cap, cap, on_equal)
    finally:
        eng.close()
    for on_equal in (False, True):
        held_to_everything(snap, oracle_mod, [[0, 1]], inst, 16, 3, on_equal)


# ---- the largest cap -----------------------------------------------------------------------------------------------------------
def test_the_largest_cap_the_lane_own_mask_and_the_int64_cut_off():
    """cap = 2^31 - 1 against numbers written out (no queue of 2^31 gangs can be walked), used 8.  Gang A: two members asking 2^31
    each (A = 2^32); gang B: two asking 2^40 each (A = 2^41).  Instants: spec cpu 10 (nobody); the override 2^62 + 8 (2^30 and
    2^21 copies, one fewer with on_equal: exact division); an override that names ANOTHER amount only — cpu is not throttled, and
    j x A for j up to 2^31 - 2 must not be formed for the lane (2^63 and beyond); a threshold within A of INT64_MAX
    (INT64_MAX - 5: gang A fits all cap copies, gang B 2^22 - 1 — the candidates end at (INT64_MAX - 0) / 2^41)."""
    snap = PR.tiny([{0: 1 << 31}, {0: 1 << 31}, {0: 1 << 40}, {0: 1 << 40}, {0: 8}], {0: 10}, flags=[P] * 4 + [C])
    FR.timed(snap, 0, [(FR.T1, FR.T1, {0: (1 << 62) + 8}, None), (FR.T2, FR.T2, {1: 5}, None), (FR.T3, FR.T3, {0: INT64_MAX - 5}, None)])
    inst = [NOW, FR.T1, FR.T2, FR.T3, FR.T4]
    gangs = [[0, 1], [2, 3]]
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            first, copies, limiting, blocker = launch(eng, gangs, inst, MAXCAP, 1 << 22, on_equal)
            eq = 1 if on_equal else 0
            assert copies[0] == [0, (1 << 30) - eq, MAXCAP, MAXCAP, 0]
            assert copies[1] == [0, (1 << 21) - eq, MAXCAP, (1 << 22) - 1, 0]
            assert limiting == [[0, 0, -1, -1, 0], [0, 0, -1, 0, 0]]
            # exact division: the refused copy stops at its first member, with on_equal the copy before it at its second
            assert blocker == [[0, eq, -1, -1, 0], [2, 2 + eq, -1, 3, 2]]
            assert first == [1, 2]
            assert (first, copies, limiting, blocker) == by_model(snap, gangs, inst, MAXCAP, 1 << 22, on_equal)
    finally:
        eng.close()


# ---- the chunk list ------------------------------------------------------------------------------------------------------------
def _many_throttles(rows_spec, timed_row, overrides, T=1030):
    """T throttles affect both members (used 8, they ask 3 each), all but ``rows_spec`` = {row: cpu threshold} with thresholds
    nothing reaches."""
    snap = PR.tiny([{0: 3}, {0: 3}, {0: 4}, {0: 4}], {0: rows_spec[T - 1] if T - 1 in rows_spec else 1 << 40}, flags=[P, P, C, C], T=T, row=T - 1)
    for t in range(T - 1):
        snap.thr_ns[t] = 0
        snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    for t, v in rows_spec.items():
        snap.thr_spec.set_row(t, {0: v}, None)
    return FR.timed(snap, timed_row, overrides)


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect the gang — more than one chunk of the LDS list holds; only the last row's override decides: 10 admits
    nobody (8 + 3 > 10), 20 two copies (8 + 12 <= 20)."""
    snap = _many_throttles({1029: 10}, 1029, [(FR.T1, FR.T2, {0: 20}, None)])
    assert len(paging.affected_throttles(snap, 0)[1]) == 1030
    first, copies, limiting, blocker = held_to_everything(snap, oracle_mod, [[0, 1]], FR.EDGE[:8], 4, want=2)
    assert first == [2] and copies[0] == [0, 0, 2, 2, 2, 2, 0, 0]
    assert limiting[0] == [1029] * 8 and blocker[0] == [0] * 8


@pytest.mark.parametrize("low,high", [(500, 1029), (5, 32)], ids=["different-chunks", "list-order-reversed"])
def test_tying_throttles_report_the_lower_row(low, high, oracle_mod):
    """Two deciding throttles among 1030: ``low`` (21) admits 2 copies throughout, ``high`` (15) 1 copy, and 2 between T1 and T2
    (21) — a tie in copies and blocker, and the lower row is the limiting one.  (5, 32): the chunk list holds row 32 in front of
    row 5 (it is filled round by round, one marked byte per lane and round), so "first seen wins" would report 32."""
    snap = _many_throttles({low: 21, high: 15}, high, [(FR.T1, FR.T2, {0: 21}, None)])
    first, copies, limiting, blocker = held_to_everything(snap, oracle_mod, [[0, 1]], FR.EDGE[:8], 4, want=2)
    assert first == [2] and copies[0] == [1, 1, 2, 2, 2, 2, 1, 1] and blocker[0] == [0] * 8
    assert limiting[0] == [high, high, low, low, low, low, high, high]


# ---- every instantiation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    """The deciding name is the last one; the others are requested and reserved but no threshold stops them.  Used 8, 3 + 3 per
    copy: spec 10 admits nobody, 20 (T1 .. T2) two copies, 100 (T3 .. T4) fifteen — there the second override also names another
    amount with a threshold of 1000."""
    d = D - 1
    other = {x: 2 for x in range(D) if x != d}
    member, running = dict(other), dict(other)
    member[d], running[d] = 3, 4
    snap = PR.tiny([member, member, running, running], {d: 10}, flags=[P, P, C, C], D=D)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {d: 20}, None), (FR.T3, FR.T4, {d: 100, (d + 1) % D: 1000} if D > 1 else {d: 100}, None)])
    for on_equal in (False, True):
        first, copies, _, _ = held_to_everything(snap, oracle_mod, [[0, 1], [1, 0]], FR.EDGE + [FR.shift(FR.T4, 1)], 16, 3, on_equal)
        assert copies[0] == copies[1] == [0, 0, 1 if on_equal else 2, 1 if on_equal else 2] + [1 if on_equal else 2] * 2 + [0, 15, 15, 0]
        assert first == [7, 7]


# ---- gang specifics --------------------------------------------------------------------------------------------------------------
def test_members_met_by_different_throttles(oracle_mod):
    """Row 0: a Throttle of namespace 0 on name 0 (10: three copies of pod 0's 3); row 1: a Throttle of namespace 2 on name 1 (5:
    one copy of pod 1's 3), with an override of 100 between T1 and T2.  Outside the window row 1 stops the second member of copy
    1, inside row 0 the first member of copy 3."""
    snap = PR.tiny([{0: 3}, {1: 3}], {1: 5}, flags=[P, P], T=2, row=1, pod_ns=[0, 2])
    snap.thr_ns[1] = 2
    snap.thr_spec.set_row(0, {0: 10}, None)
    FR.timed(snap, 1, [(FR.T1, FR.T2, {1: 100}, None)])
    for on_equal in (False, True):
        first, copies, limiting, blocker = held_to_everything(snap, oracle_mod, [[0, 1], [1, 0]], FR.EDGE, 16, 2, on_equal)
    inside = [0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert copies[0] == copies[1] == [3 if x else 1 for x in inside] and limiting[0] == limiting[1] == [0 if x else 1 for x in inside]
    assert blocker[0] == [0 if x else 1 for x in inside] and blocker[1] == [3 if x else 2 for x in inside]


def test_seventy_members_the_bad_member_in_the_second_block(oracle_mod):
    """The member ballot strides 64: the member whose namespace has no object sits at position 66.  A count of 1000 stops nobody in
    front of it (blocker 66, no limiting row); the override's 50 between T1 and T2 stops member 50."""
    n = 70
    snap = PR.tiny([{0: 1}] * n, {}, count=1000, flags=[P] * n, pod_ns=[1 if i == 66 else 0 for i in range(n)], cluster=True)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {}, 50)])
    first, copies, limiting, blocker = held_to_everything(snap, oracle_mod, [list(range(n))], FR.EDGE, 3)
    inside = [0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert first == [-1] and copies[0] == [0] * 9
    assert blocker[0] == [50 if x else 66 for x in inside] and limiting[0] == [0 if x else -1 for x in inside]


def test_more_gangs_than_the_grid_has_workgroups(oracle_mod):
    """2100 gangs of two x 3 instants in one launch: the grid (2048 workgroups at the most) strides.  Pods are shared between the
    gangs.  Used 8: spec 10 admits nobody, the override's 19 floor(11 / (a + b)) copies."""
    asks = [1, 2, 3, 12]
    snap = PR.tiny([{0: a} for a in asks] + [{0: 4}] * 2, {0: 10}, flags=[P] * 4 + [C] * 2)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {0: 19}, None)])
    inst = [FR.T0, FR.T1, FR.T3]
    pairs = [[i, j] for i in range(4) for j in range(4) if i != j]
    gangs = [pairs[(k // 3) % len(pairs)] for k in range(2100)]
    eng = E.Engine.for_snapshot(snap)
    try:
        first, copies, limiting, blocker = launch(eng, gangs, inst, CAP, 2)
    finally:
        eng.close()
    sample = list(range(0, 2100, 21))
    assert len(sample) == 100 and sample[-1] >= 2048
    walked = {}
    for k in sample:
        key = tuple(gangs[k])
        if key not in walked:
            walked[key] = HG.reference(snap, oracle_mod, gangs[k], inst, CAP, 2)
        w = walked[key]
        assert (first[k], copies[k], limiting[k], [b - 2 * k if b >= 0 else -1 for b in blocker[k]]) == w, f"gang {k} {gangs[k]}"
    assert len(walked) == len(pairs)
    for k, (i, j) in enumerate(gangs):
        a, b = asks[i], asks[j]
        row = []
        for th in (10, 19, 10):
            h = (th - 8) // (a + b)
            row.append((h, 2 * k + (0 if 8 + h * (a + b) + a > th else 1)))
        assert copies[k] == [h for h, _ in row] and blocker[k] == [p for _, p in row] and limiting[k] == [0, 0, 0]
        assert first[k] == (1 if row[1][0] >= 2 else -1)


# ---- identities ------------------------------------------------------------------------------------------------------------------
IDENTITY_CASES = ["cluster-1", "cluster-4", "stair-3", "stair-11"]


def _case(name, oracle_mod):
    return next(c for c in HG.random_cases(oracle_mod) if c[0] == name)


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_a_gang_of_one_is_the_headroom_forecast(name, oracle_mod):
    """(G1)"""
    _, snap, gangs, inst, _ = _case(name, oracle_mod)
    pods = sorted({p for g in gangs for p in g})
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            p_first, p_copies, p_limiting = eng.headroom_forecast(pods, inst, cap=CAP, want=2, on_equal=on_equal)
            first, copies, limiting, blocker = eng.headroom_forecast_gangs(pods, list(range(len(pods) + 1)), inst, cap=CAP, want=2, on_equal=on_equal)
            assert first.tobytes() == p_first.tobytes() and copies.tobytes() == p_copies.tobytes() and limiting.tobytes() == p_limiting.tobytes()
            own = np.arange(len(pods), dtype=np.int64)[:, None]
            assert np.array_equal(blocker, np.where(copies < CAP, own, -1))
    finally:
        eng.close()


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_cap_one_is_the_gang_forecast(name, oracle_mod):
    """(G2)"""
    _, snap, gangs, inst, _ = _case(name, oracle_mod)
    rows, off = HG.queue_of(gangs)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            f_first, verdicts, f_blocker = eng.forecast_gangs(rows, off, inst, on_equal)
            first, copies, _, blocker = eng.headroom_forecast_gangs(rows, off, inst, cap=1, want=1, on_equal=on_equal)
            assert np.array_equal(copies == 1, verdicts == S.VERDICT_ALLOW) and np.array_equal(copies == 0, verdicts != S.VERDICT_ALLOW)
            assert first.tobytes() == f_first.tobytes() and blocker.tobytes() == f_blocker.tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("name", IDENTITY_CASES[:2])
def test_single_instant_behind_an_applied_reconcile_is_the_gang_headroom(name, oracle_mod):
    """(G3), at NOW and at a boundary inside the window."""
    _, snap, gangs, inst, _ = _case(name, oracle_mod)
    rows, off = HG.queue_of(gangs)
    eng = E.Engine.for_snapshot(snap)
    try:
        for t in (inst[0], inst[len(inst) // 2]):
            for on_equal in (False, True):
                eng.reconcile(t, apply=True)
                _, copies, limiting, blocker = eng.headroom_forecast_gangs(rows, off, [t], cap=CAP, on_equal=on_equal)
                h_copies, h_limiting, h_blocker = eng.headroom_gangs(rows, off, cap=CAP, on_equal=on_equal)
                assert copies[:, 0].tobytes() == h_copies.tobytes() and limiting[:, 0].tobytes() == h_limiting.tobytes()
                assert blocker[:, 0].tobytes() == h_blocker.tobytes()
    finally:
        eng.close()


# ---- refusals, slots, the dry run ------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def _rise_and_fall():
    # used 4, the members ask 3 each: spec 9 admits nobody, 16 two copies (T1 .. T2), 1000 all sixteen (T3 .. T4)
    snap = FR.timed(PR.tiny([{0: 3}, {0: 3}, {0: 4}], {0: 9}, flags=[P, P, C]), 0, [(FR.T1, FR.T2, {0: 16}, None), (FR.T3, FR.T4, {0: 1000}, None)])
    return snap, FR.EDGE + [FR.shift(FR.T4, 1)]


def test_want(oracle_mod):
    snap, inst = _rise_and_fall()
    for want, first in ((1, 2), (2, 2), (3, 7), (16, 7)):
        got = held_to_everything(snap, oracle_mod, [[0, 1]], inst, want=want)
        assert got[0] == [first] and got[1][0] == [0, 0, 2, 2, 2, 2, 0, 16, 16, 0]


def test_validation_in_order_and_what_a_refused_call_leaves_alone(oracle_mod):
    snap, inst = _rise_and_fall()
    gang, off = [0, 1], [0, 2]
    want = HG.expected(snap, oracle_mod, [gang], inst, 16, 3)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    rows, offs = np.array(gang, np.int64), np.array(off, np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    hf = lambda pods, gang_off, instants, cap=16, want=1: eng.headroom_forecast_gangs(pods, gang_off, instants, cap=cap, want=want)
    raw = lambda n, r, ng, o, s, ns: L.kt_headroom_forecast_gangs_launch(eng._h, n, r, ng, o, 2, s, ns, 0, 16, 1, None)
    try:
        assert _code(lambda: eng.headroom_forecast_gangs_fetch(1, len(inst))) == -5  # KT_ERR_NOT_READY

        def every_refusal():
            # 1. the instants and a missing array
            assert _code(lambda: hf(gang, off, [])) == -1
            assert _code(lambda: hf(gang, off, [FR.T1, FR.T1])) == -1
            assert _code(lambda: hf(gang, off, [FR.T2, FR.T1])) == -1
            assert _code(lambda: hf(gang, off, [(NOW[0], 1_000_000_000)])) == -1
            assert raw(2, None, 1, offs.ctypes.data, s2.ctypes.data, n2.ctypes.data) == -1
            assert raw(2, rows.ctypes.data, 1, offs.ctypes.data, None, n2.ctypes.data) == -1
            assert raw(2, rows.ctypes.data, 1, offs.ctypes.data, s2.ctypes.data, None) == -1
            assert raw(-1, rows.ctypes.data, 1, offs.ctypes.data, s2.ctypes.data, n2.ctypes.data) == -1
            assert raw(2, rows.ctypes.data, -1, offs.ctypes.data, s2.ctypes.data, n2.ctypes.data) == -1
            # ... in front of cap: the message names the instants
            assert _code(lambda: hf(gang, off, [FR.T2, FR.T1], cap=0)) == -1 and b"ascending" in L.kt_last_error(eng._h)
            # 2. cap, then want, in front of the gang defects
            for cap, w in ((0, 1), (-3, 1), (MAXCAP + 1, 1), (16, 0), (16, 17), (16, -1)):
                assert _code(lambda: hf(gang, [0, 3], inst, cap=cap, want=w)) == -1
            assert _code(lambda: hf(gang, [0, 3], inst, cap=0, want=0)) == -1 and b"cap" in L.kt_last_error(eng._h)
            assert _code(lambda: hf(gang, [0, 3], inst, want=0)) == -1 and b"want" in L.kt_last_error(eng._h)
            # 3. the gang defects and a pod twice within one gang, in front of a row outside the table
            assert _code(lambda: hf([0, 99], [0, 3], inst)) == -1                                 # the offsets do not end at n
            assert _code(lambda: hf([0, 99], [0, 0, 2], inst)) == -1                              # an empty gang
            assert _code(lambda: hf([0, 99], [1, 2], inst)) == -1                                 # ... do not begin at 0
            assert raw(2, rows.ctypes.data, 1, None, s2.ctypes.data, n2.ctypes.data) == -1
            assert _code(lambda: hf([99, 99], off, inst)) == -1 and b"twice" in L.kt_last_error(eng._h)
            # 4. rows out of range, in front of what is unsupported
            eng.set_exchange_world(2)
            assert _code(lambda: hf([0, 99], off, inst)) == -2
            assert _code(lambda: hf([-1, 0], off, inst)) == -2
            # 5. the size limits
            many = np.zeros(2**16 + 1, np.int64)
            assert _code(lambda: hf(many, np.arange(2**16 + 2), _seconds(2**15))) == -2           # n_gangs x n_inst > 2^31
            # 6. unsupported
            assert _code(lambda: hf(gang, off, inst)) == -7
            eng.set_exchange_world(1)
            eng.set_wide_sums(1)
            assert _code(lambda: hf(gang, off, inst)) == -7                                       # `used` wider than int64
            eng.set_wide_sums(0)

        def fetched_is_wanted():
            got = eng.headroom_forecast_gangs_fetch(1, len(inst))
            assert tuple(x.tolist() for x in got) == tuple(want)

        # a refused call leaves a pending result fetchable ...
        eng.headroom_forecast_gangs_launch(gang, off, inst, 16, 3)
        every_refusal()
        fetched_is_wanted()
        # ... and a pending check and a pending reconcile report (a launch that is accepted takes both: see the slot rules)
        eng.reconcile_launch(NOW, apply=False)
        eng.check_launch(snap.n_pods, want_status=True)
        every_refusal()
        eng.check_fetch(snap.n_pods, True)
        eng.reconcile_fetch()
        assert _code(lambda: inc.headroom_forecast_gangs(gang, off, inst, cap=16)) == -7
        wide_rows = E.Engine.for_snapshot(_many_throttles({1029: 10}, 1029, []))
        try:
            n = 2 * (2**30 // 1030 + 1)  # gangs of two distinct pods: n x throttle_rows > 2^31
            assert _code(lambda: wide_rows.headroom_forecast_gangs(np.tile(np.array([0, 1], np.int64), n // 2), np.arange(0, n + 1, 2), [NOW],
                                                                   cap=16)) == -2
            assert wide_rows.headroom_forecast_gangs([0, 1], off, [NOW], cap=16)[1].tolist() == [[0]]
        finally:
            wide_rows.close()
        # n == 0 only with no gangs: KT_OK, nothing launched; the nullable outputs; the largest cap
        eng.headroom_forecast_gangs_launch([], [0], inst, 16)
        assert [x.tolist() for x in eng.headroom_forecast_gangs_fetch(0, len(inst))] == [[], [], [], []]
        eng.headroom_forecast_gangs_launch(gang, off, inst, 16, 3)
        first, none_c, none_l, none_b = eng.headroom_forecast_gangs_fetch(1, len(inst), want_copies=False, want_limiting=False, want_blocker=False)
        assert none_c is None and none_l is None and none_b is None and first.tolist() == [7]
        first, copies, _, _ = hf(gang, off, inst, cap=MAXCAP, want=30)
        assert copies[0].tolist() == [0, 0, 2, 2, 2, 2, 0, 166, 166, 0] and first.tolist() == [7]   # (1000 - 4) // 6
    finally:
        eng.close()
        inc.close()


def test_an_engine_that_was_fed_a_negative_request_is_refused(oracle_mod):
    """The last refusal: the search over the copies rests on sums that only grow.  Whoever was fed counts, gang member or not; the
    message names this call and the call that serves such an engine pod by pod; a pending result stays fetchable."""
    snap = FR.timed(PR.tiny([{0: 3}, {0: 3}, {0: 4}, {1: -1}], {0: 9}, flags=[P, P, C, C]), 0, [(FR.T1, FR.T2, {0: 16}, None)])
    eng = E.Engine.for_snapshot(snap)
    try:
        eng.forecast_gangs_launch([0, 1], [0, 2], FR.EDGE)
        assert _code(lambda: eng.headroom_forecast_gangs([0, 1], [0, 2], FR.EDGE, cap=16)) == -7
        msg = E.lib().kt_last_error(eng._h).decode()
        assert msg.startswith("headroom forecast gangs: the engine has been fed a negative request") and "kt_headroom_forecast_launch" in msg
        assert _code(lambda: eng.headroom_forecast_gangs([0, 9], [0, 2], FR.EDGE, cap=16)) == -2  # a row out of range comes first
        assert eng.forecast_gangs_fetch(1, len(FR.EDGE))[1].tolist() == [[1, 1, 0, 0, 0, 0, 1, 1, 1]]
        assert eng.headroom_forecast([0], FR.EDGE, cap=16)[1].tolist() == [[1, 1, 4, 4, 4, 4, 1, 1, 1]]  # pod by pod it is served
    finally:
        eng.close()


def test_slot_rules_and_dry_run(oracle_mod):
    """(G4) and the slots, with all four kinds of the one pending forecast result."""
    _, snap, gangs, inst, want = _case("cluster-1", oracle_mod)
    rows, off = HG.queue_of(gangs)
    ng, m = len(gangs), len(inst)
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    cands = [int(c) for c in everyone if c not in rows]
    eng = E.Engine.for_snapshot(snap)

    def fetch_ok():
        _, copies, limiting, blocker = eng.headroom_forecast_gangs_fetch(ng, m)
        return all(copies[g].tolist() == want[False][g][1] and limiting[g].tolist() == want[False][g][2] and
                   [b - off[g] if b >= 0 else -1 for b in blocker[g].tolist()] == want[False][g][3] for g in range(ng))
    go = lambda: eng.headroom_forecast_gangs_launch(rows, off, inst, CAP, 2)
    try:
        # (G4) a dry run: what reads the stored status and the reserved amounts sees them unchanged
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = [x.copy() for eq in (False, True) for x in eng.headroom(everyone, cap=MAXCAP, on_equal=eq)]
        res_before = eng.fetch_reserved()
        plain = eng.reconcile(NOW, apply=False)
        prefix = eng.preempt([rows[0]], cands, NOW)[0].tolist()
        # the launch takes the check slot and the reconcile result buffers
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        go()
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == -5
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves the result fetchable
        eng.aggregate_launch()
        go()
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        assert fetch_ok()
        # the four kinds of the one pending forecast result: only the launch's own fetch reads it
        go()
        assert _code(lambda: eng.forecast_fetch(len(rows), m)) == -5
        assert _code(lambda: eng.forecast_gangs_fetch(ng, m)) == -5
        assert _code(lambda: eng.headroom_forecast_fetch(len(rows), m)) == -5
        assert fetch_ok()
        eng.forecast_launch(rows, inst)
        assert _code(lambda: eng.headroom_forecast_gangs_fetch(ng, m)) == -5
        eng.forecast_fetch(len(rows), m)
        eng.forecast_gangs_launch(rows, off, inst)
        assert _code(lambda: eng.headroom_forecast_gangs_fetch(ng, m)) == -5
        eng.forecast_gangs_fetch(ng, m)
        eng.headroom_forecast_launch(rows, inst, CAP)
        assert _code(lambda: eng.headroom_forecast_gangs_fetch(ng, m)) == -5
        eng.headroom_forecast_fetch(len(rows), m)
        # a preempt result survives the launch, and the other way round
        eng.preempt_launch([rows[0]], cands, NOW)
        go()
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == prefix
        assert fetch_ok()
        go()
        eng.preempt_launch([rows[0]], cands, NOW)
        assert fetch_ok()
        assert eng.preempt_fetch(1, len(cands))[0].tolist() == prefix
        # a later user of the check slot drops it
        go()
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.headroom_forecast_gangs_fetch(ng, m)) == -5
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        room_after = [x for eq in (False, True) for x in eng.headroom(everyone, cap=MAXCAP, on_equal=eq)]
        res_after = eng.fetch_reserved()
        again = eng.reconcile(NOW, apply=False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, room_after))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
            assert getattr(plain.used, f).tobytes() == getattr(again.used, f).tobytes()
        assert plain.thrl_flag.tobytes() == again.thrl_flag.tobytes()
    finally:
        eng.close()


def test_host_plugin_scale_after_gang():
    """The plugin mirror's ScaleAfterGang against a twin plugin that, per boundary, reconciles and counts whole admitted copies of
    the gang by PreFilter + Reserve (tests/cpp/host_plugin_scale_after_gang_test.cpp)."""
    host = os.path.join(ROOT, "kube_throttler_amd", "host")
    subprocess.check_call(["make", "-C", host, "host_plugin_scale_after_gang_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(host, "host_plugin_scale_after_gang_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
