"""The gang forecast on the GPU: Engine.forecast_gangs (kt_forecast_gangs_launch / kt_forecast_gangs_fetch,
csrc/kt_kernels_forecast_gangs.hip) against the reference of tests/forecast_gangs_reference.py (per instant: a copy of the
snapshot, the oracle's reconcile, the oracle's in-order admission of the members) and ``paging.forecast_gangs_of`` — verdict bytes,
first position and blockers compared bit for bit.  The shapes are the smallest at which the kernel can still go wrong: instant
blocks of 64 and the ballot across them, a gang beyond one member block, a deciding throttle in the second chunk of the
affected-throttle list, one case per DT instantiation (D = 1, 8, 16), more gangs than the grid has workgroups."""
import numpy as np
import pytest

import forecast_gangs_reference as FG
import forecast_reference as FR
import preempt_gangs_reference as GR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_forecast_cpu import SEEDS

pytestmark = pytest.mark.gpu
NOW = FR.NOW
A, B, ERR = S.VERDICT_ALLOW, S.VERDICT_BLOCK, S.VERDICT_ERROR


def _queue(gangs):
    rows = [int(p) for g in gangs for p in g]
    off = np.cumsum([0] + [len(g) for g in gangs]).astype(np.int64)
    return rows, off


def launch_all(eng, gangs, instants, on_equal=False):
    """All gangs in ONE launch -> per gang (first, verdicts, blockers) with the blockers as positions inside the gang."""
    rows, off = _queue(gangs)
    first, verdicts, blockers = eng.forecast_gangs(rows, off, instants, on_equal)
    assert verdicts.shape == blockers.shape == (len(gangs), len(instants)) and first.shape == (len(gangs),)
    out = []
    for g in range(len(gangs)):
        blk = [int(b) for b in blockers[g]]
        assert all(b == -1 or off[g] <= b < off[g + 1] for b in blk), (g, blk)
        out.append((int(first[g]), verdicts[g].tolist(), [b if b < 0 else b - int(off[g]) for b in blk]))
    return out


def held_to_everything(snap, oracle_mod, gangs, instants, on_equal=False, want=None):
    eng = E.Engine.for_snapshot(snap)
    try:
        got = launch_all(eng, gangs, instants, on_equal)
    finally:
        eng.close()
    for g, members in enumerate(gangs):
        ref = want[g] if want is not None else FG.reference(snap, oracle_mod, members, instants, on_equal)
        assert got[g] == ref, f"gang {g} {members} on_equal={on_equal}: {got[g]} != {ref}"
        assert paging.forecast_gangs_of(snap, members, instants, on_equal) == ref
    return got


@pytest.mark.parametrize("seed", FG.STAIR_SEEDS)
def test_generator_a(seed, oracle_mod):
    snap, members, inst, want, _ = FG.stair_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            assert launch_all(eng, [members], inst, on_equal)[0] == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        eng.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_b(seed, oracle_mod):
    snap, gangs, want, _ = FG.cluster_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            assert launch_all(eng, gangs, FR.INSTANTS, on_equal) == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FG.DIRECTED))
def test_directed(name, oracle_mod):
    snap, members, inst = FG.DIRECTED[name]()
    for on_equal in (False, True):
        held_to_everything(snap, oracle_mod, [members], inst, on_equal)


def test_directed_the_example(oracle_mod):
    window = [B, B, A, A, A, A, B, B, B]  # EDGE = T0, T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, T3, T4
    snap, members, inst = FG.DIRECTED["each-alone-passes-the-gang-only-in-the-window"]()
    eng = E.Engine.for_snapshot(snap)
    try:
        assert launch_all(eng, [members], inst) == [(2, window, [-1 if v == A else 1 for v in window])]
        first, verdicts = eng.forecast(members, inst)  # each member alone passes at every instant
        assert first.tolist() == [0, 0] and not verdicts.any()
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FR.DIRECTED))
def test_a_gang_of_one_is_the_plain_forecast(name):
    snap, p, inst = FR.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            first, verdicts = eng.forecast([p], inst, on_equal)
            gfirst, gverdicts, gblockers = eng.forecast_gangs([p], [0, 1], inst, on_equal)
            assert gfirst.tobytes() == first.tobytes() and gverdicts.tobytes() == verdicts.tobytes()
            assert gblockers[0].tolist() == [-1 if v == A else 0 for v in verdicts[0]]
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(GR.DIRECTED))
def test_single_instant_agrees_with_preempt_gangs_without_candidates(name):
    snap, members, _ = GR.DIRECTED[name][0]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            prefix, _, blocker = eng.preempt_gangs(members, [0, len(members)], [], NOW, on_equal)
            first, _, blockers = eng.forecast_gangs(members, [0, len(members)], [NOW], on_equal)
            assert (int(first[0]) == 0) == (int(prefix[0]) == 0)
            assert int(blockers[0][0]) == int(blocker[0])
    finally:
        eng.close()


def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


@pytest.mark.parametrize("m,lo,hi", [(1, 0, 0), (1, None, None), (63, 62, 62), (64, 63, 63), (65, 64, 64), (65, 63, 64), (130, 128, 129),
                                     (130, None, None)])
def test_instant_blocks_and_the_ballot(m, lo, hi, oracle_mod):
    """The example's two-member gang (4 + 3 + 3 > 8); the override 10 is active over positions lo .. hi of the m instants."""
    inst = _seconds(m)
    ovr = [(inst[lo], inst[hi], {0: 10}, None)] if lo is not None else [(FR.shift(inst[-1], 1), None, {0: 10}, None)]
    snap = FR.timed(PR.tiny([{0: 3}, {0: 3}, {0: 4}], {0: 8}, flags=FG.P2C1), 0, ovr)
    (first, verdicts, blockers), = held_to_everything(snap, oracle_mod, [[0, 1]], inst)
    assert first == (lo if lo is not None else -1)
    assert verdicts == [A if lo is not None and lo <= k <= hi else B for k in range(m)]
    assert blockers == [-1 if v == A else 1 for v in verdicts]


def test_seventy_members_an_invalid_one_in_the_second_block(oracle_mod):
    """The member ballot strides 64: the invalid member sits at position 66; inside the window (50) member 50 is stopped first."""
    n = 70
    snap = FR.timed(PR.tiny([{0: 1}] * n, {0: 1000}, flags=[PR.PENDING] * n), 0, [(FR.T1, FR.T2, {0: 50}, None)])
    snap.pod_flags[66] = 0
    (first, verdicts, blockers), = held_to_everything(snap, oracle_mod, [list(range(n))], FR.EDGE)
    assert first == -1 and verdicts == [ERR] * 9 and blockers == [66, 66, 50, 50, 50, 50, 66, 66, 66]


def test_seventy_members_a_count_threshold_stops_member_65(oracle_mod):
    n = 70
    snap = FR.timed(PR.tiny([{0: 1}] * n, {}, count=65, flags=[PR.PENDING] * n), 0, [(FR.T1, FR.T2, {}, 70)])
    (first, verdicts, blockers), = held_to_everything(snap, oracle_mod, [list(range(n))], FR.EDGE)
    assert first == 2 and blockers == [65, 65, -1, -1, -1, -1, 65, 65, 65]


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect both members — more than one chunk of the LDS list holds; only the last row's override lets the
    gang through."""
    T = 1030
    snap = PR.tiny([{0: 3}, {0: 3}, {0: 4}], {0: 8}, flags=FG.P2C1, T=T, row=T - 1)
    for t in range(T - 1):
        snap.thr_ns[t] = 0
        snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    FR.timed(snap, T - 1, [(FR.T1, FR.T2, {0: 10}, None)])
    (first, verdicts, blockers), = held_to_everything(snap, oracle_mod, [[0, 1]], FR.EDGE[:8])
    assert first == 2 and verdicts == [B, B, A, A, A, A, B, B] and blockers == [1, 1, -1, -1, -1, -1, 1, 1]
    assert len(paging.affected_throttles(snap, 0)[1]) == T


@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    """The deciding name is the last one; the others are requested and counted but no threshold stops them."""
    d = D - 1
    other = {x: 2 for x in range(D) if x != d}
    member, running = dict(other), dict(other)
    member[d], running[d] = 3, 4
    snap = PR.tiny([member, member, running], {d: 8, **({0: 100} if D > 1 else {})}, flags=FG.P2C1, D=D)
    FR.timed(snap, 0, [(FR.T1, FR.T2, {d: 10}, None), (FR.T3, FR.T4, {d: 10, (d + 1) % D: 5} if D > 1 else {d: 9}, None)])
    for on_equal in (False, True):
        got, = held_to_everything(snap, oracle_mod, [[0, 1]], FR.EDGE + [FR.shift(FR.T4, 1)], on_equal)
        assert got[0] == (-1 if on_equal else 2)


def test_more_gangs_than_the_grid_has_workgroups(oracle_mod):
    """2050 two-member gangs in one launch: the grid strides beyond 2048.  Pods are shared between the gangs."""
    asks = [1, 2, 3, 4, 5, 3]
    snap = FR.timed(PR.tiny([{0: a} for a in asks] + [{0: 4}], {0: 10}, count=3, flags=[PR.PENDING] * 6 + [PR.COUNTED]), 0,
                    [(FR.T1, FR.T2, {0: 12}, None), (FR.T3, FR.T4, {0: 9}, 2)])
    pairs = [[i, j] for i in range(6) for j in range(6) if i != j]
    want = {tuple(g): FG.reference(snap, oracle_mod, g, FR.EDGE) for g in pairs}
    for g in pairs:
        assert paging.forecast_gangs_of(snap, g, FR.EDGE) == want[tuple(g)]
    assert len({w[0] for w in want.values()}) >= 3  # the gangs differ in their answers
    gangs = [pairs[(7 * k) % len(pairs)] for k in range(2050)]
    eng = E.Engine.for_snapshot(snap)
    try:
        got = launch_all(eng, gangs, FR.EDGE)
    finally:
        eng.close()
    for k, g in enumerate(gangs):
        assert got[k] == want[tuple(g)], f"gang {k} {g}"


def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def test_validation_and_what_a_refused_call_leaves_alone(oracle_mod):
    snap, members, inst = FG.DIRECTED["each-alone-passes-the-gang-only-in-the-window"]()
    want = FG.reference(snap, oracle_mod, members, inst)
    plain_want = FR.reference_verdicts(snap, oracle_mod, members, inst)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    rows, off = np.array(members, np.int64), np.array([0, 2], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    fg = eng.forecast_gangs
    try:
        assert _code(lambda: eng.forecast_gangs_fetch(1, len(inst))) == -5  # KT_ERR_NOT_READY

        def raw(n=2, r=rows, ng=1, o=off, m=2, s=s2, ns=n2):
            ptr = lambda a: None if a is None else a.ctypes.data
            return L.kt_forecast_gangs_launch(eng._h, n, ptr(r), ng, ptr(o), m, ptr(s), ptr(ns), 0, None)

        def every_refusal():
            # the instants come first: even with a broken gang_off
            assert _code(lambda: fg(members, [0, 2], [])) == -1                                   # n_inst < 1
            assert _code(lambda: fg(members, [0, 1], [])) == -1
            assert _code(lambda: fg(members, [0, 2], [FR.T1, FR.T1])) == -1                       # not STRICTLY ascending
            assert _code(lambda: fg(members, [0, 2], [FR.T2, FR.T1])) == -1
            assert _code(lambda: fg(members, [0, 2], [(NOW[0], 5), (NOW[0], 4)])) == -1
            assert _code(lambda: fg(members, [0, 2], [(NOW[0], 1_000_000_000)])) == -1            # inst_ns outside [0, 10^9)
            assert _code(lambda: fg(members, [0, 2], [(NOW[0], -1)])) == -1
            assert raw(r=None) == -1 and raw(s=None) == -1 and raw(ns=None) == -1                 # missing arrays
            assert raw(n=-1) == -1 and raw(ng=-1) == -1
            # every gang_off defect kt_admit_gangs_launch refuses
            assert raw(o=None) == -1
            assert _code(lambda: fg(members, [1, 2], inst)) == -1                                 # gang_off[0] != 0
            assert _code(lambda: fg(members, [0, 0, 2], inst)) == -1                              # an empty gang
            assert _code(lambda: fg(members, [0, 2, 1], inst)) == -1                              # descending
            assert _code(lambda: fg(members, [0, 1], inst)) == -1                                 # gang_off[n_gangs] != n
            assert _code(lambda: fg(members, [0, 3], inst)) == -1
            assert raw(ng=0) == -1                                                                # no gangs for a queue of 2
            assert _code(lambda: fg([], [0, 0], inst)) == -1                                      # n == 0 with n_gangs == 1
            assert _code(lambda: fg([0, 1, 0], [0, 3], inst)) == -1                               # a pod twice within ONE gang
            assert _code(lambda: fg([0, 99, 99], [0, 3], inst)) == -1                             # ... asked before the range
            assert _code(lambda: fg([0, 99], [0, 2], inst)) == -2                                 # a pod row outside the capacity
            assert _code(lambda: fg([-1], [0, 1], inst)) == -2
            many = np.zeros(2**16 + 1, np.int64)
            assert _code(lambda: fg(many, np.arange(2**16 + 2), _seconds(2**15))) == -2           # n_gangs x n_inst > 2^31
            eng.set_exchange_world(2)
            assert _code(lambda: fg(members, [0, 2], inst)) == -7                                 # KT_ERR_UNSUPPORTED
            eng.set_exchange_world(1)
            eng.set_wide_sums(1)
            assert _code(lambda: fg(members, [0, 2], inst)) == -7                                 # `used` wider than int64
            eng.set_wide_sums(0)

        # a refused call leaves a pending gang forecast and a pending gang preempt result fetchable ...
        prefix = eng.preempt_gangs(members, [0, 2], [2], NOW)
        eng.preempt_gangs_launch(members, [0, 2], [2], NOW)
        eng.forecast_gangs_launch(members, [0, 2], inst)
        every_refusal()
        got = eng.forecast_gangs_fetch(1, len(inst))
        assert (int(got[0][0]), got[1][0].tolist(), got[2][0].tolist()) == want
        again = eng.preempt_gangs_fetch(1, 1)  # (a gang launch leaves a pending preempt_gangs result fetchable)
        assert all(np.array_equal(x, y) for x, y in zip(again, prefix))
        # ... and a pending plain forecast, a pending check and a pending reconcile report
        eng.forecast_launch(members, inst)
        every_refusal()
        assert np.array_equal(eng.forecast_fetch(2, len(inst))[1], plain_want)
        eng.reconcile_launch(NOW, apply=False)
        eng.check_launch(snap.n_pods, want_status=True)
        every_refusal()
        eng.check_fetch(snap.n_pods, True)
        eng.reconcile_fetch()
        assert _code(lambda: inc.forecast_gangs(members, [0, 2], inst)) == -7
        wide_rows = E.Engine.for_snapshot(FR._run({0: 10}, T=1030, row=1029))
        try:  # n x throttle_rows > 2^31: pod 0, valid, as so many gangs of one — nothing but the matrix rule can answer -2
            big = 2**31 // 1030 + 1
            assert _code(lambda: wide_rows.forecast_gangs(np.zeros(big, np.int64), np.arange(big + 1), [NOW])) == -2
            assert "throttle_rows" in E.lib().kt_last_error(wide_rows._h).decode()
            # ... and the engine with its 1030 throttle rows answers a gang it can take (8 + 3 > 10: blocked now)
            first, verdicts, blockers = wide_rows.forecast_gangs([0], [0, 1], [NOW])
            assert first.tolist() == [-1] and verdicts.tolist() == [[B]] and blockers.tolist() == [[0]]
        finally:
            wide_rows.close()
        # the one pending forecast result is shared: the kind of the last launch decides which fetch may read it
        eng.forecast_launch(members, inst)
        assert _code(lambda: eng.forecast_gangs_fetch(1, len(inst))) == -5
        assert np.array_equal(eng.forecast_fetch(2, len(inst))[1], plain_want)
        eng.forecast_gangs_launch(members, [0, 2], inst)
        assert _code(lambda: eng.forecast_fetch(1, len(inst))) == -5
        assert eng.forecast_gangs_fetch(1, len(inst))[1][0].tolist() == want[1]
        E.paged_forecast([eng], members, inst)
        assert _code(lambda: eng.forecast_gangs_fetch(1, len(inst))) == -5
        # n == 0 with n_gangs == 0: KT_OK, nothing launched
        eng.forecast_gangs_launch([], [0], inst)
        assert eng.forecast_gangs_fetch(0, len(inst))[0].tolist() == []
        assert _code(lambda: eng.forecast_fetch(0, len(inst))) == -5
        # nullable outputs
        first, none, blockers = fg(members, [0, 2], inst, want_verdicts=False)
        assert none is None and int(first[0]) == want[0] and blockers[0].tolist() == want[2]
        first, verdicts, none = fg(members, [0, 2], inst, want_blocker=False)
        assert none is None and int(first[0]) == want[0] and verdicts[0].tolist() == want[1]
        eng.forecast_gangs_launch(members, [0, 2], inst)
        assert L.kt_forecast_gangs_fetch(eng._h, 1, None, None, None) == 0
        assert _code(lambda: eng.forecast_gangs_fetch(2, len(inst))) == -2  # more gangs than the launch had
    finally:
        eng.close()
        inc.close()


def _stored_readback(eng, rows):
    """What reads the stored status quantitatively: the headroom query (see tests/test_preempt_gpu.py)."""
    out = []
    for eq in (False, True):
        out += list(eng.headroom(rows, cap=E.HEADROOM_MAX_CAP, on_equal=eq))
    return out


def test_slot_rules_and_dry_run(oracle_mod):
    snap, gangs, want, _ = FG.cluster_reference(SEEDS[0], oracle_mod)
    rows, off = _queue(gangs)
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    eng = E.Engine.for_snapshot(snap)
    try:
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = _stored_readback(eng, everyone)
        res_before = eng.fetch_reserved()
        plain = eng.reconcile(NOW, apply=False)
        # the launch takes the check slot and the reconcile result buffers
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        eng.forecast_gangs_launch(rows, off, FR.INSTANTS)
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == -5
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves the forecast fetchable
        eng.aggregate_launch()
        eng.forecast_gangs_launch(rows, off, FR.INSTANTS)
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        verdicts = eng.forecast_gangs_fetch(len(gangs), len(FR.INSTANTS))[1]
        assert verdicts.tolist() == [w[1] for w in want[False]]
        # a later user of the check slot drops it
        eng.forecast_gangs_launch(rows, off, FR.INSTANTS)
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.forecast_gangs_fetch(len(gangs), len(FR.INSTANTS))) == -5
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        res_after = eng.fetch_reserved()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, _stored_readback(eng, everyone)))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()
