"""The elastic gang forecast on the GPU: Engine.forecast_gangs_elastic (kt_forecast_gangs_elastic_launch / _fetch,
csrc/kt_kernels_forecast_gangs_elastic.hip) against the reference of tests/forecast_gangs_elastic_reference.py (per instant: a copy
of the snapshot, the oracle's reconcile, the oracle's in-order admission of the members, then the rule) — verdict bytes, first
position, member counts and blockers compared bit for bit — and against the identities of the header on the same engine.  The shapes
are the smallest at which the kernel can still go wrong: instant counts around 64 (the follow-up launch's ballot), 70 members with the
deciding one around position 64, a union beyond the LDS capacity (by the hook and by itself), a deciding throttle in the second chunk
of the list, one case per DT instantiation, more (gang, instant) pairs than the grid has workgroups."""
import os

import numpy as np
import pytest

import forecast_gangs_elastic_reference as FE
import forecast_gangs_reference as FG
import forecast_reference as FR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S
from test_forecast_cpu import SEEDS

pytestmark = pytest.mark.gpu
NOW = FR.NOW
A, B, ERR = S.VERDICT_ALLOW, S.VERDICT_BLOCK, S.VERDICT_ERROR
HOOK = "KT_FORECAST_ELASTIC_LDS_CAP"


def _queue(gangs):
    rows = [int(p) for g in gangs for p in g]
    off = np.cumsum([0] + [len(g) for g in gangs]).astype(np.int64)
    return rows, off


def _flags(gangs, required):
    if required is None or all(r is None for r in required):
        return None
    return np.array([bool(x) for g, r in zip(gangs, required) for x in (r if r is not None else [False] * len(g))], bool)


def launch_all(eng, gangs, quorums, required, instants, on_equal=False):
    """All gangs in ONE launch -> per gang (first, verdicts, counts, blockers) with the blockers as positions inside the gang."""
    rows, off = _queue(gangs)
    first, verdicts, members, blockers = eng.forecast_gangs_elastic(rows, off, quorums, instants, _flags(gangs, required), on_equal)
    assert verdicts.shape == members.shape == blockers.shape == (len(gangs), len(instants)) and first.shape == (len(gangs),)
    out = []
    for g in range(len(gangs)):
        blk = [int(b) for b in blockers[g]]
        assert all(b == -1 or off[g] <= b < off[g + 1] for b in blk), (g, blk)
        out.append((int(first[g]), verdicts[g].tolist(), members[g].tolist(), [b if b < 0 else b - int(off[g]) for b in blk]))
    return out


def held_to_the_reference(snap, oracle_mod, members, quorum, required, instants, on_equal=False, eng=None):
    own = eng is None
    eng = eng or E.Engine.for_snapshot(snap)
    try:
        got, = launch_all(eng, [members], [quorum], [required], instants, on_equal)
    finally:
        if own:
            eng.close()
    want = FE.reference(snap, oracle_mod, members, quorum, required, instants, on_equal)
    assert got == want, f"{members} quorum {quorum} required {required} on_equal={on_equal}: {got} != {want}"
    return got


# ---- parity with the reference under the seeded rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", FG.STAIR_SEEDS)
def test_generator_a(seed, oracle_mod):
    snap, members, inst, quorum, required, want, _ = FE.stair_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            assert launch_all(eng, [members], [quorum], [required], inst, on_equal)[0] == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        eng.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_b(seed, oracle_mod):
    snap, gangs, quorums, required, want, _ = FE.cluster_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            assert launch_all(eng, gangs, quorums, required, FR.INSTANTS, on_equal) == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FE.DIRECTED))
def test_directed(name, oracle_mod):
    snap, members, quorum, required, inst = FE.DIRECTED[name]()
    for on_equal in (False, True):
        held_to_the_reference(snap, oracle_mod, members, quorum, required, inst, on_equal)


@pytest.mark.parametrize("build", [FE.failed_member_reserves_nowhere, FE.failed_member_reserves_nowhere_on_a_count])
def test_a_failed_member_reserves_on_no_throttle(build):
    """The answers derived by hand: m0 fails on A and therefore does not weigh on B, where m1 then passes."""
    snap = build()
    eng = E.Engine.for_snapshot(snap)
    try:
        for name, (members, quorum, required, want) in FE.NOWHERE.items():
            assert launch_all(eng, [members], [quorum], [required], FE.EDGE) == [want], name
        # all three rules in one launch, the gangs sharing their pods
        got = launch_all(eng, [m for m, _, _, _ in FE.NOWHERE.values()], [q for _, q, _, _ in FE.NOWHERE.values()],
                         [r for _, _, r, _ in FE.NOWHERE.values()], FE.EDGE)
        assert got == [w for _, _, _, w in FE.NOWHERE.values()]
    finally:
        eng.close()


# ---- the identities, on the same engine ----------------------------------------------------------------------------------------
def _is_the_whole_gang(eng, gangs, instants, on_equal, quorums_when_all_required):
    """(E1), both forms: byte for byte kt_forecast_gangs_launch's first, verdicts and blocker."""
    rows, off = _queue(gangs)
    first, verdicts, blockers = eng.forecast_gangs(rows, off, instants, on_equal)
    sizes = np.diff(off)
    for quorums, req in ((sizes, None), (quorums_when_all_required, np.ones(len(rows), bool))):
        efirst, everdicts, emembers, eblockers = eng.forecast_gangs_elastic(rows, off, quorums, instants, req, on_equal)
        assert efirst.tobytes() == first.tobytes() and everdicts.tobytes() == verdicts.tobytes() and eblockers.tobytes() == blockers.tobytes()
        assert np.array_equal(emembers == sizes[:, None], verdicts == A)


@pytest.mark.parametrize("seed", SEEDS)
def test_e1_generator_b(seed, oracle_mod):
    snap, gangs, _, _ = FG.cluster_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            _is_the_whole_gang(eng, gangs, FR.INSTANTS, on_equal, [1 + (seed + g) % len(m) for g, m in enumerate(gangs)])
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FG.DIRECTED))
def test_e1_directed(name):
    snap, members, inst = FG.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            _is_the_whole_gang(eng, [members], inst, on_equal, [1])
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FR.DIRECTED))
def test_e2_a_gang_of_one_is_the_plain_forecast(name):
    snap, p, inst = FR.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            first, verdicts = eng.forecast([p], inst, on_equal)
            efirst, everdicts, emembers, eblockers = eng.forecast_gangs_elastic([p], [0, 1], [1], inst, None, on_equal)
            assert efirst.tobytes() == first.tobytes() and everdicts.tobytes() == verdicts.tobytes()
            assert emembers[0].tolist() == [int(v == A) for v in verdicts[0]]
            assert eblockers[0].tolist() == [-1 if v == A else 0 for v in verdicts[0]]
    finally:
        eng.close()


@pytest.mark.parametrize("seed", [0, 3, 7, 11, 19, 42])
def test_e3_a_dry_elastic_admission_in_the_state_of_the_instant(seed, oracle_mod):
    """A second engine loaded with R_t: a dry kt_admit_gangs_elastic_launch of the gang keeps members exactly where the forecast's
    verdict at t is Success, and then the same number."""
    snap, members, inst, quorum, required, _, _ = FE.stair_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for k in (0, 2, len(inst) - 1):
            for on_equal in (False, True):
                (first, verdicts, counts, _), = launch_all(eng, [members], [quorum], [required], [inst[k]], on_equal)
                at_t = E.Engine.for_snapshot(FR.state_at(snap, oracle_mod, inst[k]))
                try:
                    _, _, kept = at_t.admit_gangs_elastic(np.array(members, np.int64), [0, len(members)], [quorum], np.array(required, bool),
                                                          on_equal=on_equal, commit=False)
                finally:
                    at_t.close()
                assert (int(kept[0]) > 0) == (verdicts[0] == A), (seed, k, on_equal)
                assert int(kept[0]) == (counts[0] if verdicts[0] == A else 0)
    finally:
        eng.close()


# ---- the smallest shapes at which the kernel can go wrong ----------------------------------------------------------------------
def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


@pytest.mark.parametrize("m,lo,hi", [(1, 0, 0), (1, None, None), (63, 62, 62), (64, 63, 63), (65, 64, 64), (65, 63, 64), (130, 128, 129),
                                     (130, None, None)])
def test_instant_blocks_and_the_ballot(m, lo, hi, oracle_mod):
    """The example's two-member gang (4 + 3 + 3 > 8) with the quorum 2; the override 10 is active over positions lo .. hi."""
    inst = _seconds(m)
    ovr = [(inst[lo], inst[hi], {0: 10}, None)] if lo is not None else [(FR.shift(inst[-1], 1), None, {0: 10}, None)]
    snap = FR.timed(PR.tiny([{0: 3}, {0: 3}, {0: 4}], {0: 8}, flags=FG.P2C1), 0, ovr)
    first, verdicts, counts, blockers = held_to_the_reference(snap, oracle_mod, [0, 1], 2, None, inst)
    inside = [lo is not None and lo <= k <= hi for k in range(m)]
    assert first == (lo if lo is not None else -1)
    assert verdicts == [A if x else B for x in inside] and counts == [2 if x else 1 for x in inside]
    assert blockers == [-1 if x else 1 for x in inside]


@pytest.mark.parametrize("pos", [63, 64, 65])
def test_seventy_members_a_required_invalid_one(pos, oracle_mod):
    """Inside the window (50) member 50 is the first that fails, but the blocker is the required member that never succeeds."""
    n = 70
    snap = FR.timed(PR.tiny([{0: 1}] * n, {0: 1000}, flags=[PR.PENDING] * n), 0, [(FR.T1, FR.T2, {0: 50}, None)])
    snap.pod_flags[pos] = 0
    required = [j == pos for j in range(n)]
    first, verdicts, counts, blockers = held_to_the_reference(snap, oracle_mod, list(range(n)), 1, required, FR.EDGE)
    assert first == -1 and verdicts == [ERR] * 9 and blockers == [pos] * 9 and counts == [69, 69, 50, 50, 50, 50, 69, 69, 69]
    # ... not required, under a quorum it does not put out of reach: the first member that fails
    first, verdicts, counts, blockers = held_to_the_reference(snap, oracle_mod, list(range(n)), 60, None, FR.EDGE)
    assert first == 0 and verdicts == [A, A, B, B, B, B, A, A, A] and blockers == [-1, -1, 50, 50, 50, 50, -1, -1, -1]


@pytest.mark.parametrize("pos", [63, 64, 65])
def test_seventy_members_the_quorum_deciding_one(pos, oracle_mod):
    """A pod count of ``pos`` admits members 0 .. pos - 1, the override one more: the quorum pos + 1 is met inside the window only."""
    n = 70
    snap = FR.timed(PR.tiny([{0: 1}] * n, {}, count=pos, flags=[PR.PENDING] * n), 0, [(FR.T1, FR.T2, {}, pos + 1)])
    first, verdicts, counts, blockers = held_to_the_reference(snap, oracle_mod, list(range(n)), pos + 1, None, FR.EDGE)
    assert first == 2 and verdicts == FE._by_window(A, B) and counts == FE._by_window(pos + 1, pos) and blockers == FE._by_window(-1, pos)


def _many_throttles(T):
    """T throttles affect both members of the example's gang; only the last row's override lets the second one through."""
    snap = PR.tiny([{0: 3}, {0: 3}, {0: 4}], {0: 8}, flags=FG.P2C1, T=T, row=T - 1)
    for t in range(T - 1):
        snap.thr_ns[t] = 0
        snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    return FR.timed(snap, T - 1, [(FR.T1, FR.T2, {0: 10}, None)])


def test_a_union_beyond_the_lds_capacity_by_the_hook(oracle_mod):
    """KT_FORECAST_ELASTIC_LDS_CAP (read when the engine is created and on kt_debug_reload_env) lowers the entries LDS holds: the
    union of 20 throttles then lives in the engine's workspace — same code, same answers."""
    snap = _many_throttles(20)
    cases = [([0, 1], 2, None), ([0, 1], 1, None), ([1, 0], 1, [False, True])]
    ask = lambda eng: [held_to_the_reference(snap, oracle_mod, m, q, r, FR.EDGE, eng=eng) for m, q, r in cases]
    plain = E.Engine.for_snapshot(snap)
    try:
        in_lds = ask(plain)
    finally:
        plain.close()
    assert in_lds[0][:2] == (2, FE._by_window(A, B)) and in_lds[1][2] == FE._by_window(2, 1)
    assert HOOK not in os.environ
    os.environ[HOOK] = "16"
    try:
        eng = E.Engine.for_snapshot(snap)
    finally:
        del os.environ[HOOK]
    try:
        in_hbm = ask(eng)
        again = ask(eng)  # the workspace is reused
        eng.reload_env()  # the switch is gone: back in LDS
        back = ask(eng)
    finally:
        eng.close()
    assert in_hbm == in_lds and again == in_lds and back == in_lds


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect both members — more than one chunk of the LDS list holds, and more than the LDS state: the union lives
    in the workspace without any hook."""
    snap = _many_throttles(1030)
    first, verdicts, counts, blockers = held_to_the_reference(snap, oracle_mod, [0, 1], 2, None, FR.EDGE[:8])
    assert first == 2 and verdicts == [B, B, A, A, A, A, B, B] and blockers == [1, 1, -1, -1, -1, -1, 1, 1] and counts == [1, 1, 2, 2, 2, 2, 1, 1]
    assert held_to_the_reference(snap, oracle_mod, [0, 1], 1, None, FR.EDGE[:8])[:2] == (0, [A] * 8)


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
        got = held_to_the_reference(snap, oracle_mod, [0, 1], 2, None, FR.EDGE + [FR.shift(FR.T4, 1)], on_equal)
        assert got[0] == (-1 if on_equal else 2)
        held_to_the_reference(snap, oracle_mod, [1, 0], 1, [True, False], FR.EDGE + [FR.shift(FR.T4, 1)], on_equal)


def test_more_pairs_than_the_grid_has_workgroups(oracle_mod):
    """230 two-member gangs x 9 instants = 2070 pairs in one launch: the grid strides beyond 2048, and first[g] is still the
    smallest passing position.  Pods are shared between the gangs."""
    asks = [1, 2, 3, 4, 5, 3]
    snap = FR.timed(PR.tiny([{0: a} for a in asks] + [{0: 4}], {0: 10}, count=3, flags=[PR.PENDING] * 6 + [PR.COUNTED]), 0,
                    [(FR.T1, FR.T2, {0: 12}, None), (FR.T3, FR.T4, {0: 9}, 2)])
    pairs = [[i, j] for i in range(6) for j in range(6) if i != j]
    rule_of = lambda k: (1 + k % 2, [k % 3 == 0, k % 5 == 0])
    gangs = [pairs[(7 * k) % len(pairs)] for k in range(230)]
    want = {}
    for k, g in enumerate(gangs):
        key = (tuple(g), k % 2, k % 3 == 0, k % 5 == 0)
        if key not in want:
            want[key] = FE.reference(snap, oracle_mod, g, *rule_of(k), FR.EDGE)
    assert len({w[0] for w in want.values()}) >= 3  # the gangs differ in their answers
    eng = E.Engine.for_snapshot(snap)
    try:
        got = launch_all(eng, gangs, [rule_of(k)[0] for k in range(230)], [rule_of(k)[1] for k in range(230)], FR.EDGE)
    finally:
        eng.close()
    for k, g in enumerate(gangs):
        assert got[k] == want[(tuple(g), k % 2, k % 3 == 0, k % 5 == 0)], f"gang {k} {g}"
        assert got[k][0] == FR.first_of([got[k][1]])[0]


# ---- validation, slots, dry run ------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    return ei.value.code


def _refused(eng, fn, code, *words):
    assert _code(fn) == code
    msg = E.lib().kt_last_error(eng._h).decode()
    assert all(w in msg for w in words), msg


def test_validation_in_order_and_what_a_refused_call_leaves_alone(oracle_mod):
    snap = FE.failed_member_reserves_nowhere()
    members, inst = [0, 1, 2], FE.EDGE
    want = FE.NOWHERE["quorum-1-m1-required"][3]
    whole_want = FG.reference(snap, oracle_mod, members, inst)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    fe = eng.forecast_gangs_elastic
    rows, off, mm = np.array(members, np.int64), np.array([0, 3], np.int64), np.array([1], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data

    def raw(n=3, r=rows, ng=1, o=off, q=mm, f=None, m=2, s=s2, ns=n2):
        return L.kt_forecast_gangs_elastic_launch(eng._h, n, ptr(r), ng, ptr(o), ptr(q), ptr(f), m, ptr(s), ptr(ns), 0, None)

    def every_refusal():
        # (1) the instants come first: even with broken offsets and a broken rule
        _refused(eng, lambda: fe(members, [0, 2], [9], []), -1, "n_inst")
        _refused(eng, lambda: fe(members, [0, 3], [9], [FR.T1, FR.T1]), -1, "strictly ascending")
        _refused(eng, lambda: fe(members, [0, 3], [1], [(NOW[0], 1_000_000_000)]), -1, "inst_ns")
        assert raw(r=None) == -1 and raw(s=None) == -1 and raw(ns=None) == -1
        assert raw(n=-1) == -1 and raw(ng=-1) == -1
        # (2) every gang_off defect, before the rule is looked at
        assert raw(o=None, q=None) == -1 and "gang_off" in L.kt_last_error(eng._h).decode()
        _refused(eng, lambda: fe(members, [1, 3], [9], inst), -1, "gang_off[0]")
        _refused(eng, lambda: fe(members, [0, 0, 3], [9, 9], inst), -1, "empty")
        _refused(eng, lambda: fe(members, [0, 3, 1], [9, 9], inst), -1, "below")
        _refused(eng, lambda: fe(members, [0, 2], [9], inst), -1, "not n")
        assert raw(ng=0) == -1
        # (3) the rule, with the admission's codes and messages, before "a pod twice" and the rows
        assert raw(q=None) == -1 and "min_members is NULL" in L.kt_last_error(eng._h).decode()
        _refused(eng, lambda: fe([0, 1, 0], [0, 3], [0], inst), -1, "min_members[0] = 0 of gang 0 is outside [1, 3]")
        _refused(eng, lambda: fe([0, 99, 99], [0, 3], [4], inst), -1, "min_members[0] = 4 of gang 0 is outside [1, 3]")
        _refused(eng, lambda: fe([0, 1, 0], [0, 3], [1], inst, np.array([0, 2, 0], np.uint8)), -1, "member_flags[1] = 0x02", "queue position 1")
        # (4) the rest of the gang forecast's list, in its order
        _refused(eng, lambda: fe([0, 1, 0], [0, 3], [1], inst), -1, "twice")
        _refused(eng, lambda: fe([0, 99, 99], [0, 3], [1], inst), -1, "twice")                     # ... asked before the range
        _refused(eng, lambda: fe([0, 99], [0, 2], [1], inst), -2, "pod row 99")
        many = np.zeros(2**16 + 1, np.int64)
        assert _code(lambda: fe(many, np.arange(2**16 + 2), np.ones(2**16 + 1, np.int64), _seconds(2**15))) == -2  # n_gangs x n_inst > 2^31
        eng.set_exchange_world(2)
        assert _code(lambda: fe(members, [0, 3], [1], inst)) == -7                                 # KT_ERR_UNSUPPORTED
        eng.set_exchange_world(1)
        eng.set_wide_sums(1)
        assert _code(lambda: fe(members, [0, 3], [1], inst)) == -7                                 # `used` wider than int64
        eng.set_wide_sums(0)

    def pending_elastic():
        got = eng.forecast_gangs_elastic_fetch(1, len(inst))
        return int(got[0][0]), got[1][0].tolist(), got[2][0].tolist(), got[3][0].tolist()

    try:
        assert _code(lambda: eng.forecast_gangs_elastic_fetch(1, len(inst))) == -5  # KT_ERR_NOT_READY
        # a refused call leaves a pending elastic forecast fetchable ...
        eng.forecast_gangs_elastic_launch(members, [0, 3], [1], inst, [False, True, False])
        every_refusal()
        assert pending_elastic() == want
        # ... and a pending forecast of another kind, a pending check and a pending reconcile report
        eng.forecast_gangs_launch(members, [0, 3], inst)
        every_refusal()
        got = eng.forecast_gangs_fetch(1, len(inst))
        assert (int(got[0][0]), got[1][0].tolist(), got[2][0].tolist()) == whole_want
        eng.reconcile_launch(NOW, apply=False)
        eng.check_launch(snap.n_pods, want_status=True)
        every_refusal()
        eng.check_fetch(snap.n_pods, True)
        eng.reconcile_fetch()
        assert _code(lambda: inc.forecast_gangs_elastic(members, [0, 3], [1], inst)) == -7
        # the one pending forecast result is shared by five kinds: the last launch decides which fetch may read it
        others = {
            "pods": (lambda: eng.forecast_launch(members, inst), lambda: eng.forecast_fetch(3, len(inst))),
            "gangs": (lambda: eng.forecast_gangs_launch(members, [0, 3], inst), lambda: eng.forecast_gangs_fetch(1, len(inst))),
            "headroom": (lambda: eng.headroom_forecast_launch(members, inst, 4), lambda: eng.headroom_forecast_fetch(3, len(inst))),
        }
        for kind, (launch, fetch) in others.items():
            launch()
            assert _code(lambda: eng.forecast_gangs_elastic_fetch(1, len(inst))) == -5, kind
            fetch()
            eng.forecast_gangs_elastic_launch(members, [0, 3], [1], inst, [False, True, False])
            assert _code(fetch) == -5, kind
            assert pending_elastic() == want
        # n == 0 with n_gangs == 0: KT_OK, nothing launched
        eng.forecast_gangs_elastic_launch([], [0], [], inst)
        assert eng.forecast_gangs_elastic_fetch(0, len(inst))[0].tolist() == []
        assert _code(lambda: eng.forecast_gangs_fetch(0, len(inst))) == -5
        # nullable outputs
        first, none, members_out, blockers = fe(members, [0, 3], [1], inst, [False, True, False], want_verdicts=False)
        assert none is None and int(first[0]) == want[0] and members_out[0].tolist() == want[2] and blockers[0].tolist() == want[3]
        first, verdicts, none, nil = fe(members, [0, 3], [1], inst, [False, True, False], want_members=False, want_blocker=False)
        assert none is None and nil is None and verdicts[0].tolist() == want[1]
        eng.forecast_gangs_elastic_launch(members, [0, 3], [1], inst)
        assert L.kt_forecast_gangs_elastic_fetch(eng._h, 1, None, None, None, None) == 0
        assert _code(lambda: eng.forecast_gangs_elastic_fetch(2, len(inst))) == -2  # more gangs than the launch had
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
    snap, gangs, quorums, required, want, _ = FE.cluster_reference(SEEDS[0], oracle_mod)
    rows, off = _queue(gangs)
    req = _flags(gangs, required)
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    eng = E.Engine.for_snapshot(snap)
    launch = lambda: eng.forecast_gangs_elastic_launch(rows, off, quorums, FR.INSTANTS, req)
    try:
        before = [eng.check(rows=everyone, on_equal=eq)[0].copy() for eq in (False, True)]
        room_before = _stored_readback(eng, everyone)
        res_before = eng.fetch_reserved()
        plain = eng.reconcile(NOW, apply=False)
        # the launch takes the check slot and the reconcile result buffers
        eng.check_launch(snap.n_pods, want_status=True)
        eng.reconcile_launch(NOW, apply=False)
        launch()
        assert _code(lambda: eng.check_fetch(snap.n_pods, True)) == -5
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves the forecast fetchable
        eng.aggregate_launch()
        launch()
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        _, verdicts, members, _ = eng.forecast_gangs_elastic_fetch(len(gangs), len(FR.INSTANTS))
        assert verdicts.tolist() == [w[1] for w in want[False]] and members.tolist() == [w[2] for w in want[False]]
        # a pending preempt result stays fetchable behind the launch
        prefix = eng.preempt_gangs(rows, off, [], NOW)
        eng.preempt_gangs_launch(rows, off, [], NOW)
        launch()
        again = eng.preempt_gangs_fetch(len(gangs), 0)
        assert np.array_equal(again[0], prefix[0]) and np.array_equal(again[2], prefix[2])
        # a later user of the check slot drops it
        launch()
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.forecast_gangs_elastic_fetch(len(gangs), len(FR.INSTANTS))) == -5
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        res_after = eng.fetch_reserved()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, _stored_readback(eng, everyone)))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()


def test_host_plugin_retry_after_elastic_gang():
    """The C++ plugin mirror's driver (tests/cpp/host_plugin_retry_after_elastic_gang_test.cpp) holds RetryAfterElasticGang to a twin
    plugin per judged instant; here the lines it prints are held to Engine.forecast_gangs_elastic on the same scenario written as
    manifests, over now ++ ``paging.override_instants_of``."""
    import re
    import subprocess
    from kube_throttler_amd import paging
    from kube_throttler_amd.objects import ClusterState
    from kube_throttler_amd.quantity import parse_rfc3339
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kube_throttler_amd", "host")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", host, "host_plugin_retry_after_elastic_gang_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "host_plugin_retry_after_elastic_gang_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    lines = re.findall(r"^RETRYELASTIC (\S+) (\d+) (\S+) (\d+) -> (\S+) (\d+) (\S+) (\S+)$", r.stdout, re.M)
    assert len(lines) == 7
    cs = ClusterState()
    cs.add_namespace("ns1", {})
    for name, app in (("m0", "a"), ("m1", "b"), ("m2", "b")):
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns1", "labels": {"app": app, "tier": "x"}},
                "spec": {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": "6"}}}]},
                "status": {"phase": "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "lead", "namespace": "ns1"},
            "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}}]},
                     "threshold": {"resourceRequests": {"cpu": "5"}},
                     "temporaryThresholdOverrides": [{"begin": "2026-01-01T22:00:00Z", "end": "2026-01-02T06:00:00Z",
                                                      "threshold": {"resourceRequests": {"cpu": "100"}}}]}})
    cs.add({"kind": "Throttle", "metadata": {"name": "tier", "namespace": "ns1"},
            "spec": {"throttlerName": "kube-throttler", "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"tier": "x"}}}]},
                     "threshold": {"resourceRequests": {"cpu": "10"}}}})
    names = [p["metadata"]["name"] for p in cs.pods]
    snap = cs.build_pages()[0].snapshot
    now = parse_rfc3339("2026-01-01T12:00:00Z")
    eng = E.Engine.for_snapshot(snap)
    try:
        for members, quorum, req, horizon, got, digits, counts, blockers in lines:
            members = members.split("+")
            instants = [now] + paging.override_instants_of(snap, now, (now[0] + int(horizon), now[1]))
            required = None if req == "-" else [c == "1" for c in req]
            (first, verdicts, cnt, blk), = launch_all(eng, [[names.index(m) for m in members]], [int(quorum)], [required], instants)
            what = f"{members} quorum {quorum} required {req} over {horizon} s"
            assert digits == "".join(str(v) for v in verdicts), what
            assert counts == ",".join(str(c) for c in cnt), what
            assert blockers == ",".join("-" if b < 0 else members[b] for b in blk), what
            assert (None if got == "never" else parse_rfc3339(got)) == (instants[first] if first >= 0 else None), what
    finally:
        eng.close()
    by = {(m, int(q), rq): (got, digits, counts, blockers) for m, q, rq, h, got, digits, counts, blockers in lines if int(h) == 86400}
    assert by[("m0+m1+m2", 1, "-")] == ("2026-01-01T12:00:00Z", "000", "1,1,1", "-,-,-")
    assert by[("m0+m1+m2", 1, "010")] == ("2026-01-01T12:00:00Z", "010", "1,1,1", "-,m1,-")
    assert by[("m0+m1+m2", 2, "-")] == ("never", "111", "1,1,1", "m0,m1,m0")


def test_the_gang_forecast_is_what_it_was_after_elastic_launches(oracle_mod):
    """(Passes with or without the feature's kernel being right.)  kt_forecast_gangs shares buffers with the elastic call: behind
    elastic launches it still answers its reference."""
    snap, gangs, want, _ = FG.cluster_reference(SEEDS[1], oracle_mod)
    rows, off = _queue(gangs)
    eng = E.Engine.for_snapshot(snap)
    try:
        before = eng.forecast_gangs(rows, off, FR.INSTANTS)
        eng.forecast_gangs_elastic(rows, off, np.ones(len(gangs), np.int64), FR.INSTANTS)
        eng.forecast_gangs_elastic(rows, off, np.diff(off), FR.INSTANTS[:3], np.ones(len(rows), bool), True)
        after = eng.forecast_gangs(rows, off, FR.INSTANTS)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
        assert [(int(f), v.tolist(), [b if b < 0 else b - int(off[g]) for b in blk.tolist()])
                for g, (f, v, blk) in enumerate(zip(*after))] == want[False]
    finally:
        eng.close()
