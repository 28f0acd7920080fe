"""The elastic gang preemption query on the GPU: Engine.preempt_gangs_elastic (kt_preempt_gangs_elastic_launch / _fetch,
csrc/kt_kernels_preempt_gangs_elastic.hip) against the reference of tests/preempt_gangs_elastic_reference.py (per k: delete the
prefix, reconcile and admit the members in order with the oracle, then the rule; the reprieve as its definition) — prefix, victim
bytes, member count and blocker compared bit for bit, with and without KT_PREEMPT_REPRIEVE — against ``paging.preempt_gangs_elastic_of``
and against the identities of the header on the same engine.  The shapes are the smallest at which the kernel can still go wrong:
candidate counts around the blocks of 64 victim bytes with the deciding candidate at a block's edge, 70 members with the deciding one
around position 64, a union of more than 64 entries, a union beyond the LDS capacity (by the hook and by itself), a deciding throttle
in the second chunk of the list, one case per DT instantiation, more gangs than the grid has workgroups."""
import os

import numpy as np
import pytest

import preempt_gangs_elastic_reference as ER
import preempt_gangs_reference as GR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from test_preempt_cpu import SEEDS
from test_preempt_gangs_cpu import gang_case

pytestmark = pytest.mark.gpu
NOW = PR.NOW
NONE = ER.NONE
P, C = PR.PENDING, PR.COUNTED
HOOK = "KT_PREEMPT_ELASTIC_LDS_CAP"


def _queue(gangs):
    rows = [int(p) for g in gangs for p in g]
    off = np.cumsum([0] + [len(g) for g in gangs]).astype(np.int64)
    return rows, off


def _flags(gangs, required):
    if required is None or all(r is None for r in required):
        return None
    return np.array([bool(x) for g, r in zip(gangs, required) for x in (r if r is not None else [False] * len(g))], bool)


def launch_all(eng, gangs, quorums, required, cands, on_equal=False, reprieve=False):
    """All gangs in ONE launch -> per gang (prefix, victims, members, blocker as a position inside the gang)."""
    rows, off = _queue(gangs)
    prefix, victims, members, blocker = eng.preempt_gangs_elastic(rows, off, quorums, cands, NOW, _flags(gangs, required), on_equal, reprieve)
    assert victims.shape == (len(gangs), len(cands)) and prefix.shape == members.shape == blocker.shape == (len(gangs),)
    out = []
    for g in range(len(gangs)):
        b = int(blocker[g])
        assert b == -1 or off[g] <= b < off[g + 1], (g, b)
        out.append((int(prefix[g]), victims[g].tolist(), int(members[g]), b if b < 0 else b - int(off[g])))
    return out


def _plain(w):
    return (w.prefix, w.victims, w.members, w.blocker)


def _reprieved(w):
    return (w.prefix, w.reprieved, w.reprieved_members, w.blocker)


def held_to_the_reference(snap, oracle_mod, members, quorum, required, cands, eng=None, want=None):
    """Both on_equal values, with and without the flag -> {on_equal: Answer}, the reference's."""
    want = want or ER.reference(snap, oracle_mod, members, quorum, required, cands)
    own = eng is None
    eng = eng or E.Engine.for_snapshot(snap)
    try:
        for eq in (False, True):
            what = f"{members} quorum {quorum} required {required} over {cands} on_equal={eq}"
            got, = launch_all(eng, [members], [quorum], [required], cands, eq)
            assert got == _plain(want[eq]), f"{what}: {got} != {want[eq]}"
            got, = launch_all(eng, [members], [quorum], [required], cands, eq, reprieve=True)
            assert got == _reprieved(want[eq]), f"{what} reprieved: {got} != {want[eq]}"
    finally:
        if own:
            eng.close()
    return want


# ---- parity with the reference under the seeded rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_clusters(seed, oracle_mod):
    snap, ruled, want, _ = ER.seeded_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for (ms, cands, quorum, required), w in zip(ruled, want):  # the cases of the CPU suite, each over its own list
            held_to_the_reference(snap, oracle_mod, ms, quorum, required, cands, eng=eng, want=w)
        # all gangs of the seed in one launch over ONE list (the longest case's, without any gang's members), against the model the
        # CPU suite holds to the reference
        gangs = [ms for ms, _, _, _ in ruled]
        everyone = {p for ms in gangs for p in ms}
        cands = [c for c in max((cs for _, cs, _, _ in ruled), key=len) if c not in everyone]
        ctx = paging.preempt_context(snap, NOW)
        for eq in (False, True):
            for reprieve in (False, True):
                got = launch_all(eng, gangs, [q for _, _, q, _ in ruled], [r for _, _, _, r in ruled], cands, eq, reprieve)
                for g, (ms, _, quorum, required) in enumerate(ruled):
                    model = paging.preempt_gangs_elastic_of(snap, ms, quorum, required, cands, NOW, eq, ctx=ctx, reprieve=reprieve)
                    assert got[g] == model, f"seed {seed} gang {g} on_equal={eq} reprieve={reprieve}: {got[g]} != {model}"
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(ER.directed_cases()))
def test_directed(name, oracle_mod):
    snap, members, quorum, required, cands = ER.directed_cases()[name]()
    want = held_to_the_reference(snap, oracle_mod, members, quorum, required, cands)
    if name in ER.HAND:
        table = ER.HAND[name][4]
        for eq in (False, True):
            assert _plain(want[eq]) + (want[eq].reprieved, want[eq].reprieved_members) == table[eq]


# ---- the identities, on the same engine ----------------------------------------------------------------------------------------
def _is_the_whole_gang(eng, snap, oracle_mod, gangs, cands, on_equal, quorums_when_all_required):
    """(P1), both forms, with and without the flag: byte for byte the gang query's prefix and victims."""
    rows, off = _queue(gangs)
    sizes = np.diff(off)
    ok = [GR.members_ok(snap, oracle_mod, ms) for ms in gangs]
    for reprieve in (False, True):
        prefix, victims, blocker = eng.preempt_gangs(rows, off, cands, NOW, on_equal, reprieve=reprieve)
        for quorums, req in ((sizes, None), (quorums_when_all_required, np.ones(len(rows), bool))):
            eprefix, evictims, emembers, eblocker = eng.preempt_gangs_elastic(rows, off, quorums, cands, NOW, req, on_equal, reprieve)
            assert eprefix.tobytes() == prefix.tobytes() and evictims.tobytes() == victims.tobytes(), (reprieve, eprefix, prefix)
            assert all(int(emembers[g]) == sizes[g] for g in range(len(gangs)) if prefix[g] >= 0)
            assert all(int(eblocker[g]) == int(blocker[g]) for g in range(len(gangs)) if ok[g]), (eblocker, blocker)


@pytest.mark.parametrize("seed", SEEDS[::2])
def test_p1_seeded_clusters(seed, oracle_mod):
    snap, cases, _, _ = gang_case(seed, oracle_mod)
    gangs = [ms for ms, _ in cases]
    everyone = {p for ms in gangs for p in ms}
    cands = [c for c in max((cs for _, cs in cases), key=len) if c not in everyone]
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            _is_the_whole_gang(eng, snap, oracle_mod, gangs, cands, on_equal, [1 + (seed + g) % len(m) for g, m in enumerate(gangs)])
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(GR.DIRECTED))
def test_p1_directed(name, oracle_mod):
    snap, ms, cands = GR.DIRECTED[name][0]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            _is_the_whole_gang(eng, snap, oracle_mod, [ms], cands, on_equal, [1])
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(PR.DIRECTED))
def test_p2_a_gang_of_one_is_the_single_query(name):
    snap, p, cands = PR.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            for reprieve in (False, True):
                prefix, victims = eng.preempt([p], cands, NOW, on_equal, reprieve=reprieve)
                eprefix, evictims, emembers, eblocker = eng.preempt_gangs_elastic([p], [0, 1], [1], cands, NOW, None, on_equal, reprieve)
                assert eprefix.tobytes() == prefix.tobytes() and evictims.tobytes() == victims.tobytes(), (name, on_equal, reprieve)
                assert int(emembers[0]) == int(prefix[0] >= 0) and int(eblocker[0]) == (-1 if prefix[0] == 0 else 0)
    finally:
        eng.close()


@pytest.mark.parametrize("seed", [1, 18, 19, 22, 23, 31])  # (seeds of SEEDS whose cases have positive prefixes and reprieves that shrink them)
def test_p3_a_dry_elastic_admission_without_the_final_victims(seed, oracle_mod):
    """A second engine that holds the cluster without the final victims, reconciled at `now` with apply: a dry
    kt_admit_gangs_elastic_launch of the gang keeps exactly out_members members."""
    snap, ruled, _, _ = ER.seeded_reference(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    asked = 0
    try:
        for ms, cands, quorum, required in ruled:
            for on_equal, reprieve in ((False, False), (True, True)):
                (prefix, victims, members, _), = launch_all(eng, [ms], [quorum], [required], cands, on_equal, reprieve)
                if prefix < 0:
                    continue
                without = PR.copy_snapshot(snap)
                for c, v in zip(cands, victims):
                    if v:
                        without.pod_flags[int(c)] = 0
                twin = E.Engine.for_snapshot(without)
                try:
                    twin.reconcile(NOW, apply=True)
                    _, _, kept = twin.admit_gangs_elastic(np.array(ms, np.int64), [0, len(ms)], [quorum], np.array(required, bool),
                                                          on_equal=on_equal, commit=False)
                finally:
                    twin.close()
                assert int(kept[0]) == members, (seed, ms, cands, on_equal, reprieve, prefix, victims)
                asked += 1
    finally:
        eng.close()
    assert asked >= 4, asked


# ---- the smallest shapes at which the kernel can go wrong ----------------------------------------------------------------------
def elastic_line(m, k_star, D=2, dim=0, **kw):
    """Member 0 (required) asks 1 of ``dim``, member 1 asks more than any threshold; candidates 2 .. m + 1 run with 1 of ``dim`` each
    (and 2 of every other name, which the threshold does not name), but the candidate in the middle of the first k_star is finished
    and counts nowhere: exactly k_star candidates have to go before member 0 fits -> (snapshot, members, candidates)."""
    other = {d: 2 for d in range(D) if d != dim}
    running = dict(other)
    running[dim] = 1
    flags = [P, P] + [C] * m
    idle = k_star // 2 if k_star >= 2 else None
    if idle is not None:
        flags[2 + idle] = C | S.POD_FINISHED
    threshold = m - k_star + 1  # `used` behind the prefix, and member 0's one
    snap = PR.tiny([{dim: 1}, {dim: 1 << 20}] + [running] * m, {dim: threshold}, flags=flags, D=D, **kw)
    return snap, [0, 1], list(range(2, m + 2))


@pytest.mark.parametrize("m,k_star", [(0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (130, 129), (130, 130)])
def test_candidate_blocks_and_the_deciding_candidate(m, k_star, oracle_mod):
    """The deciding candidate at list position 0, 62, 63, 64, 128 and 129; a candidate that is not counted below it."""
    snap, ms, cands = elastic_line(m, k_star)
    want = held_to_the_reference(snap, oracle_mod, ms, 1, [True, False], cands)
    for eq in (False, True):
        assert want[eq].prefix == (k_star if not eq else NONE if k_star == m else k_star + 1), (eq, want[eq].prefix)
    if k_star >= 2:
        assert want[False].victims[k_star // 2] == 0 and sum(want[False].victims) == k_star - 1
        assert want[False].reprieved == want[False].victims  # every counted one of them is needed


def test_no_candidates(oracle_mod):
    snap, ms, _ = elastic_line(3, 2)
    want = held_to_the_reference(snap, oracle_mod, ms, 1, [True, False], [])
    assert _plain(want[False]) == (NONE, [], 0, 0)
    want = held_to_the_reference(snap, oracle_mod, ms, 1, None, [])
    assert _plain(want[False]) == (NONE, [], 0, 0)


@pytest.mark.parametrize("pos", [63, 64, 65])
def test_seventy_members_a_required_invalid_one(pos, oracle_mod):
    n = 70
    snap = PR.tiny([{0: 1}] * n + [{0: 1}] * 3, {0: 1000}, flags=[P] * n + [C] * 3)
    snap.pod_flags[pos] = 0
    want = held_to_the_reference(snap, oracle_mod, list(range(n)), 1, [j == pos for j in range(n)], [n, n + 1, n + 2])
    assert _plain(want[False]) == (NONE, [0, 0, 0], 69, pos)
    # ... not required, under a quorum it does not put out of reach: everybody else is in as things stand
    want = held_to_the_reference(snap, oracle_mod, list(range(n)), 69, None, [n, n + 1, n + 2])
    assert _plain(want[False]) == (0, [0, 0, 0], 69, -1)


@pytest.mark.parametrize("pos", [63, 64, 65])
def test_seventy_members_the_quorum_deciding_one(pos, oracle_mod):
    """A pod count of pos + 1 with three running pods admits members 0 .. pos - 3; every victim lets one more in, and the quorum
    pos + 1 takes all three."""
    n = 70
    snap = PR.tiny([{0: 1}] * n + [{0: 1}] * 3, {}, count=pos + 1, flags=[P] * n + [C] * 3)
    want = held_to_the_reference(snap, oracle_mod, list(range(n)), pos + 1, None, [n, n + 1, n + 2])
    assert _plain(want[False]) == (3, [1, 1, 1], pos + 1, pos - 2)
    assert want[False].verdicts == [ER.B] * 3 + [ER.A] and want[False].counts == [pos - 2, pos - 1, pos, pos + 1]


def _many_throttles(T, D=2):
    """T throttles affect both members (asking 3 each) and the three running pods of 4; only the last row's threshold, 11, stops
    anybody: with one victim gone member 0 fits, with two both."""
    snap = PR.tiny([{0: 3}, {0: 3}, {0: 4}, {0: 4}, {0: 4}], {0: 11}, flags=[P, P, C, C, C], T=T, row=T - 1, D=D)
    for t in range(T - 1):
        snap.thr_ns[t] = 0
        snap.thr_spec.set_row(t, {d: 1 << 40 for d in range(snap.D)}, 1 << 40)
    return snap


MANY = [([0, 1], 2, None), ([0, 1], 1, None), ([1, 0], 1, [False, True])]


def _ask_many(snap, oracle_mod, eng=None):
    out = [held_to_the_reference(snap, oracle_mod, m, q, r, [2, 3, 4], eng=eng) for m, q, r in MANY]
    assert [w[False].prefix for w in out] == [2, 1, 2] and out[0][False].members == 2
    return [[(_plain(w[eq]), _reprieved(w[eq])) for eq in (False, True)] for w in out]


def test_a_union_of_more_than_sixty_four_entries(oracle_mod):
    _ask_many(_many_throttles(70), oracle_mod)


def test_a_union_beyond_the_lds_capacity_by_the_hook(oracle_mod):
    """KT_PREEMPT_ELASTIC_LDS_CAP (read when the engine is created and on kt_debug_reload_env) lowers the entries LDS holds: the
    union of 20 throttles then lives in the engine's workspace — same code, same answers."""
    snap = _many_throttles(20)
    plain = E.Engine.for_snapshot(snap)
    try:
        in_lds = _ask_many(snap, oracle_mod, plain)
    finally:
        plain.close()
    assert HOOK not in os.environ
    os.environ[HOOK] = "16"
    try:
        eng = E.Engine.for_snapshot(snap)
    finally:
        del os.environ[HOOK]
    try:
        in_hbm = _ask_many(snap, oracle_mod, eng)
        again = _ask_many(snap, oracle_mod, eng)  # the workspace is reused
        eng.reload_env()  # the switch is gone: back in LDS
        back = _ask_many(snap, oracle_mod, eng)
    finally:
        eng.close()
    assert in_hbm == in_lds and again == in_lds and back == in_lds


def test_deciding_throttle_in_the_second_list_chunk(oracle_mod):
    """1030 throttles affect both members — more than one chunk of the LDS list holds, and more than the LDS state: the union lives
    in the workspace without any hook."""
    _ask_many(_many_throttles(1030), oracle_mod)


@pytest.mark.parametrize("D", [1, 8, 16])
def test_every_instantiation(D, oracle_mod):
    """The deciding name is the last one; the others are requested and counted but no threshold stops them."""
    snap, ms, cands = elastic_line(70, 66, D=D, dim=D - 1)
    want = held_to_the_reference(snap, oracle_mod, ms, 1, [True, False], cands)
    assert (want[False].prefix, want[True].prefix) == (66, 67)


def test_more_gangs_than_the_grid_has_workgroups(oracle_mod):
    """2100 two-member gangs in one launch: the grid strides beyond 2048.  Pods are shared between the gangs."""
    asks = [1, 2, 3, 4, 5, 3]
    snap = PR.tiny([{0: a} for a in asks] + [{0: 4}, {0: 2}, {0: 3}], {0: 10}, count=5, flags=[P] * 6 + [C] * 3)
    cands = [6, 7, 8]
    pairs = [[i, j] for i in range(6) for j in range(6) if i != j]
    rule_of = lambda k: (1 + k % 2, [k % 3 == 0, k % 5 == 0])
    n = 2100
    gangs = [pairs[(7 * k) % len(pairs)] for k in range(n)]
    want = {}
    for k, g in enumerate(gangs):
        key = (tuple(g), k % 2, k % 3 == 0, k % 5 == 0)
        if key not in want:
            want[key] = ER.reference(snap, oracle_mod, g, *rule_of(k), cands)
    assert len({w[False].prefix for w in want.values()}) >= 3  # the gangs differ in their answers
    eng = E.Engine.for_snapshot(snap)
    try:
        for reprieve in (False, True):
            got = launch_all(eng, gangs, [rule_of(k)[0] for k in range(n)], [rule_of(k)[1] for k in range(n)], cands, False, reprieve)
            for k, g in enumerate(gangs):
                w = want[(tuple(g), k % 2, k % 3 == 0, k % 5 == 0)][False]
                assert got[k] == (_reprieved(w) if reprieve else _plain(w)), f"gang {k} {g} reprieve={reprieve}"
    finally:
        eng.close()


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
    name = "more-victims-shut-the-required-member-out"
    snap, members, quorum, required, cands = ER.hand_case(name)
    want = ER.HAND[name][4][False][:4]
    whole_want = GR.reference(snap, oracle_mod, members, cands)
    eng = E.Engine.for_snapshot(snap)
    inc = E.Engine.for_snapshot(snap, kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    pe = eng.preempt_gangs_elastic
    rows, off, mm, cc = np.array(members, np.int64), np.array([0, 2], np.int64), np.array([1], np.int64), np.array(cands, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data

    def raw(n=2, r=rows, ng=1, o=off, q=mm, f=None, nc=3, c=cc, flags=0):
        return L.kt_preempt_gangs_elastic_launch(eng._h, n, ptr(r), ng, ptr(o), ptr(q), ptr(f), nc, ptr(c), NOW[0], NOW[1], 0, flags, None)

    def last():
        return L.kt_last_error(eng._h).decode()

    def every_refusal():
        assert raw(n=-1) == -1 and raw(ng=-1) == -1
        # (1) every gang_off defect, before the rule and the flags are looked at
        assert raw(o=None, q=None, flags=2) == -1 and "gang_off" in last()
        _refused(eng, lambda: pe(members, [1, 2], [9], cands, NOW), -1, "gang_off[0]")
        _refused(eng, lambda: pe(members, [0, 0, 2], [9, 9], cands, NOW), -1, "empty")
        _refused(eng, lambda: pe(members, [0, 2, 1], [9, 9], cands, NOW), -1, "below")
        _refused(eng, lambda: pe(members, [0, 1], [9], cands, NOW), -1, "not n")
        assert raw(ng=0) == -1
        # (2) the rule, with the admission's codes and messages, before the flags
        assert raw(q=None, flags=2) == -1 and "min_members is NULL" in last()
        _refused(eng, lambda: pe([0, 0], [0, 2], [0], cands, NOW), -1, "min_members[0] = 0 of gang 0 is outside [1, 2]")
        _refused(eng, lambda: pe([0, 99], [0, 2], [3], cands, NOW), -1, "min_members[0] = 3 of gang 0 is outside [1, 2]")
        assert raw(f=np.array([0, 2], np.uint8), flags=2) == -1 and "member_flags[1] = 0x02" in last() and "queue position 1" in last()
        # (3) the flags, before everything the gang query refuses
        assert raw(flags=2, nc=-1) == -1 and "flags = 0x2" in last()
        assert raw(flags=3, r=None) == -1 and "flags = 0x3" in last()
        # (4) the gang query's list, in its order
        assert raw(nc=-1) == -1 and "n_cand" in last()
        assert raw(r=None) == -1 and raw(c=None) == -1 and "missing" in last()
        _refused(eng, lambda: pe([0, 99], [0, 2], [1], [2, 2], NOW), -2, "pod row 99")
        _refused(eng, lambda: pe(members, [0, 2], [1], [2, 99], NOW), -2, "pod row 99")
        _refused(eng, lambda: pe([0, 0], [0, 2], [1], [2, 2], NOW), -1, "candidate twice")   # ... asked before the members
        _refused(eng, lambda: pe([0, 0], [0, 2], [1], [0, 2], NOW), -1, "a member and a candidate")
        _refused(eng, lambda: pe([0, 0], [0, 2], [1], cands, NOW), -1, "twice")
        eng.set_exchange_world(2)
        assert _code(lambda: pe(members, [0, 2], [1], cands, NOW)) == -7                       # KT_ERR_UNSUPPORTED
        eng.set_exchange_world(1)
        eng.set_wide_sums(1)
        assert _code(lambda: pe(members, [0, 2], [1], cands, NOW)) == -7                       # `used` wider than int64
        eng.set_wide_sums(0)

    def pending_elastic():
        got = eng.preempt_gangs_elastic_fetch(1, len(cands))
        return int(got[0][0]), got[1][0].tolist(), int(got[2][0]), int(got[3][0])

    launch = lambda: eng.preempt_gangs_elastic_launch(members, [0, 2], [quorum], cands, NOW, required)
    try:
        assert _code(lambda: eng.preempt_gangs_elastic_fetch(1, len(cands))) == -5  # KT_ERR_NOT_READY
        # a refused call leaves a pending elastic result fetchable ...
        launch()
        every_refusal()
        assert pending_elastic() == want
        # ... and a pending preempt result of another kind, a pending forecast, a pending check and a pending reconcile report
        eng.preempt_gangs_launch(members, [0, 2], cands, NOW)
        eng.forecast_launch(members, [NOW])
        every_refusal()
        got = eng.preempt_gangs_fetch(1, len(cands))
        assert (int(got[0][0]), int(got[2][0])) == whole_want
        eng.forecast_fetch(2, 1)
        eng.reconcile_launch(NOW, apply=False)
        eng.check_launch(snap.n_pods, want_status=True)
        every_refusal()
        eng.check_fetch(snap.n_pods, True)
        eng.reconcile_fetch()
        assert _code(lambda: inc.preempt_gangs_elastic(members, [0, 2], [1], cands, NOW)) == -7
        # the one pending preempt result is shared by three kinds: the last launch decides which fetch may read it
        others = {
            "pods": (lambda: eng.preempt_launch(members, cands, NOW), lambda: eng.preempt_fetch(2, len(cands))),
            "pods reprieved": (lambda: eng.preempt_reprieve_launch(members, cands, NOW), lambda: eng.preempt_fetch(2, len(cands))),
            "gangs": (lambda: eng.preempt_gangs_launch(members, [0, 2], cands, NOW), lambda: eng.preempt_gangs_fetch(1, len(cands))),
            "gangs reprieved": (lambda: eng.preempt_gangs_reprieve_launch(members, [0, 2], cands, NOW), lambda: eng.preempt_gangs_fetch(1, len(cands))),
        }
        for kind, (other_launch, fetch) in others.items():
            other_launch()
            assert _code(lambda: eng.preempt_gangs_elastic_fetch(1, len(cands))) == -5, kind
            fetch()
            launch()
            assert _code(fetch) == -5, kind
            assert pending_elastic() == want
        # a pending forecast stays fetchable behind the launch
        first = eng.forecast(members, [NOW])
        eng.forecast_launch(members, [NOW])
        launch()
        again = eng.forecast_fetch(2, 1)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
        assert pending_elastic() == want
        # n == 0 with n_gangs == 0: KT_OK, nothing launched
        eng.preempt_gangs_elastic_launch([], [0], [], cands, NOW)
        assert eng.preempt_gangs_elastic_fetch(0, len(cands))[0].tolist() == []
        assert _code(lambda: eng.preempt_gangs_fetch(0, len(cands))) == -5
        # nullable outputs
        prefix, none, members_out, blocker = pe(members, [0, 2], [quorum], cands, NOW, required, want_victims=False)
        assert none is None and (int(prefix[0]), int(members_out[0]), int(blocker[0])) == (want[0], want[2], want[3])
        launch()
        assert L.kt_preempt_gangs_elastic_fetch(eng._h, 1, None, None, None, None) == 0
        assert _code(lambda: eng.preempt_gangs_elastic_fetch(2, len(cands))) == -2  # more gangs than the launch had
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
    snap, ruled, _, _ = ER.seeded_reference(SEEDS[0], oracle_mod)
    gangs = [ms for ms, _, _, _ in ruled]
    taken = {p for ms in gangs for p in ms}
    cands = [c for c in max((cs for _, cs, _, _ in ruled), key=len) if c not in taken]
    rows, off = _queue(gangs)
    quorums, req = [q for _, _, q, _ in ruled], _flags(gangs, [r for _, _, _, r in ruled])
    everyone = np.arange(snap.n_pods, dtype=np.int64)
    ctx = paging.preempt_context(snap, NOW)
    model = [paging.preempt_gangs_elastic_of(snap, ms, q, r, cands, NOW, ctx=ctx, reprieve=True) for ms, _, q, r in ruled]
    eng = E.Engine.for_snapshot(snap)
    launch = lambda: eng.preempt_gangs_elastic_launch(rows, off, quorums, cands, NOW, req, reprieve=True)
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
        # a pending aggregate keeps its sums, and a finalize behind the launch leaves the result fetchable
        eng.aggregate_launch()
        launch()
        eng.finalize_launch(NOW, apply=False)
        got = eng.reconcile_fetch()
        assert np.array_equal(got.used.v, plain.used.v) and np.array_equal(got.used.present, plain.used.present)
        assert np.array_equal(got.used.count, plain.used.count) and np.array_equal(got.thrl_flag, plain.thrl_flag)
        prefix, victims, members, blocker = eng.preempt_gangs_elastic_fetch(len(gangs), len(cands))
        for g in range(len(gangs)):
            b = int(blocker[g])
            assert (int(prefix[g]), victims[g].tolist(), int(members[g]), b if b < 0 else b - int(off[g])) == model[g], g
        # a later user of the check slot drops it
        launch()
        eng.check_launch(snap.n_pods)
        assert _code(lambda: eng.preempt_gangs_elastic_fetch(len(gangs), len(cands))) == -5
        # a dry run: what reads the stored status and the reserved amounts sees them unchanged
        after = [eng.check(rows=everyone, on_equal=eq)[0] for eq in (False, True)]
        res_after = eng.fetch_reserved()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(room_before, _stored_readback(eng, everyone)))
        for f in ("v", "present", "count", "has_count"):
            assert getattr(res_before, f).tobytes() == getattr(res_after, f).tobytes()
    finally:
        eng.close()


def test_the_gang_query_is_what_it_was_after_elastic_launches(oracle_mod):
    """(Passes with or without the feature's kernel being right.)  kt_preempt_gangs shares buffers with the elastic call: behind
    elastic launches it still answers its reference."""
    seed = SEEDS[1]
    snap, cases, want, _ = gang_case(seed, oracle_mod)
    eng = E.Engine.for_snapshot(snap)
    try:
        for (ms, cands), (k, b) in zip(cases, want[False]):
            off = [0, len(ms)]
            before = eng.preempt_gangs(ms, off, cands, NOW)
            before_r = eng.preempt_gangs(ms, off, cands, NOW, reprieve=True)
            eng.preempt_gangs_elastic(ms, off, [1], cands, NOW)
            eng.preempt_gangs_elastic(ms, off, [len(ms)], cands, NOW, np.ones(len(ms), bool), True, True)
            after = eng.preempt_gangs(ms, off, cands, NOW)
            after_r = eng.preempt_gangs(ms, off, cands, NOW, reprieve=True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(before + before_r, after + after_r))
            assert (int(after[0][0]), int(after[2][0])) == (k, b)
    finally:
        eng.close()


def test_host_plugin_preempt_elastic_gang():
    """The C++ plugin mirror's driver (tests/cpp/host_plugin_preempt_elastic_gang_test.cpp) holds PreemptElasticGang to a twin plugin
    per prefix; here the lines it prints are held to Engine.preempt_gangs_elastic on the same 20-pod scenario written as manifests."""
    import re
    import subprocess
    from test_host_preempt_gpu import scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kube_throttler_amd", "host")
    # always through make: a binary older than its sources must not be what gets tested
    subprocess.check_call(["make", "-C", host, "host_plugin_preempt_elastic_gang_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "host_plugin_preempt_elastic_gang_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expectations held" in r.stdout
    lines = set(re.findall(r"^PREEMPTELASTIC (\S+) (\d+) (\S+) (\S+) ([01]) -> (\S+) (\S+) (\d+)$", r.stdout, re.M))
    assert len(lines) == 22
    cs = scenario()
    names = [p["metadata"]["name"] for p in cs.pods]
    snap = cs.build_pages()[0].snapshot
    up = [f"r{i:02d}" for i in range(16)]
    lists = {"up": up, "down": up[::-1]}
    eng = E.Engine.for_snapshot(snap)
    try:
        for members, quorum, req, lst, reprieve, got, who, count in lines:
            members = members.split("+")
            required = None if req == "-" else [c == "1" for c in req]
            cands = [names.index(c) for c in lists[lst]]
            (prefix, victims, n_in, blocker), = launch_all(eng, [[names.index(m) for m in members]], [int(quorum)], [required], cands,
                                                           reprieve=reprieve == "1")
            what = f"{members} quorum {quorum} required {req} over {lst} reprieve={reprieve}"
            want = "none" if prefix < 0 else "pass" if prefix == 0 else ",".join(c for c, v in zip(lists[lst], victims) if v)
            assert (got, who, int(count)) == (want, members[blocker] if blocker >= 0 else "-", n_in), what
    finally:
        eng.close()
    by = {(m, int(q), rq, lst, rp): (got, who, int(n)) for m, q, rq, lst, rp, got, who, n in lines}
    # the scenario asks something: one member of the two takes fewer victims than both, and it is the SECOND member that gets in;
    # the reprieve shrinks the set; a required member that never fits; a required member behind one that never fits
    assert by[("cpu2+gpu2", 2, "-", "down", "0")] == ("r14,r13,r12,r09,r08,r06,r04", "cpu2", 2)
    assert by[("cpu2+gpu2", 1, "-", "down", "0")] == ("r14,r13,r12,r09,r08", "cpu2", 1)
    assert by[("cpu2+gpu2", 1, "-", "down", "1")] == ("r14,r13,r12,r08", "cpu2", 1)
    assert by[("cpu2+huge", 1, "01", "up", "0")] == ("none", "huge", 0)
    assert by[("huge+cpu2", 1, "01", "up", "1")] == ("r00,r01,r02,r04,r08", "cpu2", 1)
    assert by[("cpu2+free", 1, "-", "down", "0")] == ("pass", "-", 1)
