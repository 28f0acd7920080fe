"""kt_paged_forecast_gangs on the GPU (csrc/kt_kernels_forecast_gangs_paged.hip): a gang's first admitted instant over pages of
resource names, held to tests/paged_forecast_gangs_reference.py (per instant: the oracle's reconcile per page with the bytes OR-ed,
the members admitted in order over every page) and to ``paging.paged_forecast_gangs_of`` — first, verdict bytes and blockers, all
three bit for bit, for both isThrottledOnEqual values.  The shapes are the smallest at which the kernel can still go wrong: instant
blocks of 64 and the ballot across them, a gang beyond one member block, a deciding throttle in the second chunk of the
affected-throttle list, more gangs than the grid has workgroups, pages of unequal width, one case per DT instantiation."""
import types

import numpy as np
import pytest

import forecast_gangs_reference as FGR
import forecast_reference as FR
import paged_forecast_gangs_reference as R
import paged_preempt_gangs_reference as PPGR
import paged_preempt_reference as PPR
import preempt_reference as PR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

pytestmark = pytest.mark.gpu
NOW = FR.NOW
A, B, ERR = R.A, R.B, R.ERR
PENDING, COUNTED = PR.PENDING, PR.COUNTED
T1, T2, T3, T4, EDGE = FR.T1, FR.T2, FR.T3, FR.T4, FR.EDGE
P2C1 = [PENDING, PENDING, COUNTED]


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


def launch_all(engs, gangs, instants, on_equal=False):
    """All gangs in ONE call -> per gang (first, verdicts, blockers) with the blockers as positions inside the gang."""
    rows, off = _queue(gangs)
    first, verdicts, blockers = E.paged_forecast_gangs(engs, rows, off, instants, on_equal)
    assert verdicts.shape == blockers.shape == (len(gangs), len(instants)) and first.shape == (len(gangs),)
    out = []
    for g in range(len(gangs)):
        blk = [int(b) for b in blockers[g]]
        assert all(b == -1 or off[g] <= b < off[g + 1] for b in blk), (g, blk)
        out.append((int(first[g]), verdicts[g].tolist(), [b if b < 0 else b - int(off[g]) for b in blk]))
    return out


def held_to_everything(snaps, oracle_mod, gangs, instants, on_equals=(False, True)):
    """The engines' answer is the reference's and the closed form's -> per gang (first, verdicts, blockers) of the last on_equal."""
    states = R.states_at(snaps, oracle_mod, instants)
    engs = _engines(snaps)
    try:
        for on_equal in on_equals:
            got = launch_all(engs, gangs, instants, on_equal)
            for g, members in enumerate(gangs):
                ref = R.reference(snaps, oracle_mod, members, instants, on_equal, states=states)
                assert got[g] == ref, f"gang {g} {members} on_equal={on_equal}: {got[g]} != {ref}"
                assert paging.paged_forecast_gangs_of(snaps, members, instants, on_equal) == ref
    finally:
        _close(engs)
    return got


@pytest.mark.parametrize("seed,factor", R.GPU_CASES)
def test_random_wide_clusters(seed, factor, oracle_mod):
    snaps, gangs, want, _ = R.wide_reference(seed, factor, oracle_mod)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            assert launch_all(engs, gangs, FR.INSTANTS, on_equal) == want[on_equal], f"seed {seed} on_equal={on_equal}"
    finally:
        _close(engs)


@pytest.mark.parametrize("name", sorted(R.DIRECTED))
def test_directed(name, oracle_mod):
    snaps, members, inst, want = R.directed_reference(name, oracle_mod)
    engs = _engines(snaps)
    try:
        for on_equal, answer in R.DIRECTED[name][1].items():
            got, = launch_all(engs, [members], inst, on_equal)
            assert got == want[on_equal] == answer, f"{name} on_equal={on_equal}: {got}"
    finally:
        _close(engs)


# ---- identities ----
def _same_bytes(x, y):
    return all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(x, y))


@pytest.mark.parametrize("name", sorted(FGR.DIRECTED))
def test_one_page_returns_the_single_engine_bytes_directed(name):
    snap, members, inst = FGR.DIRECTED[name]()
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            single = eng.forecast_gangs(members, [0, len(members)], inst, on_equal)
            assert _same_bytes(E.paged_forecast_gangs([eng], members, [0, len(members)], inst, on_equal), single), name
    finally:
        eng.close()


@pytest.mark.parametrize("seed", [1, 4, 5])
def test_one_page_returns_the_single_engine_bytes_on_clusters(seed, oracle_mod):
    snap, gangs, want, _ = FGR.cluster_reference(seed, oracle_mod)
    rows, off = _queue(gangs)
    eng = E.Engine.for_snapshot(snap)
    try:
        for on_equal in (False, True):
            single = eng.forecast_gangs(rows, off, FR.INSTANTS, on_equal)
            assert _same_bytes(E.paged_forecast_gangs([eng], rows, off, FR.INSTANTS, on_equal), single)
            assert single[1].tolist() == [w[1] for w in want[on_equal]]
    finally:
        eng.close()


@pytest.mark.parametrize("seed,factor", R.GPU_CASES[:2])
def test_gangs_of_one_return_the_paged_forecast_bytes(seed, factor, oracle_mod):
    snaps, _, _, _ = R.wide_reference(seed, factor, oracle_mod)
    pods = FR.forecast_pods(seed, snaps[0], n_pods=6)
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            first, verdicts = E.paged_forecast(engs, pods, FR.INSTANTS, on_equal)
            gfirst, gverdicts, gblockers = E.paged_forecast_gangs(engs, pods, np.arange(len(pods) + 1), FR.INSTANTS, on_equal)
            assert gfirst.tobytes() == first.tobytes() and gverdicts.tobytes() == verdicts.tobytes()
            assert gblockers.tolist() == [[-1 if v == A else i for v in verdicts[i]] for i in range(len(pods))]
    finally:
        _close(engs)


@pytest.mark.parametrize("name", sorted(PPGR.DIRECTED))
def test_single_instant_agrees_with_paged_preempt_gangs_without_candidates(name):
    snaps, members, _ = PPGR.DIRECTED[name][0]()
    engs = _engines(snaps)
    try:
        for on_equal in (False, True):
            prefix, _, blocker = E.paged_preempt_gangs(engs, members, [0, len(members)], [], NOW, on_equal)
            first, _, blockers = E.paged_forecast_gangs(engs, members, [0, len(members)], [NOW], on_equal)
            assert (int(first[0]) == 0) == (int(prefix[0]) == 0)
            assert int(blockers[0][0]) == int(blocker[0])
    finally:
        _close(engs)


# ---- kernel shapes ----
def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


def example_pages(times, values1, spec1=None, requests1=None, flags=P2C1, D0=1, D1=1, dim1=0, **kw):
    """Page 0: every pod asks 1 of name 0 under no threshold and holds every override's times; page 1: the example (two members
    asking 3 each of name ``dim1``, a running pod with 4, spec 8), override k active over ``times[k]`` with ``values1[k]``."""
    requests1 = requests1 or [{dim1: 3}, {dim1: 3}, {dim1: 4}]
    s0 = PR.tiny([{0: 1}] * len(requests1), {}, flags=flags, D=D0, **kw)
    s1 = PR.tiny(requests1, {dim1: 8} if spec1 is None else spec1, flags=flags, D=D1, **kw)
    row = kw.get("row", 0)
    FR.timed(s0, row, [(b, e, {}, None) for b, e in times])
    FR.timed(s1, row, [(b, e, v, None) for (b, e), v in zip(times, values1)])
    return [s0, s1]


@pytest.mark.parametrize("m,lo,hi", [(1, 0, 0), (1, None, None), (63, 62, 62), (64, 63, 63), (65, 64, 64), (65, 63, 64), (130, 5, 5), (130, 70, 100),
                                     (130, 128, 129), (130, None, None)])
def test_instant_blocks_and_the_ballot(m, lo, hi, oracle_mod):
    """The example on page 1 (4 + 3 + 3 > 8); the override 10 is active over positions lo .. hi of the m instants: the only passing
    instants sit in the first, second or third block of 64 lanes, or nowhere; (65, 63, 64) passes at lane 63 and at lane 64 (lane 0
    of the next block)."""
    inst = _seconds(m)
    times = [(inst[lo], inst[hi])] if lo is not None else [(FR.shift(inst[-1], 1), None)]
    (first, verdicts, blockers), = held_to_everything(example_pages(times, [{0: 10}]), oracle_mod, [[0, 1]], inst, on_equals=(False,))
    assert first == (lo if lo is not None else -1)
    assert verdicts == [A if lo is not None and lo <= k <= hi else B for k in range(m)]
    assert blockers == [-1 if v == A else 1 for v in verdicts]


def test_seventy_members_an_invalid_one_at_position_65(oracle_mod):
    """The member ballot strides 64: the invalid member sits in its second block; inside the window (50 on page 1) member 50 is
    stopped first."""
    n = 70
    snaps = example_pages([(T1, T2)], [{0: 50}], spec1={0: 1000}, requests1=[{0: 1}] * n, flags=[PENDING] * n)
    for s in snaps:
        s.pod_flags[65] = 0
    (first, verdicts, blockers), = held_to_everything(snaps, oracle_mod, [list(range(n))], EDGE, on_equals=(False,))
    assert first == -1 and verdicts == [ERR] * 9 and blockers == [65, 65, 50, 50, 50, 50, 65, 65, 65]


@pytest.mark.parametrize("spec,window,blockers", [(65, 70, [65, 65, -1, -1, -1, -1, 65, 65, 65]), (70, 65, [-1, -1, 65, 65, 65, 65, -1, -1, -1])])
def test_seventy_members_a_count_threshold_stops_member_65(spec, window, blockers, oracle_mod):
    """A pod-count threshold alone, names on two pages: the count stops member 65 only outside (inside) the override."""
    n = 70
    snaps = PPR.pages_of([[{0: 1}] * n, [{0: 2}] * n], [{}, {}], [PENDING] * n, counts=[spec, spec])
    snaps = [FR.timed(s, 0, [(T1, T2, {}, window)]) for s in snaps]
    (first, verdicts, got), = held_to_everything(snaps, oracle_mod, [list(range(n))], EDGE, on_equals=(False,))
    assert got == blockers and first == blockers.index(-1)


@pytest.mark.parametrize("deciding_page", [0, 1])
def test_deciding_throttle_in_the_second_list_chunk(deciding_page, oracle_mod):
    """1030 throttles affect both members — more than one chunk of the LDS list holds; only the last row's override lets the gang
    through, and the name it decides is on page ``deciding_page``."""
    T = 1030
    snaps = example_pages([(T1, T2)], [{0: 10}], T=T, row=T - 1)
    for s in snaps:
        for t in range(T - 1):
            s.thr_ns[t] = 0
            s.thr_spec.set_row(t, {d: 1 << 40 for d in range(s.D)}, 1 << 40)
        s._keep = None
    if deciding_page == 0:
        snaps.reverse()
    assert len(paging.affected_throttles(snaps[0], 0)[1]) == T
    (first, verdicts, blockers), = held_to_everything(snaps, oracle_mod, [[0, 1]], EDGE[:8], on_equals=(False,))
    assert first == 2 and verdicts == [B, B, A, A, A, A, B, B] and blockers == [1, 1, -1, -1, -1, -1, 1, 1]


def test_more_gangs_than_the_grid_has_workgroups(oracle_mod):
    """2050 two-member gangs in one call: the grid strides beyond 2048.  Pods are shared between the gangs, and the gangs differ in
    their answers, so a gang read at the wrong stride shows."""
    asks = [1, 2, 3, 4, 5, 3]
    flags = [PENDING] * 6 + [COUNTED]
    s0 = PR.tiny([{0: 1}] * 7, {}, count=3, flags=flags, D=1)
    s1 = PR.tiny([{0: a} for a in asks] + [{0: 4}], {0: 10}, count=3, flags=flags, D=1)
    snaps = [FR.timed(s0, 0, [(T1, T2, {}, None), (T3, T4, {}, 2)]), FR.timed(s1, 0, [(T1, T2, {0: 12}, None), (T3, T4, {0: 9}, 2)])]
    pairs = [[i, j] for i in range(6) for j in range(6) if i != j]
    states = R.states_at(snaps, oracle_mod, EDGE)
    want = {tuple(g): R.reference(snaps, oracle_mod, g, EDGE, states=states) for g in pairs}
    for g in pairs:
        assert paging.paged_forecast_gangs_of(snaps, g, EDGE) == want[tuple(g)]
    assert len({w[0] for w in want.values()}) >= 3 and len({tuple(w[2]) for w in want.values()}) >= 3
    gangs = [pairs[(7 * k) % len(pairs)] for k in range(2050)]
    engs = _engines(snaps)
    try:
        got = launch_all(engs, gangs, EDGE)
    finally:
        _close(engs)
    for k, g in enumerate(gangs):
        assert got[k] == want[tuple(g)], f"gang {k} {g}"


@pytest.mark.parametrize("narrow_first", [False, True])
def test_a_three_name_page_beside_a_sixteen_name_page(narrow_first, oracle_mod):
    """The bucket comes from the widest page: name 2 of the 3-name page decides under the DT = 16 form; the wide page's name 15 is
    under a threshold nothing reaches."""
    snaps = example_pages([(T1, T2), (T3, T4)], [{2: 10}, {2: 10, 1: 1}], D0=16, D1=3, dim1=2)
    snaps[0].thr_spec.set_row(0, {15: 1 << 30}, None)
    snaps[0]._keep = None
    if narrow_first:
        snaps.reverse()
    assert sorted(s.D for s in snaps) == [3, 16]
    (first, _, _), = held_to_everything(snaps, oracle_mod, [[0, 1]], EDGE + [FR.shift(T4, 1)])
    assert first == -1  # (on_equal True, the last one asked: 10 >= 10 stops the second member)


def test_three_pages_only_the_last_decides(oracle_mod):
    snaps = example_pages([(T1, T2)], [{}], spec1={}, requests1=[{0: 1}] * 3, D0=16, D1=16)
    last = PR.tiny([{2: 3}, {2: 3}, {2: 4}], {2: 8}, flags=P2C1, D=3)
    snaps.append(FR.timed(last, 0, [(T1, T2, {2: 10}, None)]))
    (first, verdicts, blockers), = held_to_everything(snaps, oracle_mod, [[0, 1]], EDGE, on_equals=(False,))
    assert first == 2 and verdicts == R._row(A, B) and blockers == R._row(-1, 1)


def test_a_page_nobody_requests_from_flips_differs(oracle_mod):
    """``another-page-replaces-the-threshold`` with NO member requesting anything of page 1: the override names page 1's name
    alone, so page 1 — skipped for the member walk — is the page that makes page 0 read a calculated threshold without its name."""
    snaps = PPR.pages_of([[{0: 2}, {0: 2}, {0: 1}], [{}, {}, {0: 1}]], [{0: 1}, {}], P2C1)
    snaps = R._timed(snaps, [[(T1, T2, {}, None)], [(T1, T2, {0: 5}, None)]])
    (first, verdicts, blockers), = held_to_everything(snaps, oracle_mod, [[0, 1]], EDGE)
    assert first == 2 and verdicts == R._row(A, B) and blockers == R._row(-1, 0)
    assert not any(paging.pod_requests(snaps[1], p) for p in (0, 1))


@pytest.mark.parametrize("D", [4, 8, 16])
def test_every_instantiation(D, oracle_mod):
    """Both pages D wide; the deciding name is the last one of page 1, the others are requested and counted but no threshold stops
    them."""
    d = D - 1
    other = {x: 2 for x in range(D) if x != d}
    member, running = {**other, d: 3}, {**other, d: 4}
    snaps = example_pages([(T1, T2), (T3, T4)], [{d: 10}, {d: 10, 0: 5}], spec1={d: 8, 0: 100}, requests1=[member, member, running], D0=D, D1=D)
    for on_equal in (False, True):
        got, = held_to_everything(snaps, oracle_mod, [[0, 1]], EDGE + [FR.shift(T4, 1)], on_equals=(on_equal,))
        assert got[0] == (-1 if on_equal else 2)


# ---- refusals, and what a refused call leaves alone ----
def test_refusals_and_what_a_refused_call_leaves_alone(oracle_mod):
    snaps, members, inst, want = R.directed_reference("reservation-on-the-second-page", oracle_mod)
    n = snaps[0].n_pods
    engs = _engines(snaps)
    other = E.Engine.for_snapshot(PR.tiny([{0: 1}] * n, {0: 10}, T=3, row=2, D=1))
    inc = E.Engine.for_snapshot(snaps[1], kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    rows, off = np.array(members, np.int64), np.array([0, 2], np.int64)
    s2, n2 = np.array([NOW[0], NOW[0] + 1], np.int64), np.zeros(2, np.int32)
    fg = lambda es, a, o, t, **kw: E.paged_forecast_gangs(es, a, o, t, **kw)
    ptr = lambda a: None if a is None else a.ctypes.data

    def raw(h=hs, k=2, n_=2, r=rows, ng=1, o=off, m=2, s=s2, ns=n2):
        return L.kt_paged_forecast_gangs(h, k, n_, ptr(r), ng, ptr(o), m, ptr(s), ptr(ns), 0, None, None, None)

    def every_refusal():
        # the instants come first: even with a broken gang_off
        assert _code(lambda: fg(engs, members, [0, 2], [])) == -1                                   # n_inst < 1
        assert _code(lambda: fg(engs, members, [0, 1], [])) == -1
        assert _code(lambda: fg(engs, members, [0, 2], [T1, T1])) == -1                             # not STRICTLY ascending
        assert _code(lambda: fg(engs, members, [0, 1], [T2, T1])) == -1
        assert _code(lambda: fg(engs, members, [0, 2], [(NOW[0], 5), (NOW[0], 4)])) == -1
        assert _code(lambda: fg(engs, members, [0, 2], [(NOW[0], 1_000_000_000)])) == -1            # inst_ns outside [0, 10^9)
        assert _code(lambda: fg(engs, members, [0, 2], [(NOW[0], -1)])) == -1
        assert raw(r=None) == -1 and raw(s=None) == -1 and raw(ns=None) == -1                       # missing arrays
        assert raw(n_=-1) == -1 and raw(ng=-1) == -1
        # the page set
        assert _code(lambda: fg([engs[0], other], members, [0, 2], inst)) == -1                     # different throttle-row counts
        assert _code(lambda: fg([engs[0], engs[0]], members, [0, 2], inst)) == -1                   # an engine named twice
        assert raw(h=None) == -1 and raw(k=0) == -1
        # every gang_off defect kt_admit_gangs_launch refuses
        assert raw(o=None) == -1
        assert _code(lambda: fg(engs, members, [1, 2], inst)) == -1                                 # gang_off[0] != 0
        assert _code(lambda: fg(engs, members, [0, 0, 2], inst)) == -1                              # an empty gang
        assert _code(lambda: fg(engs, members, [0, 2, 1], inst)) == -1                              # descending
        assert _code(lambda: fg(engs, members, [0, 1], inst)) == -1                                 # gang_off[n_gangs] != n
        assert _code(lambda: fg(engs, members, [0, 3], inst)) == -1
        assert raw(ng=0) == -1                                                                      # no gangs for a queue of 2
        assert _code(lambda: fg(engs, [], [0, 0], inst)) == -1                                      # n == 0 with n_gangs == 1
        assert _code(lambda: fg(engs, [0, 1, 0], [0, 3], inst)) == -1                               # a pod twice within ONE gang
        assert _code(lambda: fg(engs, [0, 99, 99], [0, 3], inst)) == -1                             # ... asked before the range
        assert _code(lambda: fg(engs, [0, 99], [0, 2], inst)) == -2                                 # a row no page holds
        assert _code(lambda: fg(engs, [-1], [0, 1], inst)) == -2
        many = np.zeros(2**16 + 1, np.int64)
        assert _code(lambda: fg(engs, many, np.arange(2**16 + 2), _seconds(2**15))) == -2           # n_gangs x n_inst > 2^31
        # an engine, asked of every page
        assert _code(lambda: fg([engs[0], inc], members, [0, 2], inst)) == -7                       # KT_VARIANT_INCREMENTAL
        engs[1].set_exchange_world(2)
        assert _code(lambda: fg(engs, members, [0, 2], inst)) == -7
        engs[1].set_exchange_world(1)
        # `used` of page 1 wider than int64: found out by that page's sums kernel, the one thing that runs before the refusal
        engs[1].set_wide_sums(1)
        assert _code(lambda: fg(engs, members, [0, 2], inst)) == -7
        engs[1].set_wide_sums(0)

    try:
        want_check = [a.copy() for a in engs[0].check(rows=np.arange(n), on_equal=False)]
        want_rec = engs[0].reconcile(NOW, apply=False)
        want_pre = [a.copy() for a in engs[0].preempt_gangs(members, [0, 2], [2], NOW)]
        want_fc = [a.copy() for a in engs[0].forecast_gangs(members, [0, 2], inst)]
        want_plain = [a.copy() for a in engs[0].forecast(members, inst)]
        # a pending check and a pending reconcile report of page 0 ...
        engs[0].check_launch(n, want_status=True)
        engs[0].reconcile_launch(NOW, apply=False)
        every_refusal()
        got = engs[0].reconcile_fetch()
        assert got.used.v.tobytes() == want_rec.used.v.tobytes() and got.calc_updated.tobytes() == want_rec.calc_updated.tobytes()
        status, summary = engs[0].check_fetch(n, True)
        assert status.tobytes() == want_check[0].tobytes() and summary.tobytes() == want_check[1].tobytes()
        # ... and a pending forecast of either kind and a pending preempt result (each takes the check slot)
        engs[0].forecast_gangs_launch(members, [0, 2], inst)
        engs[0].preempt_gangs_launch(members, [0, 2], [2], NOW)
        every_refusal()
        assert [a.tobytes() for a in engs[0].preempt_gangs_fetch(1, 1)] == [a.tobytes() for a in want_pre]
        assert [a.tobytes() for a in engs[0].forecast_gangs_fetch(1, len(inst))] == [a.tobytes() for a in want_fc]
        engs[0].forecast_launch(members, inst)
        every_refusal()
        assert [a.tobytes() for a in engs[0].forecast_fetch(2, len(inst))] == [a.tobytes() for a in want_plain]
        import torch
        # pages on different devices: needs a second GPU, so this case does not run on a one-GPU machine (paged_same_cluster's
        # refusal, shared with kt_paged_admit)
        if torch.cuda.device_count() >= 2:
            far = E.Engine.for_snapshot(snaps[1], device=1)
            try:
                assert _code(lambda: fg([engs[0], far], members, [0, 2], inst)) == -7
            finally:
                far.close()
        # n == 0 with n_gangs == 0: KT_OK, nothing launched; nullable outputs
        first, verdicts, blockers = fg(engs, [], [0], inst)
        assert first.shape == (0,) and verdicts.shape == blockers.shape == (0, len(inst))
        first, none, blockers = fg(engs, members, [0, 2], inst, want_verdicts=False)
        assert none is None and int(first[0]) == want[False][0] and blockers[0].tolist() == want[False][2]
        first, verdicts, none = fg(engs, members, [0, 2], inst, want_blocker=False)
        assert none is None and int(first[0]) == want[False][0] and verdicts[0].tolist() == want[False][1]
        assert raw(m=len(inst), s=np.array([t[0] for t in inst], np.int64), ns=np.array([t[1] for t in inst], np.int32)) == 0
    finally:
        _close(engs + [other, inc])
    # n x throttle_rows beyond 2^31 bytes of matrix: refused on the host, nothing is allocated
    wide = _engines([FR._run({0: 10}, T=1030, row=1029), FR._run({0: 10}, T=1030, row=1029)])
    try:
        big = 2**31 // 1030 + 1
        assert _code(lambda: fg(wide, np.zeros(big, np.int64), np.arange(big + 1), [NOW])) == -2
        assert "throttle_rows" in E.lib().kt_last_error(wide[0]._h).decode()
        first, verdicts, blockers = fg(wide, [0], [0, 1], [NOW])
        assert first.tolist() == [-1] and verdicts.tolist() == [[B]] and blockers.tolist() == [[0]]
    finally:
        _close(wide)


def test_slots_after_a_successful_call(oracle_mod):
    snaps, members, inst, want = R.directed_reference("reservation-on-the-second-page", oracle_mod)
    engs = _engines(snaps)
    other_inst = [NOW, (NOW[0] + 60, 0)]
    try:
        reserved = [e.fetch_reserved() for e in engs]
        plain = [e.reconcile(NOW, apply=False) for e in engs]
        want_pre = [a.copy() for a in engs[0].preempt_gangs(members, [0, 2], [2], NOW)]
        for launch in (lambda: engs[0].forecast_gangs_launch(members, [0, 2], other_inst), lambda: engs[0].forecast_launch(members, other_inst)):
            launch()
            engs[0].preempt_gangs_launch(members, [0, 2], [2], NOW)
            for e in engs:
                e.reconcile_launch(NOW, apply=False)
            engs[1].aggregate_launch()
            first, verdicts, blockers = E.paged_forecast_gangs(engs, members, [0, 2], inst)
            assert (int(first[0]), verdicts[0].tolist(), blockers[0].tolist()) == want[False]
            # handed out by the call: no forecast result of either kind is pending on page 0
            assert _code(lambda: engs[0].forecast_gangs_fetch(1, len(other_inst))) == -5
            assert _code(lambda: engs[0].forecast_fetch(1, len(other_inst))) == -5
            assert [a.tobytes() for a in engs[0].preempt_gangs_fetch(1, 1)] == [a.tobytes() for a in want_pre]
            for e in engs:
                assert _code(e.reconcile_fetch) == -5  # every page's reconcile report is dropped
            engs[1].finalize_launch(NOW, apply=False)  # page 1's pending aggregate kept its sums
            got = engs[1].reconcile_fetch()
            assert got.used.v.tobytes() == plain[1].used.v.tobytes() and got.used.present.tobytes() == plain[1].used.present.tobytes()
        # a pending check of page 0 is gone: the call used its slot
        engs[0].check_launch(snaps[0].n_pods, want_status=True)
        E.paged_forecast_gangs(engs, members, [0, 2], inst)
        assert _code(lambda: engs[0].check_fetch(snaps[0].n_pods, True)) == -5
        # a dry run: reserved amounts and the stored status of every page are unchanged
        for e, before, dry in zip(engs, reserved, plain):
            after = e.fetch_reserved()
            for f in ("v", "present", "count", "has_count"):
                assert getattr(after, f).tobytes() == getattr(before, f).tobytes()
            assert e.reconcile(NOW, apply=False).calc_updated.tobytes() == dry.calc_updated.tobytes()
        # a larger call grows page 0's result buffers behind an unfetched launch
        engs[0].forecast_gangs_launch(members, [0, 2], other_inst)
        big = _seconds(130)
        first, verdicts, blockers = E.paged_forecast_gangs(engs, members * 40, np.arange(0, 82, 2), big)
        assert verdicts.shape == blockers.shape == (40, 130) and (verdicts == verdicts[0]).all()
        assert (int(first[0]), verdicts[0].tolist(), blockers[0].tolist()) == paging.paged_forecast_gangs_of(snaps, members, big)
        assert blockers[7].tolist() == [b if b < 0 else b + 14 for b in blockers[0].tolist()]
    finally:
        _close(engs)


def test_paged_engine_forecast_gangs(oracle_mod):
    from test_paged_admit_cpu import loosen
    import paged_forecast_reference as PFR
    seed, factor = R.GPU_CASES[-1]
    cs = PFR.wide_forecast_cluster(seed)
    loosen(cs, factor)
    pages = cs.build_pages()
    snaps, gangs, want, _ = R.wide_reference(seed, factor, oracle_mod)
    assert len(pages) == len(snaps) == 3
    rows, off = _queue(gangs)
    pe = paging.PagedEngine(pages)
    try:
        for on_equal in (False, True):
            first, verdicts, blockers = pe.forecast_gangs(rows, off, FR.INSTANTS, on_equal)
            assert first.tolist() == [w[0] for w in want[on_equal]] and verdicts.tolist() == [w[1] for w in want[on_equal]]
    finally:
        pe.close()
    # one page goes through the same call
    snap, members, inst = FGR.DIRECTED["each-alone-passes-the-gang-only-in-the-window"]()
    one = paging.PagedEngine([types.SimpleNamespace(snapshot=snap)])
    try:
        first, verdicts, blockers = one.forecast_gangs(members, [0, 2], inst)
        assert (int(first[0]), verdicts[0].tolist(), blockers[0].tolist()) == paging.forecast_gangs_of(snap, members, inst)
    finally:
        one.close()
