"""The reference of the gang headroom forecast (kt_headroom_forecast_gangs_launch), shared by
tests/test_headroom_forecast_gangs_cpu.py and tests/test_headroom_forecast_gangs_gpu.py.

Per instant t_k: ``forecast_reference.state_at`` (a copy of the snapshot, the oracle's reconcile at t_k written into the stored
status), then ``headroom_gangs_reference.headroom_gangs_by_oracle`` on that state: the oracle's admit of ``members * cap``, the
leading complete copies, and the first position that is not Success (its place inside the gang, the lowest row PreFilter returned
to it).  ``first`` comes from the reference copies.  Nothing here shares code with ``paging.headroom_forecast_gangs_of`` or the
kernel."""
import functools

import forecast_gangs_reference as FG
import forecast_reference as FR
import preempt_reference as PR
from headroom_gangs_reference import headroom_gangs_by_oracle
from kube_throttler_amd import snapshot as S

NONE = -1
CAP = 12      # the random cases' cap (chosen with FACTOR on the reference: see the coverage test of the CPU file)
FACTOR = 6    # thresholds (spec and overrides) times FACTOR: a few GANGS deep


def at_state(state, oracle_mod, members, cap, on_equal=False):
    """(copies, limiting, blocker position inside the gang) in one state.  An invalid member row is not walked by the oracle: the
    walk of copy 0 ends in front of it — 0 copies, and the blocker is an earlier member some throttle stops, else the invalid
    member itself (limiting -1)."""
    members = [int(p) for p in members]
    bad = next((j for j, p in enumerate(members) if not int(state.pod_flags[p]) & S.POD_VALID), None)
    if bad is None:
        return headroom_gangs_by_oracle(oracle_mod.Oracle(state), members, cap, on_equal)
    if bad > 0:
        copies, limiting, blocker = headroom_gangs_by_oracle(oracle_mod.Oracle(state), members[:bad], 1, on_equal)
        if copies == 0:
            return 0, limiting, blocker
    return 0, -1, bad


def first_of(copies, want):
    return next((k for k, c in enumerate(copies) if int(c) >= want), NONE)


def reference(snap, oracle_mod, members, instants, cap, want=1, on_equal=False, states=None):
    """-> (first, copies [len(instants)], limiting [len(instants)], blocker positions inside the gang [len(instants)])."""
    rows = []
    for k, t in enumerate(instants):
        rows.append(at_state(states[k] if states is not None else FR.state_at(snap, oracle_mod, t), oracle_mod, members, cap, on_equal))
    copies, limiting, blocker = ([r[i] for r in rows] for i in range(3))
    return first_of(copies, want), copies, limiting, blocker


def queue_of(gangs):
    """(pod_rows, gang_off) of a list of gangs, as the launch takes them."""
    off = [0]
    for g in gangs:
        off.append(off[-1] + len(g))
    return [int(p) for g in gangs for p in g], off


def expected(snap, oracle_mod, gangs, instants, cap, want=1, on_equal=False):
    """The reference as the fetch hands it out: (first [n_gangs], copies, limiting, blocker [n_gangs][m]), the blocker a queue
    position (gang_off[g] added)."""
    states = [FR.state_at(snap, oracle_mod, t) for t in instants]
    _, off = queue_of(gangs)
    out = [reference(snap, oracle_mod, g, instants, cap, want, on_equal, states=states) for g in gangs]
    blocker = [[b + off[i] if b >= 0 else -1 for b in r[3]] for i, r in enumerate(out)]
    return [r[0] for r in out], [r[1] for r in out], [r[2] for r in out], blocker


def has_negative_request(snap):
    """Some pod of the snapshot asks a negative amount: the call refuses such an engine (the refusal test's ground)."""
    return bool((snap.ctr_req < 0).any())


def loosened(snap, factor=FACTOR):
    """Thresholds (spec and overrides) of a hand-built snapshot times ``factor``, in place: queues where some copies pass and
    later ones are blocked (test_paged_admit_cpu.loosen on the tables)."""
    for tab in (snap.thr_spec, snap.ovr_thr):
        tab.v *= factor
        tab.count *= factor
    snap._keep = None
    return snap


# ---- random cases: the gang forecast's two generators, loosened ----
STAIR_SEEDS = list(range(40))
CLUSTER_SEEDS = [1, 3, 4, 5, 8, 10, 14, 19, 20, 23]


@functools.lru_cache(maxsize=None)
def stair_case(seed, oracle_mod):
    """(snapshot, [members], instants, {on_equal: [(first, copies, limiting, blocker)]}) — computed once, never modified."""
    snap, members, inst = FG.stair_case(seed)
    loosened(snap)
    states = [FR.state_at(snap, oracle_mod, t) for t in inst]
    want = {eq: [reference(snap, oracle_mod, members, inst, CAP, 2, eq, states=states)] for eq in (False, True)}
    return snap, [members], inst, want


@functools.lru_cache(maxsize=None)
def cluster_case(seed, oracle_mod):
    """The same on a manifest cluster of the forecast tests, over FR.INSTANTS, four gangs."""
    from test_paged_admit_cpu import loosen, write_status
    cs = FR.forecast_cluster(seed)
    loosen(cs, FACTOR)
    if seed % 2:
        write_status(cs, oracle_mod)
    pages = cs.build_pages()
    assert len(pages) == 1
    snap = pages[0].snapshot
    gangs = FG.cluster_gangs(seed, snap)
    states = [FR.state_at(snap, oracle_mod, t) for t in FR.INSTANTS]
    want = {eq: [reference(snap, oracle_mod, g, FR.INSTANTS, CAP, 2, eq, states=states) for g in gangs] for eq in (False, True)}
    return snap, gangs, FR.INSTANTS, want


def random_cases(oracle_mod):
    """Every random case without a negative request: [(name, snapshot, gangs, instants, want)]."""
    out = []
    for kind, seeds, make in (("stair", STAIR_SEEDS, stair_case), ("cluster", CLUSTER_SEEDS, cluster_case)):
        for seed in seeds:
            case = make(seed, oracle_mod)
            if not has_negative_request(case[0]):
                out.append((f"{kind}-{seed}",) + case)
    return out


# ---- directed cases: name -> () -> (snapshot, members, instants); those of the gang forecast without a negative request, and ----
# ---- the call's own                                                                                                         ----
tiny, timed, PENDING, COUNTED = PR.tiny, FR.timed, PR.PENDING, PR.COUNTED
T1, T2, T3, T4, EDGE = FR.T1, FR.T2, FR.T3, FR.T4, FR.EDGE


def _second_stopped_by_the_first():
    # used 4, both members ask 3: spec 9 stops the second member of copy 0 (4 + 3 + 3 > 9); the override 16 admits two copies and
    # stops the first member of the third
    return timed(tiny([{0: 3}, {0: 3}, {0: 4}], {0: 9}, flags=FG.P2C1), 0, [(T1, T2, {0: 16}, None)]), [0, 1], EDGE


def _different_throttles():
    # row 0 (all of namespace 0: both members) counts pods, row 1 is a throttle of namespace 2 — nobody's; the members ask
    # different names, so the count and each name bind at different instants
    snap = tiny([{0: 2}, {1: 3}, {0: 1, 1: 1}], {0: 7, 1: 10}, count=9, flags=FG.P2C1)
    return timed(snap, 0, [(T1, T2, {0: 100, 1: 100}, 5), (T3, T4, {1: 7}, None)]), [0, 1], EDGE + [FR.shift(T4, 1)]


def _zero_valued_name():
    # the first member names dimension 1 with 0: from copy 1 on (and for the second member of copy 0) the name is PRESENT in
    # reserved with value 0.  With requests that are not negative presence alone never decides (a member that asks v > 0 of a name
    # whose sum has reached the threshold fails step 4 too): the case holds the presence a candidate's reserved row is given to
    # the walk, inside a window whose threshold names the dimension with 0
    snap = tiny([{0: 1, 1: 0}, {0: 1}, {0: 2}], {0: 20}, flags=FG.P2C1)
    return timed(snap, 0, [(T1, T2, {0: 20, 1: 0}, None)]), [0, 1], EDGE


OWN = {
    "second-member-stopped-by-what-the-first-reserved": _second_stopped_by_the_first,
    "count-and-names-bind-at-different-instants": _different_throttles,
    "zero-valued-name-brings-presence": _zero_valued_name,
}


def directed():
    """name -> builder, negative-request cases of the gang forecast left out (built once to look)."""
    out = dict(OWN)
    for name, make in FG.DIRECTED.items():
        if not has_negative_request(make()[0]):
            out[name] = make
    return out


DIRECTED = directed()
