"""The operational reference of the elastic gang preemption query (kt_preempt_gangs_elastic_launch), shared by
tests/test_preempt_gangs_elastic_cpu.py and tests/test_preempt_gangs_elastic_gpu.py.

For k = 0 .. m_eff: ``preempt_gangs_reference._without`` — a copy of the snapshot in which the candidates c_0 .. c_{k-1} are deleted
and the oracle's reconcile at ``now`` is written into the stored status — then the oracle's in-order admission of the gang's members
in that copy.  That admission walks past a member that failed and reserves on Success only, so its summary words ARE the success
list of the elastic walk; ``forecast_gangs_elastic_reference.rule`` (quorum, required members, members that never succeed) is
applied to the lists, and the first k that passes is the prefix.  The victim mask is read off the oracle's status matrix; the
reprieve is written as its definition: put c_j back, walk again, keep it back iff the rule still holds.  Nothing here shares code
with ``paging.preempt_gangs_elastic_of`` or the kernel."""
import collections
import functools

import numpy as np

import forecast_gangs_elastic_reference as FE
import preempt_gangs_reference as GR
import preempt_reference as PR
from kube_throttler_amd import snapshot as S

NONE = -1
A, B, ERR = FE.A, FE.B, FE.ERR

# prefix; victims [len(cands)] (plain and reprieved); members in the final state (plain and reprieved); blocker as a position in
# ``members``; the verdicts and success counts of k = 0 .. m_eff (every k, also behind the prefix)
Answer = collections.namedtuple("Answer", "prefix victims members blocker reprieved reprieved_members verdicts counts")


class Walks:
    """The success lists of one gang in the states S(V), each state built once and walked at both on_equal values."""

    def __init__(self, snap, oracle_mod, members, now):
        self.snap, self.oracle_mod, self.now = snap, oracle_mod, now
        self.rows = np.asarray([int(p) for p in members], np.int64)
        self.valid = [bool(int(snap.pod_flags[p]) & S.POD_VALID) for p in self.rows]
        self.cache = {}

    def ok(self, deleted, on_equal):
        key = tuple(sorted(int(c) for c in deleted))
        if key not in self.cache:
            s = GR._without(self.snap, self.oracle_mod, key, self.now)
            o = self.oracle_mod.Oracle(s)
            self.cache[key] = {eq: [not int(w) & 3 and v for w, v in zip(o.admit(rows=self.rows, on_equal=eq)[1], self.valid)]
                               for eq in (False, True)}
        return self.cache[key][bool(on_equal)]


def touching(snap, oracle_mod, members, cands):
    """Per candidate: it is counted, and a throttle that affects at least one member matches it.  The status matrix of the oracle's
    check says who is affected by whom; the row of a member whose PreFilter is an Error names no throttle."""
    if not len(cands):
        return []
    o = oracle_mod.Oracle(snap)
    mstat, msum = o.check(rows=np.asarray(members, np.int64))
    cstat, _ = o.check(rows=np.asarray(cands, np.int64))
    union = np.zeros(snap.n_thr, bool)
    for j in range(len(members)):
        if (int(msum[j]) & 3) != ERR:
            union |= np.asarray(mstat[j][:snap.n_thr]) != 0
    counted = [(int(snap.pod_flags[c]) & (PR.COUNTED | S.POD_FINISHED)) == PR.COUNTED for c in cands]
    return [bool(counted[j] and (union & (np.asarray(cstat[j][:snap.n_thr]) != 0)).any()) for j in range(len(cands))]


def _passes(ok, never, quorum, required):
    _, verdicts, counts, _ = FE.rule([ok], never, quorum, required)
    return verdicts[0] == A, counts[0]


def reference(snap, oracle_mod, members, quorum, required, cands, now=PR.NOW):
    """-> {on_equal: Answer} of the one gang ``members`` (pod rows, in order) under the rule."""
    members, cands = [int(p) for p in members], [int(c) for c in cands]
    m_eff = PR.effective_length(snap, oracle_mod, cands)
    never = FE.never_succeeds(snap, oracle_mod, members)
    touch = touching(snap, oracle_mod, members, cands)
    walks = Walks(snap, oracle_mod, members, now)
    out = {}
    for eq in (False, True):
        oks = [walks.ok(cands[:k], eq) for k in range(m_eff + 1)]
        _, verdicts, counts, blockers = FE.rule(oks, never, quorum, required)
        prefix = next((k for k, v in enumerate(verdicts) if v == A), NONE)  # (the rule out of reach: ERR at every k)
        victims = [int(j < prefix and touch[j]) for j in range(len(cands))]
        count = counts[prefix] if prefix >= 0 else counts[0]
        # the reprieve: V = M, c_{prefix-1} first
        kept, kept_count = list(victims), count
        for j in range(prefix - 1, -1, -1):
            if not kept[j]:
                continue
            trial = list(kept)
            trial[j] = 0
            passes, n_ok = _passes(walks.ok([c for c, v in zip(cands, trial) if v], eq), never, quorum, required)
            if passes:
                kept, kept_count = trial, n_ok
        if prefix > 0:  # deleting exactly the masked pods gives the success list of S_prefix
            assert walks.ok([c for c, v in zip(cands, victims) if v], eq) == oks[prefix]
        out[eq] = Answer(prefix, victims, count, -1 if prefix == 0 else blockers[0], kept, kept_count, verdicts, counts)
    return out


# ---- the seeded cases: the clusters and gangs of tests/test_preempt_gangs_cpu.py under forecast_gangs_elastic_reference.seeded_rule ----
@functools.lru_cache(maxsize=None)
def seeded_reference(seed, oracle_mod):
    """(snapshot, [(members, candidates, quorum, required)], [{on_equal: Answer} per case], [{on_equal: whole-gang prefix} per case])
    — computed once, never modified."""
    from test_preempt_gangs_cpu import gang_case
    snap, cases, whole, _ = gang_case(seed, oracle_mod)
    ruled = [(ms, cands) + FE.seeded_rule(seed, case, len(ms)) for case, (ms, cands) in enumerate(cases)]
    want = [reference(snap, oracle_mod, ms, q, req, cands) for ms, cands, q, req in ruled]
    return snap, ruled, want, [{eq: whole[eq][case][0] for eq in (False, True)} for case in range(len(cases))]


# ---- directed cases, derived by hand: one Throttle with threshold {0: 10}, members [0, 1], quorum 1 ----
P, C = PR.PENDING, PR.COUNTED
# name -> (requests, flags, candidates, required, {on_equal: (prefix, victims, members, blocker, reprieved victims, reprieved members)},
#          {on_equal: verdicts over k} or None)
HAND = {
    # k = 0: used 9, m0 (8) fails, m1 (4) fails.  k = 1: used 6, m0 fails, m1 passes (10 > 10 is false; on equal it does not).  k = 2:
    # used 3, m0 fails (11), m1 passes.  k = 3: used 0, m0 passes and reserves 8: m1 meets 12 — more victims shut the required member out
    "more-victims-shut-the-required-member-out": (
        [{0: 8}, {0: 4}, {0: 3}, {0: 3}, {0: 3}], [P, P, C, C, C], [2, 3, 4], [False, True],
        {False: (1, [1, 0, 0], 1, 1, [1, 0, 0], 1), True: (2, [1, 1, 0], 1, 1, [1, 1, 0], 1)},
        {False: [B, A, A, B], True: [B, B, A, B]}),
    # used 9 with a pod of 4 that is no candidate.  Only k = 3 lets m1 in (4 + 4 <= 10, < 10 on equal); the reprieve puts the 3 back
    # first — it fails — and then walks past it to the small victims: both come back (4 + 1 + 1 + 4 = 10), on equal only the last one
    "reprieve-past-small-victims": (
        [{0: 8}, {0: 4}, {0: 1}, {0: 1}, {0: 3}, {0: 4}], [P, P, C, C, C, C], [2, 3, 4], [False, True],
        {False: (3, [1, 1, 1], 1, 1, [0, 0, 1], 1), True: (3, [1, 1, 1], 1, 1, [1, 0, 1], 1)}, None),
    # k = 2: used 0, both members in (4, then 4 + 4).  The reprieve puts the 8 back first — m0 fails (12) — then the 3: m0 passes
    # (3 + 4), m1 does not (3 + 4 + 4 = 11): quorum 1 with m0 required still holds, one member in
    "reprieve-changes-who-is-in": (
        [{0: 4}, {0: 4}, {0: 3}, {0: 8}], [P, P, C, C], [2, 3], [True, False],
        {False: (2, [1, 1], 2, 0, [0, 1], 1), True: (2, [1, 1], 2, 0, [0, 1], 1)}, None),
}


def hand_case(name):
    requests, flags, cands, required, _, _ = HAND[name]
    return PR.tiny(requests, {0: 10}, flags=flags), [0, 1], 1, required, cands


# ---- the directed tables of the gang preemption and of the elastic forecast that carry over, under quorum 1:
#      name -> () -> (snapshot, members, quorum, required or None, candidates) ----
def _ghost_gang(required):
    # member 1 lives in a namespace without object: its PreFilter is an Error (the ClusterThrottle needs the namespace)
    snap = PR.tiny([{0: 4}, {0: 1}, {0: 4}, {0: 4}], {0: 10}, cluster=True, flags=[P, P, C, C], pod_ns=[0, 1, 0, 0])
    return snap, [0, 1], 1, required, [2, 3]


def _invalid_gang(required):
    snap = PR.tiny([{0: 4}, {0: 1}, {0: 4}, {0: 4}], {0: 10}, flags=[P, 0, C, C])
    return snap, [0, 1], 1, required, [2, 3]


def _error_throttle():
    snap, p, cands = PR.DIRECTED["error-throttle-override-active"]()
    return snap, [p], 1, None, cands


CARRIED = {
    "error-member-not-required": lambda: _ghost_gang(None),
    "error-member-required": lambda: _ghost_gang([False, True]),
    "invalid-member-not-required": lambda: _invalid_gang(None),
    "invalid-member-required": lambda: _invalid_gang([False, True]),
    # quorum 2 of 2 with one member that never succeeds
    "quorum-out-of-reach": lambda: _ghost_gang(None)[:2] + (2, None, [2, 3]),
    "error-throttle-keeps-its-stored-status": _error_throttle,
    "stored-reserved-amounts": lambda: GR.DIRECTED["reserved"][0]()[:2] + (1, None, GR.DIRECTED["reserved"][0]()[2]),
    "stored-reserved-amounts-both-required": lambda: GR.DIRECTED["reserved"][0]()[:2] + (1, [True, True], GR.DIRECTED["reserved"][0]()[2]),
    "zero-reservation-makes-present": lambda: GR.DIRECTED["zero-reservation-makes-present"][0]()[:2] + (1, None, [2, 3]),
    "zero-reservation-makes-present-second-required": lambda: GR.DIRECTED["zero-reservation-makes-present"][0]()[:2] + (1, [False, True], [2, 3]),
    "zero-reservation-last": lambda: GR.DIRECTED["zero-reservation-last"][0]()[:2] + (2, None, [2, 3]),
    "presence-through-one-victim": lambda: (PR.DIRECTED["presence-through-one-victim"]()[0], [0], 1, None, [2, 1]),
    "error-candidate-cuts": lambda: (PR.DIRECTED["error-candidate-cuts"]()[0], [0], 1, [True], [1, 3, 2, 4, 5]),
    "three-members-too-large-together": lambda: GR.DIRECTED["three-members-too-large-together"][0]()[:2] + (1, None, [3, 4]),
    "member-exceeds-threshold": lambda: GR.DIRECTED["member-exceeds-threshold"][0]()[:2] + (1, None, [2, 3]),
}


def directed_cases():
    """name -> () -> (snapshot, members, quorum, required, candidates): the hand-derived and the carried cases together."""
    out = {name: (lambda n=name: hand_case(n)) for name in HAND}
    out.update(CARRIED)
    return out
