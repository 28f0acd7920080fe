"""The operational reference of the gang preemption query (kt_preempt_gangs_launch), shared by tests/test_preempt_gangs_cpu.py
and tests/test_preempt_gangs_gpu.py.

For k = 0 .. m_eff: a copy of the snapshot in which the candidates c_0 .. c_{k-1} are deleted, the oracle's reconcile at ``now``
written into the copy's stored status, then the oracle's in-order admission (PreFilter, and on Success Reserve) of the gang's
members.  The gang passes iff every member's verdict is Success; the first such k is the answer.  Nothing here shares code with
``paging.preempt_gangs_of`` or the kernel."""
import random

import numpy as np

import preempt_reference as PR
from kube_throttler_amd import snapshot as S

NONE = -1


def _without(snap, oracle_mod, deleted, now):
    """A copy of the cluster without the pod rows ``deleted``, every responsible throttle reconciled at now."""
    s = PR.copy_snapshot(snap)
    for c in deleted:
        s.pod_flags[int(c)] = 0
    rows = PR.responsible_rows(s)
    if len(rows):
        r = oracle_mod.Oracle(s).reconcile(now, rows=rows)
        s.apply_status(r.used, r.calc, r.calc_updated, r.thrl_flag, r.thrl_has, r.thrl_pod, r.error, rows=rows)
    return s


def first_blocked(snap, oracle_mod, members, deleted, now, on_equal):
    """The position in ``members`` of the first one whose verdict is not Success when the gang is admitted in order in the
    cluster without ``deleted`` (None: the gang passes)."""
    s = _without(snap, oracle_mod, deleted, now)
    _, summary, _ = oracle_mod.Oracle(s).admit(rows=np.asarray(members, np.int64), on_equal=on_equal)
    for j in range(len(members)):
        if int(summary[j]) & 3:
            return j
    return None


def members_ok(snap, oracle_mod, members) -> bool:
    """No member is invalid, and the oracle's check of none of them is an Error."""
    if any(not int(snap.pod_flags[p]) & S.POD_VALID for p in members):
        return False
    _, summary = oracle_mod.Oracle(snap).check(rows=np.asarray(members, np.int64), want_status=False)
    return all((int(w) & 3) != S.VERDICT_ERROR for w in summary)


def reference(snap, oracle_mod, members, cands, now=PR.NOW, on_equal=False):
    """-> (prefix, blocker): the smallest k whose S_k admits the whole gang (NONE: none does, or a member is invalid or an
    Error), and the position in ``members`` of the first member that is not Success in S_0 (-1 when the prefix is 0)."""
    members = [int(p) for p in members]
    blocker = first_blocked(snap, oracle_mod, members, [], now, on_equal)
    if blocker is None:
        return (0, -1) if members_ok(snap, oracle_mod, members) else (NONE, -1)
    if not members_ok(snap, oracle_mod, members):
        return NONE, blocker
    for k in range(1, PR.effective_length(snap, oracle_mod, cands) + 1):
        if first_blocked(snap, oracle_mod, members, cands[:k], now, on_equal) is None:
            return k, blocker
    return NONE, blocker


def check_victims(snap, oracle_mod, members, cands, prefix, victims, now=PR.NOW, on_equal=False):
    """The victim-mask property for gangs: all zero without a positive prefix, nothing at or beyond the prefix, only counted
    pods, and deleting exactly the masked pods lets the whole gang through."""
    victims = [int(v) for v in victims]
    assert len(victims) == len(cands)
    if prefix <= 0:
        assert not any(victims)
        return
    assert not any(victims[prefix:])
    masked = [c for c, v in zip(cands, victims) if v]
    for c in masked:
        assert (int(snap.pod_flags[c]) & (PR.COUNTED | S.POD_FINISHED)) == PR.COUNTED, f"victim {c} is not counted"
    assert first_blocked(snap, oracle_mod, members, masked, now, on_equal) is None, \
        f"gang {members}: deleting the masked pods {masked} does not let it through"


# ---- random cases on the clusters of tests/test_preempt_cpu.py ----
def gang_cases(seed, snap, n_cases=4):
    """[(member rows, candidate rows)]: gangs of 1 .. 4 pending pods (the fourth case, and clusters with too few pending pods,
    draw from all pods); the candidates are the other pods, shuffled and cut as ``preempt_reference.preempt_cases`` cuts them."""
    r = random.Random(15485863 * seed + 7)
    pending = [p for p in range(snap.n_pods) if (int(snap.pod_flags[p]) & PR.COUNTED) == PR.PENDING]
    out = []
    for case in range(n_cases):
        size = r.choice([1, 2, 2, 3, 4])
        pool = pending if len(pending) >= size and case != 3 else list(range(snap.n_pods))
        members = r.sample(pool, size)
        others = [c for c in range(snap.n_pods) if c not in members]
        r.shuffle(others)
        out.append((members, others[:r.choice([0, 3, len(others) // 2, len(others), len(others), len(others)])]))
    return out


# ---- directed cases on snapshots built by hand: name -> (builder of (snapshot, members, candidates), gang prefix at on_equal
#      False / True, the members' own prefixes at on_equal False / True or None where the table does not state them) ----
tiny, PENDING, COUNTED = PR.tiny, PR.PENDING, PR.COUNTED
_REQ1 = [{0: 1}] * 8
DIRECTED = {
    "two-members-throttle": (lambda: (tiny(_REQ1, {0: 4}, flags=[PENDING] * 2 + [COUNTED] * 6), [0, 1], [2, 3, 4, 5, 6, 7]),
                             (4, 5), ([3, 3], [4, 4])),
    "two-members-clusterthrottle": (lambda: (tiny(_REQ1, {0: 4}, cluster=True, flags=[PENDING] * 2 + [COUNTED] * 6), [0, 1], [2, 3, 4, 5, 6, 7]),
                                    (4, 5), ([3, 3], [4, 4])),
    "count-threshold": (lambda: (tiny(_REQ1, {}, count=4, flags=[PENDING] * 3 + [COUNTED] * 5), [0, 1, 2], [3, 4, 5, 6, 7]),
                        (4, 5), ([2, 2, 2], [3, 3, 3])),
    # the first member's zero-valued reservation makes name 0 PRESENT in reserved: step 3 (0 >= 0 on a Throttle) stops the second
    "zero-reservation-makes-present": (lambda: (tiny([{0: 0}, {0: -1}, {1: 1}, {1: 1}], {0: 0}, flags=[PENDING] * 2 + [COUNTED] * 2), [0, 1], [2, 3]),
                                       (NONE, NONE), ([0, 0], [0, 0])),
    "zero-reservation-last": (lambda: (tiny([{0: 0}, {0: -1}, {1: 1}, {1: 1}], {0: 0}, flags=[PENDING] * 2 + [COUNTED] * 2), [1, 0], [2, 3]),
                              (0, 0), ([0, 0], [0, 0])),
    "member-exceeds-threshold": (lambda: (tiny([{0: 1}, {0: 11}, {0: 4}, {0: 4}], {0: 10}, flags=[PENDING] * 2 + [COUNTED] * 2), [0, 1], [2, 3]),
                                 (NONE, NONE), None),
    "three-members-too-large-together": (lambda: (tiny([{0: 4}] * 5, {0: 10}, flags=[PENDING] * 3 + [COUNTED] * 2), [0, 1, 2], [3, 4]),
                                         (NONE, NONE), ([1, 1, 1], [1, 1, 1])),
    "member-without-namespace-object": (lambda: (tiny([{0: 1}] * 4, {0: 10}, cluster=True, flags=[PENDING] * 2 + [COUNTED] * 2, pod_ns=[0, 1, 0, 0]),
                                                 [0, 1], [2, 3]), (NONE, NONE), None),
    "reserved": (lambda: (tiny([{0: 1}] * 2 + [{0: 3}] * 3, {0: 10}, count=5, flags=[PENDING] * 2 + [COUNTED] * 3, reserved=({0: 4}, 2)),
                          [0, 1], [2, 3, 4]), (2, 3), None),
}
