"""The reference of the gang reprieve pass (kt_preempt_gangs_reprieve_launch), shared by tests/test_preempt_gangs_reprieve_cpu.py,
tests/test_preempt_gangs_reprieve_gpu.py and tests/test_host_preempt_gang_reprieve_gpu.py.

The walk of the definition, step by step, on ``preempt_gangs_reference.first_blocked(...) is None`` (delete, oracle reconcile,
oracle in-order admission of the gang) and nothing else: for j = k-1 .. 0 the candidate c_j is put back when the whole gang is
still admitted in the cluster without the remaining victims.  Nothing here shares code with ``paging.preempt_gangs_of`` or the
kernel.  The directed table is built by hand on ``preempt_reference.tiny`` and from a few manifests; ``gang_big_last`` and
``gang_wide`` build the shapes of the GPU suite."""
import preempt_gangs_reference as GR
import preempt_reference as PR
import reprieve_reference as RR
from kube_throttler_amd.objects import ClusterState

NOW, NONE = PR.NOW, GR.NONE
PENDING, COUNTED, tiny = PR.PENDING, PR.COUNTED, PR.tiny


def reference_reprieve(snap, oracle_mod, members, cands, prefix, now=NOW, on_equal=False):
    """-> the reprieved victim bytes [len(cands)] behind the gang prefix ``prefix``.  The walk starts from the WHOLE prefix deleted
    and visits every position: a candidate outside the prefix mask — not counted, or matched by no throttle that affects a member —
    changes nothing the admission of the gang reads, comes back at its turn and is not a victim, so the walk over the mask and the
    walk over the prefix end in the same set; this one needs no mask."""
    if prefix <= 0:
        return [0] * len(cands)
    members = [int(p) for p in members]
    victims = [int(j < prefix) for j in range(len(cands))]
    for j in range(prefix - 1, -1, -1):
        rest = [c for q, c in enumerate(cands) if victims[q] and q != j]
        if GR.first_blocked(snap, oracle_mod, members, rest, now, on_equal) is None:
            victims[j] = 0
    return victims


def reference(snap, oracle_mod, members, cands, now=NOW, on_equal=False):
    """-> (prefix, reprieved victims, blocker), all by delete + reconcile + in-order admission."""
    k, b = GR.reference(snap, oracle_mod, members, cands, now, on_equal)
    return k, reference_reprieve(snap, oracle_mod, members, cands, k, now, on_equal), b


# ---- directed cases ----
def labelled(pods, throttles):
    """A namespace of pods (name, labels, cpu, running) — pod rows in that order — under Throttles (name, label key, cpu) that
    select the pods carrying ``key``: "1" -> the snapshot."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    for name, labels, cpu, running in pods:
        spec = {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": {"cpu": cpu}}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {k: "1" for k in labels}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    for name, key, cpu in throttles:
        cs.add({"kind": "Throttle", "metadata": {"name": name, "namespace": "ns0"},
                "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": cpu}},
                         "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {key: "1"}}}]}}})
    return cs.build_pages()[0].snapshot


def member_specific_throttles():
    """Member A carries label a, member B label b, each asks 5; thr-a and thr-b (cpu 10) are at 9 through a small (1) and a big
    (8) pod of their own.  Each throttle needs ITS big pod gone and judges only ITS member: both small pods come back (1 + 5).
    A list entry that walked the member it does not affect — in the judge, or in the reserved prefix — would meet 1 + 5 + 5 > 10
    and keep the small pods out."""
    snap = labelled([("a", "a", "5", False), ("b", "b", "5", False), ("small-a", "a", "1", True), ("big-a", "a", "8", True),
                     ("small-b", "b", "1", True), ("big-b", "b", "8", True)], [("thr-a", "a", "10"), ("thr-b", "b", "10")])
    return snap, [0, 1], [2, 4, 3, 5]


def second_member_only():
    """thr-b (cpu 10) selects the second member (asks 3) and the candidates: small 1, big 8.  The first member (asks 9, no label
    b) is affected by nothing.  With its 9 in thr-b's reserved prefix nobody would ever come back (9 + 1 + 3 > 10) and the prefix
    itself would be NONE; without it the small pod returns."""
    snap = labelled([("first", "x", "9", False), ("second", "b", "3", False), ("small-b", "b", "1", True), ("big-b", "b", "8", True)],
                    [("thr-b", "b", "10")])
    return snap, [0, 1], [2, 3]


def _single(name):
    """A directed case of reprieve_reference as a gang of one."""
    def build():
        snap, p, cands = RR.DIRECTED[name]()
        return snap, [p], cands
    return build


# name -> (builder of (snapshot, members, candidates), prefix at on_equal False / True, reprieved victims at on_equal False / True)
DIRECTED = {
    # threshold 10, the members ask 2 and 1, a bystander uses 4, the candidates 1, 1, 6 -> only the 6 has to go
    "gang-one-one-six": (lambda: (tiny([{0: 2}, {0: 1}, {0: 4}, {0: 1}, {0: 1}, {0: 6}], {0: 10}, flags=[PENDING] * 2 + [COUNTED] * 4),
                                  [0, 1], [3, 4, 5]), (3, 3), ([0, 0, 1], [0, 0, 1])),
    # two members of 3 under 10 with four running 2s: the second member meets the first one's 3 reserved -> `used` has to come
    # down to 4 (below 4 with on_equal); each member alone is content with one victim
    "reserved-prefix-keeps-victims": (lambda: (tiny([{0: 3}, {0: 3}] + [{0: 2}] * 4, {0: 10}, flags=[PENDING] * 2 + [COUNTED] * 4),
                                               [0, 1], [2, 3, 4, 5]), (2, 3), ([1, 1, 0, 0], [1, 1, 1, 0])),
    "member-specific-throttles": (member_specific_throttles, (4, 4), ([0, 0, 1, 1], [0, 0, 1, 1])),
    "second-member-only": (second_member_only, (2, 2), ([0, 1], [0, 1])),
    "zero-reservation-makes-present": (GR.DIRECTED["zero-reservation-makes-present"][0], (NONE, NONE), ([0, 0], [0, 0])),
    "zero-valued-name-comes-back": (_single("zero-valued-name-comes-back"), (2, 2), ([0, 1], [0, 1])),
    "negative-request-candidate": (_single("negative-request-candidate"), (2, 2), ([0, 1, 0], [0, 1, 0])),
    "error-throttle-beside-a-reconciled-one": (_single("error-throttle-beside-a-reconciled-one"), (3, 3), ([0, 0, 1], [0, 0, 1])),
    # a pod count threshold of 4, three members, five running candidates of 1: the third member meets a reserved count of 2, one
    # running pod may stay (none with on_equal) — the candidates are all alike, the reserved count prefix refuses every reprieve
    "count-threshold": (GR.DIRECTED["count-threshold"][0], (4, 5), ([1, 1, 1, 1, 0], [1, 1, 1, 1, 1])),
}


# ---- the shapes of the GPU suite ----
def gang_big_last(m, D=2, dim=0, **kw):
    """Pods 0 and 1 pending, asking 1 of ``dim`` each; candidates 2 .. m + 1 running with 1 of ``dim`` each, except the last but
    one in list order, which uses m; threshold m + 1.  `used` is 2 m - 1 and has to come down to m - 1 for the second member
    (1 reserved + 1): only with the big pod gone, so the prefix is m - 1 and its mask m - 1 ones; the walk keeps the big pod out
    and puts the m - 2 small ones before it back (all but one of them with on_equal) — the masked positions straddle the blocks
    of 64 candidates -> (snapshot, members, candidates)."""
    other = {d: 2 for d in range(D) if d != dim}
    small, big = dict(other), dict(other)
    small[dim], big[dim] = 1, m
    reqs = [small] * m
    reqs[m - 2] = big
    snap = tiny([{dim: 1}] * 2 + reqs, {dim: m + 1}, flags=[PENDING] * 2 + [COUNTED] * m, D=D, **kw)
    return snap, [0, 1], list(range(2, m + 2))


def gang_wide(L, m, g=2, D=3, T=None, seed=0):
    """``reprieve_reference.wide`` with its ``g`` pending pods as ONE gang: L Throttles select every pod, the last D of the list
    bind one name each at about 0.55 of what is used, and every member asks 1 .. 2 of every name -> (snapshot, members,
    candidates)."""
    return RR.wide(L, m, D=D, T=T, seed=seed, n_pre=g)
