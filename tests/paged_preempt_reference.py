"""The reference of the paged preemption query (kt_paged_preempt), shared by tests/test_paged_preempt_cpu.py and
tests/test_paged_preempt_gpu.py.  It extends tests/preempt_reference.py to a list of page snapshots.

For a deleted set: a copy of every page's snapshot with the deleted rows' pod_flags = 0, the oracle's reconcile per page, the
``calc_updated`` and ``error`` bytes OR-ed over the pages (status.calculatedThreshold is replaced as a whole; a reconcile that is
an error is an error of the throttle), ``apply_status`` per page with the OR-ed bytes for the rows whose OR-ed error is clear,
the oracle's check of the preemptor per page, and ``paging.combine_status`` / ``verdicts``.  The prefix is the first k that
passes; the reprieve is the literal walk with this judge.  Nothing here shares code with ``paging.paged_preempt_of`` or the
kernels."""
import numpy as np

import preempt_reference as PR
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S

NOW = PR.NOW
PENDING, COUNTED = PR.PENDING, PR.COUNTED


def passes_without(snaps, oracle_mod, p, deleted, now=NOW, on_equal=False) -> bool:
    """PreFilter(p) is Success in the cluster without the pod rows ``deleted``, every responsible throttle reconciled at now
    on every page."""
    copies = [PR.copy_snapshot(s) for s in snaps]
    for s in copies:
        for c in deleted:
            s.pod_flags[int(c)] = 0
    rows = PR.responsible_rows(copies[0])
    if len(rows):
        results = [oracle_mod.Oracle(s).reconcile(now, rows=rows) for s in copies]
        updated = np.zeros(len(rows), np.uint8)
        error = np.zeros(len(rows), np.uint8)
        for r in results:
            updated |= (np.asarray(r.calc_updated[:len(rows)]) != 0).astype(np.uint8)
            error |= (np.asarray(r.error[:len(rows)]) != 0).astype(np.uint8)
        for s, r in zip(copies, results):
            s.apply_status(r.used, r.calc, updated, r.thrl_flag, r.thrl_has, r.thrl_pod, error, rows=rows)
    status = paging.combine_status([oracle_mod.Oracle(s).check(rows=np.array([p], np.int64), on_equal=on_equal)[0] for s in copies])
    return int(paging.verdicts(status)[0]) == S.VERDICT_ALLOW


def reference_prefix(snaps, oracle_mod, p, cands, now=NOW, on_equal=False) -> int:
    snap0 = snaps[0]  # validity, the error rows and the list cut are the same in every page
    if not int(snap0.pod_flags[p]) & S.POD_VALID:
        return -1
    _, summary = oracle_mod.Oracle(snap0).check(rows=np.array([p], np.int64), want_status=False)
    if (int(summary[0]) & 3) == S.VERDICT_ERROR:
        return -1
    for k in range(PR.effective_length(snap0, oracle_mod, cands) + 1):
        if passes_without(snaps, oracle_mod, p, cands[:k], now, on_equal):
            return k
    return -1


def reference_reprieve(snaps, oracle_mod, p, cands, prefix, now=NOW, on_equal=False):
    """The walk over the whole prefix (tests/reprieve_reference.py says why no mask is needed)."""
    if prefix <= 0:
        return [0] * len(cands)
    victims = [int(j < prefix) for j in range(len(cands))]
    for j in range(prefix - 1, -1, -1):
        rest = [c for q, c in enumerate(cands) if victims[q] and q != j]
        if passes_without(snaps, oracle_mod, p, rest, now, on_equal):
            victims[j] = 0
    return victims


def reference(snaps, oracle_mod, p, cands, now=NOW, on_equal=False):
    """-> (prefix, reprieved victims), all by delete + reconcile + check."""
    k = reference_prefix(snaps, oracle_mod, p, cands, now, on_equal)
    return k, reference_reprieve(snaps, oracle_mod, p, cands, k, now, on_equal)


def check_victims(snaps, oracle_mod, p, cands, prefix, victims, now=NOW, on_equal=False):
    """The victim-mask property of the prefix query: all zero without a positive prefix, nothing at or beyond the prefix, only
    counted pods, and deleting exactly the masked pods lets the preemptor through."""
    victims = [int(v) for v in victims]
    assert len(victims) == len(cands)
    if prefix <= 0:
        assert not any(victims)
        return
    assert not any(victims[prefix:])
    masked = [c for c, v in zip(cands, victims) if v]
    for c in masked:
        assert (int(snaps[0].pod_flags[c]) & (COUNTED | S.POD_FINISHED)) == COUNTED, f"victim {c} is not counted"
    assert passes_without(snaps, oracle_mod, p, masked, now, on_equal), f"pod {p}: deleting the masked pods {masked} does not let it through"


# ---- directed cases: (page snapshots, preemptor, candidates) ----
def pages_of(requests, thresholds, flags, counts=None, D=1, **kw):
    """Hand-built pages over the same pods, flags and selector (``preempt_reference.tiny`` builds each): ``requests[k]`` are
    page k's per-pod {dim: value}, ``thresholds[k]`` its throttle's {dim: value}.  A pod that carries no name of a page is a pod
    with a container that requests nothing there."""
    counts = counts or [None] * len(requests)
    return [PR.tiny(req, th, count=c, flags=flags, D=D, **kw) for req, th, c in zip(requests, thresholds, counts)]


def non_monotone():
    """Page 0, name a: threshold 10, the preemptor asks 3, a running non-candidate holds 6, the candidates hold +4, -4, +4:
    `used` is 10 -> 6, 10, 6 for k = 1, 2, 3 — it passes at k = 1 and 3 and fails at 2.  Page 1, name b: threshold 10, the
    preemptor asks 3, the non-candidate holds 4, the candidates 1, 4, 1: 10 -> 9, 5, 4 — it passes from k = 2 on.  The answer
    is 3, not max(1, 2)."""
    flags = [PENDING] + [COUNTED] * 4
    return pages_of([[{0: 3}, {0: 6}, {0: 4}, {0: -4}, {0: 4}], [{0: 3}, {0: 4}, {0: 1}, {0: 4}, {0: 1}]], [{0: 10}, {0: 10}], flags), 0, [2, 3, 4]


def second_page_line(m=70, k_star=66):
    """``preempt_reference.line`` on page 1 (the only threshold name is there), page 0 carries an unrelated name under no
    threshold: exactly k_star of the m candidates have to go, across the blocks of 64."""
    snap1, p, cands = PR.line(m, k_star, D=2, dim=1)
    snap0 = PR.tiny([{0: 1}] + [{0: 2, 1: 1}] * m, {}, flags=[PENDING] + [COUNTED] * m, D=2)
    return [snap0, snap1], p, cands


def count_only():
    """A pod-count threshold alone (2), names on two pages under no threshold: the count is judged once."""
    flags = [PENDING] + [COUNTED] * 3
    return pages_of([[{0: 1}] * 4, [{0: 2}] * 4], [{}, {}], flags, counts=[2, 2]), 0, [1, 2, 3]


def reprieve_across_pages():
    """Thresholds 10 on name a (page 0) and on name b (page 1); the preemptor asks 3 of each.  Non-candidate: a 2, b 2.
    Candidates: c0 = (a 1, b 6), c1 = (a 6, b 1), c2 = (a 1, b 1), c3 = (a 1, b 1).  `used` is a 11, b 11; the pod needs
    used + 3 <= 10 on both pages: the prefix is 2 (a 4, b 4 — after c0 alone a is 10).  The walk from [c0, c1]: c1 back makes
    a 4 + 6 + 3 > 10 — page 0 keeps it although page 1 alone (b 5 + 3) would reprieve it; c0 back makes b 4 + 6 + 3 > 10 — page 1
    keeps it although page 0 alone (a 5 + 3) would reprieve it."""
    flags = [PENDING] + [COUNTED] * 5
    a = [{0: 3}, {0: 2}, {0: 1}, {0: 6}, {0: 1}, {0: 1}]
    b = [{0: 3}, {0: 2}, {0: 6}, {0: 1}, {0: 1}, {0: 1}]
    return pages_of([a, b], [{0: 10}, {0: 10}], flags), 0, [2, 3, 4, 5]


def reprieve_one_page_decides():
    """As above with small extra victims in front: c0 = (a 1, b 0), c1 = (a 0, b 1), then the two big ones.  The prefix reaches
    the second big one; the walk puts the small ones back only where BOTH pages still pass."""
    flags = [PENDING] + [COUNTED] * 5
    a = [{0: 3}, {0: 2}, {0: 1}, {0: 0}, {0: 6}, {0: 1}]
    b = [{0: 3}, {0: 3}, {0: 0}, {0: 1}, {0: 1}, {0: 6}]
    return pages_of([a, b], [{0: 10}, {0: 10}], flags), 0, [2, 3, 4, 5]


def unequal_widths(m=9):
    """A 16-name page and a 3-name page: the DT bucket of the widest page serves the narrow one.  Name 15 of page 0 and name 2
    of page 1 are under thresholds, the other names ride along."""
    flags = [PENDING] + [COUNTED] * m
    wide = [{15: 2, 0: 1}] + [{15: 1 + j % 3, 3: 2, 7: j} for j in range(m)]
    narrow = [{2: 2}] + [{2: 1 + (j + 1) % 3, 0: 1} for j in range(m)]
    used_w, used_n = sum(q[15] for q in wide[1:]), sum(q[2] for q in narrow[1:])
    return [PR.tiny(wide, {15: used_w - 4}, flags=flags, D=16), PR.tiny(narrow, {2: used_n - 7}, flags=flags, D=3)], 0, list(range(1, m + 1))


def long_list(L=70, m=40, n_pre=3):
    """``reprieve_reference.wide`` (L affecting throttles, each name asks for its own victims) as page 0 and the same pods with
    other amounts as page 1: a list longer than 64 entries with binding names on both pages."""
    import reprieve_reference as RR
    s0, pre, cands = RR.wide(L, m, D=3, seed=0, n_pre=n_pre)
    s1, _, _ = RR.wide(L, m, D=3, seed=5, n_pre=n_pre)
    return [s0, s1], pre, cands


DIRECTED = {
    "non-monotone-pages": non_monotone,
    "second-page-name-across-blocks": second_page_line,
    "pod-count-only": count_only,
    "reprieve-across-pages": reprieve_across_pages,
    "reprieve-one-page-decides": reprieve_one_page_decides,
    "unequal-widths": unequal_widths,
}
