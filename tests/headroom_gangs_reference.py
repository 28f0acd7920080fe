"""The reference of the gang headroom (kt_headroom_gangs_launch): the admission walk itself.

``headroom_gangs(gang, cap, on_equal)`` is DEFINED as the number of leading admitted gangs of a dry gang admission over ``cap``
consecutive copies of the gang.  Before the first copy that is not admitted in full nothing is rolled back, so the plain walk
and the gang walk are in the same state there (tests/test_gang_admit_cpu.py pins "one gang of allowed pods is kto_admit"): the
number of leading COMPLETE copies of the plain admission of ``members * cap`` is the answer, and the first position of that walk
that is not Success names the blocker (its place inside the gang) and, by the row PreFilter returned to it, the limiting
throttle.  Two forms: the C oracle's ``kto_admit`` on a snapshot (at most 16 resource names), and the manifest model's
``model_admit`` (any number of names).  Nothing here reads paging.headroom_gangs_of or the engine."""
import copy

import numpy as np

from kube_throttler_amd import snapshot as S
from test_paged_admit_cpu import model_admit


def answer_of_walk(verdict_codes, rows_of_blocked, g, cap):
    """(copies, limiting, blocker position inside the gang) from the walk's verdicts (0: Success, 2: Error, else blocked) over
    ``g * cap`` positions; ``rows_of_blocked(k)``: the ascending throttle rows that are not `not-throttled` at position k."""
    k = next((i for i, v in enumerate(verdict_codes) if v != 0), None)
    if k is None:
        return cap, -1, -1
    limiting = -1 if verdict_codes[k] == 2 else min(rows_of_blocked(k))
    return k // g, limiting, k % g


def oracle_walk(o, members, cap, on_equal):
    """(status [g * cap][T], verdict codes [g * cap]) of the C oracle's admit of ``members * cap``."""
    status, summary, _ = o.admit(rows=np.tile(np.asarray(members, np.int64), cap), on_equal=on_equal)
    return status, [2 if w == 2 else 1 if w != 0 else 0 for w in summary]


def headroom_gangs_by_oracle(o, members, cap, on_equal):
    status, codes = oracle_walk(o, members, cap, on_equal)
    blocked = lambda k: [int(t) for t in np.nonzero((status[k] != S.NOT_AFFECTED) & (status[k] != S.NOT_THROTTLED))[0]]
    return answer_of_walk(codes, blocked, len(members), cap)


def headroom_gangs_by_model(cs, thr_names, members, cap, on_equal):
    """The same on the manifests (``thr_names``: throttle row -> name, as the page bundle lists them)."""
    res = model_admit(copy.deepcopy(cs), list(members) * cap, on_equal)
    codes = [{"allow": 0, "error": 2}.get(v, 1) for v, _ in res]
    blocked = lambda k: [t for t, nn in enumerate(thr_names) if res[k][1].get(nn, "not-throttled") != "not-throttled"]
    return answer_of_walk(codes, blocked, len(members), cap)
