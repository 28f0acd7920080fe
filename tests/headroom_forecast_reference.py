"""The reference of the headroom forecast (kt_headroom_forecast_launch), shared by tests/test_headroom_forecast_cpu.py and
tests/test_headroom_forecast_gpu.py.

Per instant t_k: ``forecast_reference.state_at`` (a copy of the snapshot, the oracle's reconcile at t_k written into the stored
status), then the oracle's admit of ``[p] * cap`` on that state: copies = the leading Successes, limiting = the first row of the
first refused copy that is neither not-affected nor not-throttled.  Nothing here shares code with
``paging.headroom_forecast_of`` or the kernel."""
import numpy as np

import forecast_reference as FR
import preempt_reference as PR
from kube_throttler_amd import snapshot as S

CAP = 16


def oracle_headroom(o, p, cap, on_equal=False):
    """(copies, limiting) by the oracle's admit of [p] * cap (it adds the pod's amount once per queue position)."""
    status, summary, _ = o.admit(rows=np.full(cap, p, np.int64), on_equal=on_equal)
    verdicts = summary & 3
    k = next((j for j in range(cap) if int(verdicts[j]) != S.VERDICT_ALLOW), cap)
    if k == cap or int(verdicts[k]) == S.VERDICT_ERROR:
        return k, -1
    return k, int(np.nonzero((status[k] != S.NOT_AFFECTED) & (status[k] != S.NOT_THROTTLED))[0][0])


def reference(snap, oracle_mod, pods, instants, cap, on_equal=False, states=None):
    """-> (copies int64 [len(pods)][len(instants)], limiting int32 alike); an invalid pod row is 0 and -1 throughout."""
    copies = np.zeros((len(pods), len(instants)), np.int64)
    limiting = np.full((len(pods), len(instants)), -1, np.int32)
    for k, t in enumerate(instants):
        o = oracle_mod.Oracle(states[k] if states is not None else FR.state_at(snap, oracle_mod, t))
        for i, p in enumerate(pods):
            if 0 <= int(p) < snap.n_pods and int(snap.pod_flags[int(p)]) & S.POD_VALID:
                copies[i, k], limiting[i, k] = oracle_headroom(o, int(p), cap, on_equal)
    return copies, limiting


def first_of(copies, want):
    """Per row the first position with at least ``want`` copies, or -1."""
    return [next((k for k, c in enumerate(row) if int(c) >= want), -1) for row in copies]


# ---- directed cases of the headroom forecast's own: name -> () -> (snapshot, pod row, instants) ----
T1, T2 = FR.T1, FR.T2


def _tie():
    # rows 0 and 1 both select the pod; used 8, the pod asks 3.  Row 0: cpu 14 throughout (2 copies).  Row 1: cpu 11 (1 copy),
    # 14 between T1 and T2: there both admit 2 copies and the LOWER row is the limiting one
    snap = PR.tiny([{0: 3}] + [{0: 4}] * 2, {0: 11}, flags=[PR.PENDING] + [PR.COUNTED] * 2, T=2, row=1)
    snap.thr_spec.set_row(0, {0: 14}, None)
    return FR.timed(snap, 1, [(T1, T2, {0: 14}, None)]), 0, FR.EDGE


DIRECTED = {
    # two pods run: a count of 2 admits nobody, the override's 5 three copies, from T1 to T2 inclusive
    "count-2-to-5": lambda: (FR.timed(FR._run({}, count=2), 0, [(T1, T2, {}, 5)]), 0, FR.EDGE),
    "tie-lower-row-limits": _tie,
    # the pod names dimension 1 with a value of 0: it brings the name's presence, and the name is not judged
    "zero-valued-name": lambda: (FR.timed(PR.tiny([{0: 3, 1: 0}] + [{0: 4}] * 2, {0: 20, 1: 0}, flags=[PR.PENDING] + [PR.COUNTED] * 2), 0,
                                          [(T1, T2, {0: 30, 1: 0}, None)]), 0, FR.EDGE),
    # a negative request: the sums shrink copy after copy
    "negative-request": lambda: (FR.timed(PR.tiny([{0: 2, 1: -1}] + [{0: 4, 1: 2}] * 2, {0: 15, 1: 100},
                                                  flags=[PR.PENDING] + [PR.COUNTED] * 2, reserved=({1: 1}, None)), 0,
                                          [(T1, T2, {0: 13, 1: 5}, None)]), 0, FR.EDGE),
    # reserved amounts that are present, for the name and for the count
    "reserved-present": lambda: (FR.timed(FR._run({0: 100}, reserved=({0: 4}, 1)), 0, [(T1, T2, {0: 21}, None), (FR.T3, FR.T4, {0: 40}, 6)]), 0,
                                 FR.EDGE + [FR.shift(FR.T4, 1)]),
}
