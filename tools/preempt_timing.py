"""Times the preemption query (kt_preempt_launch) beside the composed path a caller has without it; the output is the record kept
as profiles/preempt_timing.txt.
usage: python tools/preempt_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--cands 1000] [--reps 5]

On one seeded workload (thresholds a few pods below what is used, so that pending pods are blocked and victims help):
  preempt 1 x m    kt_preempt_launch + kt_preempt_fetch for one pending pod over m running candidates
  preempt n x m    the same for n = m pending pods in ONE launch
  composed 1 x m   a scratch engine per query: kt_delete_pods + kt_reconcile_launch(APPLY) + kt_check per prefix step, the prefix
                   length BISECTED (the fairest thing a caller can do today; it assumes the verdict is monotone in k, which
                   kt_preempt does not), the deleted pods fed back between steps.  n x m is n times that.
Method: warm runs first, then the minimum and the median over --reps of the wall clock around the synchronous calls."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402

NOW = (1767225600, 0)


def workload(pods, throttles, dims):
    snap = W.generate(W.small(seed=7, n_pods=pods, n_thr=throttles, n_cluster=throttles // 2, D=dims))
    T = snap.n_thr
    probe = E.Engine.for_snapshot(snap)
    used = probe.reconcile(NOW, apply=False).used
    probe.close()
    count = np.maximum(used.count[:T], 1)
    snap.thr_spec.v[:T] = np.maximum(used.v[:T] - 3 * (used.v[:T] // count[:, None]), 1)  # about three pods below `used`
    snap.thr_spec.count[:T] = np.maximum(used.count[:T] - 3, 1)
    snap.thr_ovr_off[:] = 0
    return snap


def timed(call, reps, warm=1):
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    snap = workload(a.pods, a.throttles, a.dims)
    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    counted = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED
    running = np.nonzero((fl & (counted | S.POD_FINISHED)) == counted)[0]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    cands = running[:a.cands].astype(np.int64)
    many = pending[:a.cands].astype(np.int64)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, candidates {len(cands)}, "
          f"preemptors {len(many)}, reps {a.reps}", flush=True)
    prefix, _ = eng.preempt(many, cands, NOW)
    print(f"answers over the preemptors: none {(prefix < 0).sum()}, zero {(prefix == 0).sum()}, positive {(prefix > 0).sum()} "
          f"(longest {int(prefix.max())})", flush=True)
    p = int(many[np.argmax(prefix)])  # the preemptor with the longest prefix
    one = np.array([p], np.int64)
    want = int(prefix.max())
    t_one = timed(lambda: eng.preempt(one, cands, NOW), a.reps)
    t_many = timed(lambda: eng.preempt(many, cands, NOW), a.reps)

    scratch = E.Engine.for_snapshot(snap)
    restore = snap.pod_batch(cands)

    def passes(k, state):
        """PreFilter(p) with exactly cands[:k] deleted; state[0] = how many are deleted now."""
        if k > state[0]:
            scratch.delete_pods(cands[state[0]:k])
        elif k < state[0]:
            scratch.upsert_pods(snap.pod_batch(cands[k:state[0]]), rows=cands[k:state[0]])
        state[0] = k
        scratch.reconcile_launch(NOW, apply=True)
        scratch.synchronize()  # (a few-pod kt_check does not wait for a reconcile in flight: it would read the status before it)
        _, summary = scratch.check_atomic(rows=one, want_status=False)
        return int(summary[0]) & 3 == 0

    def composed():
        state = [0]
        if passes(0, state):
            got = 0
        elif not passes(len(cands), state):
            got = -1
        else:
            lo, hi = 0, len(cands)  # fails at lo, passes at hi
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if passes(mid, state) else (mid, hi)
            got = hi
        scratch.upsert_pods(restore, rows=cands)
        return got

    got = composed()
    t_comp = timed(composed, a.reps)
    print(f"preempt, 1 preemptor x {len(cands)} candidates, launch + fetch: min {t_one[0]:.3f} ms, median {t_one[1]:.3f} ms", flush=True)
    print(f"preempt, {len(many)} preemptors x {len(cands)} candidates, launch + fetch: min {t_many[0]:.3f} ms, median {t_many[1]:.3f} ms", flush=True)
    print(f"composed (delete + reconcile(APPLY) + check per step, bisected), 1 preemptor: min {t_comp[0]:.3f} ms, median {t_comp[1]:.3f} ms "
          f"(answer {got}, preempt {want})", flush=True)
    eng.timing_enable(True)
    eng.timing_reset()
    eng.preempt(one, cands, NOW)
    ms_check, _ = eng.timing_read(E.KERNEL_CHECK)
    eng.timing_enable(False)
    t_rec = timed(lambda: eng.reconcile(NOW, apply=False), a.reps)
    print(f"inside it: the status-matrix check kernel {ms_check:.3f} ms (HIP events); beside it: the engine's own indexed reconcile, dry, "
          f"launch + fetch: median {t_rec[1]:.3f} ms (kt_preempt_launch aggregates with the DENSE scan for exact contributor counts)", flush=True)
    print(f"ratio composed / preempt, one preemptor: {t_comp[1] / t_one[1]:.2f}x; {len(many)} preemptors (composed = {len(many)} x one): "
          f"{len(many) * t_comp[1] / t_many[1]:.0f}x", flush=True)
    eng.close()
    scratch.close()


if __name__ == "__main__":
    main()
