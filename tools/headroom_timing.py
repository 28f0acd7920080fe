"""Times the headroom query (kt_headroom_launch) beside what it contains and what it replaces; the output is the record kept
as profiles/headroom_timing.txt.
usage: python tools/headroom_timing.py [--pods 100000] [--throttles 1000] [--dims 8] [--cap 16] [--reps 7]

On one seeded workload, thresholds set a few pods above what is used so that the answers spread over zero, in between and the cap:
  headroom        kt_headroom_launch + kt_headroom_fetch over every pod row, and the launch alone up to kt_synchronize
  check           the kt_check_launch with status matrix that the headroom launch contains, up to kt_synchronize, and its
                  kernel alone by the engine's HIP events (kt_timing_read)
  admit           a dry-run kt_admit_launch of [p] * cap for ONE pod, launch + fetch: the only way to the number without
                  kt_headroom_launch; beside it the headroom call for that one pod
Method: warm runs first, then the minimum and the median over --reps of the wall clock around the synchronous call."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402

NOW = (1767225600, 0)


def workload(pods, throttles, dims):
    """The seeded cluster with thresholds about 8 mean requests per name and 12 pods above `used`."""
    snap = W.generate(W.small(seed=7, n_pods=pods, n_thr=throttles, n_cluster=throttles // 2, D=dims))
    T = snap.n_thr
    probe = E.Engine.for_snapshot(snap)
    used = probe.reconcile(NOW, apply=False).used
    probe.close()
    count = np.maximum(used.count[:T], 1)
    snap.thr_spec.v[:T] = used.v[:T] + 8 * (used.v[:T] // count[:, None]) + 1
    snap.thr_spec.count[:T] = used.count[:T] + 12
    snap.thr_ovr_off[:] = 0
    return snap


def timed(call, reps, warm=2):
    """(min, median) in ms of the wall clock around `call`, which returns when its work on the device is done."""
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), float(np.median(ms))


def report(what, min_med):
    print(f"{what}: min {min_med[0]:.3f} ms, median {min_med[1]:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--cap", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()

    snap = workload(a.pods, a.throttles, a.dims)
    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    n, cap = snap.n_pods, a.cap
    print(f"library {E.version()}; pods {n}, throttle rows {eng.throttle_rows()}, D {snap.D}, cap {cap}, reps {a.reps}", flush=True)

    def headroom_launch():
        eng.headroom_launch(n, cap=cap)
        eng.synchronize()

    def check_launch():
        eng.check_launch(n, want_status=True)
        eng.synchronize()

    report(f"headroom launch + fetch, {n} pods", timed(lambda: eng.headroom(n=n, cap=cap), a.reps))
    report("headroom launch + synchronize (no fetch)", timed(headroom_launch, a.reps))
    report("check launch with status matrix + synchronize (no fetch)", timed(check_launch, a.reps))
    eng.timing_enable(True)
    eng.timing_reset()
    for _ in range(a.reps):
        check_launch()
    ms, launches = eng.timing_read(E.KERNEL_CHECK)
    eng.timing_enable(False)
    print(f"check kernel by HIP events ({eng.kernel_name(E.KERNEL_CHECK)}): mean {ms / max(launches, 1):.3f} ms over {launches} launches", flush=True)

    flags = snap.pod_flags[:n]
    p = int(np.nonzero(((flags & S.POD_VALID) != 0) & ((flags & S.POD_SCHEDULED) == 0))[0][0])
    queue = np.full(cap, p, np.int64)
    one = np.array([p], np.int64)
    report(f"dry-run admit of [p] * {cap}, one pod, launch + fetch", timed(lambda: eng.admit(queue, commit=False, want_status=False), 20))
    report("headroom of that one pod, launch + fetch", timed(lambda: eng.headroom(one, cap=cap), 20))

    copies, _ = eng.headroom(n=n, cap=cap)
    _, summary = eng.admit(queue, commit=False, want_status=False)
    lead = int(np.argmax(summary != 0)) if (summary != 0).any() else cap
    assert int(eng.headroom(one, cap=cap)[0][0]) == lead, "headroom differs from the dry-run admission's leading Success count"
    print(f"copies over all pods: zero {(copies == 0).sum()}, in between {((copies > 0) & (copies < cap)).sum()}, cap {(copies == cap).sum()}")
    eng.close()


if __name__ == "__main__":
    main()
