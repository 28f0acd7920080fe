"""Times kt_paged_forecast; the output is the record kept as profiles/forecast_paged_timing.txt.
usage: python tools/forecast_paged_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--many 256] [--instants 64] [--reps 15]

On the seeded workload of tools/preempt_paged_timing.py (thresholds about three pods below what is used, so that pending pods are
blocked) with ONE open-ended override per throttle that doubles its threshold and begins 1 .. 60 hours after `now` (row t: hour
1 + t mod 60), for one pod and for --many pending pods over --instants instants one hour apart from `now`:
  one page     kt_paged_forecast over the one engine (the new kernel) beside kt_forecast_launch + kt_forecast_fetch (the
               single-engine kernel: the yardstick) on the SAME engine, run alternately; the two must return the same bytes.
  three pages  kt_paged_forecast over three engines of 16 names each: the same pods, namespaces, selectors and override times,
               every page with request columns, thresholds and override thresholds of its own.
Method: warm runs of every shape first, then --reps rounds that alternate the variants; per variant the median, the minimum and
the maximum of the host clock around the synchronous calls (every call ends in a stream synchronise).  No gate on the time; where
the one-page paged call is slower than the plain one by more than five times the plain call's spread (max - min), the line that
follows says so."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kube_throttler_amd import engine as E, snapshot as S  # noqa: E402
from preempt_paged_timing import NOW, alternate, line, page_of  # noqa: E402


def with_overrides(snap):
    """One open-ended override per throttle row: twice spec.threshold from hour 1 + t mod 60 on (the same times on every page)."""
    T, D = snap.n_thr, snap.D
    snap.ovr_begin_s = np.array([NOW[0] + 3600 * (1 + t % 60) for t in range(T)], np.int64)
    snap.ovr_begin_ns = np.zeros(T, np.int32)
    snap.ovr_end_s = np.full(T, S.ZERO_TIME_S, np.int64)
    snap.ovr_end_ns = np.zeros(T, np.int32)
    snap.ovr_flags = np.zeros(T, np.uint8)
    snap.ovr_thr = S.Amounts(T, D)
    snap.ovr_thr.v[:T] = snap.thr_spec.v[:T] * 2
    snap.ovr_thr.present[:T] = snap.thr_spec.present[:T]
    snap.ovr_thr.count[:T] = snap.thr_spec.count[:T] * 2
    snap.ovr_thr.has_count[:T] = snap.thr_spec.has_count[:T]
    snap.thr_ovr_off[:T + 1] = np.arange(T + 1, dtype=np.uint32)
    snap._keep = None
    return snap


def answers(first):
    return f"none {(first < 0).sum()}, at once {(first == 0).sum()}, later {(first > 0).sum()} (latest position {int(first.max())})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--many", type=int, default=256)
    ap.add_argument("--instants", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    inst = [(NOW[0] + 3600 * k, 0) for k in range(a.instants)]

    snap = with_overrides(page_of(a.pods, a.throttles, a.dims, 0))
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    many = pending[:a.many].astype(np.int64)

    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, instants {len(inst)}, pods asked 1 and "
          f"{len(many)}, reps {a.reps} (alternating)", flush=True)
    first, _ = eng.forecast(many, inst)
    print(f"one page, D {snap.D}: answers over the {len(many)} pods: {answers(first)}", flush=True)
    one = np.array([int(many[np.argmax(first)])], np.int64)  # the pod that passes latest
    for rows, label in ((one, "1 pod"), (many, f"{len(many)} pods")):
        single = eng.forecast(rows, inst)
        paged = E.paged_forecast([eng], rows, inst)
        assert [x.tobytes() for x in single] == [x.tobytes() for x in paged], "one page: the bytes differ"
        t = alternate({"single": lambda: eng.forecast(rows, inst), "paged": lambda: E.paged_forecast([eng], rows, inst)}, a.reps)
        line(f"one page, {label} x {len(inst)} instants, kt_forecast_launch + kt_forecast_fetch", t["single"])
        line(f"one page, {label} x {len(inst)} instants, kt_paged_forecast (same bytes)", t["paged"])
        diff, spread = t["paged"][0] - t["single"][0], t["single"][2] - t["single"][1]
        verdict = "MORE than" if diff > 5 * spread else "within"
        print(f"    paged - plain = {diff:+.3f} ms of medians, the plain call's spread {spread:.3f} ms: {verdict} five times the spread", flush=True)
    eng.close()

    D = 16
    snaps = [with_overrides(page_of(a.pods, a.throttles, D, k, below=1)) for k in range(3)]
    engs = [E.Engine.for_snapshot(s) for s in snaps]
    E.paged_reconcile(engs, NOW, apply=True)
    first, _ = E.paged_forecast(engs, many, inst)
    print(f"three pages, D {D} each: answers over the {len(many)} pods: {answers(first)}", flush=True)
    one = np.array([int(many[np.argmax(first)])], np.int64)
    t = alternate({"one": lambda: E.paged_forecast(engs, one, inst), "many": lambda: E.paged_forecast(engs, many, inst)}, a.reps)
    line(f"three pages, 1 pod x {len(inst)} instants, kt_paged_forecast", t["one"])
    line(f"three pages, {len(many)} pods x {len(inst)} instants, kt_paged_forecast", t["many"])
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
