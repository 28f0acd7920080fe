"""Times kt_paged_headroom_forecast; the output is the record kept as profiles/headroom_forecast_paged_timing.txt.
usage: python tools/headroom_forecast_paged_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--many 256] [--instants 64] [--reps 15]

On the workload of tools/forecast_paged_timing.py (thresholds about three pods below what is used, one open-ended override per
throttle that doubles its threshold and begins 1 .. 60 hours after `now`), for one pod and for --many pending pods over
--instants instants one hour apart from `now`, cap 16 and want 2:
  one page     kt_paged_headroom_forecast over the one engine (the new kernel) beside kt_headroom_forecast_launch +
               kt_headroom_forecast_fetch (the single-engine kernel: the yardstick) on the SAME engine, run alternately; the two
               must return the same bytes.
  three pages  kt_paged_headroom_forecast over three engines of 16 names each beside kt_paged_forecast (the verdict alone) over the
               same pods and instants.
Method: that of tools/forecast_paged_timing.py — warm runs of every shape first, then --reps rounds that alternate the variants;
per variant the median, the minimum and the maximum of the host clock around the synchronous calls.  No gate on the time; where
the one-page paged call is slower than the plain one by more than five times the plain call's spread (max - min), the line that
follows says so."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kube_throttler_amd import engine as E, snapshot as S  # noqa: E402
from forecast_paged_timing import with_overrides  # noqa: E402
from preempt_paged_timing import NOW, alternate, line, page_of  # noqa: E402

CAP, WANT = 16, 2


def answers(first, copies):
    return (f"first: none {(first < 0).sum()}, at once {(first == 0).sum()}, later {(first > 0).sum()}; cells with 0 copies "
            f"{(copies == 0).sum()}, between {((copies > 0) & (copies < CAP)).sum()}, cap {(copies == CAP).sum()}")


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
    kw = dict(cap=CAP, want=WANT)

    snap = with_overrides(page_of(a.pods, a.throttles, a.dims, 0))
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    many = pending[:a.many].astype(np.int64)

    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, instants {len(inst)}, pods asked 1 and "
          f"{len(many)}, cap {CAP}, want {WANT}, reps {a.reps} (alternating)", flush=True)
    first, copies, _ = eng.headroom_forecast(many, inst, **kw)
    print(f"one page, D {snap.D}: answers over the {len(many)} pods: {answers(first, copies)}", flush=True)
    one = np.array([int(many[np.argmax(first)])], np.int64)  # the pod whose `want` copies fit latest
    for rows, label in ((one, "1 pod"), (many, f"{len(many)} pods")):
        single = eng.headroom_forecast(rows, inst, **kw)
        paged = E.paged_headroom_forecast([eng], rows, inst, **kw)
        assert [x.tobytes() for x in single] == [x.tobytes() for x in paged], "one page: the bytes differ"
        t = alternate({"single": lambda: eng.headroom_forecast(rows, inst, **kw),
                       "paged": lambda: E.paged_headroom_forecast([eng], rows, inst, **kw)}, a.reps)
        line(f"one page, {label} x {len(inst)} instants, kt_headroom_forecast_launch + kt_headroom_forecast_fetch", t["single"])
        line(f"one page, {label} x {len(inst)} instants, kt_paged_headroom_forecast (same bytes)", t["paged"])
        diff, spread = t["paged"][0] - t["single"][0], t["single"][2] - t["single"][1]
        verdict = "MORE than" if diff > 5 * spread else "within"
        print(f"    paged - plain = {diff:+.3f} ms of medians, the plain call's spread {spread:.3f} ms: {verdict} five times the spread", flush=True)
    eng.close()

    D = 16
    snaps = [with_overrides(page_of(a.pods, a.throttles, D, k, below=1)) for k in range(3)]
    engs = [E.Engine.for_snapshot(s) for s in snaps]
    E.paged_reconcile(engs, NOW, apply=True)
    first, copies, _ = E.paged_headroom_forecast(engs, many, inst, **kw)
    print(f"three pages, D {D} each: answers over the {len(many)} pods: {answers(first, copies)}", flush=True)
    one = np.array([int(many[np.argmax(first)])], np.int64)
    t = alternate({"one": lambda: E.paged_headroom_forecast(engs, one, inst, **kw),
                   "many": lambda: E.paged_headroom_forecast(engs, many, inst, **kw),
                   "verdict": lambda: E.paged_forecast(engs, many, inst)}, a.reps)
    line(f"three pages, 1 pod x {len(inst)} instants, kt_paged_headroom_forecast", t["one"])
    line(f"three pages, {len(many)} pods x {len(inst)} instants, kt_paged_headroom_forecast", t["many"])
    line(f"three pages, {len(many)} pods x {len(inst)} instants, kt_paged_forecast (the verdict alone)", t["verdict"])
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
