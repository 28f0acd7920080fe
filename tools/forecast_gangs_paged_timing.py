"""Times kt_paged_forecast_gangs; the output is the record kept as profiles/forecast_gangs_paged_timing.txt.
usage: python tools/forecast_gangs_paged_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--many 256] [--instants 64] [--reps 15]

On the workload of tools/forecast_paged_timing.py (thresholds about three pods below what is used, ONE open-ended override per
throttle that doubles its threshold and begins 1 .. 60 hours after `now`), over --instants instants one hour apart from `now`, for
--many gangs of ONE pending pod and for --many gangs of 2 .. 4 pending pods (sizes 2, 3, 4, 2, ..., consecutive pending rows):
  one page     kt_paged_forecast_gangs over the one engine (the new kernel) beside kt_forecast_gangs_launch +
               kt_forecast_gangs_fetch (the single-engine kernel: the yardstick) on the SAME engine, run alternately; the two must
               return the same bytes.
  three pages  kt_paged_forecast_gangs over three engines of 16 names each: the same pods, namespaces, selectors and override
               times, every page with request columns, thresholds and override thresholds of its own.
Method: warm runs of every shape first, then --reps rounds that alternate the variants; per variant the median, the minimum and
the maximum of the host clock around the synchronous calls (every call ends in a stream synchronise).  No gate on the time; where
the one-page paged call is slower than the single-engine one by more than five times the single-engine call's spread (max - min),
the line that follows says so."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kube_throttler_amd import engine as E, snapshot as S  # noqa: E402
from forecast_paged_timing import with_overrides  # noqa: E402
from preempt_paged_timing import NOW, alternate, line, page_of  # noqa: E402


def answers(first, verdicts):
    err = int((verdicts == 2).any(axis=1).sum())
    return (f"none {(first < 0).sum() - err}, at once {(first == 0).sum()}, later {(first > 0).sum()} (latest position {int(first.max())}), "
            f"with an Error member {err}")


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
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)
    sizes = np.array([2 + g % 3 for g in range(a.many)], np.int64)
    shapes = (("gangs of 1", pending[:a.many], np.arange(a.many + 1, dtype=np.int64)),
              ("gangs of 2-4", pending[:int(sizes.sum())], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)))

    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, instants {len(inst)}, gangs {a.many}, "
          f"reps {a.reps} (alternating)", flush=True)
    for label, rows, off in shapes:
        single = eng.forecast_gangs(rows, off, inst)
        paged = E.paged_forecast_gangs([eng], rows, off, inst)
        assert [x.tobytes() for x in single] == [x.tobytes() for x in paged], "one page: the bytes differ"
        print(f"one page, D {snap.D}, {a.many} {label} ({len(rows)} members): {answers(single[0], single[1])}", flush=True)
        t = alternate({"single": lambda: eng.forecast_gangs(rows, off, inst), "paged": lambda: E.paged_forecast_gangs([eng], rows, off, inst)},
                      a.reps)
        line(f"one page, {a.many} {label} x {len(inst)} instants, kt_forecast_gangs_launch + kt_forecast_gangs_fetch", t["single"])
        line(f"one page, {a.many} {label} x {len(inst)} instants, kt_paged_forecast_gangs (same bytes)", t["paged"])
        diff, spread = t["paged"][0] - t["single"][0], t["single"][2] - t["single"][1]
        verdict = "MORE than" if diff > 5 * spread else "within"
        print(f"    paged - single = {diff:+.3f} ms of medians, the single-engine call's spread {spread:.3f} ms: {verdict} five times the spread",
              flush=True)
    eng.close()

    D = 16
    snaps = [with_overrides(page_of(a.pods, a.throttles, D, k, below=1)) for k in range(3)]
    engs = [E.Engine.for_snapshot(s) for s in snaps]
    E.paged_reconcile(engs, NOW, apply=True)
    for label, rows, off in shapes:
        first, verdicts, _ = E.paged_forecast_gangs(engs, rows, off, inst)
        print(f"three pages, D {D} each, {a.many} {label} ({len(rows)} members): {answers(first, verdicts)}", flush=True)
    t = alternate({label: (lambda rows=rows, off=off: E.paged_forecast_gangs(engs, rows, off, inst)) for label, rows, off in shapes}, a.reps)
    for label, _, _ in shapes:
        line(f"three pages, {a.many} {label} x {len(inst)} instants, kt_paged_forecast_gangs", t[label])
    t = alternate({"plain": lambda: E.paged_forecast(engs, shapes[0][1], inst)}, a.reps)
    line(f"beside it: three pages, the same {a.many} pods x {len(inst)} instants, kt_paged_forecast", t["plain"])
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
