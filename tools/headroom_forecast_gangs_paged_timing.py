"""Times kt_paged_headroom_forecast_gangs; the output is the record kept as profiles/headroom_forecast_gangs_paged_timing.txt.
usage: python tools/headroom_forecast_gangs_paged_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--instants 64] [--loosen 1]
                                                            [--reps 15]

On the workload of tools/forecast_paged_timing.py (thresholds about three pods below what is used, one open-ended override per
throttle that doubles its threshold and begins 1 .. 60 hours after `now`; --loosen F multiplies every threshold, spec and
overrides, by F, so that copies between 0 and the cap appear and the searches run to their depth), for one gang of 4 and for 256
gangs of 8 cut from the pending pods, over --instants instants one hour apart from `now`, cap 16 and want 2:
  one page     kt_paged_headroom_forecast_gangs over the one engine (the new kernel) beside kt_headroom_forecast_gangs_launch +
               kt_headroom_forecast_gangs_fetch (the single-engine kernel: the yardstick) on the SAME engine, run alternately; the
               two must return the same bytes.
  three pages  kt_paged_headroom_forecast_gangs over three engines of 16 names each beside kt_paged_forecast_gangs (the verdict
               alone) over the same gangs and instants.
Method: that of tools/headroom_forecast_paged_timing.py — warm runs of every shape first, then --reps rounds that alternate the
variants; per variant the median, the minimum and the maximum of the host clock around the synchronous calls.  No gate on the
time; where the one-page paged call is slower than the plain one by more than five times the plain call's spread (max - min), the
line that follows says so."""
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
SHAPES = ((1, 4), (256, 8))  # (gangs, members each)


def loosened(snap, factor):
    if factor != 1:
        for tab in (snap.thr_spec, snap.ovr_thr):
            tab.v *= factor
            tab.count *= factor
    return snap


def answers(first, copies):
    return (f"first: none {(first < 0).sum()}, at once {(first == 0).sum()}, later {(first > 0).sum()}; cells with 0 copies "
            f"{(copies == 0).sum()}, between {((copies > 0) & (copies < CAP)).sum()}, cap {(copies == CAP).sum()}")


def gangs_of(pending, n_gangs, size):
    rows = pending[:n_gangs * size].astype(np.int64)
    assert len(rows) == n_gangs * size, f"{n_gangs} gangs of {size}: only {len(rows)} pending pods"
    return rows, np.arange(0, n_gangs * size + 1, size, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--instants", type=int, default=64)
    ap.add_argument("--loosen", type=int, default=1, metavar="F")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    inst = [(NOW[0] + 3600 * k, 0) for k in range(a.instants)]
    kw = dict(cap=CAP, want=WANT)

    snap = loosened(with_overrides(page_of(a.pods, a.throttles, a.dims, 0)), a.loosen)
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]

    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, thresholds x{a.loosen}, instants {len(inst)}, "
          f"gangs asked {' and '.join(f'{g} of {k}' for g, k in SHAPES)}, cap {CAP}, want {WANT}, reps {a.reps} (alternating)", flush=True)
    for n_gangs, size in SHAPES:
        rows, off = gangs_of(pending, n_gangs, size)
        label = f"{n_gangs} gang(s) of {size}"
        single = eng.headroom_forecast_gangs(rows, off, inst, **kw)
        paged = E.paged_headroom_forecast_gangs([eng], rows, off, inst, **kw)
        assert [x.tobytes() for x in single] == [x.tobytes() for x in paged], "one page: the bytes differ"
        print(f"one page, D {snap.D}, {label}: answers: {answers(single[0], single[1])}", flush=True)
        t = alternate({"single": lambda: eng.headroom_forecast_gangs(rows, off, inst, **kw),
                       "paged": lambda: E.paged_headroom_forecast_gangs([eng], rows, off, inst, **kw)}, a.reps)
        line(f"one page, {label} x {len(inst)} instants, kt_headroom_forecast_gangs_launch + kt_headroom_forecast_gangs_fetch", t["single"])
        line(f"one page, {label} x {len(inst)} instants, kt_paged_headroom_forecast_gangs (same bytes)", t["paged"])
        diff, spread = t["paged"][0] - t["single"][0], t["single"][2] - t["single"][1]
        verdict = "MORE than" if diff > 5 * spread else "within"
        print(f"    paged - plain = {diff:+.3f} ms of medians, the plain call's spread {spread:.3f} ms: {verdict} five times the spread", flush=True)
    eng.close()

    D = 16
    snaps = [loosened(with_overrides(page_of(a.pods, a.throttles, D, k, below=1)), a.loosen) for k in range(3)]
    engs = [E.Engine.for_snapshot(s) for s in snaps]
    E.paged_reconcile(engs, NOW, apply=True)
    fl = snaps[0].pod_flags[:snaps[0].n_pods]  # (the wide workload's own pending pods: D changes what the generator draws)
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    for n_gangs, size in SHAPES:
        rows, off = gangs_of(pending, n_gangs, size)
        label = f"{n_gangs} gang(s) of {size}"
        first, copies, _, _ = E.paged_headroom_forecast_gangs(engs, rows, off, inst, **kw)
        print(f"three pages, D {D} each, {label}: answers: {answers(first, copies)}", flush=True)
        t = alternate({"headroom": lambda: E.paged_headroom_forecast_gangs(engs, rows, off, inst, **kw),
                       "verdict": lambda: E.paged_forecast_gangs(engs, rows, off, inst)}, a.reps)
        line(f"three pages, {label} x {len(inst)} instants, kt_paged_headroom_forecast_gangs", t["headroom"])
        line(f"three pages, {label} x {len(inst)} instants, kt_paged_forecast_gangs (the verdict alone)", t["verdict"])
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
