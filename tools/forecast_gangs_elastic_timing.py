"""Times the elastic gang forecast (kt_forecast_gangs_elastic_launch) beside kt_forecast_gangs_launch on the identity workload; the
output is the record kept as profiles/forecast_gangs_elastic_timing.txt.
usage: python tools/forecast_gangs_elastic_timing.py [--config 2] [--instants 64] [--reps 5] [--runs 6]

The workload is tools/forecast_gangs_timing.py's: the engine of bench.py's configs[N] (W.preset(N)), pending pods as members,
--instants instants one hour apart, (a) ONE gang of 4 members and (b) 256 gangs of 8 members in ONE launch.
  gangs           kt_forecast_gangs_launch + kt_forecast_gangs_fetch: one wave per gang, lane = instant
  elastic         kt_forecast_gangs_elastic_launch + _fetch with min_members = the gang's size and member_flags = NULL — by identity
                  (E1) the same first / verdicts / blocker, asserted before the clock starts: one wave per (gang, instant) pair
  elastic seeded  (b) once more under a seeded rule: quorum randint(1, size), each member required with probability 1/4
Method: the two sides alternately, --runs runs per side in one process; a run is the median of --reps wall-clock times around the
synchronous launch + fetch (one warm call first).  Per side: the median of the runs and their spread (max - min).  Both calls share
everything in front of their kernel (the check over the members, the dense aggregate with exact counts, the dry finalize), so the
difference of the medians is the difference of the kernels (and of the 8 bytes per cell the elastic fetch copies more)."""
import argparse
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402


def one_run(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def side(label, runs):
    print(f"  {label:<46} median {np.median(runs):.3f} ms, spread {max(runs) - min(runs):.3f} ms  (runs {', '.join(f'{x:.3f}' for x in runs)})",
          flush=True)
    return float(np.median(runs)), max(runs) - min(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--instants", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=6)
    a = ap.parse_args()

    cfg = W.preset(a.config)
    snap = W.generate(cfg)
    now = (cfg.now_s, 0)
    inst = [(now[0] + 3600 * k, 0) for k in range(a.instants)]
    eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    eng.reconcile(now, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)
    print(f"library {E.version()}; configs[{a.config}]: pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, "
          f"pending pods {len(pending)}, instants {len(inst)}, reps {a.reps} per run, runs {a.runs} per side (alternating)", flush=True)

    for label, n_gangs, size in (("(a)", 1, 4), ("(b)", 256, 8)):
        members = pending[:n_gangs * size]
        off = np.arange(n_gangs + 1, dtype=np.int64) * size
        sizes = np.full(n_gangs, size, np.int64)
        first, verdicts, blockers = eng.forecast_gangs(members, off, inst)
        efirst, everdicts, emembers, eblockers = eng.forecast_gangs_elastic(members, off, sizes, inst)
        assert efirst.tobytes() == first.tobytes() and everdicts.tobytes() == verdicts.tobytes() and eblockers.tobytes() == blockers.tobytes()
        assert np.array_equal(emembers == size, verdicts == 0)
        print(f"{label} {n_gangs} x {size} members x {len(inst)} instants = {n_gangs * len(inst)} pairs; first = 0: {(first == 0).sum()}, "
              f"first >= 1: {(first >= 1).sum()}, none: {(first < 0).sum()}; members that succeed per cell: min {emembers.min()}, "
              f"mean {emembers.mean():.2f}, max {emembers.max()}", flush=True)
        gangs, elastic = [], []
        for _ in range(a.runs):
            gangs.append(one_run(lambda: eng.forecast_gangs(members, off, inst), a.reps))
            elastic.append(one_run(lambda: eng.forecast_gangs_elastic(members, off, sizes, inst), a.reps))
        g_med, g_spread = side("kt_forecast_gangs_launch + fetch:", gangs)
        e_med, e_spread = side("kt_forecast_gangs_elastic_launch + fetch (min = size):", elastic)
        d, spread = e_med - g_med, max(g_spread, e_spread)
        print(f"    elastic - gangs = {d:+.3f} ms of medians = {abs(d) / spread if spread > 0 else float('inf'):.1f} spreads "
              f"(the larger of the two spreads, {spread:.3f} ms); disjoint ranges: {max(elastic) < min(gangs) or max(gangs) < min(elastic)}",
              flush=True)
        if n_gangs > 1:
            r = random.Random(7919)
            quorum = np.array([r.randint(1, size) for _ in range(n_gangs)], np.int64)
            required = np.array([r.random() < 0.25 for _ in range(n_gangs * size)], bool)
            sfirst, sverdicts, smembers, _ = eng.forecast_gangs_elastic(members, off, quorum, inst, required)
            print(f"{label} under the seeded rule: first = 0: {(sfirst == 0).sum()}, first >= 1: {(sfirst >= 1).sum()}, none: {(sfirst < 0).sum()}, "
                  f"cells admitted with fewer than all members: {((sverdicts == 0) & (smembers < size)).sum()}", flush=True)
            side("kt_forecast_gangs_elastic_launch + fetch (seeded):",
                 [one_run(lambda: eng.forecast_gangs_elastic(members, off, quorum, inst, required), a.reps) for _ in range(a.runs)])
    eng.close()


if __name__ == "__main__":
    main()
