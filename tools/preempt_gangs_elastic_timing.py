"""Times the elastic gang preemption query (kt_preempt_gangs_elastic_launch) beside kt_preempt_gangs_launch on the identity
workload; the output is the record kept as profiles/preempt_gangs_elastic_timing.txt.
usage: python tools/preempt_gangs_elastic_timing.py [--config 2] [--reps 5] [--runs 6]

The workload: the engine of bench.py's configs[N] (W.preset(N)), pending pods as members, counted running pods as candidates; (a) ONE
gang of 4 members and (b) 256 gangs of 8 members in ONE launch, each against 64 and against 1024 candidates.
  gangs             kt_preempt_gangs_launch + kt_preempt_gangs_fetch: one wave per gang, lane = candidate position, closed form
  elastic           kt_preempt_gangs_elastic_launch + _fetch with min_members = the gang's size and member_flags = NULL — by identity
                    (P1) the same prefix and victim bytes, asserted before the clock starts: one wave per gang, the candidates one
                    after the other
  ... reprieved     both sides with the reprieve (kt_preempt_gangs_reprieve_launch / KT_PREEMPT_REPRIEVE), the same bytes again
  elastic seeded    once more under a seeded rule: quorum randint(1, size), each member required with probability 1/4
Method: the two sides alternately, --runs runs per side in one process; a run is the median of --reps wall-clock times around the
synchronous launch + fetch (one warm call first).  Per side: the median of the runs and their spread (max - min).  Both calls share
everything in front of their kernel (the check over members ++ candidates, the dense aggregate with exact counts, the dry finalize),
so the difference of the medians is the difference of the kernels (and of the 8 bytes per gang the elastic fetch copies more)."""
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
    print(f"  {label:<58} median {np.median(runs):.3f} ms, spread {max(runs) - min(runs):.3f} ms  (runs {', '.join(f'{x:.3f}' for x in runs)})",
          flush=True)
    return float(np.median(runs)), max(runs) - min(runs)


def versus(a, what, gangs_call, elastic_call):
    gangs, elastic = [], []
    for _ in range(a.runs):
        gangs.append(one_run(gangs_call, a.reps))
        elastic.append(one_run(elastic_call, a.reps))
    g_med, g_spread = side(f"kt_preempt_gangs{what}_launch + fetch:", gangs)
    e_med, e_spread = side(f"kt_preempt_gangs_elastic_launch{' (reprieve)' if what else ''} + fetch (min = size):", elastic)
    d = e_med - g_med
    print(f"    elastic - gangs = {d:+.3f} ms of medians = {abs(d) / g_spread if g_spread > 0 else float('inf'):.1f} spreads of the existing "
          f"call ({g_spread:.3f} ms; the elastic call's own: {e_spread:.3f} ms); disjoint ranges: "
          f"{max(elastic) < min(gangs) or max(gangs) < min(elastic)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=6)
    a = ap.parse_args()

    cfg = W.preset(a.config)
    snap = W.generate(cfg)
    now = (cfg.now_s, 0)
    eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    eng.reconcile(now, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    counted = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED
    running = np.nonzero((fl & (counted | S.POD_FINISHED)) == counted)[0].astype(np.int64)
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)
    print(f"library {E.version()}; configs[{a.config}]: pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, "
          f"pending pods {len(pending)}, counted running pods {len(running)}, reps {a.reps} per run, runs {a.runs} per side (alternating)", flush=True)

    for label, n_gangs, size in (("(a)", 1, 4), ("(b)", 256, 8)):
        members = pending[:n_gangs * size]
        off = np.arange(n_gangs + 1, dtype=np.int64) * size
        sizes = np.full(n_gangs, size, np.int64)
        for m in (64, 1024):
            cands = running[:m]
            for reprieve in (False, True):
                prefix, victims, blocker = eng.preempt_gangs(members, off, cands, now, reprieve=reprieve)
                eprefix, evictims, emembers, eblocker = eng.preempt_gangs_elastic(members, off, sizes, cands, now, reprieve=reprieve)
                assert eprefix.tobytes() == prefix.tobytes() and evictims.tobytes() == victims.tobytes()
                assert np.array_equal(emembers[prefix >= 0], sizes[prefix >= 0])
                print(f"{label} {n_gangs} x {size} members x {len(cands)} candidates{', reprieved' if reprieve else ''}: prefix = 0: "
                      f"{(prefix == 0).sum()}, prefix >= 1: {(prefix >= 1).sum()} (longest {prefix.max()}), none: {(prefix < 0).sum()}; "
                      f"victims {int(victims.sum())}", flush=True)
                versus(a, "_reprieve" if reprieve else "",
                       lambda: eng.preempt_gangs(members, off, cands, now, reprieve=reprieve),
                       lambda: eng.preempt_gangs_elastic(members, off, sizes, cands, now, reprieve=reprieve))
            r = random.Random(7919)
            quorum = np.array([r.randint(1, size) for _ in range(n_gangs)], np.int64)
            required = np.array([r.random() < 0.25 for _ in range(n_gangs * size)], bool)
            for reprieve in (False, True):
                sprefix, svictims, smembers, _ = eng.preempt_gangs_elastic(members, off, quorum, cands, now, required, reprieve=reprieve)
                print(f"{label} under the seeded rule{', reprieved' if reprieve else ''}: prefix = 0: {(sprefix == 0).sum()}, prefix >= 1: "
                      f"{(sprefix >= 1).sum()} (longest {sprefix.max()}), none: {(sprefix < 0).sum()}, gangs in with fewer than all members: "
                      f"{((sprefix >= 0) & (smembers < size)).sum()}; victims {int(svictims.sum())}", flush=True)
                side(f"kt_preempt_gangs_elastic_launch{' (reprieve)' if reprieve else ''} + fetch (seeded):",
                     [one_run(lambda: eng.preempt_gangs_elastic(members, off, quorum, cands, now, required, reprieve=reprieve), a.reps)
                      for _ in range(a.runs)])
    eng.close()


if __name__ == "__main__":
    main()
