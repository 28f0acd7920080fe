#!/usr/bin/env python
"""What a pod event costs the first step behind it on a cached engine: host clock around a step — kt_reconcile_launch +
kt_check_launch(all rows) + synchronise — in the steady state and behind upserts of 1, 64 and 70 000 rows (rows rewritten with
their own content: every launch of the event path runs, nothing of the result changes).  The refresh of the match cache (one
launch of the builder's list form, with the write-through to the scan view's planes) stands in front of the step's aggregate.

    python tools/match_cache_probe.py [--pods N] [--reps R]            one JSON object
    KT_ENGINE_LIB=<other build> / KT_NO_MATCH_CACHE=1 / KT_NO_MATCH_CACHE_AGG=1 select the side.
Under `rocprofv3 --kernel-trace` the kt_build_match_cache launches come in this order: the full build, `reps` refreshes of 1 row,
`reps` of 64 rows, one full build behind the 70 000-row batch (it voids the table).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kube_throttler_amd import engine as E  # noqa: E402
from kube_throttler_amd import workload as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    c = W.preset(2)
    c.n_pods_total = c.n_pods = a.pods
    snap = W.generate(c)
    now = (int(c.now_s), 0)
    eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)

    def step():
        t0 = time.perf_counter()
        eng.reconcile_launch(now, apply=True)
        eng.check_launch(snap.n_pods)
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for _ in range(10):
        step()
    out = {"pods": a.pods, "steady_us": round(statistics.median(step() for _ in range(100)), 2)}
    for n in (1, 64, 70_000):
        rows = np.arange(1000, 1000 + n, dtype=np.int64)
        batch = snap.pod_batch(rows)
        ts = []
        for _ in range(a.reps if n <= 64 else 1):
            eng.upsert_pods(batch, rows=rows)
            ts.append(step())
            step()
        out[f"first_step_after_{n}_row_upsert_us"] = round(statistics.median(ts), 2)
    out.update(builds=eng.match_cache_builds(), sweeps=eng.match_cache_scans(),
               agg_scans=eng.match_cache_agg_scans(), view_builds=eng.view_builds())
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
