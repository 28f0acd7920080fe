"""Times the headroom forecast (kt_headroom_forecast_launch) beside the verdict-only forecast over the same walk; the output is the
record kept as profiles/headroom_forecast_timing.txt.
usage: python tools/headroom_forecast_timing.py [--config 2 | --small N_PODS] [--pods 256] [--instants 37] [--runs 6]

On the engine of bench.py's configs[N] (W.preset(N)), with pending pods and --instants instants one hour apart, launch + fetch:
  (a) headroom forecast, cap = 16
  (b) headroom forecast, cap = 2^31 - 1   (headroom_fit's bisection runs wherever cap x request exceeds the room)
  (c) kt_forecast_launch + kt_forecast_fetch on the same pods and instants: the same walk, verdict only
--small N_PODS takes W.small(n_pods=N_PODS, 500 throttles, overrides on) instead: an engine whose dense aggregate is short, so
that with --pods in the thousands the per-pod kernels are what the clock sees.
Method: warm calls first, then --runs rounds that take the three sides one after the other (a, b, c, a, b, c, ...), so that a
drift of the clocks meets all sides alike; per side the median, minimum and maximum of the wall clock around the synchronous
calls.  Nothing is gated on the ratios: they are written down."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--small", type=int, default=0, metavar="N_PODS")
    ap.add_argument("--pods", type=int, default=256)
    ap.add_argument("--instants", type=int, default=37)
    ap.add_argument("--runs", type=int, default=6)
    a = ap.parse_args()

    cfg = W.small(seed=1, n_pods=a.small, n_thr=500, n_cluster=500) if a.small else W.preset(a.config)
    snap = W.generate(cfg)
    now = (cfg.now_s, 0)
    inst = [(now[0] + 3600 * k, 0) for k in range(a.instants)]
    eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    eng.reconcile(now, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    pods = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)[:a.pods]
    print(f"library {E.version()}; {'W.small' if a.small else f'configs[{a.config}]'}: pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, "
          f"pods asked {len(pods)}, instants {len(inst)}, runs {a.runs}", flush=True)

    sides = [("(a) headroom forecast, cap 16", lambda: eng.headroom_forecast(pods, inst, cap=16)),
             ("(b) headroom forecast, cap 2^31 - 1", lambda: eng.headroom_forecast(pods, inst, cap=E.HEADROOM_MAX_CAP)),
             ("(c) forecast, verdict only", lambda: eng.forecast(pods, inst))]
    _, copies, _ = sides[0][1]()
    _, big, _ = sides[1][1]()
    _, verdicts = sides[2][1]()
    print(f"answers: copies 0: {(copies == 0).mean():.2f}, between: {((copies > 0) & (copies < 16)).mean():.2f}, cap: {(copies == 16).mean():.2f} "
          f"of the (pod, instant) pairs; with the largest cap below it: {(big < E.HEADROOM_MAX_CAP).mean():.2f}; "
          f"copies > 0 exactly where the verdict is Success: {np.array_equal(copies > 0, verdicts == S.VERDICT_ALLOW)}", flush=True)
    for _, fn in sides:
        for _ in range(3):
            fn()
    ms = [[] for _ in sides]
    for _ in range(a.runs):
        for k, (_, fn) in enumerate(sides):
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = [float(np.median(x)) for x in ms]
    for k, (label, _) in enumerate(sides):
        print(f"{label}: median {med[k]:.3f} ms, min {min(ms[k]):.3f} ms, max {max(ms[k]):.3f} ms over {a.runs} runs", flush=True)
    print(f"ratio (a) / (c): {med[0] / med[2]:.2f}x; (b) / (c): {med[1] / med[2]:.2f}x; (b) / (a): {med[1] / med[0]:.2f}x", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
