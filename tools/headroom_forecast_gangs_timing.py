"""Times the gang headroom forecast (kt_headroom_forecast_gangs_launch) beside the verdict-only gang forecast on the same
arguments; the output is the record kept as profiles/headroom_forecast_gangs_timing.txt.
usage: python tools/headroom_forecast_gangs_timing.py [--config 2 | --small N_PODS] [--loosen F] [--days 30] [--runs 6]

On the engine of bench.py's configs[N] (W.preset(N)) — or W.small(n_pods=N_PODS, 500 throttles, overrides on) — with gangs cut from
the pending pods and the instants `now` ++ kt_override_instants over --days days, launch + fetch, for each of two shapes (one gang
of 4; 256 gangs of 8):
  (a) gang headroom forecast, cap = 16
  (b) gang headroom forecast, cap = 2^31 - 1   (the lane-own bisection: up to 1 + 31 gang walks per throttle and instant block)
  (c) kt_forecast_gangs_launch + kt_forecast_gangs_fetch on the same gangs and instants: one gang walk per throttle and block
--loosen F multiplies every threshold (spec and overrides) by F before the engine is built: the generated clusters are dense and
throttled (every answer is 0 copies, which the first probe of a search finds), a loosened one has answers between 0 and the cap and
searches that run to their depth.
What the search costs over the verdict is (a) / (c) and (b) / (c): at the most the number of bisection rounds.
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
    ap.add_argument("--loosen", type=int, default=1, metavar="F")
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--runs", type=int, default=6)
    a = ap.parse_args()

    cfg = W.small(seed=1, n_pods=a.small, n_thr=500, n_cluster=500) if a.small else W.preset(a.config)
    snap = W.generate(cfg)
    if a.loosen != 1:
        for tab in (snap.thr_spec, snap.ovr_thr):
            tab.v *= a.loosen
            tab.count *= a.loosen
    now = (cfg.now_s, 0)
    eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    eng.reconcile(now, apply=True)
    boundaries, total = eng.override_instants(now, (now[0] + 86400 * a.days, 0))
    inst = [now] + boundaries
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)
    print(f"library {E.version()}; {'W.small' if a.small else f'configs[{a.config}]'}: pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, "
          f"D {snap.D}, thresholds x{a.loosen}, pending pods {len(pending)}, instants {len(inst)} (now and {total} override boundaries within {a.days} days), "
          f"runs {a.runs}", flush=True)

    for n_gangs, size in ((1, 4), (256, 8)):
        rows = pending[:n_gangs * size]
        if len(rows) < n_gangs * size:
            print(f"{n_gangs} gangs of {size}: only {len(rows)} pending pods, shape left out", flush=True)
            continue
        off = np.arange(0, n_gangs * size + 1, size, dtype=np.int64)
        sides = [("(a) gang headroom forecast, cap 16", lambda: eng.headroom_forecast_gangs(rows, off, inst, cap=16)),
                 ("(b) gang headroom forecast, cap 2^31 - 1", lambda: eng.headroom_forecast_gangs(rows, off, inst, cap=E.HEADROOM_MAX_CAP)),
                 ("(c) gang forecast, verdict only", lambda: eng.forecast_gangs(rows, off, inst))]
        _, copies, _, _ = sides[0][1]()
        _, big, _, _ = sides[1][1]()
        _, verdicts, _ = sides[2][1]()
        print(f"---- {n_gangs} gang(s) of {size}, {len(inst)} instants", flush=True)
        print(f"answers: copies 0: {(copies == 0).mean():.2f}, between: {((copies > 0) & (copies < 16)).mean():.2f}, cap: {(copies == 16).mean():.2f} "
              f"of the (gang, instant) pairs; with the largest cap below it: {(big < E.HEADROOM_MAX_CAP).mean():.2f}, largest finite answer "
              f"{int(big[big < E.HEADROOM_MAX_CAP].max(initial=0))}; copies > 0 exactly where the verdict is Success: "
              f"{np.array_equal(copies > 0, verdicts == S.VERDICT_ALLOW)}", flush=True)
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
