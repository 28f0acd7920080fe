"""Times the gang forecast (kt_forecast_gangs_launch) beside the composed path a caller has without it; the output is the record
kept as profiles/forecast_gangs_timing.txt.
usage: python tools/forecast_gangs_timing.py [--config 2] [--instants 64] [--reps 5]

On the engine of bench.py's configs[N] (W.preset(N)), with pending pods as members and --instants instants one hour apart:
  (a) 1 x 4       kt_forecast_gangs_launch + kt_forecast_gangs_fetch for ONE gang of 4 members
  (b) 256 x 8     the same for 256 gangs of 8 members, ONE launch
  composed        what the same answers cost without the call, on a twin engine: per instant a kt_reconcile_launch(t, APPLY), then
                  per gang a dry kt_admit_gangs_launch of that one gang (gangs are judged independently of each other: one launch
                  per gang).  It also leaves the twin's stored status at the last instant, which the query never does.
Method: warm runs first, then the minimum and the median over --reps of the wall clock around the synchronous calls."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402
from preempt_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--instants", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    cfg = W.preset(a.config)
    snap = W.generate(cfg)
    now = (cfg.now_s, 0)
    inst = [(now[0] + 3600 * k, 0) for k in range(a.instants)]
    eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    twin = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    eng.reconcile(now, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)
    print(f"library {E.version()}; configs[{a.config}]: pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, "
          f"pending pods {len(pending)}, instants {len(inst)}, reps {a.reps}", flush=True)

    def composed(members, off):
        out = np.zeros((len(off) - 1, len(inst)), np.uint8)
        for k, t in enumerate(inst):
            twin.reconcile_launch(t, apply=True)
            twin.synchronize()
            for g in range(len(off) - 1):
                one = members[off[g]:off[g + 1]]
                out[g, k] = 0 if twin.admit_gangs(one, [0, len(one)], commit=False, want_status=False)[2][0] else 1
        return out

    for label, n_gangs, size in (("(a)", 1, 4), ("(b)", 256, 8)):
        members = pending[:n_gangs * size]
        off = np.arange(n_gangs + 1, dtype=np.int64) * size
        first, verdicts, blockers = eng.forecast_gangs(members, off, inst)
        err = (verdicts == 2).any(axis=1)
        print(f"{label} answers over the {n_gangs} gang(s) of {size}: first = 0: {(first == 0).sum()}, first >= 1: {(first >= 1).sum()}, "
              f"none: {(first < 0).sum()}, with an Error member: {err.sum()}", flush=True)
        t_q = timed(lambda: eng.forecast_gangs(members, off, inst), a.reps)
        got = composed(members, off)
        same = np.array_equal(got[~err], verdicts[~err])
        t_c = timed(lambda: composed(members, off), max(a.reps // 2, 1), warm=0)
        print(f"{label} forecast gangs, {n_gangs} x {size} members x {len(inst)} instants, launch + fetch: min {t_q[0]:.3f} ms, "
              f"median {t_q[1]:.3f} ms", flush=True)
        print(f"{label} composed (per instant reconcile(APPLY), per gang a dry admit_gangs): min {t_c[0]:.3f} ms, median {t_c[1]:.3f} ms "
              f"(same verdicts as the kernel where no member is an Error: {same}); ratio composed / forecast gangs: {t_c[1] / t_q[1]:.1f}x",
              flush=True)
    t_plain = timed(lambda: eng.forecast(pending[:2048], inst), a.reps)
    print(f"beside it: kt_forecast_launch over the same 2048 pods one by one, launch + fetch: median {t_plain[1]:.3f} ms", flush=True)
    eng.close()
    twin.close()


if __name__ == "__main__":
    main()
