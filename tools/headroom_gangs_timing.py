"""Times the gang headroom (kt_headroom_gangs_launch) beside the composed path a caller has without it; the output is the record
kept as profiles/headroom_gangs_timing.txt.
usage: python tools/headroom_gangs_timing.py [--reps 5] [--configs 2 3] [--room 200]

On the engine of bench.py's configs[N] (W.preset(N)) with its thresholds --room mean requests above `used` (as the presets stand
every pending pod is blocked and every answer is 0), reconciled once, with pending pods as members:
  (a) 1 x 4       kt_headroom_gangs_launch + kt_headroom_gangs_fetch for ONE gang of 4 members
  (b) 256 x 8     the same for 256 gangs of 8 members, ONE launch
each for cap = 64 and cap = 2^31 - 1.
  composed        what the same number costs without the call: per gang a bisection on the host (doubling k first, then halving
                  the bracket) over dry kt_admit_gangs_launch calls of k consecutive copies of the gang — "are all k admitted".
                  Each call is ONE wave walking k x members positions in sequence, and it names every pod k times, which the
                  admission queue's contract does not allow.  A gang whose answer is beyond --walk-limit copies (the cap, for a
                  gang no throttle stops) is left out of the composed path at cap = 2^31 - 1: its walk alone would be 2^31 x
                  members positions.  The answers are compared where both exist.
Method: warm runs first, then the minimum and the median over --reps of the wall clock around the synchronous calls.  A record
for the next change, not a gate."""
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
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--walk-limit", type=int, default=512)
    ap.add_argument("--room", type=int, default=200, help="thresholds this many mean requests above `used` (0: the preset as it stands)")
    a = ap.parse_args()
    for config in a.configs:
        one_config(config, a)


def one_config(config, a):
    cfg = W.preset(config)
    snap = W.generate(cfg)
    now = (cfg.now_s, 0)
    if a.room > 0:
        # as the presets stand every pending pod is blocked (every answer is 0): the thresholds are put --room mean requests per
        # name and 4 x --room pods above `used`, without overrides, as tools/headroom_timing.py does it
        T = snap.n_thr
        probe = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
        used = probe.reconcile(now, apply=False).used
        probe.close()
        count = np.maximum(used.count[:T], 1)
        snap.thr_spec.v[:T] = used.v[:T] + a.room * (used.v[:T] // count[:, None]) + 1
        snap.thr_spec.count[:T] = used.count[:T] + 4 * a.room
        snap.thr_ovr_off[:] = 0
    eng = E.Engine.for_snapshot(snap, E.VARIANT_INDEXED)
    eng.reconcile(now, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)
    print(f"library {E.version()}; configs[{config}]: pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, "
          f"pending pods {len(pending)}, reps {a.reps}", flush=True)

    def all_admitted(one, k):
        rows = np.tile(one, k)
        off = np.arange(k + 1, dtype=np.int64) * len(one)
        return bool(eng.admit_gangs(rows, off, commit=False, want_status=False)[2].all())

    def composed(members, off, cap, gangs):
        out = {}
        for g in gangs:
            one = members[off[g]:off[g + 1]]
            lo, hi = 0, 1  # lo copies are admitted; hi: the first count tried that is not (or cap + 1)
            while hi <= cap and all_admitted(one, hi):
                lo, hi = hi, hi * 2
            hi = min(hi, cap + 1)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if all_admitted(one, mid) else (lo, mid)
            out[g] = lo
        return out

    for label, n_gangs, size in (("(a)", 1, 4), ("(b)", 256, 8)):
        members = pending[:n_gangs * size]
        off = np.arange(n_gangs + 1, dtype=np.int64) * size
        for cap in (64, E.HEADROOM_MAX_CAP):
            copies, limiting, blocker = eng.headroom_gangs(members, off, cap=cap)
            print(f"{label} cap {cap}: answers over the {n_gangs} gang(s) of {size}: 0: {(copies == 0).sum()}, between: "
                  f"{((copies > 0) & (copies < cap)).sum()}, the cap: {(copies == cap).sum()}, largest below the cap: "
                  f"{int(copies[copies < cap].max()) if (copies < cap).any() else '-'}", flush=True)
            t_q = timed(lambda: eng.headroom_gangs(members, off, cap=cap), a.reps)
            print(f"{label} cap {cap}: headroom gangs, {n_gangs} x {size} members, launch + fetch: min {t_q[0]:.3f} ms, median {t_q[1]:.3f} ms",
                  flush=True)
            gangs = [g for g in range(n_gangs) if cap == 64 or copies[g] <= a.walk_limit]
            got = composed(members, off, cap, gangs)
            same = all(got[g] == int(copies[g]) for g in gangs)
            t_c = timed(lambda: composed(members, off, cap, gangs), max(a.reps // 2, 1), warm=0)
            print(f"{label} cap {cap}: composed (per gang a bisection over dry admit_gangs of k copies) over {len(gangs)} of the {n_gangs} "
                  f"gang(s): min {t_c[0]:.3f} ms, median {t_c[1]:.3f} ms (same copies as the kernel: {same}); ratio composed / headroom "
                  f"gangs: {t_c[1] / t_q[1]:.1f}x", flush=True)
    t_plain = timed(lambda: eng.headroom(pending[:2048], cap=E.HEADROOM_MAX_CAP), a.reps)
    print(f"beside it: kt_headroom_launch over the same 2048 pods one by one, cap 2^31 - 1, launch + fetch: median {t_plain[1]:.3f} ms", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
