"""Times kt_paged_headroom_gangs; the output is the record kept as profiles/headroom_gangs_paged_timing.txt.
usage: python tools/headroom_gangs_paged_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--room 200] [--reps 15]

On the workload of tools/preempt_paged_timing.py (page k: the seeded pods and selectors, the request columns rotated by k and
scaled by k + 1) with every page's thresholds loosened to --room mean requests per name (the page's mean request where the
throttle's pods use nothing of a name) and 4 x --room pods above that page's `used` (the count part is the same in every
page), no overrides, so that the answers lie between 0 and the cap; for ONE gang of 4
pending pods and for 256 gangs of 8 (consecutive pending rows), each at cap = 64 and cap = 2^31 - 1:
  (a) one page     kt_paged_headroom_gangs over the one engine (the new kernel) beside kt_headroom_gangs_launch +
                   kt_headroom_gangs_fetch (the single-engine kernel) on the SAME engine; the two must return the same bytes.
                   This is the cost of the page loop: what folding the single kernel into the one-page case would pay.
  (b) three pages  kt_paged_headroom_gangs over three engines of 16 names each beside the COMPOSITION a caller has without it on
                   the same engines: one kt_headroom_gangs_launch + kt_headroom_gangs_fetch per page and, on the host, the
                   minimum over the pages of (copies, blocker or the gang's end, limiting or +inf), mapped back to
                   (cap, -1, -1) at the cap.  The composition holds where every page carries the same count part; the same answers
                   are asserted.
Method: warm runs of every variant first, then --reps rounds that alternate the variants in one process; per variant the median,
the minimum and the maximum of the host clock around the synchronous calls.  A record for the next change, not a gate: the line
behind each pair says whether the difference of the medians is more than five times the larger of the two spreads (max - min)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kube_throttler_amd import engine as E, snapshot as S  # noqa: E402
from preempt_paged_timing import NOW, alternate, line, page_of  # noqa: E402


def loosened(snap, room):
    """Thresholds ``room`` mean requests per name and 4 x ``room`` pods above `used`, no overrides (as tools/headroom_gangs_timing.py);
    a name of which the throttle's pods use nothing (the rotated columns of pages 1..) takes the page's mean non-zero request."""
    T = snap.n_thr
    probe = E.Engine.for_snapshot(snap)
    used = probe.reconcile(NOW, apply=False).used
    probe.close()
    count = np.maximum(used.count[:T], 1)
    req = snap.ctr_req[:int(snap.pod_ctr_off[snap.n_pods])]
    floor = max(int(req[req > 0].mean()), 1) if (req > 0).any() else 1
    snap.thr_spec.v[:T] = used.v[:T] + room * np.maximum(used.v[:T] // count[:, None], floor) + 1
    snap.thr_spec.count[:T] = used.count[:T] + 4 * room
    snap.thr_ovr_off[:] = 0
    return snap


def composed(engs, rows, off, cap):
    """One single-engine gang headroom per page, then identity I3 on the host -> (copies, limiting, blocker)."""
    big32 = np.int32(0x7FFFFFFF)
    best = None
    for e in engs:
        c, l, b = e.headroom_gangs(rows, off, cap=cap)
        key = (c, np.where(b < 0, off[1:], b), np.where(l < 0, big32, l))
        if best is None:
            best = key
            continue
        less = (key[0] < best[0]) | ((key[0] == best[0]) & ((key[1] < best[1]) | ((key[1] == best[1]) & (key[2] < best[2]))))
        best = tuple(np.where(less, k, b_) for k, b_ in zip(key, best))
    at_cap = best[0] >= cap
    return (best[0], np.where(at_cap | (best[2] == big32), -1, best[2]).astype(np.int32), np.where(at_cap, -1, best[1]).astype(np.int64))


def answers(copies, cap):
    below = copies[copies < cap]
    return (f"0: {(copies == 0).sum()}, between: {((copies > 0) & (copies < cap)).sum()}, the cap: {(copies == cap).sum()}, largest below the "
            f"cap: {int(below.max()) if len(below) else '-'}")


def verdict(name_a, a, name_b, b):
    diff, spread = a[0] - b[0], max(a[2] - a[1], b[2] - b[1])
    how = "MORE than" if abs(diff) > 5 * spread else "within"
    print(f"    {name_a} - {name_b} = {diff:+.3f} ms of medians, the larger spread {spread:.3f} ms: {how} five times the spread", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--room", type=int, default=200)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    caps = (64, E.HEADROOM_MAX_CAP)

    snap = loosened(page_of(a.pods, a.throttles, a.dims, 0), a.room)
    fl = snap.pod_flags[:snap.n_pods]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0].astype(np.int64)
    shapes = [(f"{n} x {size}", pending[:n * size], np.arange(n + 1, dtype=np.int64) * size) for n, size in ((1, 4), (256, 8))]

    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, pending pods {len(pending)}, room {a.room}, "
          f"reps {a.reps} (alternating)", flush=True)
    for label, rows, off in shapes:
        for cap in caps:
            single = eng.headroom_gangs(rows, off, cap=cap)
            paged = E.paged_headroom_gangs([eng], rows, off, cap)
            assert [x.tobytes() for x in single] == [x.tobytes() for x in paged], "one page: the bytes differ"
            print(f"(a) one page, D {snap.D}, {label} members, cap {cap}: answers {answers(single[0], cap)}", flush=True)
            t = alternate({"single": lambda: eng.headroom_gangs(rows, off, cap=cap), "paged": lambda: E.paged_headroom_gangs([eng], rows, off, cap)},
                          a.reps)
            line(f"(a) one page, {label} members, cap {cap}, kt_headroom_gangs_launch + kt_headroom_gangs_fetch", t["single"])
            line(f"(a) one page, {label} members, cap {cap}, kt_paged_headroom_gangs (same bytes)", t["paged"])
            verdict("paged", t["paged"], "single", t["single"])
    eng.close()

    D = 16
    engs = [E.Engine.for_snapshot(loosened(page_of(a.pods, a.throttles, D, k), a.room)) for k in range(3)]
    E.paged_reconcile(engs, NOW, apply=True)
    for label, rows, off in shapes:
        for cap in caps:
            fused = E.paged_headroom_gangs(engs, rows, off, cap)
            comp = composed(engs, rows, off, cap)
            assert [x.tolist() for x in fused] == [x.tolist() for x in comp], "three pages: the composition disagrees"
            own = engs[0].headroom_gangs(rows, off, cap=cap)[0]
            print(f"(b) three pages, D {D} each, {label} members, cap {cap}: answers {answers(fused[0], cap)}; decided by a page >= 1: "
                  f"{int((own != fused[0]).sum())}", flush=True)
            t = alternate({"composed": lambda: composed(engs, rows, off, cap), "fused": lambda: E.paged_headroom_gangs(engs, rows, off, cap)}, a.reps)
            line(f"(b) three pages, {label} members, cap {cap}, composed: kt_headroom_gangs_launch + fetch per page, the minimum on the host",
                 t["composed"])
            line(f"(b) three pages, {label} members, cap {cap}, kt_paged_headroom_gangs (same answers)", t["fused"])
            verdict("fused", t["fused"], "composed", t["composed"])
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
