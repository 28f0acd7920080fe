"""Times kt_paged_preempt_gangs; the output is the record kept as profiles/preempt_gangs_paged_timing.txt.
usage: python tools/preempt_gangs_paged_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--cands 300] [--gangs 256] [--size 2]
                                                  [--reps 15]

On the seeded workload of tools/preempt_paged_timing.py (thresholds about three pods below what is used, so that pending pods are
blocked and victims help), for one gang and for --gangs gangs of --size pending pods against --cands running candidates, prefix alone
and with the reprieve pass:
  one page     kt_paged_preempt_gangs over the one engine (the new kernels) beside kt_preempt_gangs_launch /
               kt_preempt_gangs_reprieve_launch + kt_preempt_gangs_fetch (the single-engine kernels) on the SAME engine, run
               alternately in one visit; the two must return the same bytes (asserted).
  three pages  kt_paged_preempt_gangs over three engines of 16 names each: the pages of tools/preempt_paged_timing.py, thresholds
               about ONE pod below what is used.  Where no gang of --size has a positive prefix there (the walk then has nothing to
               do), gangs of one are timed as well.
Method: warm runs of every shape first, then --reps rounds that alternate the variants; per variant the median, the minimum and
the maximum of the host clock around the synchronous calls (every call ends in a stream synchronise)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S  # noqa: E402
from preempt_paged_timing import NOW, alternate, line, page_of  # noqa: E402


def answers(prefix):
    return f"none {(prefix < 0).sum()}, zero {(prefix == 0).sum()}, positive {(prefix > 0).sum()} (longest {int(prefix.max())})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--cands", type=int, default=300)
    ap.add_argument("--gangs", type=int, default=256)
    ap.add_argument("--size", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()

    snap = page_of(a.pods, a.throttles, a.dims, 0)
    fl = snap.pod_flags[:snap.n_pods]
    counted = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED
    running = np.nonzero((fl & (counted | S.POD_FINISHED)) == counted)[0]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    cands = running[:a.cands].astype(np.int64)
    members = pending[:a.gangs * a.size].astype(np.int64)
    n_gangs = len(members) // a.size
    members = members[:n_gangs * a.size]
    off = np.arange(n_gangs + 1, dtype=np.int64) * a.size
    one_off = np.array([0, a.size], np.int64)

    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, candidates {len(cands)}, gangs 1 and {n_gangs} "
          f"of {a.size}, reps {a.reps} (alternating)", flush=True)
    prefix, _, _ = eng.preempt_gangs(members, off, cands, NOW)
    print(f"one page, D {snap.D}: answers over the {n_gangs} gangs: {answers(prefix)}", flush=True)
    g = int(np.argmax(prefix))  # the gang with the longest prefix
    one = members[off[g]:off[g + 1]].copy()
    for rows, offs, label in ((one, one_off, "1 gang"), (members, off, f"{n_gangs} gangs")):
        for reprieve in (False, True):
            single = eng.preempt_gangs(rows, offs, cands, NOW, reprieve=reprieve)
            paged = E.paged_preempt_gangs([eng], rows, offs, cands, NOW, reprieve=reprieve)
            assert [x.tobytes() for x in single] == [x.tobytes() for x in paged], "one page: the bytes differ"
            t = alternate({"single": lambda: eng.preempt_gangs(rows, offs, cands, NOW, reprieve=reprieve),
                           "paged": lambda: E.paged_preempt_gangs([eng], rows, offs, cands, NOW, reprieve=reprieve)}, a.reps)
            kind = "prefix + reprieve" if reprieve else "prefix"
            line(f"one page, {label} of {a.size} x {len(cands)} candidates, {kind}, kt_preempt_gangs{'_reprieve' if reprieve else ''}_launch + "
                 f"kt_preempt_gangs_fetch", t["single"])
            line(f"one page, {label} of {a.size} x {len(cands)} candidates, {kind}, kt_paged_preempt_gangs (same bytes)", t["paged"])
    eng.close()

    D = 16
    snaps = [page_of(a.pods, a.throttles, D, k, below=1) for k in range(3)]
    engs = [E.Engine.for_snapshot(s) for s in snaps]
    E.paged_reconcile(engs, NOW, apply=True)
    # gangs of --size rarely fit on three tight pages: where none has a positive prefix the walk has nothing to do, and gangs of
    # one (what kt_paged_preempt answers) are timed as well
    for size in (a.size, 1):
        rows_all = members[:n_gangs * size] if size == a.size else members[:n_gangs]
        off_all = np.arange(n_gangs + 1, dtype=np.int64) * size
        prefix, mask, _ = E.paged_preempt_gangs(engs, rows_all, off_all, cands, NOW)
        walked = E.paged_preempt_gangs(engs, rows_all, off_all, cands, NOW, reprieve=True)[1]
        pos = prefix > 0
        print(f"three pages, D {D} each: answers over the {n_gangs} gangs of {size}: {answers(prefix)}; victims per positive prefix: mask "
              f"{mask[pos].sum(axis=1).mean() if pos.any() else 0:.1f}, after the walk {walked[pos].sum(axis=1).mean() if pos.any() else 0:.1f}",
              flush=True)
        g = int(np.argmax(prefix))
        one = rows_all[off_all[g]:off_all[g + 1]].copy()
        for rows, offs, label in ((one, np.array([0, size], np.int64), "1 gang"), (rows_all, off_all, f"{n_gangs} gangs")):
            t = alternate({"prefix": lambda: E.paged_preempt_gangs(engs, rows, offs, cands, NOW),
                           "reprieve": lambda: E.paged_preempt_gangs(engs, rows, offs, cands, NOW, reprieve=True)}, a.reps)
            line(f"three pages, {label} of {size} x {len(cands)} candidates, prefix, kt_paged_preempt_gangs", t["prefix"])
            line(f"three pages, {label} of {size} x {len(cands)} candidates, prefix + reprieve, kt_paged_preempt_gangs", t["reprieve"])
        if pos.any() or a.size == 1:
            break
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
