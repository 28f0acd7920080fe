"""Times kt_paged_preempt; the output is the record kept as profiles/preempt_paged_timing.txt.
usage: python tools/preempt_paged_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--cands 300] [--many 256] [--reps 15]

On the seeded workload of tools/preempt_timing.py (thresholds about three pods below what is used, so that pending pods are blocked
and victims help), for one preemptor and for --many preemptors against --cands running candidates, prefix alone and with the
reprieve pass:
  one page     kt_paged_preempt over the one engine (the new kernels) beside kt_preempt_launch / kt_preempt_reprieve_launch +
               kt_preempt_fetch (the single-engine kernels) on the SAME engine, run alternately; the two must return the same bytes.
  three pages  kt_paged_preempt over three engines of 16 names each: the same pods, namespaces and selectors, every page with
               request columns and thresholds of its own, about ONE pod below what is used (measured: three pods below gave 1 of
               256 preemptors a positive prefix over 300 candidates, one pod below 2 — most answers are KT_PREEMPT_NONE either way).
Method: warm runs of every shape first, then --reps rounds that alternate the variants; per variant the median, the minimum and
the maximum of the host clock around the synchronous calls (every call ends in a stream synchronise)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402

NOW = (1767225600, 0)


def tighten(snap, below=3):
    """Thresholds about ``below`` pods below `used`, no overrides (3: as tools/preempt_timing.py)."""
    T = snap.n_thr
    probe = E.Engine.for_snapshot(snap)
    used = probe.reconcile(NOW, apply=False).used
    probe.close()
    count = np.maximum(used.count[:T], 1)
    snap.thr_spec.v[:T] = np.maximum(used.v[:T] - below * (used.v[:T] // count[:, None]), 1)
    snap.thr_spec.count[:T] = np.maximum(used.count[:T] - below, 1)
    snap.thr_ovr_off[:] = 0
    return snap


def page_of(pods, throttles, dims, k, below=3):
    """Page k of a wide cluster: the seeded workload's pods and selectors, its request columns rotated by k and scaled by k + 1."""
    snap = W.generate(W.small(seed=7, n_pods=pods, n_thr=throttles, n_cluster=throttles // 2, D=dims))
    if k:
        nc = int(snap.pod_ctr_off[snap.n_pods])
        snap.ctr_req[:nc] = np.roll(snap.ctr_req[:nc], k, axis=1) * (k + 1)
        rolled = np.zeros(nc, np.uint32)
        for d in range(dims):
            rolled |= ((snap.ctr_present[:nc] >> np.uint32(d)) & np.uint32(1)) << np.uint32((d + k) % dims)
        snap.ctr_present[:nc] = rolled
    return tighten(snap, below)


def alternate(variants, reps):
    """{name: call} -> {name: (median, min, max) ms}; one warm run each, then `reps` rounds in which the variants take turns."""
    for call in variants.values():
        call()
    ms = {name: [] for name in variants}
    for _ in range(reps):
        for name, call in variants.items():
            t0 = time.perf_counter()
            call()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in ms.items()}


def line(what, t):
    print(f"{what}: median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--cands", type=int, default=300)
    ap.add_argument("--many", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()

    snap = page_of(a.pods, a.throttles, a.dims, 0)
    fl = snap.pod_flags[:snap.n_pods]
    counted = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED
    running = np.nonzero((fl & (counted | S.POD_FINISHED)) == counted)[0]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    cands = running[:a.cands].astype(np.int64)
    many = pending[:a.many].astype(np.int64)

    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, candidates {len(cands)}, preemptors 1 and "
          f"{len(many)}, reps {a.reps} (alternating)", flush=True)
    prefix, _ = eng.preempt(many, cands, NOW)
    print(f"one page, D {snap.D}: answers over the {len(many)} preemptors: none {(prefix < 0).sum()}, zero {(prefix == 0).sum()}, positive "
          f"{(prefix > 0).sum()} (longest {int(prefix.max())})", flush=True)
    one = np.array([int(many[np.argmax(prefix)])], np.int64)  # the preemptor with the longest prefix
    for pre, label in ((one, "1 preemptor"), (many, f"{len(many)} preemptors")):
        for reprieve in (False, True):
            single = eng.preempt(pre, cands, NOW, reprieve=reprieve)
            paged = E.paged_preempt([eng], pre, cands, NOW, reprieve=reprieve)
            assert [x.tobytes() for x in single] == [x.tobytes() for x in paged], "one page: the bytes differ"
            t = alternate({"single": lambda: eng.preempt(pre, cands, NOW, reprieve=reprieve),
                           "paged": lambda: E.paged_preempt([eng], pre, cands, NOW, reprieve=reprieve)}, a.reps)
            kind = "prefix + reprieve" if reprieve else "prefix"
            line(f"one page, {label} x {len(cands)} candidates, {kind}, kt_preempt{'_reprieve' if reprieve else ''}_launch + kt_preempt_fetch", t["single"])
            line(f"one page, {label} x {len(cands)} candidates, {kind}, kt_paged_preempt (same bytes)", t["paged"])
    eng.close()

    D = 16
    snaps = [page_of(a.pods, a.throttles, D, k, below=1) for k in range(3)]  # (see the module text)
    engs = [E.Engine.for_snapshot(s) for s in snaps]
    E.paged_reconcile(engs, NOW, apply=True)
    prefix, _ = E.paged_preempt(engs, many, cands, NOW)
    walked = E.paged_preempt(engs, many, cands, NOW, reprieve=True)[1]
    mask = E.paged_preempt(engs, many, cands, NOW)[1]
    print(f"three pages, D {D} each: answers over the {len(many)} preemptors: none {(prefix < 0).sum()}, zero {(prefix == 0).sum()}, positive "
          f"{(prefix > 0).sum()} (longest {int(prefix.max())}); victims per positive prefix: mask {mask[prefix > 0].sum(axis=1).mean() if (prefix > 0).any() else 0:.1f}, "
          f"after the walk {walked[prefix > 0].sum(axis=1).mean() if (prefix > 0).any() else 0:.1f}", flush=True)
    one = np.array([int(many[np.argmax(prefix)])], np.int64)
    for pre, label in ((one, "1 preemptor"), (many, f"{len(many)} preemptors")):
        t = alternate({"prefix": lambda: E.paged_preempt(engs, pre, cands, NOW),
                       "reprieve": lambda: E.paged_preempt(engs, pre, cands, NOW, reprieve=True)}, a.reps)
        line(f"three pages, {label} x {len(cands)} candidates, prefix, kt_paged_preempt", t["prefix"])
        line(f"three pages, {label} x {len(cands)} candidates, prefix + reprieve, kt_paged_preempt", t["reprieve"])
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
