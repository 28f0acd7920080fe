"""Times kt_admit_launch (sequential admission with reservation) on a BASELINE config.
usage: python tools/admit_bench.py [--config 2] [--queue 20000] [--pods 1000000] [--pages 1,2,4]

--pages P[,P...]: the SAME snapshot loaded into P engines and admitted through kt_paged_admit.  Combining identical pages is
the identity, so the paged answers must equal kt_admit_launch on one engine (asserted); one JSON line per P beside the
two one-engine lines (summaries only; summaries + status matrix, which is what kt_paged_admit copies to the host and what
"one_engine_us_per_pod" of the P lines quotes), and one for the host loop kt_paged_admit replaces (per pod: kt_paged_check,
then kt_set_reserved on every page) on a short queue."""
import argparse
import json
import sys
import time
import os

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=2)
ap.add_argument("--queue", type=int, default=20000)
ap.add_argument("--pods", type=int, default=1000000)
ap.add_argument("--pages", default="")
ap.add_argument("--host-queue", type=int, default=200)
a = ap.parse_args()
cfg = W.preset(a.config)
cfg.n_pods_total = cfg.n_pods = a.pods
snap = W.generate(cfg)
T = snap.n_thr
# head-room, as in tests/test_engine_gpu.py::test_admit_queue_*: the queue fills the throttles up on the way
snap.thr_spec.v[:T] = snap.thr_spec.v[:T] * 2 + 1
snap.thr_spec.count[:T] = snap.thr_spec.count[:T] * 2 + 3
eng = E.Engine.for_snapshot(snap)
eng.reconcile((1767225600, 0), apply=True)
fl = snap.pod_flags[:snap.n_pods]
pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0][:a.queue].astype(np.int64)
eng.admit(pending[:256], commit=False, want_status=False)  # warm-up (allocations)
def best_of(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best, out


best, (_, sm) = best_of(lambda: eng.admit(pending, commit=False, want_status=False))
verdict = S.summary_fields(sm)[0]
print(json.dumps({"config": a.config, "pods": int(snap.n_pods), "throttles": int(T), "queue": int(len(pending)),
                  "admitted": int((verdict == S.VERDICT_ALLOW).sum()), "blocked": int((verdict == S.VERDICT_BLOCK).sum()),
                  "seconds": best, "pods_per_s": len(pending) / best, "us_per_pod": 1e6 * best / len(pending),
                  "note": "one kt_admit_launch + kt_check_fetch (summaries only), dry run; wall clock incl. launch and D2H"}))
# what kt_paged_admit hands back: the status matrix too (the yardstick of the --pages lines)
eng.admit(pending[:256], commit=False)
best_m, (stm, smm) = best_of(lambda: eng.admit(pending, commit=False))
assert (smm == sm).all()
print(json.dumps({"config": a.config, "queue": int(len(pending)), "seconds": best_m, "us_per_pod": 1e6 * best_m / len(pending),
                  "note": "one kt_admit_launch + kt_check_fetch (summaries + status matrix), dry run; wall clock"}))

for P in [int(x) for x in a.pages.split(",") if x]:
    pages = [E.Engine.for_snapshot(snap) for _ in range(P)]
    for e in pages:
        e.reconcile((1767225600, 0), apply=True)
    E.paged_admit(pages, pending[:256])  # warm-up (allocations)
    dt, (pst, psm) = best_of(lambda: E.paged_admit(pages, pending))
    assert (psm == sm).all(), f"{P} identical pages: summaries differ from kt_admit_launch"
    assert (pst == stm).all(), f"{P} identical pages: statuses differ from kt_admit_launch"
    print(json.dumps({"pages": P, "pods": int(snap.n_pods), "throttles": int(T), "queue": int(len(pending)), "seconds": dt,
                      "us_per_pod": 1e6 * dt / len(pending), "one_engine_us_per_pod": 1e6 * best_m / len(pending),
                      "note": "kt_paged_admit, dry run, summaries + status matrix to the host; wall clock"}))
    if P > 1:
        # the host loop kt_paged_admit replaces: per pod kt_paged_check, then on Success kt_set_reserved on every page
        q = pending[:a.host_queue]
        req = [e.fetch_pod_requests(q) for e in pages]
        rows_all = np.arange(T, dtype=np.int32)
        res = [e.fetch_reserved(rows_all) for e in pages]
        t0 = time.perf_counter()
        admitted = 0
        for k, p in enumerate(q):
            st, smk = E.paged_check(pages, 1, rows=[p])
            if int(smk[0]) & 3:
                continue
            admitted += 1
            aff = np.nonzero(st[0])[0].astype(np.int32)
            if len(aff) == 0:
                continue
            for e, r, (v, pr) in zip(pages, res, req):
                r.v[aff] += v[k]
                r.present[aff] |= pr[k]
                r.count[aff] = np.where(r.has_count[aff] != 0, r.count[aff], 0) + 1
                r.has_count[aff] = 1
                sub = S.Amounts(len(aff), e.D)
                for f in ("v", "present", "count", "has_count"):
                    getattr(sub, f)[:] = getattr(r, f)[aff]
                e.set_reserved(aff, sub)
        dt_host = time.perf_counter() - t0
        print(json.dumps({"pages": P, "host_loop_queue": int(len(q)), "admitted": admitted, "seconds": dt_host,
                          "us_per_pod": 1e6 * dt_host / len(q),
                          "note": "host loop: kt_paged_check + kt_set_reserved per page per admitted pod (commits)"}))
    for e in pages:
        e.close()
eng.close()
