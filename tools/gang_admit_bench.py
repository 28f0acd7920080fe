"""Times gang admission (kt_admit_gangs_launch) beside plain admission (kt_admit_launch) on a BASELINE config: HIP events on
the stream around the launch (the status-matrix check and the queue walk), dry runs, no fetch inside the timed span.
usage: python tools/gang_admit_bench.py [--config 2] [--pods 200000] [--queue 4000] [--head-room 2,4,8] [--reps 9] [--plain-only]

Per head-room factor (thresholds x factor: how much of the queue fits) one JSON line with the median / min / max over --reps of
  plain     kt_admit_launch
  gangs1    kt_admit_gangs_launch with gangs of one pod (the same answers as plain, asserted)
  gangs8    kt_admit_gangs_launch with gangs of eight consecutive pods, and the share of them that is rolled back
--plain-only times kt_admit_launch alone: the form that also runs on a library without the gang entry points (an older commit's
tree with this file copied in), for the comparison across commits.  Run the two alternately: the spread between runs of the
SAME library is the noise the comparison has to be read against."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S, workload as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=2)
ap.add_argument("--pods", type=int, default=200000)
ap.add_argument("--queue", type=int, default=4000)
ap.add_argument("--head-room", default="2,4,8")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--plain-only", action="store_true")
a = ap.parse_args()

stream = torch.cuda.Stream()
sh = C.c_void_p(stream.cuda_stream)


def timed(launch, reps):
    """ms per call: HIP events recorded on the stream in front of and behind the launch."""
    out = []
    for _ in range(reps + 1):  # the first call allocates
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        launch()
        t1.record(stream)
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    out = sorted(out[1:])
    return {"median_ms": out[len(out) // 2], "min_ms": out[0], "max_ms": out[-1]}


for factor in [int(x) for x in a.head_room.split(",") if x]:
    cfg = W.preset(a.config)
    cfg.n_pods_total = cfg.n_pods = a.pods
    snap = W.generate(cfg)
    T = snap.n_thr
    snap.thr_spec.v[:T] = snap.thr_spec.v[:T] * factor + 1
    snap.thr_spec.count[:T] = snap.thr_spec.count[:T] * factor + 3
    eng = E.Engine.for_snapshot(snap)
    eng.reconcile((1767225600, 0), apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    queue = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0][:a.queue].astype(np.int64)
    n = len(queue)
    L, h = E.lib(), eng._h
    line = {"config": a.config, "pods": int(snap.n_pods), "throttles": int(T), "dims": int(eng.D), "queue": n, "head_room": factor,
            "reps": a.reps, "library": E.version()}
    line["plain"] = timed(lambda: eng._ck(L.kt_admit_launch(h, n, queue.ctypes.data, 0, 0, sh)), a.reps)
    _, sm = eng.check_fetch(n)
    line["plain_admitted"] = int((sm == 0).sum())
    if not a.plain_only:
        ones = np.arange(n + 1, dtype=np.int64)
        eights = np.unique(np.concatenate([np.arange(0, n, 8), [n]])).astype(np.int64)
        line["gangs1"] = timed(lambda: eng._ck(L.kt_admit_gangs_launch(h, n, queue.ctypes.data, n, ones.ctypes.data, 0, 0, sh)), a.reps)
        _, sm1 = eng.check_fetch(n)
        assert (sm1 == sm).all(), "gangs of one pod: summaries differ from kt_admit_launch"
        assert (eng.admit_gangs_fetch(n) == (sm == 0)).all()
        g8 = len(eights) - 1
        line["gangs8"] = timed(lambda: eng._ck(L.kt_admit_gangs_launch(h, n, queue.ctypes.data, g8, eights.ctypes.data, 0, 0, sh)), a.reps)
        _, sm8 = eng.check_fetch(n)
        adm = eng.admit_gangs_fetch(g8)
        line["gangs8_gangs"] = g8
        line["gangs8_rolled_back"] = int((adm == 0).sum())
        line["gangs8_members_that_reserved_in_rolled_back_gangs"] = int(((sm8 == 0) & (np.repeat(adm, np.diff(eights)) == 0)).sum())
    print(json.dumps(line), flush=True)
    eng.close()
