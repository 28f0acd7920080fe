"""Times gang admission (kt_admit_gangs_launch) beside plain admission (kt_admit_launch) on a BASELINE config: HIP events on
the stream around the launch (the status-matrix check and the queue walk), dry runs, no fetch inside the timed span.
usage: python tools/gang_admit_bench.py [--config 2] [--pods 200000] [--queue 4000] [--head-room 2,4,8] [--reps 9] [--plain-only]
       python tools/gang_admit_bench.py --elastic [--runs 6] [...]

Per head-room factor (thresholds x factor: how much of the queue fits) one JSON line with the median / min / max over --reps of
  plain     kt_admit_launch
  gangs1    kt_admit_gangs_launch with gangs of one pod (the same answers as plain, asserted)
  gangs8    kt_admit_gangs_launch with gangs of eight consecutive pods, and the share of them that is rolled back
--plain-only times kt_admit_launch alone: the form that also runs on a library without the gang entry points (an older commit's
tree with this file copied in), for the comparison across commits.  Run the two alternately: the spread between runs of the
SAME library is the noise the comparison has to be read against.
--elastic compares kt_admit_gangs_elastic_launch with min_members = the gang's size and no flags (the same answers as
kt_admit_gangs_launch, asserted) against kt_admit_gangs_launch on the same queue in gangs of eight: --runs runs per side,
alternately, a run being the median of --reps timed launches; per side the median of the runs and their spread (max - min), and
whether elastic - gangs stays within five times the spread of kt_admit_gangs_launch."""
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
ap.add_argument("--elastic", action="store_true")
ap.add_argument("--runs", type=int, default=6)
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
    if a.elastic:
        eights = np.unique(np.concatenate([np.arange(0, n, 8), [n]])).astype(np.int64)
        g8, sizes = len(eights) - 1, np.diff(eights).astype(np.int64)
        gangs = lambda: eng._ck(L.kt_admit_gangs_launch(h, n, queue.ctypes.data, g8, eights.ctypes.data, 0, 0, sh))  # noqa: E731
        elastic = lambda: eng._ck(L.kt_admit_gangs_elastic_launch(h, n, queue.ctypes.data, g8, eights.ctypes.data, sizes.ctypes.data, None, 0, 0, sh))  # noqa: E731
        gangs()
        st_g, sm_g = eng.check_fetch(n, True)
        adm = eng.admit_gangs_fetch(g8)
        elastic()
        st_e, sm_e = eng.check_fetch(n, True)
        members = eng.admit_gangs_elastic_fetch(g8)
        assert (st_e == st_g).all() and (sm_e == sm_g).all(), "min = size, no flags: status or summaries differ from kt_admit_gangs_launch"
        assert ((members > 0) == (adm != 0)).all() and (members[adm != 0] == sizes[adm != 0]).all()
        runs = {"gangs8": [], "elastic8": []}
        for _ in range(a.runs):  # alternately
            runs["gangs8"].append(timed(gangs, a.reps)["median_ms"])
            runs["elastic8"].append(timed(elastic, a.reps)["median_ms"])
        del line["plain"], line["plain_admitted"]
        line.update({"runs": a.runs, "gangs8_gangs": g8, "gangs8_rolled_back": int((adm == 0).sum())})
        for k, v in runs.items():
            v = sorted(v)
            line[k] = {"runs_ms": [round(x, 4) for x in runs[k]], "median_ms": (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, "spread_ms": v[-1] - v[0]}
        diff, bar = line["elastic8"]["median_ms"] - line["gangs8"]["median_ms"], 5 * line["gangs8"]["spread_ms"]
        line["elastic_minus_gangs_ms"], line["five_spreads_of_gangs_ms"] = diff, bar
        line["within_the_bar"] = bool(diff <= bar)
    elif not a.plain_only:
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
