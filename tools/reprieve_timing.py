"""Times the reprieve pass (kt_preempt_reprieve_launch) beside the prefix query it extends and beside the composed path a caller
has without it; the output is the record kept as profiles/reprieve_timing.txt.
usage: python tools/reprieve_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--cands 1000] [--reps 5]

On the seeded workload of tools/preempt_timing.py (thresholds a few pods below what is used):
  reprieve 1 x m   kt_preempt_reprieve_launch + kt_preempt_fetch for one pending pod over m running candidates
  reprieve n x m   the same for n = m pending pods in ONE launch
  preempt  ...     kt_preempt_launch + kt_preempt_fetch on the same inputs: the difference is what the walk adds
  composed 1 x m   a twin engine, starting from the prefix mask deleted (the prefix and its mask are taken as given: finding them is
                   what tools/preempt_timing.py times): per masked victim, last first, upsert it + kt_reconcile_launch(APPLY) +
                   kt_check, and kt_delete_pods again where the pod no longer passes.  n x m is n times that.
Method: warm runs first, then the minimum and the median over --reps of the wall clock around the synchronous calls."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S  # noqa: E402
from preempt_timing import NOW, timed, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    snap = workload(a.pods, a.throttles, a.dims)
    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    counted = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED
    running = np.nonzero((fl & (counted | S.POD_FINISHED)) == counted)[0]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    cands = running[:a.cands].astype(np.int64)
    many = pending[:a.cands].astype(np.int64)
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, candidates {len(cands)}, "
          f"preemptors {len(many)}, reps {a.reps}", flush=True)
    prefix, mask = eng.preempt(many, cands, NOW)
    prefix_r, left = eng.preempt(many, cands, NOW, reprieve=True)
    assert np.array_equal(prefix, prefix_r) and (left <= mask).all()
    masked, kept = mask.sum(axis=1), left.sum(axis=1)
    print(f"answers over the preemptors: positive prefix {(prefix > 0).sum()} (longest {int(prefix.max())}); masked victims per positive "
          f"preemptor: mean {masked[prefix > 0].mean():.1f}, most {int(masked.max())}; after the walk: mean {kept[prefix > 0].mean():.1f}, "
          f"most {int(kept.max())}", flush=True)
    i = int(np.argmax(masked))  # the preemptor with the most masked victims: the longest walk
    one = np.array([int(many[i])], np.int64)
    t_one_r = timed(lambda: eng.preempt(one, cands, NOW, reprieve=True), a.reps)
    t_one_p = timed(lambda: eng.preempt(one, cands, NOW), a.reps)
    t_many_r = timed(lambda: eng.preempt(many, cands, NOW, reprieve=True), a.reps)
    t_many_p = timed(lambda: eng.preempt(many, cands, NOW), a.reps)

    twin = E.Engine.for_snapshot(snap)
    victims = cands[mask[i] != 0]

    def passes():
        twin.reconcile_launch(NOW, apply=True)
        twin.synchronize()  # (a few-pod kt_check does not wait for a reconcile in flight: it would read the status before it)
        _, summary = twin.check_atomic(rows=one, want_status=False)
        return int(summary[0]) & 3 == 0

    def composed():
        twin.delete_pods(victims)
        out = np.ones(len(victims), bool)
        for j in range(len(victims) - 1, -1, -1):
            twin.upsert_pods(snap.pod_batch(victims[j:j + 1]), rows=victims[j:j + 1])
            if passes():
                out[j] = False
            else:
                twin.delete_pods(victims[j:j + 1])
        twin.upsert_pods(snap.pod_batch(victims[out]), rows=victims[out])
        return out

    got = composed()
    same = np.array_equal(victims[got], cands[left[i] != 0])
    t_comp = timed(composed, a.reps)
    print(f"reprieve, 1 preemptor x {len(cands)} candidates ({int(masked[i])} masked victims), launch + fetch: min {t_one_r[0]:.3f} ms, "
          f"median {t_one_r[1]:.3f} ms", flush=True)
    print(f"preempt alone, the same call: min {t_one_p[0]:.3f} ms, median {t_one_p[1]:.3f} ms -> the walk adds "
          f"{t_one_r[1] - t_one_p[1]:.3f} ms (medians)", flush=True)
    print(f"reprieve, {len(many)} preemptors x {len(cands)} candidates, launch + fetch: min {t_many_r[0]:.3f} ms, median {t_many_r[1]:.3f} ms",
          flush=True)
    print(f"preempt alone, the same call: min {t_many_p[0]:.3f} ms, median {t_many_p[1]:.3f} ms -> the walk adds "
          f"{t_many_r[1] - t_many_p[1]:.3f} ms (medians)", flush=True)
    print(f"composed walk on a twin (per victim: upsert + reconcile(APPLY) + check, delete again on a fail), 1 preemptor, "
          f"{len(victims)} victims: min {t_comp[0]:.3f} ms, median {t_comp[1]:.3f} ms (same victims as the kernel: {same})", flush=True)
    print(f"ratio composed / reprieve launch, one preemptor: {t_comp[1] / t_one_r[1]:.2f}x; composed / the walk's own share: "
          f"{t_comp[1] / max(t_one_r[1] - t_one_p[1], 1e-3):.0f}x; {len(many)} preemptors (composed = the mean walk of "
          f"{masked[prefix > 0].mean():.1f} victims x {(prefix > 0).sum()} preemptors, scaled from the one above): "
          f"{t_comp[1] / max(len(victims), 1) * masked.sum() / t_many_r[1]:.0f}x", flush=True)
    eng.close()
    twin.close()


if __name__ == "__main__":
    main()
