"""Times the gang preemption query (kt_preempt_gangs_launch) beside the composed path a caller has without it; the output is the
record kept as profiles/preempt_gangs_timing.txt.
usage: python tools/preempt_gangs_timing.py [--pods 20000] [--throttles 1000] [--dims 8] [--cands 1000] [--gangs 256] [--size 4] [--reps 5]
                                            [--reprieve]

On the seeded workload of tools/preempt_timing.py (thresholds a few pods below what is used, so that pending pods are blocked
and victims help):
  gangs G x m      kt_preempt_gangs_launch + kt_preempt_gangs_fetch for G gangs of --size pending pods over m running candidates,
                   ONE launch
  gangs 1 x m      the same for the one gang with the longest prefix
  singles          kt_preempt_launch + kt_preempt_fetch over the same member rows (what the gang form adds to the single query)
  composed 1 x m   a scratch engine: kt_delete_pods + kt_reconcile_launch(APPLY) + a dry kt_admit_gangs_launch of the one gang per
                   prefix step, the prefix length BISECTED (the fairest thing a caller can do today; it assumes the verdict is
                   monotone in k, which kt_preempt_gangs does not), the deleted pods fed back afterwards.  G gangs are G times that.
--reprieve times the reprieve pass (kt_preempt_gangs_reprieve_launch) instead; its output is the record kept as
profiles/preempt_gangs_reprieve_timing.txt:
  counts           the gangs with a positive prefix, masked victims per such gang before and after the walk
  reprieve / plain kt_preempt_gangs_reprieve_launch + kt_preempt_gangs_fetch against kt_preempt_gangs_launch + kt_preempt_gangs_fetch on
                   the same inputs, for all gangs and for the one gang with the most masked victims; the two calls ALTERNATE within
                   the run, so that drift of the machine hits both alike: the difference of the medians is the walk's share
  composed 1 x m   a twin engine, starting from the prefix mask deleted (prefix and mask taken as given): per masked victim, last
                   first, upsert it + kt_reconcile_launch(APPLY) + a dry kt_admit_gangs_launch of the one gang, and kt_delete_pods
                   again where the gang is no longer admitted — the only exact way without the call
Method: warm runs first, then the minimum and the median over --reps of the wall clock around the synchronous calls."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_throttler_amd import engine as E, snapshot as S  # noqa: E402
from preempt_timing import NOW, timed, workload  # noqa: E402


def alternated(call_a, call_b, reps):
    """(min, median) ms of each of two calls, run in turns a, b, a, b, .. after one warm run of each."""
    import time
    call_a(), call_b()
    ms = ([], [])
    for _ in range(reps):
        for which, call in enumerate((call_a, call_b)):
            t0 = time.perf_counter()
            call()
            ms[which].append((time.perf_counter() - t0) * 1e3)
    return tuple((min(x), float(np.median(x))) for x in ms)


def reprieve_mode(a, snap, eng, members, off, cands, n_gangs):
    prefix, mask, blocker = eng.preempt_gangs(members, off, cands, NOW)
    prefix_r, left, blocker_r = eng.preempt_gangs(members, off, cands, NOW, reprieve=True)
    assert np.array_equal(prefix, prefix_r) and np.array_equal(blocker, blocker_r) and (left <= mask).all()
    masked, kept = mask.sum(axis=1), left.sum(axis=1)
    pos = prefix > 0
    if not pos.any():
        print("no gang has a positive prefix: nothing to walk", flush=True)
        return
    print(f"answers over the gangs: positive prefix {int(pos.sum())} of {n_gangs} (longest {int(prefix.max())}); masked victims per such gang: "
          f"mean {masked[pos].mean():.1f}, most {int(masked.max())}; after the walk: mean {kept[pos].mean():.1f}, most {int(kept.max())}", flush=True)
    g = int(np.argmax(masked))  # the gang with the most masked victims: the longest walk
    one, one_off = members[off[g]:off[g + 1]], np.array([0, a.size], np.int64)
    t_all_r, t_all_p = alternated(lambda: eng.preempt_gangs(members, off, cands, NOW, reprieve=True),
                                  lambda: eng.preempt_gangs(members, off, cands, NOW), a.reps)
    t_one_r, t_one_p = alternated(lambda: eng.preempt_gangs(one, one_off, cands, NOW, reprieve=True),
                                  lambda: eng.preempt_gangs(one, one_off, cands, NOW), a.reps)

    twin = E.Engine.for_snapshot(snap)
    victims = cands[mask[g] != 0]

    def admitted():
        twin.reconcile_launch(NOW, apply=True)
        twin.synchronize()
        return bool(twin.admit_gangs(one, one_off, commit=False, want_status=False)[2][0])

    def composed():
        twin.delete_pods(victims)
        out = np.ones(len(victims), bool)
        for j in range(len(victims) - 1, -1, -1):
            twin.upsert_pods(snap.pod_batch(victims[j:j + 1]), rows=victims[j:j + 1])
            if admitted():
                out[j] = False
            else:
                twin.delete_pods(victims[j:j + 1])
        twin.upsert_pods(snap.pod_batch(victims[out]), rows=victims[out])
        return out

    got = composed()
    same = np.array_equal(victims[got], cands[left[g] != 0])
    t_comp = timed(composed, a.reps)
    print(f"reprieve, {n_gangs} gangs of {a.size} x {len(cands)} candidates, launch + fetch: min {t_all_r[0]:.3f} ms, median {t_all_r[1]:.3f} ms",
          flush=True)
    print(f"preempt gangs alone, the same call, alternated: min {t_all_p[0]:.3f} ms, median {t_all_p[1]:.3f} ms -> the walk adds "
          f"{t_all_r[1] - t_all_p[1]:.3f} ms (medians)", flush=True)
    print(f"reprieve, 1 gang of {a.size} x {len(cands)} candidates ({int(masked[g])} masked victims, {int(kept[g])} left), launch + fetch: "
          f"min {t_one_r[0]:.3f} ms, median {t_one_r[1]:.3f} ms", flush=True)
    print(f"preempt gangs alone, the same call, alternated: min {t_one_p[0]:.3f} ms, median {t_one_p[1]:.3f} ms -> the walk adds "
          f"{t_one_r[1] - t_one_p[1]:.3f} ms (medians)", flush=True)
    print(f"composed walk on a twin (per victim: upsert + reconcile(APPLY) + dry admit_gangs, delete again on a fail), 1 gang, "
          f"{len(victims)} victims: min {t_comp[0]:.3f} ms, median {t_comp[1]:.3f} ms (same victims as the kernel: {same})", flush=True)
    print(f"ratio composed / reprieve launch, one gang: {t_comp[1] / t_one_r[1]:.2f}x; composed / the walk's own share: "
          f"{t_comp[1] / max(t_one_r[1] - t_one_p[1], 1e-3):.0f}x; {int(pos.sum())} gangs (composed = the walk above scaled to "
          f"{int(masked.sum())} masked victims in all): {t_comp[1] / max(len(victims), 1) * masked.sum() / t_all_r[1]:.0f}x", flush=True)
    twin.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--throttles", type=int, default=1000)
    ap.add_argument("--dims", type=int, default=8)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--gangs", type=int, default=256)
    ap.add_argument("--size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reprieve", action="store_true")
    a = ap.parse_args()

    snap = workload(a.pods, a.throttles, a.dims)
    eng = E.Engine.for_snapshot(snap)
    eng.reconcile(NOW, apply=True)
    fl = snap.pod_flags[:snap.n_pods]
    counted = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED
    running = np.nonzero((fl & (counted | S.POD_FINISHED)) == counted)[0]
    pending = np.nonzero(((fl & S.POD_VALID) != 0) & ((fl & S.POD_SCHEDULED) == 0))[0]
    cands = running[:a.cands].astype(np.int64)
    n_gangs = min(a.gangs, len(pending) // a.size)
    members = pending[:n_gangs * a.size].astype(np.int64)
    off = np.arange(n_gangs + 1, dtype=np.int64) * a.size
    print(f"library {E.version()}; pods {snap.n_pods}, throttle rows {eng.throttle_rows()}, D {snap.D}, candidates {len(cands)}, "
          f"gangs {n_gangs} of {a.size}, reps {a.reps}", flush=True)
    if a.reprieve:
        reprieve_mode(a, snap, eng, members, off, cands, n_gangs)
        eng.close()
        return
    prefix, _, blocker = eng.preempt_gangs(members, off, cands, NOW)
    single, _ = eng.preempt(members, cands, NOW)
    alone = single.reshape(n_gangs, a.size)
    passable = (alone >= 0).all(axis=1)
    print(f"answers over the gangs: none {(prefix < 0).sum()}, zero {(prefix == 0).sum()}, positive {(prefix > 0).sum()} "
          f"(longest {int(prefix.max())}); above the maximum of the members' own prefixes: {int((passable & (prefix > alone.max(axis=1))).sum())}, "
          f"none although every member has a prefix: {int((passable & (prefix < 0)).sum())}", flush=True)
    g = int(np.argmax(prefix))  # the gang with the longest prefix
    one, one_off = members[off[g]:off[g + 1]], np.array([0, a.size], np.int64)
    want = int(prefix[g])
    t_all = timed(lambda: eng.preempt_gangs(members, off, cands, NOW), a.reps)
    t_one = timed(lambda: eng.preempt_gangs(one, one_off, cands, NOW), a.reps)
    t_single = timed(lambda: eng.preempt(members, cands, NOW), a.reps)

    scratch = E.Engine.for_snapshot(snap)
    restore = snap.pod_batch(cands)

    def passes(k, state):
        """A dry gang admission of the one gang with exactly cands[:k] deleted; state[0] = how many are deleted now."""
        if k > state[0]:
            scratch.delete_pods(cands[state[0]:k])
        elif k < state[0]:
            scratch.upsert_pods(snap.pod_batch(cands[k:state[0]]), rows=cands[k:state[0]])
        state[0] = k
        scratch.reconcile_launch(NOW, apply=True)
        scratch.synchronize()
        return bool(scratch.admit_gangs(one, one_off, commit=False, want_status=False)[2][0])

    def composed():
        state = [0]
        if passes(0, state):
            got = 0
        elif not passes(len(cands), state):
            got = -1
        else:
            lo, hi = 0, len(cands)  # fails at lo, passes at hi
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if passes(mid, state) else (mid, hi)
            got = hi
        scratch.upsert_pods(restore, rows=cands)
        return got

    got = composed()
    t_comp = timed(composed, a.reps)
    print(f"preempt gangs, {n_gangs} gangs of {a.size} x {len(cands)} candidates, launch + fetch: min {t_all[0]:.3f} ms, median {t_all[1]:.3f} ms", flush=True)
    print(f"preempt gangs, 1 gang of {a.size} x {len(cands)} candidates, launch + fetch: min {t_one[0]:.3f} ms, median {t_one[1]:.3f} ms", flush=True)
    print(f"preempt (single pods), the same {len(members)} rows x {len(cands)} candidates, launch + fetch: min {t_single[0]:.3f} ms, "
          f"median {t_single[1]:.3f} ms", flush=True)
    print(f"composed (delete + reconcile(APPLY) + dry admit_gangs per step, bisected), 1 gang: min {t_comp[0]:.3f} ms, median {t_comp[1]:.3f} ms "
          f"(answer {got}, preempt gangs {want})", flush=True)
    t_rec = timed(lambda: eng.reconcile(NOW, apply=False), a.reps)
    print(f"beside it: the engine's own indexed reconcile, dry, launch + fetch: median {t_rec[1]:.3f} ms (the launch aggregates with the DENSE "
          f"scan for exact contributor counts, as kt_preempt_launch does)", flush=True)
    print(f"ratio composed / preempt gangs, one gang: {t_comp[1] / t_one[1]:.2f}x; {n_gangs} gangs (composed = {n_gangs} x one): "
          f"{n_gangs * t_comp[1] / t_all[1]:.0f}x", flush=True)
    eng.close()
    scratch.close()


if __name__ == "__main__":
    main()
