"""bench.py end to end on the GPU: a plain run times exactly --steps steps, prints the headline line only, and what
--dump-outputs writes is the oracle's result for the same seeded snapshot (configs[1]: 10k pods x 100 throttles)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_the_requested_steps_and_dumps_the_oracles_result(tmp_path):
    from kube_throttler_amd import snapshot as S, workload as W
    from oracle import kt_oracle as O
    out = tmp_path / "dump"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "pod_throttle_decisions_per_sec" and line["unit"] == "decisions/s" and line["higher_is_better"]
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "int64"
    assert abs(line["ms_per_step"] * 7 - line["timed_region_s"] * 1e3) < 1e-3 * max(1.0, line["timed_region_s"] * 1e3)
    assert not {"roofline", "cpu_baseline", "latency", "extra_configs"} & set(line)

    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    cfg = W.preset(1)
    cfg.pod_begin, cfg.n_pods = 0, cfg.n_pods_total
    snap = W.generate(cfg)
    o = O.Oracle(snap)
    need = S.THR_VALID | S.THR_RESPONSIBLE
    rows = np.nonzero((snap.thr_flags[:snap.n_thr] & need) == need)[0]
    want = o.reconcile((cfg.now_s, 0), rows=rows, nthreads=4)
    n = len(rows)
    assert np.array_equal(d["used_v"][rows], want.used.v[:n].astype(np.float64))
    assert np.array_equal(d["used_count"][rows], want.used.count[:n].astype(np.float64))
    flags = (d["thrl_flag"][rows].astype(np.uint64) * (1 << np.arange(32, dtype=np.uint64))).sum(axis=1)
    assert np.array_equal(flags, want.thrl_flag[:n].astype(np.uint64))
    snap.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
    _, summary = o.check(nthreads=4, want_status=False)
    assert len(d["summary_verdict"]) == snap.n_pods
    assert np.array_equal(d["summary_verdict"], (summary & np.uint64(3)).astype(np.float32))
    assert np.array_equal(d["summary_n_active"], ((summary >> np.uint64(24)) & np.uint64(0xFFFFF)).astype(np.float32))
