"""bench.py --dump-outputs: what the last timed step computed, written as float32 / float64 .npy files that two builds can be
compared with.  Driven on CPU with the oracle's results standing in for the engine's (same attribute layout, no GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (bench.py imports torch inside main() only)
from kube_throttler_amd import workload as W  # noqa: E402
from oracle import kt_oracle as O  # noqa: E402

NOW = (1767225600, 0)


def _step_result(seed=5):
    snap = W.generate(W.small(seed=seed, n_pods=3000, n_thr=64, n_cluster=32))
    o = O.Oracle(snap)
    rec = o.reconcile(NOW, nthreads=2)
    snap.apply_status(rec.used, rec.calc, rec.calc_updated, rec.thrl_flag, rec.thrl_has, rec.thrl_pod, rec.error)
    _, summary = o.check(nthreads=2, want_status=False)
    return rec, summary


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_float_lossless_and_repeatable(tmp_path):
    rec, summary = _step_result()
    assert (summary != 0).any() and (rec.used.v != 0).any()
    total = bench.dump_outputs(str(tmp_path / "a"), rec, summary)
    bench.dump_outputs(str(tmp_path / "b"), rec, summary)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert total == sum(x.nbytes for x in a.values()) <= 64 << 20
    assert "pod_rows" not in a and "throttle_rows" not in a
    T = rec.used.n
    # every integer comes back exactly: amounts and counts, bitmask words from their bit planes, the summary from its fields
    assert np.array_equal(a["used_v"].astype(np.int64), rec.used.v[:T])
    assert np.array_equal(a["calc_count"].astype(np.int64), rec.calc.count[:T])
    weights = (1 << np.arange(32, dtype=np.uint64))
    for name, word in (("used_present", rec.used.present), ("thrl_flag", rec.thrl_flag), ("thrl_has", rec.thrl_has)):
        assert a[name].shape == (T, 32)
        assert np.array_equal((a[name].astype(np.uint64) * weights).sum(axis=1), word[:T].astype(np.uint64)), name
    back = (a["summary_verdict"].astype(np.uint64) | a["summary_n_exceeds"].astype(np.uint64) << np.uint64(4)
            | a["summary_n_active"].astype(np.uint64) << np.uint64(24) | a["summary_n_insufficient"].astype(np.uint64) << np.uint64(44))
    assert np.array_equal(back, summary)


def test_a_flipped_low_bit_is_a_whole_unit(tmp_path):
    rec, summary = _step_result()
    bench.dump_outputs(str(tmp_path / "a"), rec, summary)
    rec.thrl_flag[3] ^= 1
    summary = summary.copy()
    summary[7] ^= np.uint64(1)
    bench.dump_outputs(str(tmp_path / "b"), rec, summary)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert np.abs(a["thrl_flag"] - b["thrl_flag"]).max() == 1.0
    assert np.abs(a["summary_verdict"] - b["summary_verdict"]).max() == 1.0


def test_large_outputs_are_a_fixed_sample(tmp_path, monkeypatch):
    rec, summary = _step_result()
    monkeypatch.setattr(bench, "DUMP_MAX_POD_ROWS", 500)
    monkeypatch.setattr(bench, "DUMP_MAX_THROTTLE_ROWS", 20)
    bench.dump_outputs(str(tmp_path / "a"), rec, summary)
    bench.dump_outputs(str(tmp_path / "b"), rec, summary)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert np.array_equal(a["pod_rows"], b["pod_rows"]) and np.array_equal(a["throttle_rows"], b["throttle_rows"])
    rows = a["pod_rows"].astype(np.int64)
    assert len(rows) == 500 and np.all(np.diff(rows) > 0) and rows[-1] < len(summary)
    assert np.array_equal(a["summary_verdict"], (summary[rows] & np.uint64(3)).astype(np.float32))
    t_rows = a["throttle_rows"].astype(np.int64)
    assert a["used_v"].shape == (20, rec.used.D)
    assert np.array_equal(a["used_count"].astype(np.int64), rec.used.count[t_rows])
