"""The validation pass of kt_upsert_throttles on its own (kt_validate_throttles: no engine, no GPU): every malformed batch of
tests/throttle_batches.py answers its code and text, every valid edge batch answers KT_OK — at 8 and at 16 dimensions, which is
what tests/test_throttle_events_gpu.py feeds live engines afterwards.  tests/cpp/throttle_batch_test.cpp compiles the pass's
translation unit directly and holds it against batches whose offsets point far outside their arrays."""
import os
import subprocess

import numpy as np
import pytest

import throttle_batches as TB
from kube_throttler_amd import engine as E
from kube_throttler_amd import workload as W

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kube_throttler_amd", "host")


@pytest.fixture(scope="module")
def built():
    E.build()
    return E.lib()


@pytest.mark.parametrize("dims", [8, 16])
@pytest.mark.parametrize("name", TB.MALFORMED_NAMES)
def test_a_malformed_batch_is_refused(name, dims, built):
    batch, rows, code, text = TB.malformed(name, D=dims, rows=(5, 1, 3), throttle_capacity=8, namespace_capacity=2)
    rc, msg = E.validate_throttles(batch, dims, 8, 2, rows=rows)
    assert rc == code, (rc, msg)
    assert text in msg, msg


@pytest.mark.parametrize("dims", [2, 8, 16])
@pytest.mark.parametrize("name", TB.VALID_NAMES)
def test_a_valid_edge_batch_passes(name, dims, built):
    batch, rows = TB.valid(name, D=dims)
    assert E.validate_throttles(batch, dims, 8, 2, rows=rows) == (E.KT_OK, "")


def test_rows_default_to_the_batch_index(built):
    """rows == NULL: entry i goes to row i, so a capacity of two refuses the third entry and a capacity of three takes all."""
    b = TB.base_batch(8)
    assert E.validate_throttles(b, 8, 3, 2) == (E.KT_OK, "")
    rc, msg = E.validate_throttles(b, 8, 2, 2)
    assert rc == TB.OUT_OF_RANGE and "throttle row 2" in msg, (rc, msg)
    rc, msg = E.validate_throttles(b, 8, 3, 1)   # throttle 2 lives in namespace 1; the ClusterThrottle's namespace id is not looked at
    assert rc == TB.OUT_OF_RANGE and "throttle 2: namespace id 1" in msg, (rc, msg)


def test_the_text_fits_a_short_buffer(built):
    import ctypes as C
    batch, rows, code, _ = TB.malformed("preq-operator-4")
    st = batch.as_struct()
    for n in (0, 1, 8):
        buf = C.create_string_buffer(b"\xAA" * 16, 16)
        assert built.kt_validate_throttles(C.byref(st), rows.ctypes.data, 8, 8, 2, buf, n) == code
        assert buf.raw[n:] == b"\xAA" * (16 - n) and (n == 0 or b"\0" in buf.raw[:n])
    assert built.kt_validate_throttles(C.byref(st), rows.ctypes.data, 8, 8, 2, None, 0) == code


@pytest.mark.parametrize("kw", [dict(seed=83, n_pods=64, n_thr=96, n_cluster=48), dict(seed=83, n_pods=64, n_thr=96, n_cluster=48, D=16),
                                dict(seed=91, n_pods=64, n_thr=80, n_cluster=30, overrides=1),
                                dict(seed=81, n_pods=64, n_thr=96, n_cluster=48, n_missing_ns=1, n_invalid_pod_sel=1)])
def test_generated_workloads_pass(kw, built):
    """What the generator makes is what the suite feeds: every throttle table of it passes, whole and as one-row batches."""
    snap = W.generate(W.small(**kw))
    assert E.validate_throttles(snap, snap.D, snap.n_thr, snap.n_ns) == (E.KT_OK, "")
    for t in range(0, snap.n_thr, 7):
        assert E.validate_throttles(snap.throttle_batch([t]), snap.D, snap.n_thr, snap.n_ns, rows=np.array([t], np.int32)) == (E.KT_OK, "")


def test_offsets_far_outside_their_arrays():
    subprocess.check_call(["make", "-C", HOST, "throttle_batch_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "throttle_batch_test")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout.splitlines()[-1]
