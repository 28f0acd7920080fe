"""Throttle batches for the validation pass of kt_upsert_throttles (kube_throttler_amd/csrc/kt_throttle_batch.cpp).

ONE list of named malformed batches, each made from the small valid batch of ``base_batch`` by one mutation, with the code and a
piece of the text the pass answers — one per refusal include/kt_engine.h lists above kt_upsert_throttles — and a few valid edge
batches that must pass.  tests/test_throttle_batch_cpu.py runs every entry through kt_validate_throttles alone (no engine, no GPU);
tests/test_throttle_events_gpu.py feeds the same entries to a live engine, which must refuse them and stay as it was.  No other
malformed batch is fed to an engine anywhere: what the CPU test has not seen refused never reaches a compile or a kernel.

A helper module, not a conftest: it is imported by name."""
import ctypes as C

import numpy as np

from kube_throttler_amd import snapshot as S

INVALID, OUT_OF_RANGE, OVERFLOW = -1, -2, -4   # KT_ERR_INVALID_ARGUMENT, KT_ERR_OUT_OF_RANGE, KT_ERR_OVERFLOW_RISK
BEYOND = (1 << 60) + 1


def base_batch(D=8):
    """Three throttles.  0: a Throttle of namespace 0 with two terms ({k1 In (1, 2)}; {k2 Exists, k3 NotIn (5)}), one override,
    stored status and a reservation.  1: a ClusterThrottle with one term (pods {k1 In (1)}, namespaces {k4 In (7), k6 NotIn (8, 9)}), no override.
    2: a Throttle of namespace 1 with one term ({k5 DoesNotExist}) and one override."""
    b = S.Snapshot(D, 4)
    b.alloc_namespaces(0, 0)
    b.alloc_pods(0, 0, 0)
    b.alloc_throttles(3, 2, 4)
    need = S.THR_VALID | S.THR_RESPONSIBLE
    b.thr_flags[:] = [need, need | S.THR_CLUSTER, need]
    b.thr_ns[:] = [0, 0, 1]
    b.thr_spec.set_row(0, {0: 4000, 1: 1 << 30}, 10)
    b.thr_spec.set_row(1, {0: 8000})
    b.thr_spec.set_row(2, {}, 3)
    b.thr_used.set_row(0, {0: 500}, 2)
    b.thr_calc.set_row(0, {0: 4000, 1: 1 << 30}, 10)
    b.thr_reserved.set_row(0, {0: 100}, 1)
    b.thr_thrl_flag[0], b.thr_thrl_has[0] = 0, 3
    b.thr_ovr_off[:] = [0, 1, 1, 2]
    b.ovr_begin_s[:] = [1767225000, 1767225000]
    b.ovr_end_s[:] = [1767229000, 1767229000]
    b.ovr_thr.set_row(0, {0: 6000})
    b.ovr_thr.set_row(1, {}, 5)
    b.thr_term_off[:] = [0, 2, 3, 4]
    b.preq.add(S.OP_IN, 1, [1, 2])
    b.preq.add(S.OP_EXISTS, 2)
    b.preq.add(S.OP_NOT_IN, 3, [5])
    b.preq.add(S.OP_IN, 1, [1])
    b.preq.add(S.OP_DOES_NOT_EXIST, 5)
    b.nreq.add(S.OP_IN, 4, [7])
    b.nreq.add(S.OP_NOT_IN, 6, [8, 9])
    b.term_preq_off[:] = [0, 1, 3, 4, 5]
    b.term_nreq_off[:] = [0, 0, 0, 2, 2]
    return b


class _NoValues:
    """a requirement pool whose value array is NULL"""

    def __init__(self, reqs):
        self.reqs = reqs

    def __len__(self):
        return len(self.reqs)

    def as_struct(self):
        st = self.reqs.as_struct()
        st.val = C.POINTER(C.c_uint32)()
        return st


def _pool(name, field, i, v):
    def mutate(b, rows, cap):
        pool = getattr(b, name)
        getattr(pool, field)[i] = v
        pool._arrs = None
    return mutate


def _set(field, i, v):
    def mutate(b, rows, cap):
        a = getattr(b, field)
        a[i] = v(cap) if callable(v) else v
    return mutate


def _present(table, i):
    def mutate(b, rows, cap):
        getattr(b, table).present[i] |= np.uint32(1 << b.D)
    return mutate


def _amount(table, i, count=False):
    def mutate(b, rows, cap):
        a = getattr(b, table)
        if count:
            a.count[i], a.has_count[i] = -BEYOND, 1
        else:
            a.v[i, b.D - 1] = BEYOND
            a.present[i] |= np.uint32(1 << (b.D - 1))
    return mutate


def _row(i, v):
    def mutate(b, rows, cap):
        rows[i] = v(cap) if callable(v) else v
    return mutate


def _null_values(name):
    def mutate(b, rows, cap):
        setattr(b, name, _NoValues(getattr(b, name)))
    return mutate


def _or(field, i):
    def mutate(b, rows, cap):
        getattr(b, field)[i] |= np.uint32(1 << b.D)
    return mutate


OTHER_D = "another D"   # (not a mutation of the arrays: the batch is made for another dimension count)

# (name, mutation, code, a piece of the text)
MALFORMED = [
    ("row-outside-capacity-behind-valid-entries", _row(2, lambda cap: cap["thr"]), OUT_OF_RANGE, "throttle row"),
    ("row-negative", _row(0, -1), OUT_OF_RANGE, "throttle row -1"),
    ("namespace-id-at-the-capacity", _set("thr_ns", 2, lambda cap: cap["ns"]), OUT_OF_RANGE, "throttle 2: namespace id"),
    ("another-D", OTHER_D, INVALID, "batch D="),
    ("thr_ovr_off-starts-late", _set("thr_ovr_off", 0, 1), INVALID, "thr_ovr_off[0] = 1"),
    ("thr_ovr_off-decreases", _set("thr_ovr_off", 1, 2), INVALID, "thr_ovr_off[2] = 1"),
    ("thr_term_off-starts-late", _set("thr_term_off", 0, 1), INVALID, "thr_term_off[0] = 1"),
    ("thr_term_off-decreases", _set("thr_term_off", 2, 1), INVALID, "thr_term_off[2] = 1"),
    ("term_preq_off-starts-late", _set("term_preq_off", 0, 1), INVALID, "term_preq_off / term_nreq_off[0] = 1"),
    ("term_preq_off-decreases", _set("term_preq_off", 2, 0), INVALID, "term_preq_off[2] = 0"),
    ("term_preq_off-ends-beyond-the-pool", _set("term_preq_off", 4, 6), OUT_OF_RANGE, "selector terms reference 6 / 2 requirements, pools hold 5 / 2"),
    ("term_nreq_off-starts-late", _set("term_nreq_off", 0, 1), INVALID, "term_preq_off / term_nreq_off[0] = 1"),
    ("term_nreq_off-decreases", _set("term_nreq_off", 4, 0), INVALID, "term_nreq_off[4] = 0"),
    ("term_nreq_off-ends-beyond-the-pool", _set("term_nreq_off", 4, 1 << 31), OUT_OF_RANGE, "selector terms reference 5 / 2147483648 requirements"),
    ("preq.val_off-starts-late", _pool("preq", "val_off", 0, 1), INVALID, "preq.val_off[0] = 1"),
    ("preq.val_off-decreases", _pool("preq", "val_off", 3, 1), INVALID, "preq.val_off[3] = 1"),
    ("nreq.val_off-starts-late", _pool("nreq", "val_off", 0, 1), INVALID, "nreq.val_off[0] = 1"),
    ("nreq.val_off-decreases", _pool("nreq", "val_off", 2, 0), INVALID, "nreq.val_off[2] = 0"),
    ("preq-values-without-an-array", _null_values("preq"), INVALID, "preq.val_off[5] = 4"),
    ("nreq-values-without-an-array", _null_values("nreq"), INVALID, "nreq.val_off[2] = 3"),
    ("preq-operator-4", _pool("preq", "op", 1, 4), INVALID, "preq.op[1] = 4"),
    ("nreq-operator-255", _pool("nreq", "op", 0, 255), INVALID, "nreq.op[0] = 255"),
    ("term-flag-unknown", _set("term_flags", 1, 4), INVALID, "term_flags[1] = 4"),
    ("spec-mask-names-a-dimension-beyond-D", _present("thr_spec", 0), INVALID, "thr_spec.present[0]"),
    ("calc-mask-names-a-dimension-beyond-D", _present("thr_calc", 1), INVALID, "thr_calc.present[1]"),
    ("used-mask-names-a-dimension-beyond-D", _present("thr_used", 2), INVALID, "thr_used.present[2]"),
    ("reserved-mask-names-a-dimension-beyond-D", _present("thr_reserved", 0), INVALID, "thr_reserved.present[0]"),
    ("override-mask-names-a-dimension-beyond-D", _present("ovr_thr", 1), INVALID, "ovr_thr.present[1]"),
    ("throttled-flag-names-a-dimension-beyond-D", _or("thr_thrl_flag", 1), INVALID, "thr_thrl_has | thr_thrl_flag[1]"),
    ("throttled-keys-name-a-dimension-beyond-D", _or("thr_thrl_has", 2), INVALID, "thr_thrl_has | thr_thrl_flag[2]"),
    ("used-beyond-2^60", _amount("thr_used", 1), OVERFLOW, "throttle 1: status.used / reserved beyond 2^60"),
    ("used-count-beyond-2^60", _amount("thr_used", 2, count=True), OVERFLOW, "throttle 2: status.used / reserved beyond 2^60"),
    ("reserved-beyond-2^60", _amount("thr_reserved", 0), OVERFLOW, "throttle 0: status.used / reserved beyond 2^60"),
]
MALFORMED_NAMES = [m[0] for m in MALFORMED]


def malformed(name, D=8, rows=(0, 1, 2), throttle_capacity=8, namespace_capacity=2):
    """The malformed batch ``name`` for an engine of this shape, aimed at these three rows -> (batch, rows int32, code, text)."""
    _, mutate, code, text = MALFORMED[MALFORMED_NAMES.index(name)]
    rows = np.array(rows, dtype=np.int32)
    assert len(rows) == 3 and namespace_capacity >= 2
    if mutate is OTHER_D:
        return base_batch(D - 1 if D == S.KT_MAX_DIMS else D + 1), rows, code, text
    b = base_batch(D)
    mutate(b, rows, {"thr": throttle_capacity, "ns": namespace_capacity})
    return b, rows, code, text


# ---- valid edge batches: (name, batch, rows or None)
def _no_throttles(D):
    b = S.Snapshot(D, 4)
    b.alloc_namespaces(0, 0)
    b.alloc_pods(0, 0, 0)
    b.alloc_throttles(0, 0, 0)
    return b, None


def _no_terms(D):
    b = base_batch(D)
    one = b.throttle_batch([2])
    one.thr_term_off[:] = [0, 0]
    one.preq, one.nreq = S.Reqs(), S.Reqs()
    return one, None


def _no_overrides(D):
    return base_batch(D).throttle_batch([1]), None


def _empty_requirement_ranges(D):
    b = base_batch(D)
    b.term_preq_off[:] = [0, 1, 1, 4, 5]   # the second term of throttle 0 selects with nothing; the pool entries stay
    b.term_nreq_off[:] = [0, 0, 0, 0, 2]
    return b, None


def _one_row_twice(D):
    return base_batch(D), np.array([4, 1, 4], dtype=np.int32)


def _last_dimension_in_every_mask(D):
    b = base_batch(D)
    top = np.uint32(1 << (D - 1))
    for t in ("thr_spec", "thr_calc", "thr_used", "thr_reserved", "ovr_thr"):
        getattr(b, t).present[:] |= top
    b.thr_thrl_flag[:] |= top
    b.thr_thrl_has[:] |= top
    b.thr_used.v[0, D - 1] = -(1 << 60)   # the bound itself is inside
    return b, None


VALID = [("no-throttles", _no_throttles), ("a-throttle-without-terms", _no_terms), ("a-throttle-without-overrides", _no_overrides),
         ("a-term-with-empty-requirement-ranges", _empty_requirement_ranges), ("rows-name-one-row-twice", _one_row_twice),
         ("the-base-batch", lambda D: (base_batch(D), None)), ("the-last-dimension-in-every-mask", _last_dimension_in_every_mask)]
VALID_NAMES = [v[0] for v in VALID]


def valid(name, D=8):
    return VALID[VALID_NAMES.index(name)][1](D)
