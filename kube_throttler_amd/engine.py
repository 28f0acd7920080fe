"""ctypes binding of the C-ABI in include/kt_engine.h (libkt_engine.so, hand-written HIP for gfx950).

There is no CPU fallback: a missing library or a box without a GPU raises :class:`EngineError`.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import snapshot as S

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_CSRC, "libkt_engine.so")
# A/B runs only (a fix shown red on the previous library, green on this one): another build of the SAME C-ABI
if os.environ.get("KT_ENGINE_LIB"):
    LIB_PATH = os.path.abspath(os.environ["KT_ENGINE_LIB"])
_LIB = None

KT_OK = 0
ERR_NAMES = {-1: "KT_ERR_INVALID_ARGUMENT", -2: "KT_ERR_OUT_OF_RANGE", -3: "KT_ERR_DEVICE", -4: "KT_ERR_OVERFLOW_RISK",
             -5: "KT_ERR_NOT_READY", -6: "KT_ERR_NO_DEVICE", -7: "KT_ERR_UNSUPPORTED"}
RECONCILE_APPLY = 0x1
ADMIT_COMMIT = 0x1
GANG_MEMBER_REQUIRED = 0x1
VARIANT_INCREMENTAL = 0x100  # | VARIANT_INDEXED: pod events keep the `used` partials current (N2)
CHECK_STATUS_MATRIX = 0x1
KERNEL_CHECK, KERNEL_AGGREGATE, KERNEL_FINALIZE, KERNEL_PREPARE, KERNEL_REDUCE = 0, 1, 2, 3, 4
VARIANT_INDEXED, VARIANT_DENSE = 0, 1

EXPORTS = [
    "kt_version", "kt_engine_create", "kt_engine_destroy", "kt_last_error", "kt_upsert_namespaces", "kt_upsert_pods",
    "kt_upsert_throttles", "kt_delete_namespaces", "kt_delete_pods", "kt_delete_throttles", "kt_load_snapshot",
    "kt_set_reserved", "kt_set_status", "kt_reconcile_launch", "kt_aggregate_launch", "kt_partial_used_buffer",
    "kt_use_partial_buffer", "kt_finalize_launch", "kt_reconcile_fetch", "kt_check_launch", "kt_check_fetch", "kt_throttle_rows", "kt_sweep_launch",
    "kt_check_device_summary", "kt_fetch_pod_requests", "kt_timing_enable", "kt_timing_read", "kt_timing_reset",
    "kt_synchronize", "kt_kernel_name", "kt_admit_launch", "kt_fetch_reserved", "kt_reconcile_fetch_next_override",
    "kt_check", "kt_upsert_namespace", "kt_upsert_pod", "kt_upsert_throttle", "kt_comm_unique_id", "kt_comm_init",
    "kt_comm_allreduce_partial", "kt_comm_destroy", "kt_reconcile_rows_launch", "kt_set_exchange_world", "kt_counter", "kt_reconcile_fetch_used_hi",
    "kt_set_wide_sums", "kt_partial_words", "kt_partial_layout", "kt_debug_reload_env", "kt_affected_pods", "kt_paged_check", "kt_paged_reconcile",
    "kt_paged_admit", "kt_admit_gangs_launch", "kt_admit_gangs_fetch", "kt_paged_admit_gangs",
    "kt_admit_gangs_elastic_launch", "kt_admit_gangs_elastic_fetch", "kt_paged_admit_gangs_elastic",
    "kt_headroom_launch", "kt_headroom_fetch", "kt_paged_headroom", "kt_preempt_launch", "kt_preempt_fetch",
    "kt_preempt_reprieve_launch", "kt_preempt_gangs_launch", "kt_preempt_gangs_reprieve_launch", "kt_preempt_gangs_fetch", "kt_forecast_launch", "kt_forecast_fetch", "kt_forecast_gangs_launch", "kt_forecast_gangs_fetch", "kt_override_instants",
    "kt_forecast_gangs_elastic_launch", "kt_forecast_gangs_elastic_fetch",
    "kt_preempt_gangs_elastic_launch", "kt_preempt_gangs_elastic_fetch",
    "kt_paged_preempt", "kt_paged_forecast", "kt_debug_match_planes", "kt_debug_match_codes", "kt_debug_match_runs", "kt_paged_preempt_gangs",
    "kt_paged_forecast_gangs", "kt_headroom_gangs_launch", "kt_headroom_gangs_fetch", "kt_paged_headroom_gangs",
    "kt_headroom_forecast_launch", "kt_headroom_forecast_fetch", "kt_paged_headroom_forecast",
    "kt_headroom_forecast_gangs_launch", "kt_headroom_forecast_gangs_fetch", "kt_paged_headroom_forecast_gangs",
    "kt_validate_throttles",
]
HEADROOM_MAX_CAP = 0x7FFFFFFF
PREEMPT_NONE = -1
PREEMPT_REPRIEVE = 0x1
FORECAST_NONE = -1
COUNTER_FEW_CHECKS, COUNTER_COMPILES, COUNTER_INDEX_CHUNKS, COUNTER_INDEX_WORDS, COUNTER_NS_WORD_VISITS, COUNTER_NS_ROWS = range(6)
COUNTER_NS_CHUNK_VISITS, COUNTER_INDEX_IMAGE_WORDS, COUNTER_SLOW_THROTTLES, COUNTER_PACKED_WORDS = 6, 7, 8, 9
COUNTER_AGG_WORKGROUPS = 11
COUNTER_VIEW_BUILDS = 10
COUNTER_MATCH_CACHE_BUILDS, COUNTER_MATCH_CACHE_SCANS, COUNTER_MATCH_CACHE_PLANES = 12, 13, 14
COUNTER_MATCH_CACHE_AGG_SCANS = 15


def partial_layout(n_dims: int) -> dict:
    """kt_partial_layout(): the layout of one throttle's row of the partial-`used` buffer as the library's kernels are
    compiled (no engine, no GPU needed) -> {stride, values, presence, pods, errors} in int64 words."""
    v = [C.c_int32() for _ in range(5)]
    rc = lib().kt_partial_layout(int(n_dims), *[C.byref(x) for x in v])
    if rc != KT_OK:
        raise EngineError(rc, f"kt_partial_layout({n_dims})")
    return dict(zip(("stride", "values", "presence", "pods", "errors"), (int(x.value) for x in v)))


def validate_throttles(batch: S.Snapshot, n_dims: int, throttle_capacity: int, namespace_capacity: int, rows=None):
    """kt_validate_throttles(): the validation pass of kt_upsert_throttles over ``batch`` for an engine of this shape (no engine,
    no GPU needed) -> (code, text): KT_OK and '' or what the feed call would answer and kt_last_error would say."""
    st = batch.as_struct()
    a = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    err = C.create_string_buffer(256)
    rc = lib().kt_validate_throttles(C.byref(st), None if a is None else a.ctypes.data, int(n_dims), int(throttle_capacity),
                                     int(namespace_capacity), err, len(err))
    return rc, err.value.decode()


def version() -> str:
    """kt_version(): library version + hash of the kernel sources it was built from."""
    return lib().kt_version().decode()


def paged_check(engines, n, rows=None, on_equal=False):
    """kt_paged_check: kt_check on every page engine (one per page of <= 16 resource names), combined in the library ->
    (status matrix [n][T], summary words [n])."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    T = engines[0].throttle_rows()
    rows_a = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    if rows_a is None:
        rows_a = np.arange(n, dtype=np.int64)
    status = np.zeros((max(n, 1), max(T, 1)), np.uint8)
    summary = np.zeros(max(n, 1), np.uint64)
    rc = lib().kt_paged_check(hs, len(engines), n, rows_a.ctypes.data, int(on_equal), summary.ctypes.data, status.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_check: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return status[:n, :T], summary[:n]


def paged_admit(engines, rows, on_equal=False, commit=False):
    """kt_paged_admit: the queue ``rows`` admitted in order over the page engines (PreFilter, and Reserve on Success, with
    every page's names) -> (status matrix [n][T] at each pod's turn, summary words [n]), combined over the pages."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    T = engines[0].throttle_rows()
    rows_a = np.ascontiguousarray(rows, dtype=np.int64)
    n = len(rows_a)
    status = np.zeros((max(n, 1), max(T, 1)), np.uint8)
    summary = np.zeros(max(n, 1), np.uint64)
    rc = lib().kt_paged_admit(hs, len(engines), n, rows_a.ctypes.data if n else None, int(on_equal),
                              ADMIT_COMMIT if commit else 0, summary.ctypes.data, status.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_admit: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return status[:n, :T], summary[:n]


def _gang_offsets(gang_off):
    g = np.ascontiguousarray(gang_off, dtype=np.int64)
    if g.ndim != 1 or len(g) < 1:
        raise ValueError("gang_off: [n_gangs + 1] offsets, starting at 0 and ending at the queue length")
    return g


def paged_admit_gangs(engines, rows, gang_off, on_equal=False, commit=False):
    """kt_paged_admit_gangs: the queue ``rows`` in consecutive gangs ``[gang_off[g], gang_off[g + 1])`` admitted all or nothing
    over the page engines -> (status matrix [n][T] and summary words [n] at each pod's turn, admitted byte per gang)."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    T = engines[0].throttle_rows()
    rows_a = np.ascontiguousarray(rows, dtype=np.int64)
    g = _gang_offsets(gang_off)
    n, ng = len(rows_a), len(g) - 1
    status = np.zeros((max(n, 1), max(T, 1)), np.uint8)
    summary = np.zeros(max(n, 1), np.uint64)
    admitted = np.zeros(max(ng, 1), np.uint8)
    rc = lib().kt_paged_admit_gangs(hs, len(engines), n, rows_a.ctypes.data if n else None, ng, g.ctypes.data, int(on_equal),
                                    ADMIT_COMMIT if commit else 0, summary.ctypes.data, status.ctypes.data, admitted.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_admit_gangs: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return status[:n, :T], summary[:n], admitted[:ng]


def _elastic_rule(min_members, required, n, ng):
    """min_members [n_gangs] int64 and the flag bytes [n] (None: no member is required) of an elastic gang call."""
    mm = np.ascontiguousarray(min_members, dtype=np.int64)
    if mm.shape != (ng,):
        raise ValueError(f"min_members: one quorum per gang ({ng}), got shape {mm.shape}")
    if required is None:
        return mm, None
    rq = np.ascontiguousarray(required)
    if rq.shape != (n,):
        raise ValueError(f"required: one entry per queue position ({n}), got shape {rq.shape}")
    if rq.dtype == np.bool_:
        rq = rq.astype(np.uint8) * GANG_MEMBER_REQUIRED
    return mm, np.ascontiguousarray(rq, dtype=np.uint8)


def paged_admit_gangs_elastic(engines, rows, gang_off, min_members, required=None, on_equal=False, commit=False):
    """kt_paged_admit_gangs_elastic: the queue ``rows`` in consecutive gangs, gang g kept once ``min_members[g]`` members and every
    ``required`` one (bool, or flag bytes with GANG_MEMBER_REQUIRED, per queue position) succeeded, over the page engines ->
    (status matrix [n][T] and summary words [n] at each pod's turn, members that stay reserved per gang: 0 rolled back)."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    T = engines[0].throttle_rows()
    rows_a = np.ascontiguousarray(rows, dtype=np.int64)
    g = _gang_offsets(gang_off)
    n, ng = len(rows_a), len(g) - 1
    mm, rq = _elastic_rule(min_members, required, n, ng)
    status = np.zeros((max(n, 1), max(T, 1)), np.uint8)
    summary = np.zeros(max(n, 1), np.uint64)
    members = np.zeros(max(ng, 1), np.int64)
    rc = lib().kt_paged_admit_gangs_elastic(hs, len(engines), n, rows_a.ctypes.data if n else None, ng, g.ctypes.data,
                                            mm.ctypes.data if ng else None, None if rq is None or not n else rq.ctypes.data, int(on_equal),
                                            ADMIT_COMMIT if commit else 0, summary.ctypes.data, status.ctypes.data, members.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_admit_gangs_elastic: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return status[:n, :T], summary[:n], members[:ng]


def paged_headroom(engines, rows, cap, on_equal=False):
    """kt_paged_headroom: how many copies of each pod of ``rows`` the throttles still admit over the page engines — the leading
    Success verdicts of a dry-run admission of ``[pod] * cap`` — -> (copies int64 [n] in [0, cap], limiting throttle row
    int32 [n], -1 when all ``cap`` copies are admitted)."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    rows_a = np.ascontiguousarray(rows, dtype=np.int64)
    n = len(rows_a)
    copies = np.zeros(max(n, 1), np.int64)
    limiting = np.zeros(max(n, 1), np.int32)
    rc = lib().kt_paged_headroom(hs, len(engines), n, rows_a.ctypes.data if n else None, int(on_equal), int(cap),
                                 copies.ctypes.data, limiting.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_headroom: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return copies[:n], limiting[:n]


def paged_headroom_gangs(engines, pod_rows, gang_off, cap, on_equal=False, want_limiting=True, want_blocker=True):
    """kt_paged_headroom_gangs: kt_headroom_gangs_launch + kt_headroom_gangs_fetch over the page engines, on the cluster of all
    resource names -> (copies int64 [n_gangs] in [0, cap], limiting throttle row int32 [n_gangs] or None, blocker int64 [n_gangs]
    or None).  Per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` the number of leading admitted gangs of a dry paged gang
    admission of ``members * cap``; the queue position of the first member of the first copy that is not admitted whose
    combined verdict is not Success, and the lowest throttle row that stops it there (both -1 when all ``cap`` copies are
    admitted; limiting -1 when the blocker's verdict is an Error)."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    a = np.ascontiguousarray(pod_rows, dtype=np.int64)
    g = _gang_offsets(gang_off)
    n, ng = len(a), len(g) - 1
    copies = np.zeros(max(ng, 1), np.int64)
    limiting = np.zeros(max(ng, 1), np.int32) if want_limiting else None
    blocker = np.zeros(max(ng, 1), np.int64) if want_blocker else None
    rc = lib().kt_paged_headroom_gangs(hs, len(engines), n, a.ctypes.data if n else None, ng, g.ctypes.data, int(on_equal), int(cap),
                                       copies.ctypes.data, None if limiting is None else limiting.ctypes.data,
                                       None if blocker is None else blocker.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_headroom_gangs: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return copies[:ng], (None if limiting is None else limiting[:ng]), (None if blocker is None else blocker[:ng])


def paged_preempt(engines, pod_rows, cand_rows, now, on_equal=False, reprieve=False, want_victims=True):
    """kt_paged_preempt: kt_preempt_launch (``reprieve``: kt_preempt_reprieve_launch) over the page engines, on the cluster of all
    resource names -> (prefix int64 [n], victims uint8 [n][n_cand] or None).  prefix: the smallest k for which the pod passes
    PreFilter once the candidates ``cand_rows[:k]`` are gone and every responsible throttle has been reconciled at ``now`` on
    every page; 0: it already passes; PREEMPT_NONE: no prefix helps.  A throttle reads its calculated threshold on every page
    when any page's reconcile replaces it (or any page has it stored), and keeps its stored status on every page when its
    reconcile is an error on any page."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    a = np.ascontiguousarray(pod_rows, dtype=np.int64)
    c = np.ascontiguousarray(cand_rows, dtype=np.int64)
    n, m = len(a), len(c)
    prefix = np.zeros(max(n, 1), np.int64)
    flat = np.zeros(max(n * m, 1), np.uint8) if want_victims else None
    rc = lib().kt_paged_preempt(hs, len(engines), n, a.ctypes.data if n else None, m, c.ctypes.data if m else None, int(now[0]), int(now[1]),
                                int(on_equal), PREEMPT_REPRIEVE if reprieve else 0, prefix.ctypes.data,
                                None if flat is None else flat.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_preempt: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return prefix[:n], (None if flat is None else flat[:n * m].reshape(n, m))


def paged_preempt_gangs(engines, pod_rows, gang_off, cand_rows, now, on_equal=False, reprieve=False, want_victims=True):
    """kt_paged_preempt_gangs: kt_preempt_gangs_launch (``reprieve``: kt_preempt_gangs_reprieve_launch) over the page engines, on the
    cluster of all resource names -> (prefix int64 [n_gangs], victims uint8 [n_gangs][n_cand] or None, blocker int64 [n_gangs]).
    Per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` the smallest k for which an in-order admission — PreFilter, and on Success
    Reserve on every page — admits every member once the candidates ``cand_rows[:k]`` are gone and every responsible throttle has
    been reconciled at ``now`` on every page; 0: the gang already passes; PREEMPT_NONE: no prefix helps.  blocker: the queue
    position of the first member that is not Success with nothing deleted, over every page (-1 when prefix == 0)."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    a = np.ascontiguousarray(pod_rows, dtype=np.int64)
    c = np.ascontiguousarray(cand_rows, dtype=np.int64)
    g = _gang_offsets(gang_off)
    n, m, ng = len(a), len(c), len(g) - 1
    prefix = np.zeros(max(ng, 1), np.int64)
    blocker = np.zeros(max(ng, 1), np.int64)
    flat = np.zeros(max(ng * m, 1), np.uint8) if want_victims else None
    rc = lib().kt_paged_preempt_gangs(hs, len(engines), n, a.ctypes.data if n else None, ng, g.ctypes.data, m, c.ctypes.data if m else None,
                                      int(now[0]), int(now[1]), int(on_equal), PREEMPT_REPRIEVE if reprieve else 0, prefix.ctypes.data,
                                      None if flat is None else flat.ctypes.data, blocker.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_preempt_gangs: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return prefix[:ng], (None if flat is None else flat[:ng * m].reshape(ng, m)), blocker[:ng]


def paged_forecast(engines, pod_rows, instants, on_equal=False, want_verdicts=True):
    """kt_paged_forecast: kt_forecast_launch + kt_forecast_fetch over the page engines, on the cluster of all resource names ->
    (first int64 [n], verdicts uint8 [n][n_inst] or None).  Per pod the KT_VERDICT_* of PreFilter once every valid and responsible
    throttle has been reconciled at each of the strictly ascending ``instants`` on every page, and the first position whose
    verdict is Success (FORECAST_NONE: none).  At each instant a throttle reads its calculated threshold on every page when any
    page's reconcile replaces it (or any page has it stored), and keeps its stored status on every page when its reconcile is an
    error on any page."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    a = np.ascontiguousarray(pod_rows, dtype=np.int64)
    inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
    inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
    n, m = len(a), len(inst_s)
    first = np.zeros(max(n, 1), np.int64)
    flat = np.zeros(max(n * m, 1), np.uint8) if want_verdicts else None
    rc = lib().kt_paged_forecast(hs, len(engines), n, a.ctypes.data if n else None, m, inst_s.ctypes.data if m else None,
                                 inst_ns.ctypes.data if m else None, int(on_equal), first.ctypes.data,
                                 None if flat is None else flat.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_forecast: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return first[:n], (None if flat is None else flat[:n * m].reshape(n, m))


def paged_forecast_gangs(engines, pod_rows, gang_off, instants, on_equal=False, want_verdicts=True, want_blocker=True):
    """kt_paged_forecast_gangs: kt_forecast_gangs_launch + kt_forecast_gangs_fetch over the page engines, on the cluster of all
    resource names -> (first int64 [n_gangs], verdicts uint8 [n_gangs][n_inst] or None, blocker int64 [n_gangs][n_inst] or None).
    Per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` and per instant the KT_VERDICT_* of an in-order admission of its members —
    PreFilter, and on Success Reserve on every page — once every valid and responsible throttle has been reconciled at that
    instant on every page, the first position whose verdict is Success (FORECAST_NONE: none), and per instant the queue position
    of the first member that is not admitted, over every page (-1 where the gang passes).  At each instant a throttle reads its
    calculated threshold on every page when any page's reconcile replaces it (or any page has it stored), and keeps its stored
    status on every page when its reconcile is an error on any page."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    a = np.ascontiguousarray(pod_rows, dtype=np.int64)
    g = _gang_offsets(gang_off)
    inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
    inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
    n, m, ng = len(a), len(inst_s), len(g) - 1
    first = np.zeros(max(ng, 1), np.int64)
    flat = np.zeros(max(ng * m, 1), np.uint8) if want_verdicts else None
    blk = np.zeros(max(ng * m, 1), np.int64) if want_blocker else None
    rc = lib().kt_paged_forecast_gangs(hs, len(engines), n, a.ctypes.data if n else None, ng, g.ctypes.data, m,
                                       inst_s.ctypes.data if m else None, inst_ns.ctypes.data if m else None, int(on_equal),
                                       first.ctypes.data, None if flat is None else flat.ctypes.data,
                                       None if blk is None else blk.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_forecast_gangs: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return (first[:ng], (None if flat is None else flat[:ng * m].reshape(ng, m)),
            (None if blk is None else blk[:ng * m].reshape(ng, m)))


def paged_headroom_forecast(engines, pod_rows, instants, *, cap, want=1, on_equal=False, want_copies=True, want_limiting=True):
    """kt_paged_headroom_forecast: kt_headroom_forecast_launch + kt_headroom_forecast_fetch over the page engines, on the cluster
    of all resource names -> (first int64 [n], copies int64 [n][n_inst] or None, limiting int32 [n][n_inst] or None).  Per pod and
    per instant the number of leading Success verdicts a dry-run paged admission of ``cap`` copies of the pod returns once every
    valid and responsible throttle has been reconciled at that instant on every page, the lowest throttle row that stops the next
    copy (-1: all ``cap`` are admitted), and the first position with at least ``want`` copies (FORECAST_NONE: none).  At each
    instant a throttle reads its calculated threshold on every page when any page's reconcile replaces it (or any page has it
    stored), and keeps its stored status on every page when its reconcile is an error on any page."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    a = np.ascontiguousarray(pod_rows, dtype=np.int64)
    inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
    inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
    n, m = len(a), len(inst_s)
    first = np.zeros(max(n, 1), np.int64)
    copies = np.zeros(max(n * m, 1), np.int64) if want_copies else None
    limiting = np.zeros(max(n * m, 1), np.int32) if want_limiting else None
    rc = lib().kt_paged_headroom_forecast(hs, len(engines), n, a.ctypes.data if n else None, m, inst_s.ctypes.data if m else None,
                                          inst_ns.ctypes.data if m else None, int(on_equal), int(cap), int(want), first.ctypes.data,
                                          None if copies is None else copies.ctypes.data,
                                          None if limiting is None else limiting.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_headroom_forecast: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return (first[:n], (None if copies is None else copies[:n * m].reshape(n, m)),
            (None if limiting is None else limiting[:n * m].reshape(n, m)))


def paged_headroom_forecast_gangs(engines, pod_rows, gang_off, instants, *, cap, want=1, on_equal=False, want_copies=True,
                                  want_limiting=True, want_blocker=True):
    """kt_paged_headroom_forecast_gangs: kt_headroom_forecast_gangs_launch + kt_headroom_forecast_gangs_fetch over the page engines,
    on the cluster of all resource names -> (first int64 [n_gangs], copies int64 [n_gangs][n_inst] or None, limiting int32
    [n_gangs][n_inst] or None, blocker int64 [n_gangs][n_inst] or None).  Per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` and per
    instant the number of leading admitted gangs a dry-run paged gang admission of ``cap`` consecutive copies returns once every
    valid and responsible throttle has been reconciled at that instant on every page, the queue position of the first member of
    the first refused copy that is not admitted and the lowest throttle row that stops it (-1 / -1: all ``cap`` copies are
    admitted), and the first position with at least ``want`` copies (FORECAST_NONE: none).  At each instant a throttle reads its
    calculated threshold on every page when any page's reconcile replaces it (or any page has it stored), and keeps its stored
    status on every page when its reconcile is an error on any page."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    a = np.ascontiguousarray(pod_rows, dtype=np.int64)
    g = _gang_offsets(gang_off)
    inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
    inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
    n, m, ng = len(a), len(inst_s), len(g) - 1
    first = np.zeros(max(ng, 1), np.int64)
    copies = np.zeros(max(ng * m, 1), np.int64) if want_copies else None
    limiting = np.zeros(max(ng * m, 1), np.int32) if want_limiting else None
    blk = np.zeros(max(ng * m, 1), np.int64) if want_blocker else None
    rc = lib().kt_paged_headroom_forecast_gangs(hs, len(engines), n, a.ctypes.data if n else None, ng, g.ctypes.data, m,
                                                inst_s.ctypes.data if m else None, inst_ns.ctypes.data if m else None, int(on_equal),
                                                int(cap), int(want), first.ctypes.data, None if copies is None else copies.ctypes.data,
                                                None if limiting is None else limiting.ctypes.data,
                                                None if blk is None else blk.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_headroom_forecast_gangs: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return (first[:ng], (None if copies is None else copies[:ng * m].reshape(ng, m)),
            (None if limiting is None else limiting[:ng * m].reshape(ng, m)), (None if blk is None else blk[:ng * m].reshape(ng, m)))


def paged_reconcile(engines, now, apply=True):
    """kt_paged_reconcile: a reconcile on every page engine -> (per-page ReconcileResult list, replaced_any [T], error_any [T])."""
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    T = engines[0].throttle_rows()
    results = [ReconcileResult(T, e.D) for e in engines]
    structs = (KtStatus * len(engines))(*[r.as_struct() for r in results])
    replaced, err = np.zeros(max(T, 1), np.uint8), np.zeros(max(T, 1), np.uint8)
    rc = lib().kt_paged_reconcile(hs, len(engines), int(now[0]), int(now[1]), RECONCILE_APPLY if apply else 0, T, structs,
                                  replaced.ctypes.data, err.ctypes.data)
    if rc != KT_OK:
        raise EngineError(rc, "kt_paged_reconcile: " + "; ".join(lib().kt_last_error(e._h).decode() for e in engines))
    return results, replaced[:T], err[:T]


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class KtConfig(C.Structure):
    _fields_ = [("n_dims", C.c_int32), ("max_labels", C.c_int32), ("pod_capacity", C.c_int64),
                ("throttle_capacity", C.c_int32), ("namespace_capacity", C.c_int32), ("device", C.c_int32),
                ("kernel_variant", C.c_int32)]


class KtStatus(C.Structure):
    _fields_ = [("used", S.KtAmounts), ("calc", S.KtAmounts), ("calc_at_nonzero", C.POINTER(C.c_uint8)),
                ("thrl_flag", C.POINTER(C.c_uint32)), ("thrl_has", C.POINTER(C.c_uint32)),
                ("thrl_pod", C.POINTER(C.c_uint8)), ("msgs_fp", C.POINTER(C.c_uint64)),
                ("error", C.POINTER(C.c_uint8))]


def build(force: bool = False) -> str:
    """Compile libkt_engine.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(-6, f"{LIB_PATH} is missing: build it with kube_throttler_amd.engine.build() "
                                  "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.kt_version.restype = C.c_char_p
        L.kt_last_error.restype = C.c_char_p
        L.kt_last_error.argtypes = [C.c_void_p]
        L.kt_kernel_name.restype = C.c_char_p
        L.kt_kernel_name.argtypes = [C.c_void_p, C.c_int32]
        L.kt_engine_create.argtypes = [C.POINTER(KtConfig), C.POINTER(C.c_void_p)]
        L.kt_engine_destroy.argtypes = [C.c_void_p]
        for name in ("kt_upsert_namespaces", "kt_upsert_pods", "kt_upsert_throttles"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(S.KtSnapshot), C.c_void_p]
        L.kt_delete_namespaces.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.kt_upsert_namespace.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.kt_delete_pods.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.kt_delete_throttles.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.kt_load_snapshot.argtypes = [C.c_void_p, C.POINTER(S.KtSnapshot)]
        if hasattr(L, "kt_validate_throttles"):  # (KT_ENGINE_LIB may name an older build)
            L.kt_validate_throttles.argtypes = [C.POINTER(S.KtSnapshot), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int32]
        L.kt_set_reserved.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(S.KtAmounts)]
        L.kt_set_status.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(KtStatus)]
        L.kt_reconcile_launch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_void_p]
        L.kt_reconcile_rows_launch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
        L.kt_aggregate_launch.argtypes = [C.c_void_p, C.c_void_p]
        L.kt_partial_used_buffer.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.kt_use_partial_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.kt_finalize_launch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_void_p]
        L.kt_reconcile_fetch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(KtStatus)]
        L.kt_check_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.kt_sweep_launch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p]
        L.kt_check_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.kt_check.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.kt_comm_unique_id.argtypes = [C.c_void_p]
        L.kt_comm_init.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.kt_comm_allreduce_partial.argtypes = [C.c_void_p, C.c_void_p]
        L.kt_comm_destroy.argtypes = [C.c_void_p]
        L.kt_set_exchange_world.argtypes = [C.c_void_p, C.c_int32]
        L.kt_set_wide_sums.argtypes = [C.c_void_p, C.c_int32]
        L.kt_partial_words.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.kt_partial_layout.argtypes = [C.c_int32] + [C.POINTER(C.c_int32)] * 5
        L.kt_debug_reload_env.argtypes = [C.c_void_p]
        L.kt_debug_match_planes.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        if hasattr(L, "kt_debug_match_codes"):  # (KT_ENGINE_LIB may name an older build: the A/B runs of tools/gpu_ab.sh)
            L.kt_debug_match_runs.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            L.kt_debug_match_codes.argtypes =[C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.kt_affected_pods.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.kt_paged_check.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.kt_paged_reconcile.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_uint32, C.c_int32,
                                         C.POINTER(KtStatus), C.c_void_p, C.c_void_p]
        L.kt_paged_admit.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p,
                                     C.c_void_p]
        L.kt_counter.argtypes = [C.c_void_p, C.c_int32]
        L.kt_reconcile_fetch_used_hi.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
        L.kt_counter.restype = C.c_int64
        L.kt_throttle_rows.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.kt_check_device_summary.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.kt_fetch_pod_requests.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_timing_enable.argtypes = [C.c_void_p, C.c_int32]
        L.kt_timing_read.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.kt_timing_reset.argtypes = [C.c_void_p]
        L.kt_synchronize.argtypes = [C.c_void_p, C.c_void_p]
        L.kt_reconcile_fetch_next_override.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_admit_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.kt_fetch_reserved.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(S.KtAmounts)]
        L.kt_admit_gangs_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
        L.kt_admit_gangs_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.kt_admit_gangs_elastic_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                    C.c_uint32, C.c_void_p]
        L.kt_admit_gangs_elastic_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.kt_paged_admit_gangs_elastic.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_paged_admit_gangs.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_headroom_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
        L.kt_headroom_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.kt_headroom_gangs_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
        L.kt_headroom_gangs_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_paged_headroom.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                        C.c_void_p]
        L.kt_paged_headroom_gangs.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_paged_preempt.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.kt_paged_preempt_gangs.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                             C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_preempt_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_void_p]
        L.kt_preempt_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.kt_preempt_reprieve_launch.argtypes = L.kt_preempt_launch.argtypes
        L.kt_preempt_gangs_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                              C.c_int32, C.c_int32, C.c_void_p]
        L.kt_preempt_gangs_reprieve_launch.argtypes = L.kt_preempt_gangs_launch.argtypes
        L.kt_preempt_gangs_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_preempt_gangs_elastic_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p]
        L.kt_preempt_gangs_elastic_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_paged_forecast.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p]
        L.kt_paged_forecast_gangs.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_paged_headroom_forecast.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_paged_headroom_forecast_gangs.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_forecast_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.kt_forecast_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.kt_headroom_forecast_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                                  C.c_int64, C.c_void_p]
        L.kt_headroom_forecast_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_forecast_gangs_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_int32, C.c_void_p]
        L.kt_forecast_gangs_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_forecast_gangs_elastic_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.kt_forecast_gangs_elastic_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_headroom_forecast_gangs_launch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                        C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
        L.kt_headroom_forecast_gangs_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kt_override_instants.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int64)]
        _LIB = L
    return _LIB


class ReconcileResult:
    """Rows [0, n) of a reconcile pass; attribute names as in the oracle's result."""

    def __init__(self, n, D):
        self.used, self.calc = S.Amounts(n, D), S.Amounts(n, D)
        m = max(n, 1)
        self.calc_updated = np.zeros(m, np.uint8)
        self.thrl_flag = np.zeros(m, np.uint32)
        self.thrl_has = np.zeros(m, np.uint32)
        self.thrl_pod = np.zeros(m, np.uint8)
        self.error = np.zeros(m, np.uint8)

    def as_struct(self) -> KtStatus:
        p8, p32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        return KtStatus(self.used.as_struct(), self.calc.as_struct(), self.calc_updated.ctypes.data_as(p8),
                        self.thrl_flag.ctypes.data_as(p32), self.thrl_has.ctypes.data_as(p32),
                        self.thrl_pod.ctypes.data_as(p8), None, self.error.ctypes.data_as(p8))


class Engine:
    """One engine = one GPU's worth of pod rows plus the (replicated) throttle tables."""

    def __init__(self, n_dims, max_labels, pod_capacity, throttle_capacity, namespace_capacity, device=-1,
                 kernel_variant=VARIANT_INDEXED):
        self._h = C.c_void_p()
        self.D = n_dims
        cfg = KtConfig(n_dims, max_labels, pod_capacity, throttle_capacity, namespace_capacity, device, kernel_variant)
        rc = lib().kt_engine_create(C.byref(cfg), C.byref(self._h))
        if rc != KT_OK:
            raise EngineError(rc, lib().kt_last_error(None).decode())

    @classmethod
    def for_snapshot(cls, snap: S.Snapshot, kernel_variant=VARIANT_INDEXED, device=-1, pod_capacity=None):
        e = cls(snap.D, max(snap.L, 1), pod_capacity or max(snap.n_pods, 1), max(snap.n_thr, 1), max(snap.n_ns, 1),
                device, kernel_variant)
        e.load_snapshot(snap)
        return e

    def close(self):
        if self._h:
            lib().kt_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != KT_OK:
            raise EngineError(rc, lib().kt_last_error(self._h).decode())

    # ---- state feed
    def load_snapshot(self, snap: S.Snapshot):
        st = snap.as_struct()
        self._ck(lib().kt_load_snapshot(self._h, C.byref(st)))

    @staticmethod
    def _rows(rows, dtype):
        if rows is None:
            return None, None
        a = np.ascontiguousarray(rows, dtype=dtype)
        return a, a.ctypes.data

    def upsert_namespaces(self, batch: S.Snapshot, rows=None):
        st = batch.as_struct()
        a, p = self._rows(rows, np.int32)
        self._ck(lib().kt_upsert_namespaces(self._h, C.byref(st), p))

    def upsert_namespace(self, row, exists, label_keys=(), label_pairs=()):
        """kt_upsert_namespace: one Namespace event through the flat form (what the plugin mirror calls)."""
        keys = np.ascontiguousarray(label_keys, dtype=np.uint32)
        pairs = np.ascontiguousarray(label_pairs, dtype=np.uint32)
        self._ck(lib().kt_upsert_namespace(self._h, int(row), 1 if exists else 0, len(keys), keys.ctypes.data, pairs.ctypes.data))

    def upsert_pods(self, batch: S.Snapshot, rows=None):
        st = batch.as_struct()
        a, p = self._rows(rows, np.int64)
        self._ck(lib().kt_upsert_pods(self._h, C.byref(st), p))

    def upsert_throttles(self, batch: S.Snapshot, rows=None):
        st = batch.as_struct()
        a, p = self._rows(rows, np.int32)
        self._ck(lib().kt_upsert_throttles(self._h, C.byref(st), p))

    def delete_pods(self, rows):
        a, p = self._rows(rows, np.int64)
        self._ck(lib().kt_delete_pods(self._h, len(a), p))

    def delete_throttles(self, rows):
        a, p = self._rows(rows, np.int32)
        self._ck(lib().kt_delete_throttles(self._h, len(a), p))

    def delete_namespaces(self, rows):
        a, p = self._rows(rows, np.int32)
        self._ck(lib().kt_delete_namespaces(self._h, len(a), p))

    def set_reserved(self, rows, amounts: S.Amounts):
        a, p = self._rows(rows, np.int32)
        st = amounts.as_struct()
        self._ck(lib().kt_set_reserved(self._h, len(a), p, C.byref(st)))

    def set_status(self, rows, used: S.Amounts, calc: S.Amounts, calc_at_nonzero, thrl_flag, thrl_has, thrl_pod,
                   msgs_fp=None):
        a, p = self._rows(rows, np.int32)
        n = len(a)
        keep = [np.ascontiguousarray(calc_at_nonzero, np.uint8), np.ascontiguousarray(thrl_flag, np.uint32),
                np.ascontiguousarray(thrl_has, np.uint32), np.ascontiguousarray(thrl_pod, np.uint8),
                np.ascontiguousarray(msgs_fp if msgs_fp is not None else np.zeros(n), np.uint64)]
        st = KtStatus(used.as_struct(), calc.as_struct(), keep[0].ctypes.data_as(C.POINTER(C.c_uint8)),
                      keep[1].ctypes.data_as(C.POINTER(C.c_uint32)), keep[2].ctypes.data_as(C.POINTER(C.c_uint32)),
                      keep[3].ctypes.data_as(C.POINTER(C.c_uint8)), keep[4].ctypes.data_as(C.POINTER(C.c_uint64)), None)
        self._ck(lib().kt_set_status(self._h, n, p, C.byref(st)))

    # ---- reconcile
    def reconcile_launch(self, now, apply=True, stream=None):
        self._ck(lib().kt_reconcile_launch(self._h, int(now[0]), int(now[1]), RECONCILE_APPLY if apply else 0, stream))

    def reconcile_rows(self, now, rows, apply=True) -> "ReconcileResult":
        """Reconcile of the listed throttle rows only (one workqueue key each, throttle_controller.go:84-133)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._ck(lib().kt_reconcile_rows_launch(self._h, int(now[0]), int(now[1]), RECONCILE_APPLY if apply else 0,
                                                len(rows), rows.ctypes.data_as(C.c_void_p), None))
        return self.reconcile_fetch()

    def aggregate_launch(self, stream=None):
        self._ck(lib().kt_aggregate_launch(self._h, stream))

    def partial_used_buffer(self):
        ptr, n = C.c_void_p(), C.c_int64()
        self._ck(lib().kt_partial_used_buffer(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def use_partial_buffer(self, device_ptr, n_int64):
        self._ck(lib().kt_use_partial_buffer(self._h, device_ptr, n_int64))

    # ---- native RCCL exchange of the partials (kt_comm_*): multi-GPU without a framework in the process
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = lib().kt_comm_unique_id(buf)
        if rc != 0:
            raise EngineError(rc, lib().kt_last_error(None).decode())
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        self._ck(lib().kt_comm_init(self._h, rank, world, C.create_string_buffer(unique_id, 128)))

    def comm_allreduce_partial(self, stream=None):
        self._ck(lib().kt_comm_allreduce_partial(self._h, stream))

    def comm_destroy(self):
        self._ck(lib().kt_comm_destroy(self._h))

    def reconcile_fetch_used_hi(self, n=None):
        """High 64 bits of the last reconcile's `used` values -> (int64 [n][D], any value beyond int64?)."""
        n = self.throttle_rows() if n is None else n
        hi = np.zeros((max(n, 1), self.D), np.int64)
        anyw = C.c_int32()
        self._ck(lib().kt_reconcile_fetch_used_hi(self._h, n, hi.ctypes.data_as(C.c_void_p), C.byref(anyw)))
        return hi[:n], bool(anyw.value)

    def few_checks_served(self) -> int:
        """kt_check calls that took the few-pod path (kt_kernels_few.hip) so far."""
        return int(lib().kt_counter(self._h, 0))

    def compiles(self) -> int:
        """Selector program compiles + index builds so far (Throttle events that leave the selectors alone do not count)."""
        return int(lib().kt_counter(self._h, 1))

    def set_exchange_world(self, world: int):
        """Ranks whose partials the CALLER sums with its own collective (kt_comm_init declares it by itself)."""
        self._ck(lib().kt_set_exchange_world(self._h, world))

    def affected_pods(self, pod_rows, throttle_rows):
        """kt_affected_pods: [n][m] — 1 where the throttle's selector matches the pod as held now (affectedPods restricted to
        the named pods), 0 where not, 255 for a pod whose PreFilter is an error."""
        pr = np.ascontiguousarray(pod_rows, dtype=np.int64)
        tr = np.ascontiguousarray(throttle_rows, dtype=np.int32)
        out = np.zeros((max(len(pr), 1), max(len(tr), 1)), np.uint8)
        self._ck(lib().kt_affected_pods(self._h, len(pr), pr.ctypes.data, len(tr), tr.ctypes.data, out.ctypes.data))
        return out[:len(pr), :len(tr)]

    def reload_env(self):
        """kt_debug_reload_env: re-read the A/B switches (KT_NO_* environment variables) — they are read once, at creation."""
        self._ck(lib().kt_debug_reload_env(self._h))

    def match_planes(self, view=False):
        """kt_debug_match_planes: (words[planes, n], rows) — the match cache's table (view=False: n pod rows, rows = None) or the
        planes of the countable scan view (view=True: n records and the pod row of each).  EngineError (not ready) where there
        is nothing current to copy."""
        n, planes = C.c_int64(), C.c_int32()
        self._ck(lib().kt_debug_match_planes(self._h, int(view), 0, None, None, C.byref(n), C.byref(planes)))
        cap = max(int(n.value), 1)
        out = np.zeros((int(planes.value), cap), dtype=np.uint64)
        rows = np.zeros(cap, dtype=np.int64)
        self._ck(lib().kt_debug_match_planes(self._h, int(view), cap, out.ctypes.data, rows.ctypes.data if view else None, C.byref(n), C.byref(planes)))
        return out[:, :int(n.value)], (rows[:int(n.value)] if view else None)

    def match_codes(self, view=False):
        """kt_debug_match_codes: (records[n, 16] as bytes, rows) — the match-code record of every pod row (byte 0: the count 0..15
        or 0xFF for "read the planes"; bytes 1..15: codes k << 6 | bit, ascending), or (view=True) of every record of the countable
        scan view, with the pod row of each.  EngineError (not ready) where there is nothing current to copy."""
        n = C.c_int64()
        self._ck(lib().kt_debug_match_codes(self._h, int(view), 0, None, None, C.byref(n)))
        cap = max(int(n.value), 1)
        out = np.zeros((cap, 16), dtype=np.uint8)
        rows = np.zeros(cap, dtype=np.int64)
        self._ck(lib().kt_debug_match_codes(self._h, int(view), cap, out.ctypes.data, rows.ctypes.data if view else None, C.byref(n)))
        return out[:int(n.value)], (rows[:int(n.value)] if view else None)

    def match_runs(self, ns_row, k):
        """kt_debug_match_runs: (word, seg_lo, seg_hi) of plane k for the pods of namespace row ns_row (word -1: the list is shorter)."""
        w, lo, hi = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._ck(lib().kt_debug_match_runs(self._h, int(ns_row), int(k), C.byref(w), C.byref(lo), C.byref(hi)))
        return int(w.value), int(lo.value), int(hi.value)

    def index_stats(self) -> dict:
        """The compiled selector index (after the first launch): LDS-sized chunks, 64-bit words of term numbers, namespace rows,
        and the words a pod visits on average over the namespace rows in use."""
        ch, words, visits, rows, cvis, iw, slow = (int(lib().kt_counter(self._h, k)) for k in (
            COUNTER_INDEX_CHUNKS, COUNTER_INDEX_WORDS, COUNTER_NS_WORD_VISITS, COUNTER_NS_ROWS, COUNTER_NS_CHUNK_VISITS, COUNTER_INDEX_IMAGE_WORDS,
            COUNTER_SLOW_THROTTLES))
        return {"chunks": ch, "words": words, "image_words": iw, "namespace_rows": rows,
                "word_visits_per_namespace": round(visits / rows, 3) if rows > 0 else None,
                "chunks_per_namespace": round(cvis / rows, 3) if rows > 0 else None, "slow_throttles": slow}

    def packed_words(self) -> int:
        """64-bit words per pod of the packed fold the last full aggregate scan ran with (0: the plain fold)."""
        return int(lib().kt_counter(self._h, COUNTER_PACKED_WORDS))

    def aggregate_workgroups(self) -> int:
        """Workgroups of the last full aggregate scan's launch (more than 256: the two-per-CU form ran)."""
        return int(lib().kt_counter(self._h, COUNTER_AGG_WORKGROUPS))

    def view_builds(self) -> int:
        """Scan view builds so far (either view); pod events that fit the views are patched in and do not count."""
        return int(lib().kt_counter(self._h, COUNTER_VIEW_BUILDS))

    def match_cache_builds(self) -> int:
        """Full builds of the match cache so far (one per compile / table clear; pod events refresh their rows and do not count)."""
        return int(lib().kt_counter(self._h, COUNTER_MATCH_CACHE_BUILDS))

    def match_cache_planes(self) -> int:
        """The longest namespace word list of the compiled single-chunk program as the last sweep of every row counted it (0: not
        counted); programs with more than four are not cached."""
        return int(lib().kt_counter(self._h, COUNTER_MATCH_CACHE_PLANES))

    def match_cache_scans(self) -> int:
        """PreFilter sweeps served from the match cache so far (0 under KT_NO_MATCH_CACHE=1 and for programs
        the cache does not take: several chunks, slow shapes, a namespace word list longer than four, more than 8 dimensions)."""
        return int(lib().kt_counter(self._h, COUNTER_MATCH_CACHE_SCANS))

    def match_cache_agg_scans(self) -> int:
        """Full aggregate scans that replayed the match cache so far (0 under KT_NO_MATCH_CACHE_AGG=1 or KT_NO_MATCH_CACHE=1 and
        wherever the aggregate does not run its two-per-CU form over a program the cache takes)."""
        return int(lib().kt_counter(self._h, COUNTER_MATCH_CACHE_AGG_SCANS))

    def partial_words(self) -> int:
        return self.throttle_rows() * partial_layout(self.D)["stride"]

    def set_wide_sums(self, mode: int):
        """1: always the two-block (limb sums) form of the partial buffer — what every rank of a multi-rank exchange must
        agree on; 0: decided per engine (single rank)."""
        self._ck(lib().kt_set_wide_sums(self._h, mode))

    def pending_partial_words(self):
        """(int64 words, two-block form?) of the aggregate that is pending."""
        n, w = C.c_int64(), C.c_int32()
        self._ck(lib().kt_partial_words(self._h, C.byref(n), C.byref(w)))
        return int(n.value), bool(w.value)

    def finalize_launch(self, now, apply=True, stream=None):
        self._ck(lib().kt_finalize_launch(self._h, int(now[0]), int(now[1]), RECONCILE_APPLY if apply else 0, stream))

    def throttle_rows(self) -> int:
        n = C.c_int32()
        self._ck(lib().kt_throttle_rows(self._h, C.byref(n)))
        return n.value

    def reconcile_fetch(self, n=None) -> ReconcileResult:
        n = self.throttle_rows() if n is None else n
        r = ReconcileResult(n, self.D)
        st = r.as_struct()
        self._ck(lib().kt_reconcile_fetch(self._h, n, C.byref(st)))
        return r

    def next_override(self, n=None):
        """NextOverrideHappensIn of the last reconcile: (instant seconds, nanoseconds, has) per throttle row."""
        n = self.throttle_rows() if n is None else n
        sec, nsec, has = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        self._ck(lib().kt_reconcile_fetch_next_override(self._h, n, sec.ctypes.data, nsec.ctypes.data, has.ctypes.data))
        return sec[:n], nsec[:n], has[:n]

    def reconcile(self, now, apply=True) -> ReconcileResult:
        self.reconcile_launch(now, apply)
        return self.reconcile_fetch()

    # ---- check
    def check_launch(self, n, rows=None, on_equal=False, want_status=False, stream=None):
        a, p = self._rows(rows, np.int64)
        self._ck(lib().kt_check_launch(self._h, n, p, int(on_equal), CHECK_STATUS_MATRIX if want_status else 0, stream))

    def sweep_launch(self, now, apply=True, on_equal=False, stream=None):
        """kt_sweep_launch: PreFilter sweep of every pod row against the stored status + reconcile of every throttle, one pass
        over the pod tables; read the results with check_fetch(pod rows) / reconcile_fetch()."""
        self._ck(lib().kt_sweep_launch(self._h, int(now[0]), int(now[1]), RECONCILE_APPLY if apply else 0, int(on_equal), stream))

    def check_fetch(self, n, want_status=False):
        T = self.throttle_rows()
        summary = np.zeros(max(n, 1), np.uint64)
        status = np.zeros((max(n, 1), max(T, 1)), np.uint8) if want_status else None
        self._ck(lib().kt_check_fetch(self._h, n, summary.ctypes.data, None if status is None else status.ctypes.data))
        return (None if status is None else status[:n, :T]), summary[:n]

    def check(self, rows=None, n=None, on_equal=False, want_status=True):
        n = len(rows) if rows is not None else n
        self.check_launch(n, rows, on_equal, want_status)
        return self.check_fetch(n, want_status)

    def check_atomic(self, rows=None, n=None, on_equal=False, want_status=True):
        """kt_check: launch + fetch under one engine lock (safe next to other threads using the engine)."""
        a, p = self._rows(rows, np.int64)
        n = len(a) if a is not None else n
        T = self.throttle_rows()
        summary = np.zeros(max(n, 1), np.uint64)
        status = np.zeros((max(n, 1), max(T, 1)), np.uint8) if want_status else None
        self._ck(lib().kt_check(self._h, n, p, int(on_equal), summary.ctypes.data,
                                None if status is None else status.ctypes.data))
        return (None if status is None else status[:n, :T]), summary[:n]

    def checker(self, n: int, on_equal=False):
        """Pre-bound kt_check(n pods, summaries only) for latency-sensitive callers: (rows, summary, call) — fill rows[:],
        call(), read summary[:]; no per-call allocation or argument marshalling beyond the foreign call itself."""
        rows = np.zeros(n, np.int64)
        summary = np.zeros(n, np.uint64)
        fn, h = lib().kt_check, self._h
        rp, sp, eq = C.c_void_p(rows.ctypes.data), C.c_void_p(summary.ctypes.data), int(on_equal)

        def call():
            rc = fn(h, n, rp, eq, sp, None)
            if rc != KT_OK:
                self._ck(rc)
        return rows, summary, call

    # ---- sequential admission with reservation (N1): results are read like a check's
    def admit(self, rows=None, n=None, on_equal=False, commit=False, want_status=True):
        a, p = self._rows(rows, np.int64)
        n = len(a) if a is not None else n
        self._ck(lib().kt_admit_launch(self._h, n, p, int(on_equal), ADMIT_COMMIT if commit else 0, None))
        return self.check_fetch(n, want_status)

    def admit_gangs(self, rows, gang_off, on_equal=False, commit=False, want_status=True):
        """kt_admit_gangs_launch: the queue ``rows`` in consecutive gangs ``[gang_off[g], gang_off[g + 1])``, each admitted all or
        nothing (a gang with a member that is not admitted is rolled back before the next one starts) ->
        (status matrix, summary words — both as PreFilter answered at each pod's turn —, admitted byte per gang)."""
        n, ng = self.admit_gangs_launch(rows, gang_off, on_equal, commit)
        status, summary = self.check_fetch(n, want_status)
        return status, summary, self.admit_gangs_fetch(ng)

    def admit_gangs_launch(self, rows, gang_off, on_equal=False, commit=False, stream=None):
        """kt_admit_gangs_launch alone -> (queue length, gangs): read the results with check_fetch and admit_gangs_fetch."""
        a, p = self._rows(rows, np.int64)
        g = _gang_offsets(gang_off)
        n, ng = len(a), len(g) - 1
        self._ck(lib().kt_admit_gangs_launch(self._h, n, p, ng, g.ctypes.data, int(on_equal), ADMIT_COMMIT if commit else 0, stream))
        return n, ng

    def admit_gangs_fetch(self, n_gangs):
        admitted = np.zeros(max(n_gangs, 1), np.uint8)
        self._ck(lib().kt_admit_gangs_fetch(self._h, n_gangs, admitted.ctypes.data))
        return admitted[:n_gangs]

    def admit_gangs_elastic(self, rows, gang_off, min_members, required=None, on_equal=False, commit=False, want_status=True):
        """kt_admit_gangs_elastic_launch: the queue ``rows`` in consecutive gangs ``[gang_off[g], gang_off[g + 1])``; gang g is kept
        once at least ``min_members[g]`` members succeeded and every ``required`` one did (bool, or flag bytes with
        GANG_MEMBER_REQUIRED, per queue position; None: none), else rolled back -> (status matrix, summary words — both as PreFilter
        answered at each pod's turn —, members that stay reserved per gang: 0 rolled back).  Member i of gang g is in iff
        ``members[g] > 0`` and its summary word says Success."""
        n, ng = self.admit_gangs_elastic_launch(rows, gang_off, min_members, required, on_equal, commit)
        status, summary = self.check_fetch(n, want_status)
        return status, summary, self.admit_gangs_elastic_fetch(ng)

    def admit_gangs_elastic_launch(self, rows, gang_off, min_members, required=None, on_equal=False, commit=False, stream=None):
        """kt_admit_gangs_elastic_launch alone -> (queue length, gangs): read the results with check_fetch and
        admit_gangs_elastic_fetch (the counts) or admit_gangs_fetch (the bytes)."""
        a, p = self._rows(rows, np.int64)
        g = _gang_offsets(gang_off)
        n, ng = len(a), len(g) - 1
        mm, rq = _elastic_rule(min_members, required, n, ng)
        self._ck(lib().kt_admit_gangs_elastic_launch(self._h, n, p, ng, g.ctypes.data, mm.ctypes.data if ng else None,
                                                     None if rq is None or not n else rq.ctypes.data, int(on_equal),
                                                     ADMIT_COMMIT if commit else 0, stream))
        return n, ng

    def admit_gangs_elastic_fetch(self, n_gangs):
        members = np.zeros(max(n_gangs, 1), np.int64)
        self._ck(lib().kt_admit_gangs_elastic_fetch(self._h, n_gangs, members.ctypes.data))
        return members[:n_gangs]

    # ---- headroom: how many copies of a pod the throttles still admit
    def headroom_launch(self, n, rows=None, cap=1, on_equal=False, stream=None):
        a, p = self._rows(rows, np.int64)
        self._ck(lib().kt_headroom_launch(self._h, n, p, int(on_equal), int(cap), stream))

    def headroom_fetch(self, n, want_limiting=True):
        copies = np.zeros(max(n, 1), np.int64)
        limiting = np.zeros(max(n, 1), np.int32) if want_limiting else None
        self._ck(lib().kt_headroom_fetch(self._h, n, copies.ctypes.data, None if limiting is None else limiting.ctypes.data))
        return copies[:n], (None if limiting is None else limiting[:n])

    def headroom(self, rows=None, n=None, *, cap, on_equal=False):
        """kt_headroom_launch + kt_headroom_fetch: per pod the number of leading Success verdicts a dry-run admission of
        ``[pod] * cap`` returns, and the lowest throttle row that stops the next copy (-1: all ``cap`` are admitted) ->
        (copies int64 [n], limiting int32 [n]).  Reserved amounts and stored status are left as they are."""
        n = len(rows) if rows is not None else n
        self.headroom_launch(n, rows, cap, on_equal)
        return self.headroom_fetch(n)

    # ---- headroom, for gangs: how many copies of a whole gang the throttles still admit
    def headroom_gangs_launch(self, pod_rows, gang_off, cap=1, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        g = _gang_offsets(gang_off)
        self._ck(lib().kt_headroom_gangs_launch(self._h, len(a), p if len(a) else None, len(g) - 1, g.ctypes.data, int(on_equal), int(cap), stream))

    def headroom_gangs_fetch(self, n_gangs, want_limiting=True, want_blocker=True):
        copies = np.zeros(max(n_gangs, 1), np.int64)
        limiting = np.zeros(max(n_gangs, 1), np.int32) if want_limiting else None
        blocker = np.zeros(max(n_gangs, 1), np.int64) if want_blocker else None
        self._ck(lib().kt_headroom_gangs_fetch(self._h, n_gangs, copies.ctypes.data, None if limiting is None else limiting.ctypes.data,
                                               None if blocker is None else blocker.ctypes.data))
        return copies[:n_gangs], (None if limiting is None else limiting[:n_gangs]), (None if blocker is None else blocker[:n_gangs])

    def headroom_gangs(self, pod_rows, gang_off, *, cap, on_equal=False):
        """kt_headroom_gangs_launch + kt_headroom_gangs_fetch: per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` the number of
        leading admitted gangs of a dry-run gang admission of ``cap`` consecutive copies of it, the lowest throttle row that stops
        the first member of the next copy that is not admitted (-1: all ``cap`` copies are admitted, or that member's verdict is an
        Error) and that member's queue position (-1: all are admitted) -> (copies int64 [n_gangs], limiting int32 [n_gangs],
        blocker int64 [n_gangs]).  Gangs are judged independently of each other, each against the stored reserved amounts.
        Reserved amounts and stored status are left as they are."""
        self.headroom_gangs_launch(pod_rows, gang_off, cap, on_equal)
        return self.headroom_gangs_fetch(len(_gang_offsets(gang_off)) - 1)

    # ---- preempt: the shortest victim prefix that lets a blocked pod through
    def preempt_launch(self, pod_rows, cand_rows, now, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        c, q = self._rows(cand_rows, np.int64)
        self._ck(lib().kt_preempt_launch(self._h, len(a), p if len(a) else None, len(c), q if len(c) else None, int(now[0]), int(now[1]),
                                         int(on_equal), stream))

    def preempt_reprieve_launch(self, pod_rows, cand_rows, now, on_equal=False, stream=None):
        """kt_preempt_reprieve_launch: kt_preempt_launch and, behind it on the same stream, the reprieve pass that shrinks the
        victim bytes to a minimal set; fetched with ``preempt_fetch``."""
        a, p = self._rows(pod_rows, np.int64)
        c, q = self._rows(cand_rows, np.int64)
        self._ck(lib().kt_preempt_reprieve_launch(self._h, len(a), p if len(a) else None, len(c), q if len(c) else None, int(now[0]),
                                                  int(now[1]), int(on_equal), stream))

    def preempt_fetch(self, n, n_cand, want_victims=True):
        prefix = np.zeros(max(n, 1), np.int64)
        flat = np.zeros(max(n * n_cand, 1), np.uint8) if want_victims else None
        self._ck(lib().kt_preempt_fetch(self._h, n, prefix.ctypes.data, None if flat is None else flat.ctypes.data))
        return prefix[:n], (None if flat is None else flat[:n * n_cand].reshape(n, n_cand))

    def preempt(self, pod_rows, cand_rows, now, on_equal=False, want_victims=True, reprieve=False):
        """kt_preempt_launch + kt_preempt_fetch: per preemptor the smallest k for which the pod passes PreFilter once the
        candidates ``cand_rows[:k]`` are gone and every throttle has been reconciled at ``now`` (0: it already passes against a
        fresh reconcile, PREEMPT_NONE: no prefix helps), and the victim bytes [n][n_cand] — 1 for the counted candidates below
        the prefix that a throttle affecting the pod matches -> (prefix int64 [n], victims uint8 [n][n_cand] or None).  A dry
        run: stored status and reserved amounts stay as they are.  ``reprieve``: the victims are walked back, last first, and
        each stays back as long as the pod still passes (kt_preempt_reprieve_launch) — the prefix is the same, the victim bytes
        are a minimal set."""
        (self.preempt_reprieve_launch if reprieve else self.preempt_launch)(pod_rows, cand_rows, now, on_equal)
        return self.preempt_fetch(len(pod_rows), len(cand_rows), want_victims)

    # ---- preempt, for gangs: the shortest victim prefix that lets a whole gang in
    def preempt_gangs_launch(self, pod_rows, gang_off, cand_rows, now, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        c, q = self._rows(cand_rows, np.int64)
        g = _gang_offsets(gang_off)
        self._ck(lib().kt_preempt_gangs_launch(self._h, len(a), p if len(a) else None, len(g) - 1, g.ctypes.data, len(c), q if len(c) else None,
                                               int(now[0]), int(now[1]), int(on_equal), stream))

    def preempt_gangs_reprieve_launch(self, pod_rows, gang_off, cand_rows, now, on_equal=False, stream=None):
        """kt_preempt_gangs_reprieve_launch: kt_preempt_gangs_launch and, behind it on the same stream, the reprieve pass that
        shrinks every gang's victim bytes to a minimal set; fetched with ``preempt_gangs_fetch``."""
        a, p = self._rows(pod_rows, np.int64)
        c, q = self._rows(cand_rows, np.int64)
        g = _gang_offsets(gang_off)
        self._ck(lib().kt_preempt_gangs_reprieve_launch(self._h, len(a), p if len(a) else None, len(g) - 1, g.ctypes.data, len(c),
                                                        q if len(c) else None, int(now[0]), int(now[1]), int(on_equal), stream))

    def preempt_gangs_fetch(self, n_gangs, n_cand, want_victims=True):
        prefix = np.zeros(max(n_gangs, 1), np.int64)
        blocker = np.zeros(max(n_gangs, 1), np.int64)
        flat = np.zeros(max(n_gangs * n_cand, 1), np.uint8) if want_victims else None
        self._ck(lib().kt_preempt_gangs_fetch(self._h, n_gangs, prefix.ctypes.data, None if flat is None else flat.ctypes.data,
                                              blocker.ctypes.data))
        return prefix[:n_gangs], (None if flat is None else flat[:n_gangs * n_cand].reshape(n_gangs, n_cand)), blocker[:n_gangs]

    def preempt_gangs(self, pod_rows, gang_off, cand_rows, now, on_equal=False, want_victims=True, reprieve=False):
        """kt_preempt_gangs_launch + kt_preempt_gangs_fetch: per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` the smallest k for
        which an in-order admission of its members (each admitted member reserves against the throttles the later ones meet)
        admits all of them once the candidates ``cand_rows[:k]`` are gone and every throttle has been reconciled at ``now``
        (PREEMPT_NONE: no prefix does), the victim bytes, and the queue position of the first member that is not admitted with
        nothing deleted (-1 where the prefix is 0) -> (prefix int64 [n_gangs], victims uint8 [n_gangs][n_cand] or None, blocker
        int64 [n_gangs]).  Gangs are judged independently of each other, each against the stored reserved amounts.  A dry run:
        stored status and reserved amounts stay as they are.  ``reprieve``: every gang's victims are walked back, last first, and
        each stays back as long as the whole gang is still admitted (kt_preempt_gangs_reprieve_launch) — prefix and blocker are the
        same, the victim bytes are a minimal set."""
        (self.preempt_gangs_reprieve_launch if reprieve else self.preempt_gangs_launch)(pod_rows, gang_off, cand_rows, now, on_equal)
        return self.preempt_gangs_fetch(len(_gang_offsets(gang_off)) - 1, len(cand_rows), want_victims)

    # ---- preempt, for elastic gangs: the shortest victim prefix that lets a gang's quorum in
    def preempt_gangs_elastic_launch(self, pod_rows, gang_off, min_members, cand_rows, now, required=None, on_equal=False, reprieve=False,
                                     stream=None):
        a, p = self._rows(pod_rows, np.int64)
        c, q = self._rows(cand_rows, np.int64)
        g = _gang_offsets(gang_off)
        n, ng = len(a), len(g) - 1
        mm, rq = _elastic_rule(min_members, required, n, ng)
        self._ck(lib().kt_preempt_gangs_elastic_launch(self._h, n, p if n else None, ng, g.ctypes.data, mm.ctypes.data if ng else None,
                                                       None if rq is None or not n else rq.ctypes.data, len(c), q if len(c) else None,
                                                       int(now[0]), int(now[1]), int(on_equal), PREEMPT_REPRIEVE if reprieve else 0, stream))

    def preempt_gangs_elastic_fetch(self, n_gangs, n_cand, want_victims=True):
        prefix, members, blocker = (np.zeros(max(n_gangs, 1), np.int64) for _ in range(3))
        flat = np.zeros(max(n_gangs * n_cand, 1), np.uint8) if want_victims else None
        self._ck(lib().kt_preempt_gangs_elastic_fetch(self._h, n_gangs, prefix.ctypes.data, None if flat is None else flat.ctypes.data,
                                                      members.ctypes.data, blocker.ctypes.data))
        return (prefix[:n_gangs], (None if flat is None else flat[:n_gangs * n_cand].reshape(n_gangs, n_cand)), members[:n_gangs],
                blocker[:n_gangs])

    def preempt_gangs_elastic(self, pod_rows, gang_off, min_members, cand_rows, now, required=None, on_equal=False, reprieve=False,
                              want_victims=True):
        """kt_preempt_gangs_elastic_launch + kt_preempt_gangs_elastic_fetch: per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` the
        smallest k for which an in-order walk of its members — a member that succeeds reserves against the throttles the later
        ones meet, one that fails reserves nowhere — has at least ``min_members[g]`` successes and every ``required`` member (bool,
        or flag bytes with GANG_MEMBER_REQUIRED, per queue position; None: none) among them, once the candidates ``cand_rows[:k]``
        are gone and every throttle has been reconciled at ``now`` (PREEMPT_NONE: no prefix does, or members that never succeed put
        the rule out of reach) -> (prefix int64 [n_gangs]; victims uint8 [n_gangs][n_cand] or None; members int64 [n_gangs]: how
        many succeed in the final state, in S_0 where there is no prefix; blocker int64 [n_gangs]: the first required member that
        does not succeed with nothing deleted, else the first member that does not, -1 where the prefix is 0).  ``reprieve``: the
        victims are walked back, last first, and each stays back as long as the rule still holds.  A dry run."""
        self.preempt_gangs_elastic_launch(pod_rows, gang_off, min_members, cand_rows, now, required, on_equal, reprieve)
        return self.preempt_gangs_elastic_fetch(len(_gang_offsets(gang_off)) - 1, len(cand_rows), want_victims)

    # ---- forecast: the first instant at which a blocked pod passes
    def forecast_launch(self, pod_rows, instants, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
        inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
        m = len(inst_s)
        self._ck(lib().kt_forecast_launch(self._h, len(a), p if len(a) else None, m, inst_s.ctypes.data if m else None,
                                          inst_ns.ctypes.data if m else None, int(on_equal), stream))

    def forecast_fetch(self, n, n_inst, want_verdicts=True):
        first = np.zeros(max(n, 1), np.int64)
        flat = np.zeros(max(n * n_inst, 1), np.uint8) if want_verdicts else None
        self._ck(lib().kt_forecast_fetch(self._h, n, first.ctypes.data, None if flat is None else flat.ctypes.data))
        return first[:n], (None if flat is None else flat[:n * n_inst].reshape(n, n_inst))

    def forecast(self, pod_rows, instants, on_equal=False, want_verdicts=True):
        """kt_forecast_launch + kt_forecast_fetch: per pod the KT_VERDICT_* of PreFilter once every valid and responsible throttle
        has been reconciled at each of the strictly ascending ``instants`` [(seconds, nanoseconds)] — each on the state as it is
        now, not on top of the previous instant — and the first position whose verdict is Success (FORECAST_NONE: none) ->
        (first int64 [n], verdicts uint8 [n][n_inst] or None).  A dry run: stored status and reserved amounts stay as they are."""
        self.forecast_launch(pod_rows, instants, on_equal)
        return self.forecast_fetch(len(pod_rows), len(instants), want_verdicts)

    # ---- forecast, for gangs: the first instant at which a whole gang is admitted
    def forecast_gangs_launch(self, pod_rows, gang_off, instants, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        g = _gang_offsets(gang_off)
        inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
        inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
        m = len(inst_s)
        self._ck(lib().kt_forecast_gangs_launch(self._h, len(a), p if len(a) else None, len(g) - 1, g.ctypes.data, m,
                                                inst_s.ctypes.data if m else None, inst_ns.ctypes.data if m else None, int(on_equal), stream))

    def forecast_gangs_fetch(self, n_gangs, n_inst, want_verdicts=True, want_blocker=True):
        first = np.zeros(max(n_gangs, 1), np.int64)
        flat = np.zeros(max(n_gangs * n_inst, 1), np.uint8) if want_verdicts else None
        blk = np.zeros(max(n_gangs * n_inst, 1), np.int64) if want_blocker else None
        self._ck(lib().kt_forecast_gangs_fetch(self._h, n_gangs, first.ctypes.data, None if flat is None else flat.ctypes.data,
                                               None if blk is None else blk.ctypes.data))
        return (first[:n_gangs], (None if flat is None else flat[:n_gangs * n_inst].reshape(n_gangs, n_inst)),
                (None if blk is None else blk[:n_gangs * n_inst].reshape(n_gangs, n_inst)))

    def forecast_gangs(self, pod_rows, gang_off, instants, on_equal=False, want_verdicts=True, want_blocker=True):
        """kt_forecast_gangs_launch + kt_forecast_gangs_fetch: per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` and per instant
        the KT_VERDICT_* of an in-order admission of its members (each admitted member reserves against the throttles the later
        ones meet) once every valid and responsible throttle has been reconciled at that instant, the first position whose
        verdict is Success (FORECAST_NONE: none), and per instant the queue position of the first member that is not admitted
        (-1 where the gang passes) -> (first int64 [n_gangs], verdicts uint8 [n_gangs][n_inst] or None, blocker int64
        [n_gangs][n_inst] or None).  Gangs are judged independently of each other, each against the stored reserved amounts.
        A dry run: stored status and reserved amounts stay as they are."""
        self.forecast_gangs_launch(pod_rows, gang_off, instants, on_equal)
        return self.forecast_gangs_fetch(len(_gang_offsets(gang_off)) - 1, len(instants), want_verdicts, want_blocker)

    # ---- forecast, for elastic gangs: the first instant at which a gang's quorum fits
    def forecast_gangs_elastic_launch(self, pod_rows, gang_off, min_members, instants, required=None, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        g = _gang_offsets(gang_off)
        n, ng = len(a), len(g) - 1
        mm, rq = _elastic_rule(min_members, required, n, ng)
        inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
        inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
        m = len(inst_s)
        self._ck(lib().kt_forecast_gangs_elastic_launch(self._h, n, p if n else None, ng, g.ctypes.data, mm.ctypes.data if ng else None,
                                                        None if rq is None or not n else rq.ctypes.data, m,
                                                        inst_s.ctypes.data if m else None, inst_ns.ctypes.data if m else None,
                                                        int(on_equal), stream))

    def forecast_gangs_elastic_fetch(self, n_gangs, n_inst, want_verdicts=True, want_members=True, want_blocker=True):
        cells = max(n_gangs * n_inst, 1)
        first = np.zeros(max(n_gangs, 1), np.int64)
        flat = np.zeros(cells, np.uint8) if want_verdicts else None
        mem = np.zeros(cells, np.int64) if want_members else None
        blk = np.zeros(cells, np.int64) if want_blocker else None
        self._ck(lib().kt_forecast_gangs_elastic_fetch(self._h, n_gangs, first.ctypes.data, None if flat is None else flat.ctypes.data,
                                                       None if mem is None else mem.ctypes.data, None if blk is None else blk.ctypes.data))
        shaped = lambda x: None if x is None else x[:n_gangs * n_inst].reshape(n_gangs, n_inst)
        return first[:n_gangs], shaped(flat), shaped(mem), shaped(blk)

    def forecast_gangs_elastic(self, pod_rows, gang_off, min_members, instants, required=None, on_equal=False, want_verdicts=True,
                               want_members=True, want_blocker=True):
        """kt_forecast_gangs_elastic_launch + kt_forecast_gangs_elastic_fetch: per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]``
        and per instant an in-order walk of its members once every valid and responsible throttle has been reconciled at that
        instant — a member that succeeds reserves against the throttles the later ones meet, one that fails reserves nowhere —
        and the elastic rule on it: Success iff at least ``min_members[g]`` members succeed and every ``required`` one does (bool,
        or flag bytes with GANG_MEMBER_REQUIRED, per queue position; None: none); Error at every instant where members that never
        succeed put the rule out of reach -> (first int64 [n_gangs]: the first position whose verdict is Success, FORECAST_NONE:
        none; verdicts uint8 [n_gangs][n_inst]; members int64 [n_gangs][n_inst]: how many succeed, admitted or not; blocker int64
        [n_gangs][n_inst]: the first required member that does not succeed, else the first member that does not, -1 where the
        verdict is Success) — each of the last three None where not wanted.  A dry run."""
        self.forecast_gangs_elastic_launch(pod_rows, gang_off, min_members, instants, required, on_equal)
        return self.forecast_gangs_elastic_fetch(len(_gang_offsets(gang_off)) - 1, len(instants), want_verdicts, want_members, want_blocker)

    # ---- headroom forecast: how many copies of a pod the throttles admit at each instant
    def headroom_forecast_launch(self, pod_rows, instants, cap, want=1, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
        inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
        m = len(inst_s)
        self._ck(lib().kt_headroom_forecast_launch(self._h, len(a), p if len(a) else None, m, inst_s.ctypes.data if m else None,
                                                   inst_ns.ctypes.data if m else None, int(on_equal), int(cap), int(want), stream))

    def headroom_forecast_fetch(self, n, n_inst, want_copies=True, want_limiting=True):
        first = np.zeros(max(n, 1), np.int64)
        copies = np.zeros(max(n * n_inst, 1), np.int64) if want_copies else None
        limiting = np.zeros(max(n * n_inst, 1), np.int32) if want_limiting else None
        self._ck(lib().kt_headroom_forecast_fetch(self._h, n, first.ctypes.data, None if copies is None else copies.ctypes.data,
                                                  None if limiting is None else limiting.ctypes.data))
        return (first[:n], (None if copies is None else copies[:n * n_inst].reshape(n, n_inst)),
                (None if limiting is None else limiting[:n * n_inst].reshape(n, n_inst)))

    def headroom_forecast(self, pod_rows, instants, *, cap, want=1, on_equal=False):
        """kt_headroom_forecast_launch + kt_headroom_forecast_fetch: per pod and per instant the number of leading Success
        verdicts a dry-run admission of ``cap`` copies of the pod returns once every valid and responsible throttle has been
        reconciled at that instant (each on the state as it is now), the lowest throttle row that stops the next copy (-1: all
        ``cap`` are admitted), and the first position with at least ``want`` copies (FORECAST_NONE: none) -> (first int64 [n],
        copies int64 [n][n_inst], limiting int32 [n][n_inst]).  A dry run: stored status and reserved amounts stay as they are."""
        self.headroom_forecast_launch(pod_rows, instants, cap, want, on_equal)
        return self.headroom_forecast_fetch(len(pod_rows), len(instants))

    # ---- headroom forecast, for gangs: how many copies of a whole gang the throttles admit at each instant
    def headroom_forecast_gangs_launch(self, pod_rows, gang_off, instants, cap, want=1, on_equal=False, stream=None):
        a, p = self._rows(pod_rows, np.int64)
        g = _gang_offsets(gang_off)
        inst_s = np.ascontiguousarray([int(t[0]) for t in instants], dtype=np.int64)
        inst_ns = np.ascontiguousarray([int(t[1]) for t in instants], dtype=np.int32)
        m = len(inst_s)
        self._ck(lib().kt_headroom_forecast_gangs_launch(self._h, len(a), p if len(a) else None, len(g) - 1, g.ctypes.data, m,
                                                         inst_s.ctypes.data if m else None, inst_ns.ctypes.data if m else None,
                                                         int(on_equal), int(cap), int(want), stream))

    def headroom_forecast_gangs_fetch(self, n_gangs, n_inst, want_copies=True, want_limiting=True, want_blocker=True):
        cells = max(n_gangs * n_inst, 1)
        first = np.zeros(max(n_gangs, 1), np.int64)
        copies = np.zeros(cells, np.int64) if want_copies else None
        limiting = np.zeros(cells, np.int32) if want_limiting else None
        blk = np.zeros(cells, np.int64) if want_blocker else None
        self._ck(lib().kt_headroom_forecast_gangs_fetch(self._h, n_gangs, first.ctypes.data, None if copies is None else copies.ctypes.data,
                                                        None if limiting is None else limiting.ctypes.data,
                                                        None if blk is None else blk.ctypes.data))
        shaped = lambda x: None if x is None else x[:n_gangs * n_inst].reshape(n_gangs, n_inst)
        return first[:n_gangs], shaped(copies), shaped(limiting), shaped(blk)

    def headroom_forecast_gangs(self, pod_rows, gang_off, instants, *, cap, want=1, on_equal=False):
        """kt_headroom_forecast_gangs_launch + kt_headroom_forecast_gangs_fetch: per gang ``pod_rows[gang_off[g]:gang_off[g + 1]]``
        and per instant the number of leading admitted gangs a dry-run gang admission of ``cap`` consecutive copies of the gang
        returns once every valid and responsible throttle has been reconciled at that instant (each on the state as it is now), the
        lowest throttle row that stops the first member of the first refused copy that is not admitted, that member's queue
        position (both -1: all ``cap`` are admitted), and the first position with at least ``want`` copies (FORECAST_NONE: none)
        -> (first int64 [n_gangs], copies int64 [n_gangs][n_inst], limiting int32 [n_gangs][n_inst], blocker int64
        [n_gangs][n_inst]).  A dry run: stored status and reserved amounts stay as they are."""
        self.headroom_forecast_gangs_launch(pod_rows, gang_off, instants, cap, want, on_equal)
        return self.headroom_forecast_gangs_fetch(len(_gang_offsets(gang_off)) - 1, len(instants))

    def override_instants(self, from_, until, cap=None):
        """kt_override_instants: the sorted, distinct instants in (from_, until] at which some valid and responsible throttle's
        CalculateThreshold can change (every override ``begin``, and ``end`` + 1 ns) -> ([(seconds, nanoseconds)], total).
        ``cap``: at most so many (the earliest) are returned; None: all of them."""
        total = C.c_int64(0)
        args = (int(from_[0]), int(from_[1]), int(until[0]), int(until[1]))
        if cap is None:
            self._ck(lib().kt_override_instants(self._h, *args, 0, None, None, C.byref(total)))
            cap = total.value
        out_s, out_ns = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
        self._ck(lib().kt_override_instants(self._h, *args, int(cap), out_s.ctypes.data if cap else None, out_ns.ctypes.data if cap else None,
                                            C.byref(total)))
        k = min(int(cap), total.value)
        return [(int(a), int(b)) for a, b in zip(out_s[:k], out_ns[:k])], total.value

    def fetch_reserved(self, rows=None) -> S.Amounts:
        rows = np.arange(self.throttle_rows(), dtype=np.int32) if rows is None else rows
        a, p = self._rows(rows, np.int32)
        out = S.Amounts(len(a), self.D)
        st = out.as_struct()
        self._ck(lib().kt_fetch_reserved(self._h, len(a), p, C.byref(st)))
        return out

    def check_device_summary(self) -> int:
        ptr = C.c_void_p()
        self._ck(lib().kt_check_device_summary(self._h, C.byref(ptr)))
        return ptr.value

    def fetch_pod_requests(self, rows=None, n=None):
        a, p = self._rows(rows, np.int64)
        n = len(a) if a is not None else n
        v = np.zeros((max(n, 1), self.D), np.int64)
        present = np.zeros(max(n, 1), np.uint32)
        self._ck(lib().kt_fetch_pod_requests(self._h, n, p, v.ctypes.data, present.ctypes.data))
        return v[:n], present[:n]

    # ---- measurement
    def timing_enable(self, on=True):
        self._ck(lib().kt_timing_enable(self._h, int(on)))

    def timing_reset(self):
        self._ck(lib().kt_timing_reset(self._h))

    def timing_read(self, kernel):
        ms, n = C.c_double(), C.c_int64()
        self._ck(lib().kt_timing_read(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def synchronize(self, stream=None):
        self._ck(lib().kt_synchronize(self._h, stream))

    def kernel_name(self, kernel) -> str:
        return lib().kt_kernel_name(self._h, kernel).decode()
