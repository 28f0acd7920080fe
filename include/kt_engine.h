/*
 * kt_engine.h — C-ABI of the MI355X-native throttle-evaluation engine (libkt_engine.so).
 *
 * kube-throttler has no FFI of any kind today (pure Go, CGO_ENABLED=0 — Makefile:3,10), so this is a
 * NEW seam.  It is cut exactly where the Go plugin does its per-pod x per-throttle work, and each
 * entry point names the reference code whose body it replaces.  The outer plugin API stays untouched:
 *   PluginName / NewPlugin / PreFilter / Reserve / Unreserve  (pkg/scheduler_plugin/plugin.go:45,63,148,217,240)
 * The cgo stubs a maintainer would add are shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns int32_t: KT_OK (0) or a negative KT_ERR_*; text via kt_last_error().
 *   - the caller owns every pointer it passes; the engine copies during the call and retains nothing
 *     (cgo rule: C must not keep Go memory).  Output buffers are caller-allocated.
 *   - strings never cross: labels, namespaces, resource names are interned to ids by the caller
 *     (include/kt_snapshot.h documents the id spaces and the flat batch format).
 *   - rows are caller-managed dense indices: pod row in [0, pod_capacity), throttle row in
 *     [0, throttle_capacity), namespace id in [0, namespace_capacity).  Upserting a row replaces it.
 *   - `stream` arguments are a hipStream_t (NULL = the engine's own stream).  *_launch calls are
 *     asynchronous on that stream; results stay in HBM until a *_fetch call copies them out.
 *   - all entry points may be called from any OS thread; calls on one engine are serialised internally.
 */
#ifndef KT_ENGINE_H
#define KT_ENGINE_H

#include <stdint.h>
#include "kt_snapshot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KT_OK 0
#define KT_ERR_INVALID_ARGUMENT (-1)
#define KT_ERR_OUT_OF_RANGE (-2)   /* row / id / dimension outside the configured capacity */
#define KT_ERR_DEVICE (-3)         /* HIP runtime error (message has the hipError string) */
#define KT_ERR_OVERFLOW_RISK (-4)  /* a value beyond 2^60 (upsert), or pod requests that ADD UP beyond 2^60 in one dimension
                                      (reconcile: where resource.Quantity would promote to big decimals): rescale it */
#define KT_ERR_NOT_READY (-5)      /* fetch without a preceding launch */
#define KT_ERR_NO_DEVICE (-6)      /* no gfx950 device visible: there is NO CPU fallback */
#define KT_ERR_UNSUPPORTED (-7)    /* the request exceeds what this entry point supports (message says what) */

/* per (pod, throttle) status — v1alpha1.CheckThrottleStatus (throttle_types.go:119-126) + not-affected / error */
#define KT_STATUS_NOT_AFFECTED 0
#define KT_STATUS_NOT_THROTTLED 1
#define KT_STATUS_ACTIVE 2
#define KT_STATUS_INSUFFICIENT 3
#define KT_STATUS_POD_REQUESTS_EXCEEDS_THRESHOLD 4
#define KT_STATUS_ERROR 255

/* per-pod summary word: what KubeThrottler.PreFilter derives (plugin.go:148-215).
 * bits 0-1  verdict: 0 framework.Success, 1 UnschedulableAndUnresolvable, 2 framework.Error
 * bits 4-23 #throttles[pod-requests-exceeds-threshold], 24-43 #throttles[active], 44-63 #throttles[insufficient] */
#define KT_VERDICT_SUCCESS 0
#define KT_VERDICT_UNSCHEDULABLE 1
#define KT_VERDICT_ERROR 2
#define KT_SUMMARY_VERDICT(w) ((uint32_t)((w) & 3u))
#define KT_SUMMARY_EXCEEDS(w) ((uint32_t)(((w) >> 4) & 0xFFFFFu))
#define KT_SUMMARY_ACTIVE(w) ((uint32_t)(((w) >> 24) & 0xFFFFFu))
#define KT_SUMMARY_INSUFFICIENT(w) ((uint32_t)(((w) >> 44) & 0xFFFFFu))

typedef struct kt_engine kt_engine; /* opaque */

typedef struct kt_config {
  int32_t n_dims;             /* D: resource dimensions (<= KT_MAX_DIMS) */
  int32_t max_labels;         /* labels kept per pod (<= KT_MAX_LABELS) */
  int64_t pod_capacity;       /* pod rows held in HBM */
  int32_t throttle_capacity;  /* Throttle + ClusterThrottle rows (< 2^20) */
  int32_t namespace_capacity;
  int32_t device;             /* HIP device ordinal; -1 = current device */
  int32_t kernel_variant;     /* low byte: 0 = default (indexed); 1 = dense P x T scan (reference shape, for cross-checks);
                                 | KT_VARIANT_INCREMENTAL: see below */
} kt_config;
/* Incremental event path, indexed kernels only: the engine keeps the per-throttle `used` partials of
 * its pod rows current across kt_upsert_pods / kt_delete_pods by delta scans over just the touched rows (old content
 * out, new content in — which also covers the label-change symmetric difference of throttle_controller.go:469-500),
 * so that a reconcile no longer rescans every pod: kt_aggregate_launch becomes a copy.  A change of throttles or
 * namespaces voids the partials; the next reconcile rescans once.  Results are identical to a full rescan. */
#define KT_VARIANT_INCREMENTAL 0x100

/* Library / device facts (for logs and bench JSON). */
const char* kt_version(void);

/* Replaces the controller construction in NewPlugin (plugin.go:63-146) for the evaluation state:
 * allocates the SoA tables in HBM.  Fails with KT_ERR_NO_DEVICE when no GPU is present. */
int32_t kt_engine_create(const kt_config* cfg, kt_engine** out);
int32_t kt_engine_destroy(kt_engine* e);
/* Last error text of this engine (or of kt_engine_create when e == NULL); valid until the next call. */
const char* kt_last_error(kt_engine* e);

/* ---- state feed: what the informer event handlers push (throttle_controller.go:400-536,
 *      clusterthrottle_controller.go:428-570).  A batch is a kt_snapshot whose sections may be empty
 *      (n_ns / n_pods / n_thr = 0).  rows == NULL means batch index i -> row i. ------------------------ */
/* Namespaces: the object of each row (ns_valid[i] == 0: the row has no object, its pods answer Error) and its labels.  A batch may
 * name a row more than once: the LAST entry wins.  kt_upsert_namespaces, kt_upsert_namespace and kt_delete_namespaces validate the
 * whole batch before anything of it is kept: a refused batch (a row outside namespace_capacity: KT_ERR_OUT_OF_RANGE) leaves the
 * engine as it was — every namespace it names, the compiled program and the views included; nothing is recompiled for it.
 * An accepted namespace event is host work only: the next launch compiles the program again.  A result that is pending when the
 * event arrives (kt_check_launch, kt_reconcile_launch, kt_forecast_launch and the other *_launch calls) is not touched by it: its
 * fetch returns either the exact answer of the state at its launch or KT_ERR_NOT_READY, never anything else. */
int32_t kt_upsert_namespaces(kt_engine* e, const kt_snapshot* batch, const int32_t* ns_rows);
/* Pods: the effective request of each pod is computed ON DEVICE from the batch's containers —
 * resourcelist.PodRequestResourceList (pkg/resourcelist/resourcelist.go:27-46) + ResourceAmountOfPod
 * (resource_amount.go:71-76).
 * The arrays are copied during the call.  A batch that fits a 64 KB pinned slot (an informer event, or a few dozen
 * coalesced ones) does NOT wait for the device: the call enqueues one kernel and returns; every other entry point — a
 * kt_check issued right behind it included — first waits for the newest such call, so the order "feed the event, then
 * the next PreFilter sees it" holds (kt_delete_pods and kt_upsert_pod likewise).  Larger batches block as before.
 * A batch may name a pod row more than once (coalesced informer events — Add, then Update of one pod): the entries are applied
 * in batch order, the LAST one wins, exactly as if they had arrived in separate calls (incremental engines included).
 * The whole batch is validated before anything of it is kept: a refused batch (a row or namespace id outside the capacity, more
 * labels than the engine keeps, a request beyond 2^60) leaves the engine as it was — its bounds, its "a negative request was fed"
 * mark, its views and its compiled program included. */
int32_t kt_upsert_pods(kt_engine* e, const kt_snapshot* batch, const int64_t* pod_rows);
/* Throttles: spec (threshold, overrides, selector), stored status and reserved amounts of each row.
 * The whole batch is validated before anything of it is kept — by kt_upsert_throttles, kt_upsert_throttle and kt_load_snapshot
 * alike, with the one pass kt_validate_throttles exports (below).  Refused are
 *   - a row outside throttle_capacity, at any position of the batch, and a namespaced Throttle whose namespace id lies at or beyond
 *     namespace_capacity (KT_ERR_OUT_OF_RANGE);
 *   - a batch whose D differs from the engine's;
 *   - thr_ovr_off / thr_term_off / term_preq_off / term_nreq_off / preq.val_off / nreq.val_off that do not start at 0 or that
 *     decrease; term_preq_off / term_nreq_off that end beyond preq.n / nreq.n (KT_ERR_OUT_OF_RANGE); a non-empty value range
 *     with val == NULL;
 *   - an operator above KT_OP_DOES_NOT_EXIST, a term flag outside KT_TERM_POD_SEL_INVALID | KT_TERM_NS_SEL_INVALID;
 *   - a presence mask of thr_spec / thr_calc / thr_used / thr_reserved / ovr_thr, or thr_thrl_flag | thr_thrl_has, with a bit at or
 *     above n_dims;
 *   - status.used or a reserved amount beyond 2^60 (KT_ERR_OVERFLOW_RISK);
 * KT_ERR_INVALID_ARGUMENT where no other code is named, and kt_last_error names the array and the position.  The pass reads
 * nothing beyond what the counts and the offsets it has already checked cover.  A refused call leaves the engine as it was: every
 * throttle row, the row count, the compiled program, the views, the match cache and the pending results included; nothing is
 * recompiled for it.
 * A batch may name a row more than once (coalesced informer events): the entries are applied in batch order, the LAST one wins.
 * An accepted event whose rows keep what the selector program is compiled from — the VALID / RESPONSIBLE / CLUSTER flags, the
 * namespace id, the terms with their flags and requirements — only uploads the throttle tables again: a threshold, an override,
 * a status or a reservation costs no compile.  Anything else (a fresh row beyond the row count included) costs ONE compile per
 * gap between launches, however many events the gap holds.
 * Pending results: kt_check_fetch and kt_reconcile_fetch answer KT_ERR_NOT_READY behind an accepted throttle event (the results
 * describe the old throttle set and its row count); a pending query result (kt_headroom_launch, kt_forecast_launch,
 * kt_preempt_launch, kt_admit_gangs_launch and their kin) answers the exact state at its launch or KT_ERR_NOT_READY, never
 * anything else — also when the event grows the row count and with it every per-throttle buffer. */
int32_t kt_upsert_throttles(kt_engine* e, const kt_snapshot* batch, const int32_t* thr_rows);
/* The validation pass of kt_upsert_throttles on its own: needs no engine and no device.  n_dims, throttle_capacity and
 * namespace_capacity are those of the kt_config the batch is meant for; thr_rows may be NULL (batch index i -> row i).  Returns
 * what kt_upsert_throttles would answer before it stores anything, with the text of kt_last_error in err[0, err_len) (err may be
 * NULL). */
int32_t kt_validate_throttles(const kt_snapshot* batch, const int32_t* thr_rows, int32_t n_dims, int32_t throttle_capacity,
                              int32_t namespace_capacity, char* err, int32_t err_len);
/* The rows lose their objects and labels, as by kt_upsert_namespaces with ns_valid == 0; the pods that name them stay.  The whole
 * batch is validated first, see above. */
int32_t kt_delete_namespaces(kt_engine* e, int32_t n, const int32_t* ns_rows);
/* Pods leave by row.  A batch may name a row more than once, and rows that hold no pod (never fed, or deleted before — a Delete and
 * the DeletedFinalStateUnknown tombstone of one pod, a work queue drained into one call); both are no-ops beyond the first: the
 * rows end up empty and their pods are taken out of `used` once (incremental engines included).  Every row must lie inside
 * pod_capacity. */
int32_t kt_delete_pods(kt_engine* e, int64_t n, const int64_t* pod_rows);
/* Throttles leave by row: the rows end up empty (their stored status, reservations and matrix columns zero), the row count stays.
 * A batch may name a row more than once, and rows that hold nothing (never fed, or deleted before).  Every row must lie inside
 * throttle_capacity: the whole batch is checked first, a refused batch (KT_ERR_OUT_OF_RANGE) leaves the engine as it was.  An
 * accepted batch costs one compile per gap; pending results as for kt_upsert_throttles. */
int32_t kt_delete_throttles(kt_engine* e, int32_t n, const int32_t* thr_rows);
/* Clears everything and ingests a whole snapshot (rows = indices).  The snapshot is validated BEFORE anything is cleared: its
 * size against the capacity, its throttles by the pass of kt_upsert_throttles, its pods by that of kt_upsert_pods.  A refused load
 * leaves the engine as it was — pods, namespaces, throttles, bounds, the "a negative request was fed" mark, views, match cache,
 * compiled program and pending results. */
int32_t kt_load_snapshot(kt_engine* e, const kt_snapshot* s);

/* ---- single-object forms of the state feed: what ONE informer event handler call pushes (OnAdd / OnUpdate of a
 *      Pod, Throttle / ClusterThrottle, Namespace: throttle_controller.go:400-536, clusterthrottle_controller.go:428-570).
 *      Every pointer is a direct argument to pointer-free memory, no struct of pointers crosses the boundary: a cgo
 *      call may pass Go slices' backing arrays as they are (cgo pointer rule, also on the reference's go 1.20 — no
 *      runtime.Pinner needed).  Same semantics, validation and errors as the batch forms above. -------------------- */
int32_t kt_upsert_namespace(kt_engine* e, int32_t ns_row, int32_t exists, int32_t n_labels, const uint32_t* label_keys,
                            const uint32_t* label_pairs);
/* ctr_req: [n_ctr][D] (D = kt_config.n_dims); ovh: [D] or NULL; ovh_present: bit 31 = spec.overhead != nil */
int32_t kt_upsert_pod(kt_engine* e, int64_t pod_row, uint32_t ns, uint32_t flags, int32_t n_labels, const uint32_t* label_keys,
                      const uint32_t* label_pairs, int32_t n_ctr, const uint8_t* ctr_init, const uint32_t* ctr_present,
                      const int64_t* ctr_req, uint32_t ovh_present, const int64_t* ovh);
/* amounts of the throttle as four rows — 0 spec.threshold, 1 status.calculatedThreshold.threshold, 2 status.used,
 * 3 reserved: amt_v [4][D], amt_present [4], amt_count [4], amt_has_count [4].  Overrides: n_ovr rows (ovr_v [n_ovr][D]).
 * Selector: n_terms terms; term_preq_off / term_nreq_off [n_terms+1] index the two requirement pools, each given as
 * (n, op [n], key [n], val_off [n+1], val []) like kt_reqs.  The shapes are held against each other before anything is
 * stored (offset arrays start at 0 and never decrease, operators are KT_OP_*, masks name dimensions below n_dims, term flags
 * are KT_TERM_*): a slice passed in the wrong position answers KT_ERR_INVALID_ARGUMENT naming the argument (kt_last_error)
 * instead of feeding a wrong selector silently.  It is the validation pass of kt_upsert_throttles over the one-row batch the
 * arguments make: the text names the array by its kt_snapshot field (thr_spec.present for amt_present[0], preq.op for preq_op). */
int32_t kt_upsert_throttle(kt_engine* e, int32_t thr_row, uint32_t flags, uint32_t ns, const int64_t* amt_v,
                           const uint32_t* amt_present, const int64_t* amt_count, const uint8_t* amt_has_count,
                           uint32_t thrl_flag, uint32_t thrl_has, uint64_t status_msgs_fp, uint64_t spec_msgs_fp, int32_t n_ovr,
                           const int64_t* ovr_begin_s, const int32_t* ovr_begin_ns, const int64_t* ovr_end_s,
                           const int32_t* ovr_end_ns, const uint8_t* ovr_flags, const int64_t* ovr_v, const uint32_t* ovr_present,
                           const int64_t* ovr_count, const uint8_t* ovr_has_count, int32_t n_terms, const uint8_t* term_flags,
                           const uint32_t* term_preq_off, const uint32_t* term_nreq_off, uint32_t n_preq, const uint8_t* preq_op,
                           const uint32_t* preq_key, const uint32_t* preq_val_off, const uint32_t* preq_val, uint32_t n_nreq,
                           const uint8_t* nreq_op, const uint32_t* nreq_key, const uint32_t* nreq_val_off, const uint32_t* nreq_val);

/* Scheduler-side reserved amounts per throttle — the value reservedResourceAmount(nn) returns
 * (pkg/controllers/reserved_resource_amounts.go:113-126,148-156); the pod map itself stays in Go.
 * The whole batch is validated before the first row is stored (an amount beyond 2^60: KT_ERR_OVERFLOW_RISK, nothing is changed);
 * kt_set_status below likewise. */
int32_t kt_set_reserved(kt_engine* e, int32_t n, const int32_t* thr_rows, const kt_amounts* reserved);
/* Stored CR status as the informer cache holds it (what CheckThrottledFor reads, throttle_types.go:128-153). */
typedef struct kt_status {
  kt_amounts used;           /* status.used */
  kt_amounts calc;           /* status.calculatedThreshold.threshold */
  uint8_t* calc_at_nonzero;  /* !status.calculatedThreshold.calculatedAt.IsZero() ; as an OUTPUT: calculatedThreshold replaced, calculatedAt := now */
  uint32_t* thrl_flag;       /* status.throttled.resourceRequests values */
  uint32_t* thrl_has;        /* ... keys */
  uint8_t* thrl_pod;         /* status.throttled.resourceCounts.pod */
  uint64_t* msgs_fp;         /* fingerprint of status.calculatedThreshold.messages (0 = none); input only */
  uint8_t* error;            /* output only: reconcile returned an error for this throttle (selector) */
} kt_status;
int32_t kt_set_status(kt_engine* e, int32_t n, const int32_t* thr_rows, const kt_status* status);

/* ---- reconcile: [Cluster]ThrottleController.reconcile, aggregation part (throttle_controller.go:103-133,
 *      clusterthrottle_controller.go:106-136) for EVERY responsible throttle in one pass:
 *      affectedPods (:221-246 / :224-270) -> used = fold ResourceAmount.Add (resource_amount.go:91-110)
 *      -> CalculateThreshold(now) (throttle_types.go:65-106) -> throttled = IsThrottled(used, true)
 *      (resource_amount.go:127-159).  kt_reconcile_launch = aggregate + finalize on one GPU (it leaves the partial
 *      buffer zeroed: the sums are consumed by the finalize, the next scan starts from a clean buffer).
 *      Multi-GPU (pods row-sharded, throttles replicated): kt_aggregate_launch, all-reduce(sum, int64)
 *      over the buffer kt_partial_used_buffer returns, then kt_finalize_launch. -------------------------- */
#define KT_RECONCILE_APPLY 0x1u /* store the new status as the engine's stored status (UpdateStatus) */
int32_t kt_reconcile_launch(kt_engine* e, int64_t now_s, int32_t now_ns, uint32_t flags, void* stream);
/* The same for a SUBSET of throttle rows — the reference reconciles ONE throttle per workqueue key
 * (pkg/controllers/throttle_controller.go:84-133, controller.go:89-122): only the listed rows resolve
 * CalculateThreshold(now), get a new `used` / `throttled` and (with KT_RECONCILE_APPLY) have their stored status
 * replaced; every other row keeps its stored status and reports it unchanged (calc_at_nonzero = 0, no next-override
 * instant).  The scan itself still covers all throttles (it is one pass over the pods either way). */
int32_t kt_reconcile_rows_launch(kt_engine* e, int64_t now_s, int32_t now_ns, uint32_t flags, int32_t n,
                                 const int32_t* throttle_rows, void* stream);
int32_t kt_aggregate_launch(kt_engine* e, void* stream);
int32_t kt_partial_used_buffer(kt_engine* e, void** device_ptr, int64_t* n_int64);
/* Optional: aggregate into / finalize from a CALLER-owned device buffer of >= n_int64 words (e.g. the
 * storage of a framework tensor handed to RCCL) instead of the engine's own. NULL restores the default. */
int32_t kt_use_partial_buffer(kt_engine* e, void* device_ptr, int64_t n_int64);
int32_t kt_finalize_launch(kt_engine* e, int64_t now_s, int32_t now_ns, uint32_t flags, void* stream);
/* ---- multi-GPU without any framework: one process (or thread) per GPU, each with its own engine over its shard of
 *      the pod rows and a replica of the throttles.  The only exchange of a reconcile is the sum of the partial-`used`
 *      buffers; kt_comm_* runs it as ONE RCCL all-reduce (ncclInt64, ncclSum; xGMI between the GPUs of a node) on the
 *      stream the kernels run on:   kt_aggregate_launch -> kt_comm_allreduce_partial -> kt_finalize_launch.
 *      Rank 0 creates the 128-byte id and hands it to the other ranks by any channel the host has (the Go side would
 *      use its own RPC / a ConfigMap); librccl.so is loaded on the first kt_comm_* call. ------------------------------ */
#define KT_COMM_ID_BYTES 128
int32_t kt_comm_unique_id(void* out_id128);
int32_t kt_comm_init(kt_engine* e, int32_t rank, int32_t world, const void* id128);
/* in-place sum over all ranks of this engine's partial buffer (the caller's, if kt_use_partial_buffer set one) — exactly
 * the words the preceding kt_aggregate_launch filled.  KT_ERR_NOT_READY when no aggregate is pending, or when throttles /
 * namespaces changed since it ran (the ranks would disagree on the word count): aggregate again. */
int32_t kt_comm_allreduce_partial(kt_engine* e, void* stream);
/* A caller that sums the partial buffers with its OWN collective (kt_partial_used_buffer / kt_use_partial_buffer) declares
 * the number of ranks here, so that the engine's exact-range guard covers the sum over all of them (2^60 per rank up to 4
 * ranks, 2^62 / world beyond); kt_comm_init does it by itself. */
int32_t kt_set_exchange_world(kt_engine* e, int32_t world);
/* Wide sums (two blocks of limb sums, see kt_reconcile_fetch_used_hi) change the LAYOUT of the exchanged buffer, and
 * whether a rank's requests leave int64 is a local fact: with more than one rank an engine never goes wide by itself
 * (the aggregate answers KT_ERR_OVERFLOW_RISK instead, as rounds 1-2 did) — the host switches EVERY rank with
 * mode = 1 (always two blocks; exact either way), mode = 0 returns to the per-engine decision.  Not for incremental engines. */
int32_t kt_set_wide_sums(kt_engine* e, int32_t mode);
/* Words (int64) of the aggregate that is pending, and whether they are the two-block form: what a caller's own
 * collective has to sum.  KT_ERR_NOT_READY without a pending kt_aggregate_launch. */
int32_t kt_partial_words(kt_engine* e, int64_t* n_int64, int32_t* wide);
/* The layout of one throttle's row of the partial buffer, for n_dims resource dimensions (int64 words): `stride` words per
 * throttle row; the summed request values start at off_values (n_dims words), the per-key contributor counts — presence
 * travels as counts so that it can be summed — at off_presence (n_dims words), then the counted pods at off_pods and the
 * pods whose selector evaluation failed at off_errors (one word each).  With wide sums the buffer holds two such blocks of
 * throttle_rows x stride words (low 32-bit limbs, then the rest: kt_partial_words).  No engine and no device needed: a host
 * that exchanges the buffer with its own collective — or a test that builds one by hand — lays it out by THIS query, which
 * returns what the kernels compile against (partial_stride / partial_off_* in csrc/kt_device.h). */
int32_t kt_partial_layout(int32_t n_dims, int32_t* stride, int32_t* off_values, int32_t* off_presence, int32_t* off_pods,
                          int32_t* off_errors);
int32_t kt_comm_destroy(kt_engine* e);

/* Copies the last reconcile's result for throttle rows [0, n) into caller arrays (synchronises). */
int32_t kt_reconcile_fetch(kt_engine* e, int32_t n, const kt_status* out);
/* resource.Quantity never overflows (Add promotes to big decimals, pkg/resourcelist/resourcelist.go:48-54).  When the
 * requests of the pods an engine holds add up beyond int64 at the scale they were fed with, the reconcile sums their
 * low 32-bit limbs and the rest separately (two scans, both blocks cross the exchange: kt_partial_used_buffer then
 * reports twice the words) and kt_finalize joins them in 128 bits: `used`, the throttled flags and the check that
 * follows are exact up to 2^124.  kt_reconcile_fetch returns the LOW 64 bits of every value, this call the HIGH 64 bits
 * of rows [0, n) x n_dims (two's complement; out_any_wide, nullable: some value really left int64).  A status fed back
 * through kt_set_status / kt_upsert_throttles is int64.  Not available to KT_VARIANT_INCREMENTAL engines and
 * kt_admit_launch (KT_ERR_OVERFLOW_RISK / KT_ERR_UNSUPPORTED there). */
int32_t kt_reconcile_fetch_used_hi(kt_engine* e, int32_t n, int64_t* out_hi, int32_t* out_any_wide);
/* ThrottleSpecBase.NextOverrideHappensIn(now) (throttle_types.go:37-63) of the last reconcile for throttle rows
 * [0, n), as the INSTANT of the next override boundary (the controller's enqueueAfter delay is instant - now,
 * throttle_controller.go:201-208); has[i] = 0 when nothing lies ahead or the row was not reconciled. Synchronises. */
int32_t kt_reconcile_fetch_next_override(kt_engine* e, int32_t n, int64_t* next_s, int32_t* next_ns, uint8_t* has);

/* ---- check: KubeThrottler.PreFilter (plugin.go:148-215) = ThrottleController.CheckThrottled
 *      (throttle_controller.go:349-397) + ClusterThrottleController.CheckThrottled
 *      (clusterthrottle_controller.go:378-425) -> [Cluster]Throttle.CheckThrottledFor
 *      (throttle_types.go:128-153, clusterthrottle_types.go:30-55) for n pods at once against the stored
 *      status + reserved amounts.  pod_rows == NULL checks rows [0, n).  on_equal is the
 *      isThrottledOnEqual argument (PreFilter passes false). ------------------------------------------- */
#define KT_CHECK_STATUS_MATRIX 0x1u /* also produce the n x throttle_rows status matrix (parity / reason strings) */
int32_t kt_check_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                        void* stream);
/* The PreFilter sweep of EVERY pod row against the stored status and the reconcile of every throttle as ONE pass over the
 * pod tables: what a host that re-evaluates the whole cluster calls instead of kt_check_launch(all rows) followed by
 * kt_reconcile_launch.  Results (kt_check_fetch for rows [0, pod rows in use), kt_reconcile_fetch) are bit for bit those
 * of that pair: the verdicts are PreFilter's against the status stored BEFORE this reconcile (plugin.go:148-215 reads the
 * informer cache the controllers write later), the new status is reconcile's (throttle_controller.go:84-133).  One
 * selector scan per pod instead of two where the program allows it (one index chunk, no slow list, requests that pack);
 * otherwise the two launches run one after the other inside the call.  flags: KT_RECONCILE_APPLY. */
int32_t kt_sweep_launch(kt_engine* e, int64_t now_s, int32_t now_ns, uint32_t flags, int32_t on_equal, void* stream);
/* out_summary [n] ; out_status [n][n_throttle_rows] (nullable; needs KT_CHECK_STATUS_MATRIX), where
 * n_throttle_rows = 1 + highest throttle row ever upserted (kt_throttle_rows). Synchronises. */
int32_t kt_check_fetch(kt_engine* e, int64_t n, uint64_t* out_summary, uint8_t* out_status);
/* kt_check_launch + kt_check_fetch as ONE critical section on the engine's own stream (out_status nullable: no
 * matrix is produced then).  This is the form a PreFilter shim calls when other threads use the engine concurrently
 * (Unreserve from binding goroutines plugin.go:240-257, reconcile workers controller.go:52-122): results of a
 * separate launch / fetch pair may be replaced by another thread's launch in between. */
/* With n <= 8 and out_status == NULL (one PreFilter call: the verdict; the status row is only needed to word the reasons
 * of a blocked pod) the call takes the few-pod path: it holds the engine lock SHARED, launches one wave per index chunk
 * on a high-priority stream of its own and spins on a sequence number the kernel writes to pinned host memory behind
 * the summary words — no copy, no stream synchronisation, and no waiting for the kernels of a reconcile another thread
 * launched (while those run it sees the status as stored before that reconcile: the CheckRecs are double-buffered). */
int32_t kt_check(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint64_t* out_summary,
                 uint8_t* out_status);
/* affectedPods for pods the caller names — pkg/controllers/throttle_controller.go:221-246, clusterthrottle_controller.go:224-270
 * restricted to n pod rows x m throttle rows: out[i * m + j] = 1 when throttle_rows[j]'s selector (its namespace side
 * included) matches pod_rows[i] as the engine holds it now, 0 when not, KT_STATUS_ERROR when the pod's PreFilter is an
 * error (unknown namespace object, an unconvertible selector reached first).  The caller adds shouldCountIn
 * (throttle_controller.go:217-219: it knows scheduler name and node of its pods).  This is what unreserveAffectedPods
 * (throttle_controller.go:135-155) iterates over: behind a reconcile, a reservation is released only for a pod that is in the
 * reconciled throttle's affected set — a pod whose labels changed after Reserve is not.  Cost: one small check launch, on the
 * engine's ONE check slot: a kt_check_launch that was pending is dropped (its kt_check_fetch answers KT_ERR_NOT_READY; kt_check,
 * the one-call form a shim uses beside other threads, is not affected). */
int32_t kt_affected_pods(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t m, const int32_t* throttle_rows, uint8_t* out);
/* ---- sequential admission with reservation: for i = 0..n-1 IN ORDER,
 *      PreFilter(pod_rows[i]) (plugin.go:148-215) and, on Success, Reserve(pod_rows[i]) (plugin.go:217-239 ->
 *      [Cluster]ThrottleController.Reserve, throttle_controller.go:271-300 -> reservedResourceAmounts.addPod,
 *      reserved_resource_amounts.go:66-77): ResourceAmountOfPod(pod) is added to the reserved amount of every
 *      throttle that affects the pod, and the following pods of the queue are checked against it.  One launch
 *      replaces n PreFilter + Reserve round trips.  Results are read with kt_check_fetch: out_summary[i] /
 *      out_status[i][*] are what PreFilter returned for pod i AT ITS TURN.
 *      flags: KT_ADMIT_COMMIT keeps the resulting reserved amounts in the engine (as if Reserve had been called
 *      for every admitted pod; read them back with kt_fetch_reserved); without it the call is a dry run.
 *      Every admitted pod ADDS its amount: the reference's cache is a map keyed by pod (reserved_resource_amounts.go:
 *      130-135), so a pod whose amount is already part of the reserved totals, or that occurs twice in the queue, must
 *      not be in it — the caller ends the queue there and takes that pod through kt_check + its own map (the C++ plugin
 *      mirror's AdmitQueue does exactly that).
 *      Limit: n x throttle_rows <= 2^31 (the status matrix).  The reserved amounts of all throttles live in LDS while
 *      they fit (throttle_rows x (8 x n_dims + 16) <= ~156 KB), beyond that in HBM (same results, L2 latency per
 *      pod). ---------------------------------------------------------------------------------------------------- */
#define KT_ADMIT_COMMIT 0x1u
int32_t kt_admit_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                        void* stream);
/* ---- gang admission: the queue cut into CONSECUTIVE gangs that are admitted all or nothing (a batch / ML job whose pods
 *      only run together).  Gang g = queue positions [gang_off[g], gang_off[g + 1]); for g = 0..n_gangs-1 IN ORDER:
 *      (1) every member, in order, gets PreFilter (plugin.go:148-215) against the stored status plus the CURRENT reserved
 *          amounts — those of admitted members of its own gang included — and, on Success, Reserve (plugin.go:217-239),
 *          exactly as kt_admit_launch does;
 *      (2) all members are evaluated, also behind one that failed: each reports what it met at its turn;
 *      (3) the gang is admitted iff every member's verdict is Success (an Error verdict, an invalid pod row or a pod
 *          affected by more throttles than the kernel's list holds fails its gang).  Otherwise every member that reserved
 *          gets Unreserve (plugin.go:240-257 -> [Cluster]ThrottleController.UnReserve -> reservedResourceAmounts.removePod,
 *          reserved_resource_amounts.go:79-90) on every throttle (and every page) before the next gang starts: the reserved
 *          amounts are then exactly what they were before the gang — values, pod count, WHICH resource names are present
 *          and whether a count is present (the reference recomputes the total over the remaining pod map,
 *          reserved_resource_amounts.go:148-156: a name only a rolled-back pod brought in disappears again);
 *      (4) out_summary[i] / out_status[i][*] (kt_check_fetch) stay what PreFilter returned at the pod's turn, also in a
 *          gang that is rolled back; out_admitted[g] (kt_admit_gangs_fetch) = 1 admitted, 0 rolled back;
 *      (5) KT_ADMIT_COMMIT keeps the final reserved amounts, without it the call is a dry run.
 *      A gang of one pod is kt_admit_launch's admission of that pod (a failed single pod reserved nothing).  One launch:
 *      the rollback runs in the kernel that walks the queue (kt_admit_gangs, the gang form of kt_admit), on the state it
 *      holds in LDS; it costs the entries the gang touched, not a copy of the state.
 *      gang_off: [n_gangs + 1], gang_off[0] == 0, gang_off[n_gangs] == n, strictly increasing — an empty gang, offsets
 *      that decrease or do not span the queue are KT_ERR_INVALID_ARGUMENT before anything is launched; n_gangs == 0 only
 *      with n == 0.  Everything kt_admit_launch refuses is refused alike (wide `used`, n x throttle_rows > 2^31), and its
 *      duplicate-pod rule holds: a pod whose amount is already reserved, or that is named twice, must not be in the
 *      queue (the C++ plugin mirror's AdmitGangs takes such a gang through PreFilter / Reserve / Unreserve per member).
 *      The gang form keeps 4 x throttle_rows more bytes of state per page, and 4 x throttle_rows once, than kt_admit_launch
 *      (the LDS / HBM crossover of kt_admit_launch itself is unchanged).
 *      kt_admit_gangs_fetch synchronises; KT_ERR_NOT_READY without a pending gang launch (a later kt_admit_launch /
 *      kt_paged_admit* on the engine drops it). -------------------------------------------------------------------------- */
int32_t kt_admit_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                              int32_t on_equal, uint32_t flags, void* stream);
int32_t kt_admit_gangs_fetch(kt_engine* e, int64_t n_gangs, uint8_t* out_admitted);
/* ---- elastic gangs: a gang is admitted once its QUORUM of members fits (Coscheduling's PodGroup.minMember, Volcano's
 *      minAvailable, Kueue's partial admission), and a member can be made mandatory (a per-task minAvailable: the launcher of an
 *      MPI job, the head of a Ray cluster).  No prefix or subset of a gang can be judged without the walk — each admitted member
 *      reserves against the throttles the later ones meet — so the quorum is decided where the walk runs.  Gangs as in
 *      kt_admit_gangs_launch; min_members [n_gangs]; member_flags [n], nullable (no member is required), bit 0 =
 *      KT_GANG_MEMBER_REQUIRED.  For g = 0..n_gangs-1 IN ORDER:
 *      (1)  the walk is kt_admit_gangs_launch's, rules (1), (2) and (4) unchanged: every member, in order, against the stored
 *           status plus the CURRENT reserved amounts, Reserve on Success; every member is evaluated, also behind one that failed;
 *           out_summary[i] / out_status[i][*] (kt_check_fetch) are what PreFilter returned at the pod's turn;
 *      (2)  a member SUCCEEDS iff its verdict at its turn is Success — an Error verdict, an invalid pod row or a pod affected by
 *           more throttles than the kernel's list holds does not;
 *      (3)  gang g is admitted iff at least min_members[g] members succeeded AND every member whose flag byte has
 *           KT_GANG_MEMBER_REQUIRED succeeded;
 *      (4)  in an admitted gang the members that succeeded stay reserved, the others never reserved; out_members[g]
 *           (kt_admit_gangs_elastic_fetch) is the number that stay, at least 1;
 *      (5)  a gang that is not admitted is rolled back exactly as rule (3) of kt_admit_gangs_launch describes — values, pod count,
 *           which names are present and whether a count is present — and out_members[g] = 0;
 *      (6)  no per-pod output beyond the existing ones is needed: member i of gang g is in iff out_members[g] > 0 and its
 *           summary word says Success;
 *      (7)  KT_ADMIT_COMMIT keeps the final reserved amounts, without it the call is a dry run;
 *      (8)  with min_members[g] == size of g for every gang and member_flags == NULL, and with every member flagged required at
 *           any min_members, the call is kt_admit_gangs_launch byte for byte: status, summary, reserved amounts, and
 *           out_members[g] > 0 where out_admitted[g];
 *      (9)  a gang of one pod with min_members = 1 is kt_admit_launch's admission of that pod;
 *      (10) refused before anything is launched, in this order: every gang_off defect kt_admit_gangs_launch refuses;
 *           min_members == NULL with n_gangs > 0; a min_members[g] outside [1, size of g] (KT_ERR_INVALID_ARGUMENT, the message
 *           names the gang and both numbers); a flag byte with a bit other than bit 0 (KT_ERR_INVALID_ARGUMENT, the message names
 *           the queue position); then everything kt_admit_launch refuses.  A refused call leaves the reserved amounts alone, with
 *           KT_ADMIT_COMMIT too;
 *      (11) the call uses the gang slot of kt_admit_gangs_launch: behind it kt_admit_gangs_elastic_fetch answers the counts and
 *           kt_admit_gangs_fetch the bytes (1 where the count is above 0); behind a plain kt_admit_gangs_launch the elastic fetch
 *           answers KT_ERR_NOT_READY (no counts were kept);
 *      (12) an engine without throttle rows decides on the host from the summaries, with the same rule; n == 0 is KT_OK and
 *           launches nothing;
 *      (13) the duplicate-pod rule of kt_admit_launch holds (the C++ plugin mirror's AdmitElasticGangs takes such a gang through
 *           PreFilter / Reserve / Unreserve per member).
 *      One launch: kt_admit_gangs_elastic, the third form of kt_admit's walk; it keeps the state of the gang form and no more, and
 *      the caller's arrays are not referenced after return. ----------------------------------------------------------------- */
#define KT_GANG_MEMBER_REQUIRED 0x1u
int32_t kt_admit_gangs_elastic_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                      const int64_t* min_members /* [n_gangs] */, const uint8_t* member_flags /* [n], nullable */,
                                      int32_t on_equal, uint32_t flags, void* stream);
int32_t kt_admit_gangs_elastic_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_members);
/* ---- headroom: how many copies of a pod the throttles still admit — what a Deployment, Job or autoscaler asks before it
 *      creates pods.  headroom(pod, cap, on_equal) is the number of LEADING Success verdicts kt_admit_launch returns, as a dry
 *      run (no KT_ADMIT_COMMIT), for the queue [pod] * cap against the stored status and the current reserved amounts:
 *      PreFilter (plugin.go:148-215) and, on Success, Reserve (plugin.go:217-239 -> [Cluster]ThrottleController.Reserve,
 *      throttle_controller.go:271-300 -> reservedResourceAmounts.addPod, reserved_resource_amounts.go:66-77), copy after copy —
 *      every copy adds ResourceAmountOfPod(pod) once to every throttle that affects the pod, and the next copy's
 *      CheckThrottledFor sees it in steps 3 and 4 (throttle_types.go:142-150).  out_copies[i] lies in [0, cap].
 *      out_limiting[i] is the lowest throttle row whose status is not KT_STATUS_NOT_THROTTLED in the row PreFilter returns
 *      for the first copy that is NOT admitted; -1 when all cap copies are admitted.  A pod whose PreFilter is an Error
 *      (selector / namespace error, plugin.go:154-168) and an invalid pod row report 0 copies and -1; a pod no throttle
 *      affects reports cap and -1.  The copies are FURTHER pods of the same shape: a pod whose own amount is already part of
 *      the reserved totals is answered as the totals stand.
 *      The number has a closed form per (pod, throttle, resource name) — the minimum over the affecting throttles, and there
 *      over the pod count and every requested name, of the copies that amount alone lets through — so nothing is walked in
 *      sequence: one kt_check launch with the status matrix (which throttles affect which pod) and one launch of kt_headroom
 *      (csrc/kt_kernels_headroom.hip), one wave per pod.  The call never changes reserved amounts, stored status or a pending
 *      reconcile.
 *      pod_rows == NULL: rows [0, n); n == 0 is KT_OK and launches nothing.  cap outside [1, KT_HEADROOM_MAX_CAP] is
 *      KT_ERR_INVALID_ARGUMENT; n x throttle_rows > 2^31 (the status matrix) KT_ERR_OUT_OF_RANGE; a stored `used` wider than
 *      int64 KT_ERR_UNSUPPORTED, as for kt_admit_launch.
 *      kt_headroom_fetch synchronises (out_limiting nullable); KT_ERR_NOT_READY without a pending kt_headroom_launch.  The
 *      launch uses the engine's ONE check slot: a kt_check_launch that was pending is dropped (as with kt_affected_pods), and
 *      a later kt_check_launch / kt_check / kt_sweep_launch / kt_admit_launch / kt_admit_gangs_launch / kt_paged_admit* /
 *      kt_affected_pods on the engine drops a pending kt_headroom_launch.  The one exception is a kt_check that the few-pod
 *      path serves (at most 8 named pods, no status matrix: KT_COUNTER_FEW_CHECKS): it runs beside the slot on buffers of its
 *      own, and a pending kt_headroom_launch, like a pending kt_check_launch, stays fetchable behind it. ------------------ */
#define KT_HEADROOM_MAX_CAP 0x7FFFFFFF
int32_t kt_headroom_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, int64_t cap, void* stream);
int32_t kt_headroom_fetch(kt_engine* e, int64_t n, int64_t* out_copies, int32_t* out_limiting /* nullable */);
/* ---- headroom, for gangs: how many copies of a whole gang the throttles still admit — what a batch controller asks before it
 *      creates replicas of a job that scales in units of a gang (one launcher plus N workers, a JobSet replica, a Ray worker
 *      group).  Gang g is pod_rows[gang_off[g] .. gang_off[g + 1]), as in kt_admit_gangs_launch.  headroom_gangs(gang, cap,
 *      on_equal) is the number of LEADING admitted gangs in a dry kt_admit_gangs_launch (no KT_ADMIT_COMMIT) over a queue of cap
 *      consecutive copies of the gang, against the stored status and the current reserved amounts.  Before the first gang that
 *      is rolled back every earlier copy was admitted in full, so copy j meets on throttle t the stored reserved row of t plus
 *      j x A_t, A_t = what one admitted copy reserves on t: a pod count of one per member t affects, the value of every resource
 *      name such a member carries, and the presence of all those names, zero-valued ones included; from copy 1 on the count
 *      and those names are present in `reserved`.  Given that, throttles are independent: the answer is the minimum over the
 *      affecting throttles of h_t, the leading copies t alone lets through.  With non-negative requests passes_t(j) is monotone
 *      in j, so h_t is found by search, and the judge of every probe is the gang walk of kt_admit_gangs itself.
 *      out_copies[g] lies in [0, cap].  out_blocker[g] is the queue position (in pod_rows, as kt_forecast_gangs_fetch's
 *      blockers) of the first member of copy out_copies[g] — the first copy that is not admitted — whose verdict at its turn is
 *      not Success; -1 when all cap copies are admitted.  out_limiting[g] is the lowest throttle row whose status is not
 *      KT_STATUS_NOT_THROTTLED in the row PreFilter returns to that member at its turn; -1 when there is no blocker or the
 *      blocker's verdict is an Error.  A gang with a member whose PreFilter is an Error, or whose row is invalid, reports 0
 *      copies; its blocker is the first position of copy 0 that is not Success (an earlier member a throttle stops counts).  A
 *      gang no throttle affects reports cap, -1, -1.  Gangs are judged independently, each against the stored reserved amounts:
 *      a pod may occur in several gangs; the copies are FURTHER pods of the same shapes.  A gang of one pod is
 *      kt_headroom_launch on that pod, byte for byte, in out_copies and out_limiting.
 *      One kt_check launch with the status matrix over the members, then one launch of kt_headroom_gangs
 *      (csrc/kt_kernels_headroom_gangs.hip): one wave per gang, lane = a candidate number of copies, a 64-ary search per
 *      throttle (six rounds at the most for cap = 2^31 - 1).  The call never changes reserved amounts, stored status or a
 *      pending reconcile.
 *      Refused before anything is launched, in this order: every gang_off defect kt_admit_gangs_launch refuses and a pod named
 *      twice within one gang (KT_ERR_INVALID_ARGUMENT), a pod row outside the table (KT_ERR_OUT_OF_RANGE), cap outside
 *      [1, KT_HEADROOM_MAX_CAP] (KT_ERR_INVALID_ARGUMENT), n x throttle_rows > 2^31 (KT_ERR_OUT_OF_RANGE), a stored `used` wider
 *      than int64 (KT_ERR_UNSUPPORTED), and an engine that has been fed a negative request (KT_ERR_UNSUPPORTED: the search rests
 *      on sums that only grow; kt_headroom_launch keeps serving such an engine pod by pod; the mark is set by an ACCEPTED pod batch
 *      and stays when that pod is deleted or overwritten — only kt_load_snapshot clears it).  n == 0 is KT_OK and launches
 *      nothing.
 *      Slots: the engine's ONE check slot, exactly as kt_headroom_launch uses it.  A pending kt_headroom_launch and a pending
 *      kt_headroom_gangs_launch replace each other, and a fetch of the other kind answers KT_ERR_NOT_READY.
 *      kt_headroom_gangs_fetch synchronises. ------------------------------------------------------------------------------ */
int32_t kt_headroom_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int32_t on_equal,
                                 int64_t cap, void* stream);
int32_t kt_headroom_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_copies, int32_t* out_limiting /* nullable */,
                                int64_t* out_blocker /* nullable */);
/* ---- preempt: the shortest victim prefix that lets a blocked pod through — what priority preemption asks, and what the
 *      scheduler's own preemption never asks of throttles (PreFilter answers UnschedulableAndUnresolvable).
 *      A pod is COUNTED when VALID & SCHED_MATCH & SCHEDULED & !FINISHED (throttle_controller.go:217-219).  For preemptor
 *      p = pod_rows[i] and the caller-ordered candidates c_0 .. c_{m-1} = cand_rows (typically by ascending priority; the engine
 *      has no priority field and needs none), state S_k is the cluster in which c_0 .. c_{k-1} no longer exist and every
 *      responsible throttle has been reconciled at `now`: affectedPods -> used = fold ResourceAmount.Add, CalculateThreshold(now),
 *      throttled = IsThrottled(used, true) (throttle_controller.go:116-133, throttle_types.go:65-106, resource_amount.go:127-159).
 *      Reserved amounts are unchanged; a throttle whose reconcile reports an error keeps its stored status in every S_k, as
 *      kt_reconcile_fetch's `error` byte defines.
 *      out_prefix[i] is the smallest k in [0, m_eff] for which PreFilter(p) (plugin.go:148-215) in S_k is Success: 0 = p already
 *      passes against a fresh reconcile; KT_PREEMPT_NONE = no prefix helps (pod-requests-exceeds-threshold, candidates exhausted,
 *      a p whose PreFilter is an Error, an invalid pod row).  m_eff: the list is CUT before the first candidate whose own check
 *      row is an Error or whose row is invalid — deleting such a pod could change a throttle's reconcile error, which this query
 *      does not model.  Candidates that are not counted, or that no throttle affecting p matches, contribute nothing; they may
 *      be in the list and are never in the victim mask.
 *      out_victims[i][j] (nullable, [n][n_cand]) is 1 iff j < out_prefix[i], c_j is counted and at least one throttle that affects
 *      p matches c_j: deleting exactly the masked pods gives p the same verdict as deleting the whole prefix (no assumption
 *      about the signs of requests).  Row i is all zero when out_prefix[i] <= 0.
 *      Presence is exact (resource_amount.go:91-110,151-155): a resource name stays present in `used` only while a remaining
 *      counted pod carries it — decided by exact contributor counts, not by stored presence bits — and the pod count of `used`
 *      is present only while a pod is counted.  Every k is evaluated (no bisection): one kt_check launch with the status matrix
 *      over pod_rows ++ cand_rows, an aggregate and a dry finalize at `now` of the call's own, and one launch of kt_preempt
 *      (csrc/kt_kernels_preempt.hip), one wave per preemptor, lane = candidate position.  The aggregate is the dense scan (its
 *      partial rows count every contributor; the indexed scan of a rescanning engine only marks names as seen): its cost grows
 *      with pods x throttles.
 *      The call is a dry run: stored status and reserved amounts are not changed.
 *      Refused before anything is launched: n_cand < 0, a preemptor that is also a candidate, a candidate named twice, a missing
 *      row array (KT_ERR_INVALID_ARGUMENT); n x throttle_rows, n_cand x throttle_rows or their sum — the bytes of the one check's
 *      matrix — > 2^31 (KT_ERR_OUT_OF_RANGE); `used` wider than int64, a KT_VARIANT_INCREMENTAL engine, an exchange world above 1
 *      (KT_ERR_UNSUPPORTED).  Where pod batches since the last aggregate leave it unknown whether `used` still fits int64, the one
 *      thing that runs before the refusal is the kernel that sums the |requests|; the check slot, the reconcile report and the
 *      result buffers are untouched by a refused call.  n == 0 is KT_OK and launches
 *      nothing; n_cand == 0 answers 0 or KT_PREEMPT_NONE per pod.  kt_preempt_fetch synchronises; KT_ERR_NOT_READY without a
 *      pending kt_preempt_launch.
 *      Slots: the launch uses the engine's ONE check slot exactly as kt_headroom_launch does — a pending kt_check_launch or
 *      kt_headroom_launch is dropped, and a later kt_check_launch / kt_check (other than the few-pod path) / kt_sweep_launch /
 *      kt_admit* / kt_headroom_launch / kt_affected_pods drops a pending kt_preempt_launch.  Its dry finalize writes the reconcile
 *      result buffers: the report of a pending kt_reconcile_launch / kt_finalize_launch is dropped (kt_reconcile_fetch answers
 *      KT_ERR_NOT_READY; a status stored with KT_RECONCILE_APPLY stays stored).  Its aggregate runs beside the partial buffer:
 *      a pending kt_aggregate_launch keeps its sums.  The results live in buffers of their own, so a kt_reconcile_launch issued
 *      on the same stream after the launch leaves it fetchable.
 *      More than KT_MAX_DIMS resource names: kt_paged_preempt.  Out of scope: several ranks (the reprieve pass that shrinks the
 *      victim set further is kt_preempt_reprieve_launch below). --------------------------------------------------------- */
#define KT_PREEMPT_NONE (-1)
int32_t kt_preempt_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows, int64_t now_s,
                          int32_t now_ns, int32_t on_equal, void* stream);
int32_t kt_preempt_fetch(kt_engine* e, int64_t n, int64_t* out_prefix, uint8_t* out_victims /* [n][n_cand], nullable */);
/* ---- preempt, reprieved: the prefix of kt_preempt_launch with its victim mask shrunk to a minimal set — the second half of
 *      what kube-scheduler's selectVictimsOnNode does for every preemption: starting from "all potential victims removed", the
 *      victims are put back one by one, most important first, and each stays back as long as the preemptor still fits.
 *      Notation as for kt_preempt_launch.  For preemptor p let k = out_prefix and M the prefix victim mask defined there.  k <= 0:
 *      the row is all zero, as there.  Otherwise V = M, and for j = k-1, k-2, .., 0 in that order, for each j with M[j] = 1, let
 *      V' = V \ {c_j}: state S(V') is the cluster in which exactly the pods of V' no longer exist and every responsible throttle
 *      has been reconciled at `now` (reserved amounts unchanged; a throttle whose reconcile is an error keeps its stored status, the
 *      rule of S_k).  If PreFilter(p) is Success in S(V'), V := V' — c_j is reprieved — otherwise c_j stays a victim.
 *      out_victims[i][j] = 1 iff c_j is in V at the end; out_prefix is what kt_preempt_launch reports.
 *      Presence in `used` is exact, as in the prefix query: putting a pod back increments the contributor count of every resource
 *      name it carries, a name is present iff its count is positive, and the pod count of `used` is present iff a pod is counted.
 *      The definition is operational — the walk, step by step, with no monotonicity assumption — so requests of either sign are
 *      answered as the walk answers them.  For non-negative requests the result is minimal: putting any single remaining victim
 *      back makes p fail; and the last masked candidate is never reprieved (the prefix is the shortest).
 *      The call is kt_preempt_launch followed, on the same stream, by ONE launch of kt_preempt_reprieve
 *      (csrc/kt_kernels_reprieve.hip) that rewrites the victim bytes in place: one wave per preemptor, lanes = the reconciled
 *      throttles that affect it, each holding the `used` of its throttle in the current state (in LDS; a list that outgrows it
 *      lives in a workspace of the engine's own, grown like the result buffers only once the stream of an unfetched launch has
 *      drained).  A preemptor with prefix <= 0 costs one load.  The walk is sequential per preemptor and independent across them.
 *      m_eff, the list cut, every refusal and its code, "a refused call leaves the check slot, the reconcile report and the
 *      result buffers alone", n == 0 and n_cand == 0, and the slot rules are those of kt_preempt_launch: the two launches share
 *      the one pending result, fetched with kt_preempt_fetch — a later launch of either kind replaces it.
 *      More than KT_MAX_DIMS resource names: kt_paged_preempt with KT_PREEMPT_REPRIEVE.  Out of scope: several ranks. ---- */
int32_t kt_preempt_reprieve_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows, int64_t now_s,
                                   int32_t now_ns, int32_t on_equal, void* stream);
/* ---- preempt, for gangs: the shortest victim prefix that lets a WHOLE gang in — where kt_preempt_launch and kt_admit_gangs_launch
 *      meet.  The maximum of the members' own prefixes is not the answer: each admitted member RESERVES against the throttles the
 *      later members meet (plugin.go:217-239, reservedResourceAmounts.addPod).
 *      Notation as for kt_preempt_launch: counted pods, the candidates c_0 .. c_{m-1} = cand_rows, state S_k, the m_eff cut, "a
 *      throttle whose reconcile is an error keeps its stored status in every S_k", exact presence from contributor counts.  Gang g
 *      is the queue positions [gang_off[g], gang_off[g + 1]) of pod_rows, as in kt_admit_gangs_launch.  Gangs are judged
 *      INDEPENDENTLY of each other, each against the stored reserved amounts: a query about alternatives, not a queue (a pod may be
 *      a member of several gangs).
 *      out_prefix[g] is the smallest k in [0, m_eff] for which a dry kt_admit_gangs_launch of the one gang g would admit it with
 *      S_k as the stored status: its members get PreFilter in order, each sees the reserved amounts as stored plus what the earlier
 *      members of its own gang reserved at their turn, and every verdict is Success.  Reserve is exactly kt_admit's: for every
 *      throttle whose byte in the member's matrix row is nonzero the pod's value is added for every name it carries, the presence
 *      word is OR-ed with ALL names it carries (zero-valued ones included), the pod count gets +1 and becomes present.
 *      KT_PREEMPT_NONE: no k works, a member's PreFilter is an Error, or a member's row is invalid.
 *      out_victims[g][j] (nullable, [n_gangs][n_cand]) is 1 iff j < out_prefix[g], c_j is counted and a throttle that affects at
 *      least one member matches c_j; the row is all zero when the prefix is <= 0.
 *      out_blocker[g] (nullable) is the queue position (index into pod_rows) of the first member whose verdict is not Success when
 *      the gang is walked in S_0 — all earlier members were admitted, so the sums it met are exact — and -1 when out_prefix[g] == 0.
 *      A gang of one pod reports exactly what kt_preempt_launch reports for that pod.
 *      The verdict is in closed form and two-dimensional: deleting a prefix lowers `used` by a prefix sum over the candidates,
 *      being admitted raises `reserved` by a prefix sum over the members.  One kt_check launch over pod_rows ++ cand_rows, the
 *      aggregate and dry finalize of kt_preempt_launch, and one launch of kt_preempt_gangs (csrc/kt_kernels_preempt_gangs.hip):
 *      one wave per gang, lane = candidate position, the scans once per throttle and block of 64 candidates, the member loop
 *      wave-uniform.  Every k is evaluated, sums are formed in 128 bits; requests of either sign are answered as the definition
 *      answers them.  The call is a dry run: stored status and reserved amounts are not changed.
 *      Refused before anything is launched: every gang_off defect kt_admit_gangs_launch refuses, a pod named twice within ONE
 *      gang, a member that is also a candidate, a candidate named twice, a missing array, n_cand < 0 (KT_ERR_INVALID_ARGUMENT);
 *      the 2^31 matrix rule of kt_preempt_launch on n, n_cand and their sum (KT_ERR_OUT_OF_RANGE); `used` wider than int64, a
 *      KT_VARIANT_INCREMENTAL engine, an exchange world above 1 (KT_ERR_UNSUPPORTED; the |request| sums kernel runs first where the
 *      sums are unknown).  A refused call leaves the check slot, the reconcile report and every result buffer alone.  n == 0 is
 *      allowed only with n_gangs == 0: KT_OK, nothing is launched.
 *      Slots: the launch uses the check slot and the reconcile report exactly as kt_preempt_launch does, and its result SHARES the
 *      one pending preempt result, as kt_preempt_reprieve_launch does: a later launch of any of the preempt calls replaces it.
 *      kt_preempt_fetch after a gang launch answers KT_ERR_NOT_READY, and so does kt_preempt_gangs_fetch after a plain launch; a
 *      pending kt_forecast_launch stays fetchable.  kt_preempt_gangs_fetch synchronises.
 *      More than KT_MAX_DIMS resource names: kt_paged_preempt_gangs.  Out of scope: several ranks (the reprieve pass that shrinks
 *      a gang's victim set further is kt_preempt_gangs_reprieve_launch below). ------------------------------------------------- */
int32_t kt_preempt_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_cand,
                                const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, void* stream);
int32_t kt_preempt_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_prefix /* [n_gangs], nullable */,
                               uint8_t* out_victims /* [n_gangs][n_cand], nullable */, int64_t* out_blocker /* [n_gangs], nullable */);
/* ---- preempt, for gangs, reprieved: the prefix of kt_preempt_gangs_launch with its victim mask shrunk to a minimal set — what
 *      kt_preempt_reprieve_launch is to kt_preempt_launch.  The members' own reprieved sets do not compose into the gang's answer:
 *      each admitted member reserves against the throttles the later members meet (two members asking 3 each under a threshold of
 *      10 with four running pods of 2: each member alone keeps one victim, the gang needs two).
 *      Notation as for kt_preempt_gangs_launch: counted pods, the candidates c_0 .. c_{m-1}, the m_eff cut, gang g = the queue
 *      positions [gang_off[g], gang_off[g + 1]).  For gang g let k = out_prefix[g] and M the victim mask, exactly as
 *      kt_preempt_gangs_launch reports them.  k <= 0: the row is all zero.  Otherwise V = M, and for j = k-1, k-2, .., 0 in that
 *      order, for each j with M[j] = 1, let V' = V \ {c_j}: state S(V') is the cluster in which exactly the pods of V' no longer
 *      exist and every responsible throttle has been reconciled at `now` (stored reserved amounts unchanged; a throttle whose
 *      reconcile is an error, or that is not valid and responsible, keeps its stored status: the rule of S_k).  If a dry
 *      kt_admit_gangs_launch of the one gang g, with S(V') as the stored status, admits it — members in order, each sees the
 *      stored reservations plus what the earlier members of its gang reserved, every verdict Success; Reserve exactly kt_admit's:
 *      the value of every name carried, the presence of all names carried (zero-valued ones included), count + 1 — then V := V',
 *      c_j is reprieved; otherwise c_j stays a victim.
 *      out_victims[g][j] = 1 iff c_j is in V at the end; out_prefix and out_blocker are what kt_preempt_gangs_launch reports.
 *      Presence in `used` is exact, by contributor counts, as in kt_preempt_reprieve_launch.  The definition is the walk itself,
 *      with no monotonicity assumption: requests of either sign are answered as the walk answers them.  Gangs are judged
 *      independently of each other.  A gang of one pod yields byte for byte what kt_preempt_reprieve_launch yields for that pod.
 *      The call is kt_preempt_gangs_launch followed, on the same stream, by ONE launch of kt_preempt_gangs_reprieve
 *      (csrc/kt_kernels_preempt_gangs_reprieve.hip) that rewrites the victim bytes in place: one wave per gang, lanes = the
 *      reconciled throttles that affect some member, each holding the `used` of its throttle in the current state (in LDS, or in
 *      the engine's reprieve workspace where the list outgrows it) and judging the members in order on it under the reserved
 *      prefix.  A gang with prefix <= 0 costs one load; n_cand == 0 launches no walk.
 *      Every refusal, its code and its order, "a refused call leaves the check slot, the reconcile report and every result buffer
 *      alone", n == 0 only with n_gangs == 0, and the slot rules are those of kt_preempt_gangs_launch.  The result is the one
 *      pending gang result, fetched with kt_preempt_gangs_fetch: a later launch of any of the four preempt calls replaces it; a
 *      pending kt_forecast_launch stays fetchable.
 *      More than KT_MAX_DIMS resource names: kt_paged_preempt_gangs with KT_PREEMPT_REPRIEVE.  Out of scope: several ranks. -- */
int32_t kt_preempt_gangs_reprieve_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_cand,
                                         const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, void* stream);
/* ---- preempt, for elastic gangs: the shortest victim prefix that lets a gang's QUORUM in — what kt_admit_gangs_elastic_launch is
 *      to kt_admit_gangs_launch, asked of kt_preempt_gangs_launch.  That call can only say which victims let the WHOLE gang in; for
 *      an elastic job that evicts too many pods, or is KT_PREEMPT_NONE although one eviction would start the job.
 *      Notation as for kt_preempt_gangs_launch: counted pods, the candidates c_0 .. c_{m-1}, state S_k, the m_eff cut, exact
 *      presence from contributor counts; a throttle whose reconcile is an error, or that is not valid and responsible, keeps its
 *      stored status in every S_k.  Gangs are judged INDEPENDENTLY, each against the stored reserved amounts.  The rule arrays are
 *      those of kt_admit_gangs_elastic_launch: min_members[g] in [1, size of gang g], member_flags[i] per queue position (NULL: no
 *      member is required; bit 0 = KT_GANG_MEMBER_REQUIRED).  flags: 0 or KT_PREEMPT_REPRIEVE.  A dry run.
 *      THE WALK of gang g in a state: the members go in order; each is judged against the state plus what the earlier members that
 *      SUCCEEDED reserved (Reserve is kt_admit's: the value of every name carried, the presence of all names carried, zero-valued
 *      ones included, count + 1); a member that fails reserves nowhere; every member is evaluated, also behind one that failed; a
 *      member whose PreFilter is an Error or whose row is invalid never succeeds; a member is judged on every throttle that affects
 *      it (there is no list capacity).  The state PASSES iff at least min_members[g] members succeed and every required one does.
 *      out_prefix[g]: the smallest k in [0, m_eff] whose S_k passes; KT_PREEMPT_NONE if none does, and if the rule is out of reach:
 *      a required member never succeeds, or size - (members that never succeed) < min_members[g].  The verdict is NOT monotone in k
 *      (a longer prefix can let an optional member in whose reservation shuts a required one out): every k up to the first pass is
 *      evaluated, nothing is bisected.
 *      out_victims[g][j] (nullable, [n_gangs][n_cand]) without the flag: 1 iff j < out_prefix[g], c_j is counted and a throttle that
 *      affects at least one member of g — succeeding or not; the row of an Error member names no throttle — matches c_j.  Deleting
 *      exactly the masked pods gives the success list of S_prefix.  All zero for a prefix <= 0.  With KT_PREEMPT_REPRIEVE: V = M,
 *      and for j = prefix-1 .. 0 over the masked positions c_j is put back (V' = V \ {c_j}) and stays back iff S(V') passes the
 *      rule — S(V') as kt_preempt_gangs_reprieve_launch defines it, the walk above as the judge, nothing assumed about signs.
 *      out_members[g] (nullable): the members that succeed in the final state — S_prefix, or S(V) behind the reprieve; S_0 where
 *      the prefix is KT_PREEMPT_NONE.
 *      out_blocker[g] (nullable): -1 iff out_prefix[g] == 0; otherwise the queue position of the first required member that does
 *      not succeed in S_0, and if there is none, of the first member that does not.
 *      (P1) min_members[g] = size with NULL flags, or every member required: prefix and victims are kt_preempt_gangs_launch's byte
 *           for byte (with the flag: kt_preempt_gangs_reprieve_launch's), out_members = size wherever the prefix is >= 0, and the
 *           blocker is equal for gangs whose members are all valid and not Error.
 *      (P2) a gang of one with min 1: kt_preempt_launch's / kt_preempt_reprieve_launch's prefix and victim row.
 *      (P3) prefix >= 0, members within kt_admit's list capacity: on a second engine that holds the cluster without the final
 *           victims, reconciled at `now` with KT_RECONCILE_APPLY, a dry kt_admit_gangs_elastic_launch of the gang returns
 *           out_members[g].
 *      Refused before anything is launched, in this order: every gang_off defect; the min_members / member_flags refusals of
 *      kt_admit_gangs_elastic_launch with the same codes and messages; a flags bit other than KT_PREEMPT_REPRIEVE
 *      (KT_ERR_INVALID_ARGUMENT); everything kt_preempt_gangs_launch refuses, in its order.  A refused call leaves the check slot,
 *      the reconcile report and every result buffer alone.  n == 0 is allowed only with n_gangs == 0.
 *      Slots are those of kt_preempt_gangs_launch; the result is the third kind of the one pending preempt result: the other
 *      preempt fetches answer KT_ERR_NOT_READY behind this launch and kt_preempt_gangs_elastic_fetch answers the same behind
 *      theirs; a pending forecast stays fetchable.  The rule arrays travel on the launch's stream and are not referenced after
 *      return.  kt_preempt_gangs_elastic_fetch synchronises.
 *      One kt_check launch over pod_rows ++ cand_rows, the aggregate and dry finalize of kt_preempt_launch, and ONE launch of
 *      kt_preempt_gangs_elastic (csrc/kt_kernels_preempt_gangs_elastic.hip): one wave per gang, the union of the members' throttles
 *      as a compact state (in LDS, or in a device workspace where it outgrows it) that candidate c_{k-1} moves from S_{k-1} to S_k,
 *      the members walked in order on it; the reprieve runs in the same kernel.  A candidate that touches no throttle of the union
 *      costs one ballot.  Out of scope: more than KT_MAX_DIMS resource names, several ranks, elastic headroom. ------------------- */
int32_t kt_preempt_gangs_elastic_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                        const int64_t* min_members /* [n_gangs] */, const uint8_t* member_flags /* [n], nullable */,
                                        int64_t n_cand, const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal,
                                        uint32_t flags, void* stream);
int32_t kt_preempt_gangs_elastic_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_prefix /* [n_gangs], nullable */,
                                       uint8_t* out_victims /* [n_gangs][n_cand], nullable */, int64_t* out_members /* [n_gangs], nullable */,
                                       int64_t* out_blocker /* [n_gangs], nullable */);
/* ---- forecast: the first instant at which a blocked pod passes — the one axis no other query looks along.
 *      temporaryThresholdOverrides make every threshold a step function of the clock (throttle_types.go:65-106,
 *      temporary_threshold_override.go:57-70): a pod that PreFilter rejects now may pass when a night-time override begins or a
 *      freeze window ends.  For pod p = pod_rows[i] and the instants t_0 < t_1 < .. < t_{m-1} (inst_s / inst_ns, m = n_inst), state
 *      R_t is the cluster as the engine holds it now with every valid and responsible throttle reconciled at instant t:
 *      affectedPods -> used = fold ResourceAmount.Add, CalculateThreshold(t), throttled = IsThrottled(used, true), and the rule
 *      "calculatedThreshold is replaced only if threshold or messages differ by value, and calculatedAt becomes non-zero only then"
 *      (throttle_controller.go:116-133).  Reserved amounts are unchanged; a throttle whose reconcile reports an error keeps its
 *      stored status in every R_t, as kt_reconcile_fetch's `error` byte defines.  This is exactly what
 *      kt_reconcile_launch(t, KT_RECONCILE_APPLY) followed by kt_check would report if each t were applied to the state as it is
 *      now, and not on top of the previous instant.
 *      out_verdicts[i][k] (nullable, [n][n_inst]) is the KT_VERDICT_* of PreFilter(p) (plugin.go:148-215) in R_{t_k};
 *      out_first[i] is the smallest k whose verdict is KT_VERDICT_SUCCESS, or KT_FORECAST_NONE.  A pod whose PreFilter is an
 *      Error, or whose row is invalid, reports KT_VERDICT_ERROR at every instant and KT_FORECAST_NONE; a pod no throttle affects
 *      reports Success at every instant and 0.  With inst = [now], out_first == 0 exactly where kt_preempt_launch at `now`
 *      reports prefix 0.
 *      Two facts of the reconcile the kernel depends on (finalize_throttle in csrc/kt_kernels_finalize.hip, at its "replace the
 *      stored calculatedThreshold" step):
 *        (1) after a reconcile the check reads status.calculatedThreshold iff the stored calculatedAt was already non-zero or this
 *            reconcile replaces it; it reads spec.threshold otherwise (throttle_types.go:129-132).  A never-reconciled throttle
 *            whose computed threshold equals the empty stored one by value therefore keeps being read through spec.threshold.
 *        (2) the messages fingerprint of CalculateThreshold depends on parse errors only and never on t; the comparison of the
 *            threshold by value does depend on t.
 *      An override is active at t iff begin <= t && (end is zero || t <= end): BOTH ends are inclusive; an override with a parse
 *      error is never active.  The first active override wins per resource name and for the pod count; an active override that
 *      omits a name leaves it unthrottled; without an active override spec.threshold holds.
 *      One kt_check launch with the status matrix over pod_rows, the aggregate and dry finalize (at t_0) of kt_preempt_launch —
 *      the dense scan with exact contributor counts, and the `error` bytes — and one launch of kt_forecast
 *      (csrc/kt_kernels_forecast.hip): one wave per pod, lane = instant position, every instant judged in parallel.
 *      The call is a dry run: stored status and reserved amounts are not changed.
 *      Refused before anything is launched: n_inst < 1, instants that are not strictly ascending, an inst_ns outside [0, 10^9), a
 *      missing array (KT_ERR_INVALID_ARGUMENT); n x throttle_rows or n x n_inst > 2^31 (KT_ERR_OUT_OF_RANGE); `used` wider than
 *      int64, a KT_VARIANT_INCREMENTAL engine, an exchange world above 1 (KT_ERR_UNSUPPORTED; the |request| sums probe runs first
 *      where the sums are not known, as for kt_preempt_launch).  A refused call leaves the check slot, the reconcile report and all
 *      result buffers alone.  n == 0 is KT_OK and launches nothing.  kt_forecast_fetch synchronises; KT_ERR_NOT_READY without a
 *      pending kt_forecast_launch.
 *      Slots: those of kt_preempt_launch — the launch uses the engine's ONE check slot (a pending kt_check_launch or
 *      kt_headroom_launch is dropped; a later user of the slot drops a pending forecast), its dry finalize drops the report of a
 *      pending kt_reconcile_launch, a pending kt_aggregate_launch keeps its sums.  The results live in buffers of their own, grown
 *      only once the stream of an unfetched launch has drained: a pending forecast and a pending kt_preempt_launch result are
 *      independent — after one launch of each, in either order, both are fetchable.
 *      More than KT_MAX_DIMS resource names: kt_paged_forecast.  Out of scope: several ranks. ---------------------------- */
#define KT_FORECAST_NONE (-1)
int32_t kt_forecast_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns,
                           int32_t on_equal, void* stream);
int32_t kt_forecast_fetch(kt_engine* e, int64_t n, int64_t* out_first, uint8_t* out_verdicts /* [n][n_inst], nullable */);
/* ---- forecast, for gangs: the first instant at which a whole gang is admitted — what kt_preempt_gangs_launch is to
 *      kt_preempt_launch.  The members' own forecasts do not compose into the gang's: each admitted member reserves against the
 *      throttles the later members meet (two members asking 3 each with `used` 4 under a spec of 8: each member alone passes at
 *      every instant, the gang only inside an override of 10).
 *      Notation as for kt_forecast_launch: the instants t_0 < .. < t_{m-1}, state R_t, "a throttle whose reconcile is an error, or
 *      that is not valid and responsible, keeps its stored status in every R_t", the two facts about the replace rule, both
 *      override ends inclusive.  Gang g is the queue positions [gang_off[g], gang_off[g + 1]) of pod_rows, as in
 *      kt_admit_gangs_launch.  Gangs are judged independently of each other, each against the stored reserved amounts; a pod may
 *      be a member of several gangs.
 *      out_verdicts[g][k] (nullable, [n_gangs][n_inst]) is KT_VERDICT_SUCCESS iff a dry kt_admit_gangs_launch of the one gang g,
 *      with R_{t_k} as the stored status, admits it — members in order, each sees the stored reservations plus what the earlier
 *      members of its gang reserved at their turn, every verdict Success; Reserve exactly kt_admit's: the value of every name
 *      carried, the presence of all names carried (zero-valued ones included), count + 1, and the count becomes present — and
 *      KT_VERDICT_UNSCHEDULABLE otherwise.  A gang with a member whose PreFilter is an Error, or whose row is invalid, reports
 *      KT_VERDICT_ERROR at every instant.
 *      out_first[g] (nullable) is the smallest k whose verdict is KT_VERDICT_SUCCESS, or KT_FORECAST_NONE.
 *      out_blocker[g][k] (nullable, [n_gangs][n_inst]) is the queue position (index into pod_rows) of the first member that is not
 *      Success when the gang is walked in R_{t_k} — an Error or invalid member is not Success; all earlier members were admitted,
 *      so the sums it met are exact — and -1 where the verdict is Success.
 *      A gang of one pod reports byte for byte what kt_forecast_launch reports for that pod (blocker: its own position where
 *      blocked).  With inst = [now], out_first[g] == 0 exactly where kt_preempt_gangs_launch at `now` with no candidates reports
 *      prefix 0, and out_blocker[g][0] equals its out_blocker[g].
 *      One kt_check launch with the status matrix over pod_rows, the aggregate and dry finalize (at t_0) of kt_forecast_launch,
 *      and one launch of kt_forecast_gangs (csrc/kt_kernels_forecast_gangs.hip): one wave per gang, lane = instant position, the
 *      member loop wave-uniform — `used`, the request rows and the reserved prefix do not depend on the instant, only the
 *      threshold values and the throttled flags are the lane's own.  The call is a dry run: stored status and reserved amounts
 *      are not changed.
 *      Refused before anything is launched, the instants first: n_inst < 1, instants that are not strictly ascending, an inst_ns
 *      outside [0, 10^9), a missing array, every gang_off defect kt_admit_gangs_launch refuses, a pod named twice within ONE gang
 *      (KT_ERR_INVALID_ARGUMENT); a pod row outside the capacity, n x throttle_rows or n_gangs x n_inst > 2^31
 *      (KT_ERR_OUT_OF_RANGE); `used` wider than int64, a KT_VARIANT_INCREMENTAL engine, an exchange world above 1
 *      (KT_ERR_UNSUPPORTED; the |request| sums probe runs first where the sums are not known).  A refused call leaves the check
 *      slot, the reconcile report and every result buffer alone.  n == 0 is allowed only with n_gangs == 0: KT_OK, nothing is
 *      launched.
 *      Slots: those of kt_forecast_launch — the ONE check slot, its dry finalize drops a pending reconcile report, a pending
 *      kt_aggregate_launch keeps its sums, a pending preempt result of any of the four kinds stays fetchable.  The result SHARES
 *      the one pending forecast result, as the gang preempt calls share the preempt result: a later kt_forecast_launch,
 *      kt_forecast_gangs_launch, kt_paged_forecast or kt_paged_forecast_gangs on the engine replaces it.  kt_forecast_fetch after a gang launch answers
 *      KT_ERR_NOT_READY, and so does kt_forecast_gangs_fetch after a plain or paged launch.  kt_forecast_gangs_fetch synchronises.
 *      More than KT_MAX_DIMS resource names: kt_paged_forecast_gangs.  Out of scope: several ranks. ---------------------------- */
int32_t kt_forecast_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_inst,
                                 const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, void* stream);
int32_t kt_forecast_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_first /* [n_gangs], nullable */,
                                uint8_t* out_verdicts /* [n_gangs][n_inst], nullable */,
                                int64_t* out_blocker /* [n_gangs][n_inst], nullable */);
/* ---- forecast, for elastic gangs: the first instant at which a gang's QUORUM fits — what kt_admit_gangs_elastic_launch is to
 *      kt_admit_gangs_launch, asked over instants: the backoff of a job admitted with minMember that does not start today.
 *      kt_forecast_gangs_launch can only say when the WHOLE gang fits; for an elastic job that is too late, or never.
 *      Notation as for kt_forecast_gangs_launch: the instants t_0 < .. < t_{m-1}, state R_t, "a throttle whose reconcile is an error,
 *      or that is not valid and responsible, keeps its stored status in every R_t", both override ends inclusive, gang g = the queue
 *      positions [gang_off[g], gang_off[g + 1]) of pod_rows.  min_members [n_gangs] and member_flags [n] (nullable: no member is
 *      required; bit 0 = KT_GANG_MEMBER_REQUIRED) as in kt_admit_gangs_elastic_launch.  Gangs are judged independently of each
 *      other, each against the stored reserved amounts; a pod may be a member of several gangs.  The call is a dry run.
 *      The walk, per gang g and instant t_k:
 *      (1)  the members are walked in order in R_{t_k}, exactly as rule (1) of kt_admit_gangs_elastic_launch walks them: each is
 *           judged against the stored status of R_{t_k} plus what the earlier members of g that SUCCEEDED reserved;
 *      (2)  Reserve is kt_admit's: the value of every name carried, the presence of all names carried (zero-valued ones included),
 *           count + 1, and the count becomes present;
 *      (3)  a member that does not succeed reserves on NO throttle — not on the one that stopped it, and not on the others that
 *           affect it either; every member is evaluated, also behind one that failed;
 *      (4)  a member whose PreFilter is an Error (summary word 2), or whose row is invalid, does not succeed at any instant; a
 *           member no throttle affects succeeds and reserves nowhere;
 *      (5)  the forecast has no list capacity: the clause "affected by more throttles than the kernel's list holds" of the
 *           admission's rule (2) does not apply, a member affected by any number of throttles is judged on all of them.
 *      The outputs (all nullable, [n_gangs][n_inst] but out_first):
 *      (6)  out_members[g][k] is the number of members that succeed at t_k — reported whether or not the gang is admitted, so a
 *           caller sees how far from its quorum the gang is;
 *      (7)  out_verdicts[g][k] is KT_VERDICT_ERROR at every k iff the rule can be met at no instant because of members that never
 *           succeed: a required member is an Error or invalid member, or (size of g - such members) < min_members[g].  Otherwise
 *           it is KT_VERDICT_SUCCESS iff out_members[g][k] >= min_members[g] and every required member succeeded at t_k, and
 *           KT_VERDICT_UNSCHEDULABLE otherwise;
 *      (8)  out_first[g] ([n_gangs]) is the smallest k whose verdict is KT_VERDICT_SUCCESS, or KT_FORECAST_NONE;
 *      (9)  out_blocker[g][k] is -1 where the verdict is Success; otherwise the queue position of the first REQUIRED member that did
 *           not succeed at t_k, or, if there is none, of the first member that did not succeed.
 *      Identities:
 *      (E1) with min_members[g] == size of g for every gang and member_flags == NULL, out_first, out_verdicts and out_blocker are
 *           kt_forecast_gangs_launch's byte for byte, and out_members[g][k] equals the size of g exactly where the verdict is
 *           Success; the same holds with every member flagged required at any min_members;
 *      (E2) a gang of one pod with min_members = 1 reports kt_forecast_launch's first and verdict bytes for that pod;
 *      (E3) with inst = [t]: on an engine whose stored status IS R_t, a dry kt_admit_gangs_elastic_launch of the one gang g returns
 *           out_members > 0 exactly where this call's verdict is Success, and then the same number (for members within that
 *           kernel's list capacity).
 *      Refused before anything is launched, in this order: what kt_forecast_gangs_launch refuses about the instants (n_inst < 1,
 *      an inst_ns outside [0, 10^9), instants that are not strictly ascending, a missing array); every gang_off defect; the
 *      min_members / member_flags refusals of clause (10) of kt_admit_gangs_elastic_launch, with the same codes and messages; then
 *      the rest of kt_forecast_gangs_launch's list in its order — a pod named twice within ONE gang, a pod row outside the capacity,
 *      n x throttle_rows or n_gangs x n_inst > 2^31, `used` wider than int64, a KT_VARIANT_INCREMENTAL engine, an exchange world
 *      above 1.  A refused call leaves the check slot, the reconcile report and every result buffer alone.  n == 0 is allowed only
 *      with n_gangs == 0: KT_OK, nothing is launched.
 *      Slots: those of kt_forecast_gangs_launch.  The result SHARES the one pending forecast result as a kind of its own: every
 *      other forecast fetch answers KT_ERR_NOT_READY behind this launch, and kt_forecast_gangs_elastic_fetch answers the same
 *      behind theirs.  min_members and member_flags travel on the launch's stream; the caller's arrays are not referenced after
 *      return.  kt_forecast_gangs_elastic_fetch synchronises.
 *      One kt_check launch with the status matrix over pod_rows, the aggregate and dry finalize (at t_0) of kt_forecast_launch, one
 *      launch of kt_forecast_gangs_elastic (csrc/kt_kernels_forecast_gangs_elastic.hip) — one wave per (gang, instant) pair, the
 *      judge member-major: the union of the members' throttles as a compact state in LDS (or, beyond its capacity, in a workspace
 *      in device memory), the members in order against it — and one small launch behind it for out_first.
 *      Out of scope: more than KT_MAX_DIMS resource names, several ranks. ------------------------------------------------------ */
int32_t kt_forecast_gangs_elastic_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                         const int64_t* min_members /* [n_gangs] */, const uint8_t* member_flags /* [n], nullable */,
                                         int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, void* stream);
int32_t kt_forecast_gangs_elastic_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_first /* [n_gangs], nullable */,
                                        uint8_t* out_verdicts /* [n_gangs][n_inst], nullable */,
                                        int64_t* out_members /* [n_gangs][n_inst], nullable */,
                                        int64_t* out_blocker /* [n_gangs][n_inst], nullable */);
/* ---- headroom forecast: how many copies of a pod the throttles admit at each instant — kt_headroom_launch ("how many, now") and
 *      kt_forecast_launch ("whether, when") asked at once: how many replicas fit once the night override begins, and at which
 *      instant `want` replicas fit.
 *      Notation as for kt_forecast_launch: the instants t_0 < .. < t_{m-1}, state R_t, "a throttle whose reconcile is an error, or
 *      that is not valid and responsible, keeps its stored status in every R_t", the two facts about the replace rule, both
 *      override ends inclusive; reserved amounts are read as they stand.
 *      out_copies[i][k] (nullable, [n][n_inst]) is headroom(p_i, cap, on_equal) as kt_headroom_launch defines it, evaluated in
 *      R_{t_k}: the number of leading Success verdicts of a dry kt_admit_launch over [p_i] * cap with R_{t_k} as the stored
 *      status.  It lies in [0, cap].
 *      out_limiting[i][k] (nullable, [n][n_inst]) is the lowest throttle row whose status is not KT_STATUS_NOT_THROTTLED in the row
 *      PreFilter returns for the first copy that is not admitted in R_{t_k}, and -1 where all `cap` copies are admitted.
 *      out_first[i] (nullable) is the smallest k with out_copies[i][k] >= want, or KT_FORECAST_NONE.
 *      A pod whose PreFilter is an Error, or whose row is invalid: 0 copies at every instant, limiting -1, KT_FORECAST_NONE.  A pod
 *      no throttle affects: `cap` at every instant, limiting -1, first 0.  A pod with a negative request is served, as by
 *      kt_headroom_launch.
 *      Identities:
 *        (I1) with cap == want == 1, out_copies[i][k] == 1 exactly where kt_forecast_launch reports KT_VERDICT_SUCCESS, and
 *             out_first is byte for byte kt_forecast_fetch's; an Error verdict is 0 copies and limiting -1.
 *        (I2) with inst = [t] on an engine whose last action was kt_reconcile_launch(t, KT_RECONCILE_APPLY) plus fetch,
 *             out_copies[:][0] and out_limiting[:][0] are byte for byte what kt_headroom_launch plus fetch report with the same cap
 *             and on_equal.
 *        (I3) the call is a dry run: stored status, reserved amounts and a pending kt_aggregate_launch's sums are unchanged.
 *      One kt_check launch with the status matrix over pod_rows, the aggregate and dry finalize (at t_0) of kt_forecast_launch, and
 *      one launch of kt_headroom_forecast (csrc/kt_kernels_headroom_forecast.hip): one wave per pod, lane = instant position; the
 *      lane computes its instant's threshold as kt_forecast does and takes kt_headroom's closed form per amount; the answer is
 *      the lexicographic minimum of (copies, throttle row) over the affecting throttles.
 *      Refused before anything is launched, in this order: the instants as kt_forecast_launch refuses them and a missing pod_rows
 *      with n > 0 (KT_ERR_INVALID_ARGUMENT); cap outside [1, KT_HEADROOM_MAX_CAP] or want outside [1, cap]
 *      (KT_ERR_INVALID_ARGUMENT); a pod row outside the table, n x throttle_rows or n x n_inst > 2^31 (KT_ERR_OUT_OF_RANGE); `used`
 *      wider than int64, a KT_VARIANT_INCREMENTAL engine, an exchange world above 1 (KT_ERR_UNSUPPORTED; the |request| sums probe
 *      runs first where the sums are not known).  A refused call leaves the check slot, the reconcile report and every result
 *      buffer alone.  n == 0 is KT_OK and launches nothing.
 *      Slots: those of kt_forecast_launch — the ONE check slot, its dry finalize drops a pending reconcile report, a pending
 *      kt_aggregate_launch keeps its sums, a pending preempt result of any kind stays fetchable.  The result SHARES the one pending
 *      forecast result as its third kind: a later forecast launch of any kind replaces it; kt_forecast_fetch and
 *      kt_forecast_gangs_fetch after this launch answer KT_ERR_NOT_READY, and kt_headroom_forecast_fetch answers it after theirs.
 *      kt_headroom_forecast_fetch synchronises.
 *      More than KT_MAX_DIMS resource names: kt_paged_headroom_forecast.  Whole gangs: kt_headroom_forecast_gangs_launch.  Out of
 *      scope: several ranks. ----------------------------------------------------------------------------------------------- */
int32_t kt_headroom_forecast_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s,
                                    const int32_t* inst_ns, int32_t on_equal, int64_t cap, int64_t want, void* stream);
int32_t kt_headroom_forecast_fetch(kt_engine* e, int64_t n, int64_t* out_first /* [n], nullable */,
                                   int64_t* out_copies /* [n][n_inst], nullable */, int32_t* out_limiting /* [n][n_inst], nullable */);
/* ---- headroom forecast, for gangs: how many copies of a whole gang the throttles admit at each instant — kt_headroom_gangs_launch
 *      ("how many, now") and kt_forecast_gangs_launch ("whether, when") asked at once: how many more replicas of a training job
 *      fit once the night override begins, and at which instant `want` of them fit.
 *      The notation (instants t_0 < .. < t_{m-1}, state R_t) and the rule about throttles that keep their stored status are those of
 *      kt_forecast_launch; gang g is the queue positions [gang_off[g], gang_off[g + 1]) as in kt_admit_gangs_launch.
 *      out_copies[g][k], out_blocker[g][k] and out_limiting[g][k] (each nullable, [n_gangs][n_inst]) are exactly what
 *      kt_headroom_gangs_launch defines, evaluated with R_{t_k} as the stored status: the number of leading admitted gangs of a dry
 *      kt_admit_gangs_launch over `cap` consecutive copies of the gang; the queue position (index into pod_rows) of the first member
 *      of the first refused copy that is not Success; the lowest throttle row that stops that member at its turn.  Blocker and
 *      limiting are -1 where all `cap` copies are admitted, limiting also where the blocker's verdict is an Error.
 *      A gang with an Error or invalid member reports 0 copies at every instant; its walk ends in front of that member, and an earlier
 *      member that some throttle stops at t_k is the blocker there.  A gang no throttle affects: `cap`, -1, -1 and first 0.
 *      out_first[g] (nullable) is the smallest k with out_copies[g][k] >= want, or KT_FORECAST_NONE.
 *      Identities:
 *        (G1) a gang of one pod reports byte for byte the first, copies and limiting that kt_headroom_forecast_launch reports for
 *             that pod; its blocker is its own position where copies < cap, else -1.
 *        (G2) with cap == want == 1, out_copies[g][k] == 1 exactly where kt_forecast_gangs_launch reports KT_VERDICT_SUCCESS, and
 *             out_first and out_blocker are byte for byte those of kt_forecast_gangs_fetch.
 *        (G3) with inst = [t] on an engine whose last action was kt_reconcile_launch(t, KT_RECONCILE_APPLY) plus fetch, column 0 is
 *             byte for byte what kt_headroom_gangs_launch plus fetch report with the same cap and on_equal.
 *        (G4) the call is a dry run: stored status, reserved amounts and a pending kt_aggregate_launch's sums are unchanged.
 *      One kt_check launch with the status matrix over pod_rows, the aggregate and dry finalize (at t_0) of kt_forecast_launch, and
 *      one launch of kt_headroom_forecast_gangs (csrc/kt_kernels_headroom_forecast_gangs.hip): one wave per gang, lane = instant
 *      position; the lane computes its instant's threshold as kt_forecast_gangs does and bisects the copies of its OWN instant, every
 *      probe judged by the gang walk of admission itself with the candidate's reserved row (1 + 31 rounds at the most); the answer
 *      is the lexicographic minimum of (copies, blocker, throttle row) over the affecting throttles.
 *      Refused before anything is launched, in this order: the instants as kt_forecast_launch refuses them and a missing array; cap
 *      outside [1, KT_HEADROOM_MAX_CAP], then want outside [1, cap]; every gang_off defect kt_admit_gangs_launch refuses, a pod named
 *      twice within ONE gang (KT_ERR_INVALID_ARGUMENT); a pod row outside the table; n x throttle_rows or n_gangs x n_inst > 2^31
 *      (KT_ERR_OUT_OF_RANGE); what kt_forecast_gangs_launch refuses as unsupported (the |request| sums probe runs first where the sums
 *      are not known); an engine that has been fed a negative request — the search over the copies rests on sums that only grow,
 *      kt_headroom_forecast_launch serves such an engine pod by pod (KT_ERR_UNSUPPORTED).  A refused call leaves the check slot, the
 *      reconcile report and every result buffer alone.  n == 0 is allowed only with n_gangs == 0: KT_OK, nothing is launched.
 *      Slots: those of kt_forecast_gangs_launch; a pending preempt result of any kind stays fetchable.  The result SHARES the one
 *      pending forecast result as its fourth kind: a later forecast launch of any kind replaces it, and each of the four fetches
 *      answers KT_ERR_NOT_READY after a launch of another kind.  kt_headroom_forecast_gangs_fetch synchronises.
 *      More than KT_MAX_DIMS resource names: kt_paged_headroom_forecast_gangs.  Out of scope: several ranks. -------------------- */
int32_t kt_headroom_forecast_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                          int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, int64_t cap,
                                          int64_t want, void* stream);
int32_t kt_headroom_forecast_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_first /* [n_gangs], nullable */,
                                         int64_t* out_copies /* [n_gangs][n_inst], nullable */,
                                         int32_t* out_limiting /* [n_gangs][n_inst], nullable */,
                                         int64_t* out_blocker /* [n_gangs][n_inst], nullable */);
/* The sorted, distinct instants in (from, until] at which the CalculateThreshold of some valid and responsible throttle can change:
 * every parsed non-zero `begin` of an override, and for every parsed non-zero `end` the instant end + 1 ns — the FIRST instant at
 * which the override is no longer active.  That is deliberately not the `end` that NextOverrideHappensIn
 * (kt_reconcile_fetch_next_override) reports: at `end` itself the override is still active (both ends are inclusive).  Overrides
 * with a parse error contribute nothing.  Writes the earliest min(total, cap) instants to out_s / out_ns and the full count to
 * *out_total; cap == 0 with NULL arrays just counts.  Host-only: reads the engine's host copy of the throttle specs under the
 * launch lock and launches nothing.  Together with `now` in front, the instants a host passes to kt_forecast_launch. */
int32_t kt_override_instants(kt_engine* e, int64_t from_s, int32_t from_ns, int64_t until_s, int32_t until_ns, int64_t cap, int64_t* out_s,
                             int32_t* out_ns, int64_t* out_total);
/* Current reserved amounts of n throttle rows (after kt_set_reserved / kt_admit_launch(KT_ADMIT_COMMIT)). */
int32_t kt_fetch_reserved(kt_engine* e, int32_t n, const int32_t* throttle_rows, const kt_amounts* out);
int32_t kt_throttle_rows(kt_engine* e, int32_t* out_rows);
/* Device pointer of the per-pod summary words of the last check (stays valid until the next check). */
int32_t kt_check_device_summary(kt_engine* e, void** device_ptr);

/* Effective per-pod requests as held in HBM (parity of the resourcelist summation): out_v [n][D]. */
int32_t kt_fetch_pod_requests(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t* out_v, uint32_t* out_present);

/* ---- measurement: HIP-event timing of the engine's own kernels on the stream they run on. ------------- */
#define KT_KERNEL_CHECK 0
#define KT_KERNEL_AGGREGATE 1
#define KT_KERNEL_FINALIZE 2
#define KT_KERNEL_PREPARE 3
#define KT_KERNEL_REDUCE 4 /* slab reduction that follows the aggregate scan kernel (when it privatises in LDS) */
#define KT_KERNEL_COUNT 5
int32_t kt_timing_enable(kt_engine* e, int32_t on);
/* Sum of durations (ms) and launch count since the last reset for one kernel family; synchronises. */
int32_t kt_timing_read(kt_engine* e, int32_t kernel, double* total_ms, int64_t* launches);
int32_t kt_timing_reset(kt_engine* e);
int32_t kt_synchronize(kt_engine* e, void* stream);
/* symbol of the HIP kernel LAST dispatched for a family (to match rocprofv3 kernel-trace rows) */
const char* kt_kernel_name(kt_engine* e, int32_t kernel);
/* event counters (-1: unknown counter) */
#define KT_COUNTER_FEW_CHECKS 0 /* kt_check calls served by the few-pod path (shared lock, no copy, no stream sync) */
#define KT_COUNTER_COMPILES 1   /* selector program compiles + index builds so far (a Throttle event that leaves every
                                   selector, namespace and flag of its rows as stored — a threshold edit, a status update —
                                   only re-uploads the throttle tables and does not count) */
#define KT_COUNTER_INDEX_CHUNKS 2 /* LDS-sized chunks of the compiled selector index (0 before the first compile) */
#define KT_COUNTER_INDEX_WORDS 3  /* 64-bit words of term numbers of the compiled program (all chunks) */
#define KT_COUNTER_NS_WORD_VISITS 4 /* sum over the namespace rows in use of the words a pod of that namespace visits */
#define KT_COUNTER_NS_ROWS 5      /* namespace rows the compiled program covers */
#define KT_COUNTER_NS_CHUNK_VISITS 6  /* sum over the namespace rows of the index chunks that hold a word list of the row: the chunk
                                         passes a namespace-ordered scan makes per namespace, summed */
#define KT_COUNTER_INDEX_IMAGE_WORDS 7 /* words over all chunk images (>= INDEX_WORDS: the grouped plan keeps copies of a word in
                                          the chunks of every group of namespaces that visits it) */
#define KT_COUNTER_SLOW_THROTTLES 8 /* throttles of the compiled program that are walked term by term instead of through the index
                                      (an unconvertible podSelector term; more than 512 selector terms) */
#define KT_COUNTER_PACKED_WORDS 9   /* 64-bit words per pod of the packed fold the last full aggregate scan ran with (1..8; 0: the
                                      plain fold — a negative request, sums beyond int64, fields that do not fit) */
#define KT_COUNTER_VIEW_BUILDS 10   /* builds of a scan view so far, the aggregate's or the check sweep's (a pod event that fits the
                                      views is patched into them in place and does not count) */
#define KT_COUNTER_AGG_WORKGROUPS 11 /* workgroups (= slabs) of the last full aggregate scan's launch: up to 256 at one workgroup per CU,
                                      up to 512 in the two-per-CU form of single-chunk packed scans (KT_AGG_ONE_PER_CU=1 keeps one) */
#define KT_COUNTER_MATCH_CACHE_BUILDS 12 /* full builds of the match cache so far: the per-pod matched-term words single-chunk programs
                                            keep between PreFilter sweeps.  One after every compile and after a table clear; pod events refresh
                                            their rows only and do not count (KT_NO_MATCH_CACHE=1: no table, the scans as before) */
#define KT_COUNTER_MATCH_CACHE_SCANS 13  /* PreFilter sweeps served from the match cache so far (the lean sweep of every row; the aggregate
                                            scans count in KT_COUNTER_MATCH_CACHE_AGG_SCANS).  The sweep replays the table's 16-byte
                                            match-code records; KT_NO_MATCH_CODES=1: its planes, counted alike */
#define KT_COUNTER_MATCH_CACHE_PLANES 14 /* the longest namespace word list of the compiled single-chunk program, as the last sweep of every
                                            row counted it (0: not counted yet, or several chunks): more than 4 = not cached */
#define KT_COUNTER_MATCH_CACHE_AGG_SCANS 15 /* full aggregate scans that replayed the match cache so far: the two-per-CU form over the scan
                                               view's planes (KT_NO_MATCH_CACHE_AGG=1 keeps the aggregate's selector scan while the sweep
                                               still replays) */
int64_t kt_counter(kt_engine* e, int32_t which);
/* ---- More resource names than one engine has dimensions (KT_MAX_DIMS): PAGES.  The reference sums and compares any resource
 *      name (pkg/resourcelist/resourcelist.go:27-54, resource_amount.go:127-159).  The host builds the same cluster once per
 *      page of <= KT_MAX_DIMS names — every page engine holds every pod row and every throttle row, with the requests /
 *      thresholds of ITS names — and these calls run a step on every page and combine the results.  The combination is
 *      exact: every step of CheckThrottledFor (throttle_types.go:128-153) is `count part OR exists a resource name ...`; the
 *      count part needs no name (every page computes it alike) and the name part of the cluster is the OR over the pages:
 *          exceeds <=> some page says exceeds; else active <=> some page says active; else insufficient <=> some page says so;
 *      a pod-level Error shows in every page.  (kube_throttler_amd/paging.py is the same statement in Python.) -------------- */
/* kt_check on every page, combined: out_status [n][throttle rows] (nullable) and out_summary [n] (nullable; verdict and the
 * three class counts of the COMBINED row).  The engines are called one after the other (each call is its own critical section). */
int32_t kt_paged_check(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal,
                       uint64_t* out_summary, uint8_t* out_status);
/* kt_reconcile_launch + kt_reconcile_fetch on every page: page_out[k] receives page k's result for throttle rows [0, n) —
 * `used`, calculatedThreshold and `throttled` are per resource name, each name comes from the page that owns it; the pod
 * counts and the pod flag are the same in every page.  replaced_any[i] (nullable) = calculatedThreshold replaced in some
 * page (it is replaced as a whole), error_any[i] (nullable) = the reconcile of row i failed.
 * Failure: with KT_RECONCILE_APPLY every page is first reconciled as a dry run — a page that cannot (LDS budgets, sums out of
 * range) fails the call before ANY page has stored a new status; an error after that (device errors) is returned once every
 * launched page's result has been drained, never with pending reconciles left behind. */
int32_t kt_paged_reconcile(kt_engine* const* pages, int32_t n_pages, int64_t now_s, int32_t now_ns, uint32_t flags, int32_t n,
                           const kt_status* page_out, uint8_t* replaced_any, uint8_t* error_any);
/* kt_admit_launch over the pages: the queue pod_rows[0..n) (NULL: rows [0, n)) admitted IN ORDER, pod i checked against the
 * reserved amounts of every page as the pods admitted before it left them, its verdict the combination above over every page,
 * and on Success ResourceAmountOfPod(pod) added to every affected throttle in every page (each page its own names' amounts; the
 * pod count in every page).  One kt_check of page 0 (which throttles affect which pod: the selector side is the same in every
 * page) and ONE kernel (kt_admit, the kernel of kt_admit_launch: one wave, the selector scan once per pod, the name part of the four steps evaluated
 * against every page) on page 0's stream.  Synchronous: out_summary [n] and out_status [n][throttle rows] (both nullable)
 * receive what PreFilter returned for pod i AT ITS TURN, combined over the pages; n_pages == 1 is
 * kt_admit_launch + kt_check_fetch (the same launch, synchronous).  flags: KT_ADMIT_COMMIT keeps every page's resulting reserved amounts (kt_fetch_reserved
 * per page); without it the call is a dry run.  Duplicate pods: as for kt_admit_launch, every admitted pod ADDS its amount, so
 * a pod whose amount is already reserved, or that occurs twice in the queue, must not be in it.
 * Refused: pages with different throttle-row counts or an engine named twice (KT_ERR_INVALID_ARGUMENT), pages on different
 * devices or a page whose stored `used` is wider than int64 (KT_ERR_UNSUPPORTED), n x throttle_rows > 2^31
 * (KT_ERR_OUT_OF_RANGE).  Every page is locked exclusively for the call, in address order.  Ordering: the streams of pages
 * 1.. are synchronised before the launch (their uploads and earlier kernels have completed; their newest feed kernel is
 * ordered on the device).  The call uses page 0's check slot (a pending kt_check_launch of page 0 is dropped, as with
 * kt_affected_pods).  The state of all pages lives in LDS while the sum over the pages of throttle_rows x (8 x n_dims + 16)
 * plus the list fits 160 KiB, beyond that in HBM on page 0. */
int32_t kt_paged_admit(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                       uint64_t* out_summary, uint8_t* out_status);
/* kt_admit_gangs_launch over the pages, synchronous, as kt_paged_admit is kt_admit_launch over the pages (the same refusals,
 * locking and ordering; n_pages == 1 is kt_admit_gangs_launch + kt_check_fetch + kt_admit_gangs_fetch): a gang that is not
 * admitted as a whole is rolled back on every page.  out_summary [n], out_status [n][throttle rows] and out_gang_admitted
 * [n_gangs] are all nullable. */
int32_t kt_paged_admit_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                             const int64_t* gang_off, int32_t on_equal, uint32_t flags, uint64_t* out_summary, uint8_t* out_status,
                             uint8_t* out_gang_admitted);
/* kt_admit_gangs_elastic_launch over the pages, synchronous, as kt_paged_admit_gangs is kt_admit_gangs_launch over the pages (the
 * same refusals, in clause (10)'s order, locking and ordering; n_pages == 1 is kt_admit_gangs_elastic_launch + kt_check_fetch +
 * kt_admit_gangs_elastic_fetch): a kept gang's succeeded members stay reserved on every page, a gang that misses its quorum or a
 * required member is rolled back on every page.  out_summary [n], out_status [n][throttle rows] and out_members [n_gangs] are all
 * nullable. */
int32_t kt_paged_admit_gangs_elastic(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                     const int64_t* gang_off, const int64_t* min_members, const uint8_t* member_flags, int32_t on_equal,
                                     uint32_t flags, uint64_t* out_summary, uint8_t* out_status, int64_t* out_members);
/* kt_headroom_launch over the pages, synchronous (n_pages == 1 is kt_headroom_launch + kt_headroom_fetch): the copies of
 * pod_rows[i] that every page's names and the pod count (page 0) still admit — the name part is the minimum over the pages —
 * and the limiting throttle row.  One kt_check of page 0 and ONE kt_headroom launch over every page's tables on page 0's stream.
 * Refusals, locking (every page exclusively, in address order) and ordering are kt_paged_admit's; cap as for
 * kt_headroom_launch.  Uses page 0's check slot.  out_copies [n] and out_limiting [n] are both nullable. */
int32_t kt_paged_headroom(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal,
                          int64_t cap, int64_t* out_copies, int32_t* out_limiting);
/* kt_headroom_gangs_launch over the pages, synchronous (n_pages == 1 returns byte for byte what kt_headroom_gangs_launch +
 * kt_headroom_gangs_fetch return): out_copies[g] = the number of LEADING admitted gangs of a dry kt_paged_admit_gangs over `cap`
 * consecutive copies of gang g, against every page's stored status and current reserved amounts.  out_blocker[g] and
 * out_limiting[g] are kt_headroom_gangs_launch's, read off the COMBINED row the paged admission returns to that member at its
 * turn: the queue position of the first member of the first copy that is not admitted whose combined verdict is not Success, and
 * the lowest throttle row whose combined status is not KT_STATUS_NOT_THROTTLED there; the -1 rules, the Error / invalid-member
 * rule and the rule for a gang no throttle affects are the single-engine ones.  What pages add to the definition:
 *   - an admitted copy reserves on every page, each page its own names' values and the presence of all the names the member
 *     carries on that page; the pod count is judged once, on page 0;
 *   - each page reads the threshold kt_admit reads on that page (that page's stored calculatedAt flag).  Nothing is reconciled:
 *     the call is held to paged admission, not to the preemption family's "replaced as a whole" rule;
 *   - copy j passes on throttle t iff the in-order member walk passes on every page, each against its own reserved row plus
 *     j x (what one admitted copy reserves there): the answer is the lexicographic minimum over all (throttle, page) pairs of
 *     (copies, first stopped member, throttle row).  Where every page carries the same count part it equals the minimum over
 *     the pages' own kt_headroom_gangs answers of (copies, blocker or the gang size if -1, limiting or +inf if -1), mapped back
 *     to (cap, -1, -1) at the cap; a gang of one pod equals kt_paged_headroom in copies and limiting.
 * One kt_check of page 0 with the status matrix over the members of all gangs and ONE kernel (kt_headroom_gangs_paged: one wave
 * per gang, lane = a candidate number of copies, the running minimum cuts the search over pages as well as over throttles) on
 * page 0's stream.  Refused, before anything is launched and before a check slot or pending result of any page is touched:
 * what kt_headroom_gangs_launch refuses about its arguments (pod_rows missing, every gang_off defect, a pod twice within ONE
 * gang, cap outside [1, KT_HEADROOM_MAX_CAP]: KT_ERR_INVALID_ARGUMENT; a pod row outside a page's capacity, n x throttle_rows
 * > 2^31: KT_ERR_OUT_OF_RANGE), what kt_paged_headroom refuses about the page set (different throttle-row counts, an engine named
 * twice: KT_ERR_INVALID_ARGUMENT; different devices: KT_ERR_UNSUPPORTED), and per page with KT_ERR_UNSUPPORTED a stored `used`
 * wider than int64 or an engine that has been fed a negative request — on ANY page: the search rests on sums that only grow.
 * n == 0 with n_gangs == 0 is KT_OK and launches nothing.  Locking (every page exclusively, in address order) and ordering are
 * kt_paged_admit's.  The call uses page 0's check slot and page 0's headroom result buffers and hands the results out:
 * afterwards no headroom result of either kind is pending on page 0 (kt_headroom_fetch and kt_headroom_gangs_fetch answer
 * KT_ERR_NOT_READY), a pending kt_check_launch of page 0 is gone, and stored status and reserved amounts of no page have
 * changed.  out_copies, out_limiting and out_blocker [n_gangs] are all nullable.  One rank only. */
int32_t kt_paged_headroom_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                const int64_t* gang_off, int32_t on_equal, int64_t cap, int64_t* out_copies, int32_t* out_limiting,
                                int64_t* out_blocker);
/* kt_preempt_launch and, with KT_PREEMPT_REPRIEVE in `flags`, kt_preempt_reprieve_launch over the pages, synchronous: their
 * definitions on the cluster of ALL names — counted pods, S_k, the m_eff cut, the victim mask, exact presence by contributor
 * counts, the operational walk with no monotonicity assumption, KT_PREEMPT_NONE.  n_pages == 1 returns byte for byte what
 * kt_preempt_launch (kt_preempt_reprieve_launch) + kt_preempt_fetch return.  The answer is NOT a combination of per-page calls
 * (with requests of either sign a page may pass at k, fail at k + 1 and pass again, so the maximum of the pages' prefixes is
 * wrong), which is why the kernels see every page.  What pages add to the definition:
 *   - every page reconciles its own names at `now`; the pod count is the same in every page and is judged once, on page 0;
 *   - the name part of the four CheckThrottledFor steps combines by the rule above: a (throttle, k) pair fails iff the count
 *     part or some page's name part fails;
 *   - status.calculatedThreshold is replaced as a whole (throttle_controller.go:116-133 compares it by value over all names):
 *     a throttle reads status.calculatedThreshold on EVERY page iff, on SOME page, calculatedAt is set in the stored status or
 *     the dry reconcile replaces it; otherwise it reads spec.threshold on every page.  (The stored flag is part of the OR: the
 *     answer stays right between a kt_paged_reconcile with KT_RECONCILE_APPLY and the host's status write-back, when the
 *     pages' stored flags may disagree);
 *   - a throttle keeps its stored status in every state iff its reconcile is an error on some page or it is not valid and
 *     responsible; the stored status is then read on every page;
 *   - which candidates are counted, which throttles match which pod, the error rows and m_eff come from ONE check of page 0
 *     over pod_rows ++ cand_rows (the selector side is the same in every page; a pod-level error shows in every page).
 * On page 0's stream, in order: that check; for every page its dense aggregate (beside its partial buffer) and its dry finalize
 * at `now`; the copy of the page descriptors; one launch of kt_preempt_paged; with the flag one launch of
 * kt_preempt_reprieve_paged (csrc/kt_kernels_preempt_paged.hip), whose list state is sized with the sum of the pages' names
 * (in LDS, beyond that in a workspace of page 0).  out_prefix [n] and out_victims [n][n_cand] are both nullable.
 * Refused before anything is launched, and before any page's check slot, reconcile report or result buffer is touched: what
 * kt_paged_admit refuses about the page set (different throttle-row counts, an engine named twice: KT_ERR_INVALID_ARGUMENT;
 * different devices: KT_ERR_UNSUPPORTED), what kt_preempt_launch refuses about its arguments (and flags other than
 * KT_PREEMPT_REPRIEVE: KT_ERR_INVALID_ARGUMENT), and what it refuses about an engine, asked of every page: a
 * KT_VARIANT_INCREMENTAL engine, an exchange world above 1, a `used` wider than int64 (KT_ERR_UNSUPPORTED) — as there, the one
 * thing that may run first is a page's kernel that sums the |requests|.  n == 0 is KT_OK and launches nothing; n_cand == 0
 * answers 0 or KT_PREEMPT_NONE per pod.  Locking (every page exclusively, in address order) and ordering are kt_paged_admit's.
 * Slots: the call uses page 0's check slot (a pending kt_check_launch / kt_headroom_launch of page 0 is dropped) and page 0's
 * preempt result buffers — the results are handed out by the call, so a preempt result that was pending on page 0 is gone
 * afterwards (kt_preempt_fetch answers KT_ERR_NOT_READY) while a pending kt_forecast_launch of page 0 stays fetchable; every
 * page's dry finalize writes that page's reconcile result buffers, so every page's pending reconcile report is dropped (a status
 * stored with KT_RECONCILE_APPLY stays stored); a pending kt_aggregate_launch of any page keeps its sums.  The call is a dry
 * run: stored status and reserved amounts of no page change.  A device error after the first launch is returned once the
 * stream has drained; no page keeps a pending result.
 * The gang forms over pages: kt_paged_preempt_gangs.  Out of scope: several ranks. */
#define KT_PREEMPT_REPRIEVE 0x1u
int32_t kt_paged_preempt(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_cand,
                         const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, uint32_t flags,
                         int64_t* out_prefix /* [n], nullable */, uint8_t* out_victims /* [n][n_cand], nullable */);
/* kt_preempt_gangs_launch (with KT_PREEMPT_REPRIEVE in `flags`: kt_preempt_gangs_reprieve_launch) + kt_preempt_gangs_fetch over the
 * pages, synchronous: their definition, word for word, on the cluster of ALL names — S_k, the in-order admission of the members
 * with Reserve on every throttle that affects the member, the list cut m_eff, the error rows, KT_PREEMPT_NONE, the victim mask,
 * the blocker and the reprieve walk.  n_pages == 1 returns byte for byte what the single-engine calls return; a gang of one pod
 * answers what kt_paged_preempt answers for that pod, plus the blocker.  The answer is NOT a combination of per-page calls, for
 * kt_paged_preempt's three reasons and one of the gang's own: an admitted member reserves on EVERY page, so neither the maximum of
 * the pages' own gang prefixes nor the maximum of the members' own paged prefixes is the gang's.  What pages add:
 *   - ONE check of page 0 over pod_rows ++ cand_rows yields which throttles affect which member, which candidates are counted and
 *     matched, the error rows, m_eff and "a member is an Error or invalid";
 *   - the pod count is page 0's: the threshold's, `used`'s, the calculated threshold's and the stored and running reserved count;
 *     a name part is judged on its own page;
 *   - the gang passes in S_k iff, for every throttle of the union of the members' affecting throttles, the in-order member walk
 *     passes on page 0 with the count part and passes the name part on every page;
 *   - each page carries its own running reserved prefix, from that page's stored reserved row: a member the throttle affects adds
 *     its value of every name of that page it carries, the presence of ALL that page's names it carries (zero-valued ones
 *     included) and count + 1.  Judging member j with the reservations of all earlier affected members stays exact: the gang
 *     passes only if every member passes every page;
 *   - stored and use-calc are kt_paged_preempt's whole-throttle facts (an OR over the pages); a throttle that keeps its stored
 *     status reads the STORED calculated threshold on every page, never a page's fresh one;
 *   - out_blocker[g]: the minimum, over throttles AND pages, of the first stopped queue position in S_0 (an Error or invalid
 *     member counts as stopped); -1 when out_prefix[g] == 0;
 *   - out_victims[g][j] = 1 iff j < prefix, c_j is counted and a throttle affecting some member matches c_j (decided once, on
 *     page 0); with the flag, what the reprieve walk leaves: the joint judge is an in-order admission of the gang over every page,
 *     one verdict per candidate, and a candidate that is put back is put back on every page.
 * On page 0's stream, in order: that check; for every page its dense aggregate (beside its partial buffer) and its dry finalize
 * at `now`; the copy of the gang offsets and of the page descriptors; one launch of kt_preempt_gangs_paged; with the flag one
 * launch of kt_preempt_gangs_reprieve_paged (csrc/kt_kernels_preempt_gangs_paged.hip), whose list state is sized with the sum of
 * the pages' names (in LDS, beyond that in a workspace of page 0); the copies out.  out_prefix [n_gangs], out_victims
 * [n_gangs][n_cand] and out_blocker [n_gangs] are all nullable.
 * Refused before anything is allocated or launched, and before any page's check slot, reconcile report or result buffer is
 * touched: what kt_paged_preempt refuses about the page set (different throttle-row counts, an engine named twice:
 * KT_ERR_INVALID_ARGUMENT; different devices: KT_ERR_UNSUPPORTED), about the flags (KT_ERR_INVALID_ARGUMENT) and about every
 * page's engine (a KT_VARIANT_INCREMENTAL engine, an exchange world above 1, a `used` wider than int64: KT_ERR_UNSUPPORTED — as
 * there, the one thing that may run first is a page's kernel that sums the |requests|), and what kt_preempt_gangs_launch refuses
 * about its arguments (every gang_off defect, a pod twice in one gang, a member that is also a candidate, a candidate twice, a
 * missing array, n_cand < 0: KT_ERR_INVALID_ARGUMENT; a row that no page holds, n, n_cand or their sum times throttle_rows above
 * 2^31: KT_ERR_OUT_OF_RANGE).  n == 0 is allowed only with n_gangs == 0: KT_OK, nothing is launched; n_cand == 0 answers 0 or
 * KT_PREEMPT_NONE per gang, with blockers.  Locking (every page exclusively, in address order) and ordering are kt_paged_admit's.
 * Slots are kt_paged_preempt's: the call uses page 0's check slot and page 0's preempt result buffers — the results are handed
 * out by the call, so afterwards no preempt result is pending on page 0 for either fetch (kt_preempt_fetch and
 * kt_preempt_gangs_fetch answer KT_ERR_NOT_READY) while a pending kt_forecast_launch of page 0 stays fetchable; every page's
 * pending reconcile report is dropped; a pending kt_aggregate_launch of any page keeps its sums.  The call is a dry run: stored
 * status and reserved amounts of no page change.  A device error after the first launch is returned once the stream has drained;
 * no page keeps a pending result.
 * Out of scope: several ranks. */
int32_t kt_paged_preempt_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                               const int64_t* gang_off, int64_t n_cand, const int64_t* cand_rows, int64_t now_s, int32_t now_ns,
                               int32_t on_equal, uint32_t flags, int64_t* out_prefix /* [n_gangs], nullable */,
                               uint8_t* out_victims /* [n_gangs][n_cand], nullable */, int64_t* out_blocker /* [n_gangs], nullable */);
/* kt_forecast_launch + kt_forecast_fetch over the pages, synchronous: their definition on the cluster of ALL names — R_k, the
 * verdict bytes, KT_FORECAST_NONE, the error rows.  n_pages == 1 returns byte for byte what kt_forecast_launch +
 * kt_forecast_fetch return.  The answer is NOT a combination of per-page calls: status.calculatedThreshold is compared and
 * replaced as a whole, over all names (throttle_controller.go:116-133), so whether a throttle reads its calculated threshold or
 * spec.threshold at instant t is one fact for all pages, and it changes from instant to instant (an override that names only a
 * later page's resource replaces the threshold, and page 0 must then read a calculated threshold that omits its own names) —
 * which is why the kernel sees every page.  Per affecting throttle (they come from ONE check of page 0 over pod_rows: the selector
 * side is the same in every page, a pod-level error shows in every page):
 *   - whole-throttle facts, an OR over the pages: `stored` — the dry reconcile is an error on some page, or the throttle is not
 *     valid and responsible: the stored status is read on every page at every instant; `calc_at_any` — calculatedAt is set in
 *     the stored status of some page (the answer stays right between a kt_paged_reconcile with KT_RECONCILE_APPLY and the
 *     host's status write-back, when the pages' stored flags may disagree);
 *   - a stored throttle is judged once over every page: the count part on page 0, every page's name part, against the stored
 *     calculatedThreshold where calc_at_any holds and spec.threshold otherwise; a failure means the pod never passes;
 *   - otherwise, per instant t_k, every page computes CalculateThreshold(t_k) over its names exactly as kt_forecast_launch does
 *     (activity is decided by the instants, the same on every page; the first active override wins per name of that page) and
 *     `differs` is the OR over the pages of: the page's calculated threshold differs by value from the page's stored one over its
 *     names, or the page's messages fingerprint differs; page 0 adds the comparison of the pod count (the same in every page).
 *     The throttle reads status.calculatedThreshold on EVERY page iff calc_at_any || differs, else spec.threshold on every
 *     page; status.throttled is IsThrottled(used, true) against the calculated threshold either way.  The pod fails the throttle
 *     at t_k iff the count part (page 0) or some page's name part of the four CheckThrottledFor steps fails against the threshold
 *     read.  A page none of whose names the pod requests is still part of `differs`: it can replace the threshold for the others.
 * The instants kt_override_instants reports are the same for every page — every page holds every override's times and parse flags
 * — so a host asks page 0.
 * On page 0's stream, in order: that check; for every page its dense aggregate (beside its partial buffer) and its dry finalize
 * at t_0; the copy of the page descriptors; one launch of kt_forecast_paged (csrc/kt_kernels_forecast_paged.hip: one wave per
 * pod, lane = instant position, the two fail accumulators and `differs` kept across the pages, one walk of the overrides per page
 * and block of 64 instants); the copies out.  out_first [n] and out_verdicts [n][n_inst] are both nullable.
 * Refused before anything is launched, and before any page's check slot, reconcile report or result buffer is touched: what
 * kt_paged_admit refuses about the page set (different throttle-row counts, an engine named twice: KT_ERR_INVALID_ARGUMENT;
 * different devices: KT_ERR_UNSUPPORTED), what kt_forecast_launch refuses about its arguments (n_inst < 1, instants that are not
 * strictly ascending, an inst_ns outside [0, 10^9), a missing array: KT_ERR_INVALID_ARGUMENT; a pod row outside a page's
 * capacity, n x throttle_rows or n x n_inst above 2^31: KT_ERR_OUT_OF_RANGE), and what it refuses about an engine, asked of every
 * page: a KT_VARIANT_INCREMENTAL engine, an exchange world above 1, a `used` wider than int64 (KT_ERR_UNSUPPORTED) — as there,
 * the one thing that may run first is a page's kernel that sums the |requests|.  n == 0 is KT_OK and launches nothing.  Locking
 * (every page exclusively, in address order) and ordering are kt_paged_admit's.
 * Slots: the call uses page 0's check slot (a pending kt_check_launch / kt_headroom_launch of page 0 is dropped) and page 0's
 * forecast result buffers, grown only once the stream of an unfetched launch has drained — the results are handed out by the call,
 * so a forecast that was pending on page 0 is gone afterwards (kt_forecast_fetch answers KT_ERR_NOT_READY) while a pending
 * kt_preempt_launch result of page 0 stays fetchable; every page's dry finalize writes that page's reconcile result buffers, so
 * every page's pending reconcile report is dropped (a status stored with KT_RECONCILE_APPLY stays stored); a pending
 * kt_aggregate_launch of any page keeps its sums.  The call is a dry run: stored status and reserved amounts of no page change.
 * A device error after the first launch is returned once the stream has drained; no page keeps a pending result.
 * Out of scope: several ranks. */
int32_t kt_paged_forecast(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s,
                          const int32_t* inst_ns, int32_t on_equal, int64_t* out_first /* [n], nullable */,
                          uint8_t* out_verdicts /* [n][n_inst], nullable */);
/* kt_forecast_gangs_launch + kt_forecast_gangs_fetch over pages, synchronous: what they return for the gangs [gang_off[g],
 * gang_off[g + 1]) of pod_rows on the cluster of ALL names.  The definition (R_t, the dry kt_admit_gangs_launch of the one gang,
 * Reserve, verdicts, first, blocker) is kt_forecast_gangs_launch's; the rules about pages are kt_paged_forecast's (ONE check of page
 * 0 over pod_rows, `stored` and `calc_at_any` as an OR over the pages, `differs` as an OR over EVERY page, the throttle reads
 * status.calculatedThreshold on every page iff calc_at_any || differs) and kt_paged_preempt_gangs' (an admitted member reserves on
 * EVERY page, each page from its own stored reserved row: the value of every name of that page it carries, the presence of all
 * of them, and on page 0 count + 1; the pod count is judged on page 0 only; the blocker is the minimum over throttles AND pages of
 * the first stopped queue position — the first member that stops on some page has met exact reserved prefixes there, and no page
 * stops an earlier one).
 * The answer is NOT a combination of existing calls.  The members' own paged forecasts do not compose: each admitted member reserves
 * against the throttles the later members meet (two members asking 3 each of a page-1 name with `used` 4 under a spec of 8: each
 * member alone passes at every instant, the gang only inside an override of 10).  The pages' own gang forecasts do not compose
 * either: the calculated threshold is replaced as a whole, so a page that holds nothing the gang requests can replace the
 * threshold for the pages that do, at some instants and not at others.
 * Identities:
 *   - n_pages == 1 returns byte for byte what kt_forecast_gangs_launch + kt_forecast_gangs_fetch return on that engine;
 *   - a gang of one pod reports byte for byte what kt_paged_forecast reports for that pod (blocker: its own position where it is
 *     not Success);
 *   - with inst = [now], out_first[g] == 0 exactly where kt_paged_preempt_gangs at `now` with no candidates reports prefix 0, and
 *     out_blocker[g][0] equals its out_blocker[g].
 * On page 0's stream, in order: that check; for every page its dense aggregate and its dry finalize at t_0; the copies of the gang
 * offsets and the page descriptors; one launch of kt_forecast_gangs_paged (csrc/kt_kernels_forecast_gangs_paged.hip: one wave per
 * gang, lane = instant position; per throttle and block of 64 instants one pass over the pages' overrides that settles `differs`,
 * skipped where calc_at_any holds, and one pass that walks the members once per page); the copies out.  out_first [n_gangs],
 * out_verdicts and out_blocker [n_gangs][n_inst] are all nullable.
 * Refused before anything is launched, and before any page's check slot, reconcile report or result buffer is touched, the
 * instants first: what kt_forecast_gangs_launch refuses about its arguments (n_inst < 1, instants that are not strictly ascending,
 * an inst_ns outside [0, 10^9), a missing array, every gang_off defect, a pod named twice within ONE gang: KT_ERR_INVALID_ARGUMENT;
 * a pod row outside a page's capacity, n x throttle_rows or n_gangs x n_inst above 2^31: KT_ERR_OUT_OF_RANGE), what kt_paged_forecast
 * refuses about the page set (different throttle-row counts, an engine named twice: KT_ERR_INVALID_ARGUMENT; different devices:
 * KT_ERR_UNSUPPORTED) and about every page's engine (a KT_VARIANT_INCREMENTAL engine, an exchange world above 1, a `used` wider
 * than int64: KT_ERR_UNSUPPORTED) — as there, the one thing that may run first is a page's kernel that sums the |requests|.
 * n == 0 is allowed only with n_gangs == 0: KT_OK, nothing is launched.  Locking and ordering are kt_paged_admit's.
 * Slots: kt_paged_forecast's.  The call uses page 0's check slot and page 0's forecast result buffers and hands the results out:
 * afterwards no forecast result of either kind is pending on page 0 (kt_forecast_fetch and kt_forecast_gangs_fetch answer
 * KT_ERR_NOT_READY) while a pending preempt result of page 0 stays fetchable; every page's pending reconcile report is dropped; a
 * pending kt_aggregate_launch of any page keeps its sums.  The call is a dry run: stored status and reserved amounts of no page
 * change.  A device error after the first launch is returned once the stream has drained; no page keeps a pending result.
 * Out of scope: several ranks. */
int32_t kt_paged_forecast_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                const int64_t* gang_off, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal,
                                int64_t* out_first /* [n_gangs], nullable */, uint8_t* out_verdicts /* [n_gangs][n_inst], nullable */,
                                int64_t* out_blocker /* [n_gangs][n_inst], nullable */);
/* kt_headroom_forecast_launch + kt_headroom_forecast_fetch over the pages, synchronous: what they return on the cluster of ALL
 * names.  out_copies[i][k] is the number of leading Success verdicts of a dry kt_paged_admit over [p_i] * cap with R_{t_k} as the
 * stored status of every page (every valid and responsible throttle reconciled at t_k on every page, on the state as it is now);
 * out_limiting[i][k] is the lowest throttle row whose COMBINED status is not KT_STATUS_NOT_THROTTLED in the row the first refused
 * copy gets, and -1 where all `cap` copies are admitted; out_first[i] is the smallest k with out_copies[i][k] >= want, or
 * KT_FORECAST_NONE.  A pod whose PreFilter is an Error on page 0, or whose row is invalid: 0 / -1 / KT_FORECAST_NONE.  A pod no
 * throttle affects: cap / -1 / 0.  Negative requests are served, as kt_headroom_launch and kt_paged_headroom serve them.
 * The answer is NOT a combination of existing calls.  The minimum of the pages' own kt_headroom_forecast_launch answers is wrong:
 * status.calculatedThreshold is compared and replaced as a whole, so a page that holds nothing the pod requests can replace the
 * threshold for the pages that do, at some instants and not at others.  kt_paged_headroom once per instant would need the status
 * applied at each instant: not a dry run.
 * The rules about pages are kt_paged_forecast's, word for word: the affecting throttles come from ONE check of page 0; `stored` and
 * `calc_at_any` are ORs over the pages; `differs` is the OR over EVERY page (pages none of whose names the pod requests included;
 * page 0 adds the count comparison); the throttle reads status.calculatedThreshold on every page iff calc_at_any || differs, else
 * spec.threshold on every page; status.throttled is IsThrottled(used, true) against the calculated threshold either way.  The
 * rules about headroom are kt_paged_headroom's: the pod count is judged on page 0 only; each page judges its own names against its
 * own reserved row and presence bits; the throttle's number is the minimum over the count and every needed name of every page;
 * the answer is the lexicographic minimum of (copies, throttle row) over the affecting throttles.
 * Identities:
 *   (P1) n_pages == 1 returns byte for byte what kt_headroom_forecast_launch + kt_headroom_forecast_fetch return on that engine.
 *   (I1) with cap == want == 1, out_copies[i][k] == 1 exactly where kt_paged_forecast reports KT_VERDICT_SUCCESS and out_first is
 *        byte for byte kt_paged_forecast's; an Error verdict is 0 copies and limiting -1, a Block verdict limiting >= 0.
 *   (I2) with inst = [t] on pages whose last action was kt_paged_reconcile(t, KT_RECONCILE_APPLY) and whose stored calculatedAt
 *        flags then agree across the pages for every affecting throttle, out_copies[:][0] and out_limiting[:][0] are byte for byte
 *        kt_paged_headroom's with the same cap and on_equal.  Where the flags disagree this call follows kt_paged_forecast (the
 *        throttle has been replaced once some page says so: calc_at_any) and kt_paged_headroom reads each page's own flag.
 *   (I3) the call is a dry run: stored status, reserved amounts and a pending kt_aggregate_launch's sums are unchanged on every page.
 * On page 0's stream, in order: that check; for every page its dense aggregate and its dry finalize at t_0; the copy of the page
 * descriptors; one launch of kt_headroom_forecast_paged (csrc/kt_kernels_headroom_forecast_paged.hip: one wave per pod, lane =
 * instant position; `differs` and the two running minima against the calculated and the spec threshold kept across the pages, one
 * walk of the overrides per page and block of 64 instants); the copies out.  All three outputs are nullable.
 * Refused before anything is launched, and before any page's check slot, reconcile report or result buffer is touched, in this
 * order: a missing page array, n_pages < 1, a NULL page, n < 0 (KT_ERR_INVALID_ARGUMENT); the instants as kt_forecast_launch
 * refuses them and a missing pod_rows with n > 0 (KT_ERR_INVALID_ARGUMENT); cap outside [1, KT_HEADROOM_MAX_CAP], then want outside
 * [1, cap] (KT_ERR_INVALID_ARGUMENT); what kt_paged_admit refuses about the page set and the rows (different throttle-row counts,
 * an engine named twice: KT_ERR_INVALID_ARGUMENT; different devices: KT_ERR_UNSUPPORTED; a pod row outside a page's capacity:
 * KT_ERR_OUT_OF_RANGE); n x throttle_rows or n x n_inst above 2^31 (KT_ERR_OUT_OF_RANGE); and what kt_forecast_launch refuses about
 * an engine, asked of every page: a KT_VARIANT_INCREMENTAL engine, an exchange world above 1, a `used` wider than int64
 * (KT_ERR_UNSUPPORTED) — as in kt_paged_forecast, the one thing that may run first is a page's kernel that sums the |requests|.
 * n == 0 is KT_OK and launches nothing.  Locking and ordering are kt_paged_admit's.
 * Slots: kt_paged_forecast's.  The call uses page 0's check slot and page 0's forecast result buffers, grown only once the stream
 * of an unfetched launch has drained, and hands the results out: afterwards no forecast result of any kind is pending on page 0
 * (kt_forecast_fetch, kt_forecast_gangs_fetch and kt_headroom_forecast_fetch answer KT_ERR_NOT_READY) while a pending preempt
 * result of page 0 stays fetchable; every page's pending reconcile report is dropped.  A device error after the first launch is
 * returned once the stream has drained; no page keeps a pending result.
 * Whole gangs: kt_paged_headroom_forecast_gangs.  Out of scope: several ranks. */
int32_t kt_paged_headroom_forecast(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_inst,
                                   const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, int64_t cap, int64_t want,
                                   int64_t* out_first /* [n], nullable */, int64_t* out_copies /* [n][n_inst], nullable */,
                                   int32_t* out_limiting /* [n][n_inst], nullable */);
/* kt_headroom_forecast_gangs_launch + kt_headroom_forecast_gangs_fetch over the pages, synchronous: what they return on the cluster
 * of ALL names.  out_copies[g][k] is the number of leading admitted gangs of a dry kt_paged_admit_gangs over `cap` consecutive
 * copies of gang g with R_{t_k} as the stored status of every page (every valid and responsible throttle reconciled at t_k on every
 * page, on the state as it is now); out_blocker[g][k] is the queue position of the first member of the first refused copy whose
 * COMBINED verdict is not Success; out_limiting[g][k] is the lowest throttle row whose combined status is not
 * KT_STATUS_NOT_THROTTLED in that member's row at its turn.  Both are -1 where all `cap` copies pass; limiting is also -1 where the
 * blocker's verdict is an Error.  out_first[g] is the smallest k with out_copies[g][k] >= want, or KT_FORECAST_NONE.  A gang with an
 * Error or invalid member reports 0 copies at every instant: its walk ends in front of that member, and an earlier member that some
 * throttle stops at t_k on some page is the blocker there.  A gang no throttle affects: cap / -1 / -1 and first 0.
 * The answer is NOT a combination of existing calls.  The minimum of the pages' own kt_headroom_forecast_gangs_launch answers is
 * wrong: status.calculatedThreshold is compared and replaced as a whole, so a page that holds nothing the gang requests can replace
 * the threshold for the pages that do, at some instants and not at others.  kt_paged_headroom_gangs once per instant would need the
 * status applied at each instant — not a dry run — and reads each page's own calculatedAt flag, not the forecast's whole-throttle
 * rule.
 * The rules about pages and thresholds are kt_paged_forecast_gangs', word for word: the affecting throttles and the Error members
 * come from ONE check of page 0; `stored` and `calc_at_any` are ORs over the pages; `differs` is the OR over EVERY page (pages none
 * of whose names any member requests included; page 0 adds the count comparison); the throttle reads status.calculatedThreshold on
 * every page iff calc_at_any || differs, else spec.threshold on every page; the throttled bits are IsThrottled(used, true) against
 * the calculated threshold either way.  A throttle that keeps its stored status — its reconcile is an error, or it is not valid and
 * responsible, on some page — is read on every page against its stored calculated threshold where calc_at_any holds and against
 * spec.threshold otherwise: NOT the page's own calculatedAt flag, which kt_paged_headroom_gangs reads.
 * The rules about pages and copies are kt_paged_headroom_gangs': an admitted copy reserves on every page, each page its own names'
 * values and the presence of the names a member carries there; the pod count is judged and reserved once, on page 0; copy j passes
 * on throttle t iff the in-order member walk passes on every page, each page against its own reserved row plus j x what one copy
 * reserves there; per instant every (throttle, page) pair is a throttle of its own and the answer is the lexicographic minimum over
 * the pairs of (copies, first stopped position, throttle row); a page k != 0 none of whose names an affected member requests with
 * a non-zero value is skipped in the walk — never in `differs`.
 * Identities:
 *   (P1) n_pages == 1 returns byte for byte what kt_headroom_forecast_gangs_launch + kt_headroom_forecast_gangs_fetch return on
 *        that engine.
 *   (G1) a gang of one pod reports byte for byte the first, copies and limiting of kt_paged_headroom_forecast for that pod; its
 *        blocker is its own position where copies < cap, else -1.
 *   (G2) with cap == want == 1, out_copies[g][k] == 1 exactly where kt_paged_forecast_gangs reports KT_VERDICT_SUCCESS; out_first
 *        and out_blocker are byte for byte its own.
 *   (G3) with inst = [t] on pages whose last action was kt_paged_reconcile(t, KT_RECONCILE_APPLY) and whose stored calculatedAt
 *        flags then agree across the pages for every affecting throttle, column 0 is byte for byte kt_paged_headroom_gangs' answer
 *        with the same cap and on_equal.  Where the flags disagree this call follows kt_paged_forecast_gangs (the throttle has been
 *        replaced once some page says so: calc_at_any) and kt_paged_headroom_gangs reads each page's own flag.
 *   (G4) the call is a dry run: stored status, reserved amounts and a pending kt_aggregate_launch's sums are unchanged on every
 *        page.
 * On page 0's stream, in order: that check; for every page its dense aggregate and its dry finalize at t_0; the copies in (the
 * instants, the gang offsets, the page descriptors); one launch of kt_headroom_forecast_gangs_paged
 * (csrc/kt_kernels_headroom_forecast_gangs_paged.hip: one wave per gang, lane = instant position; per block of 64 instants a first
 * pass over the pages for `differs`, a second in which every lane searches the copies of its own instant page by page, its range
 * cut at its running minimum over the pairs before); the copies out.  All four outputs are nullable.
 * Refused before anything is launched, and before any page's check slot, reconcile report or result buffer is touched, in this
 * order: a missing page array, n_pages < 1, a NULL page, n < 0 (KT_ERR_INVALID_ARGUMENT); the instants as kt_forecast_launch
 * refuses them and a missing array (KT_ERR_INVALID_ARGUMENT); cap outside [1, KT_HEADROOM_MAX_CAP], then want outside [1, cap]
 * (KT_ERR_INVALID_ARGUMENT); every gang_off defect kt_admit_gangs_launch refuses and a pod named twice within ONE gang
 * (KT_ERR_INVALID_ARGUMENT); what kt_paged_admit refuses about the page set and the rows (different throttle-row counts, an engine
 * named twice: KT_ERR_INVALID_ARGUMENT; different devices: KT_ERR_UNSUPPORTED; a pod row outside a page's capacity:
 * KT_ERR_OUT_OF_RANGE); n x throttle_rows or n_gangs x n_inst above 2^31 (KT_ERR_OUT_OF_RANGE); what kt_forecast_gangs_launch
 * refuses about an engine, asked of every page: a KT_VARIANT_INCREMENTAL engine, an exchange world above 1, a `used` wider than
 * int64 (KT_ERR_UNSUPPORTED) — as in the siblings, the one thing that may run first is a page's kernel that sums the |requests|;
 * and last an engine that has been fed a negative request, on ANY page (KT_ERR_UNSUPPORTED: the search over the copies rests on
 * sums that only grow; kt_paged_headroom_forecast serves such pages pod by pod).
 * n == 0 is allowed only with n_gangs == 0: KT_OK, nothing is launched.  Locking and ordering are kt_paged_admit's.
 * Slots: kt_paged_forecast's.  The call uses page 0's check slot and page 0's forecast result buffers, grown only once the stream
 * of an unfetched launch has drained, and hands the results out: afterwards no forecast result of any kind is pending on page 0
 * (kt_forecast_fetch, kt_forecast_gangs_fetch, kt_headroom_forecast_fetch and kt_headroom_forecast_gangs_fetch answer
 * KT_ERR_NOT_READY) while a pending preempt result of page 0 stays fetchable; every page's pending reconcile report is dropped; a
 * pending kt_aggregate_launch of any page keeps its sums.  A device error after the first launch is returned once the stream has
 * drained; no page keeps a pending result.
 * Out of scope: several ranks. */
int32_t kt_paged_headroom_forecast_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                         const int64_t* gang_off, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns,
                                         int32_t on_equal, int64_t cap, int64_t want, int64_t* out_first /* [n_gangs], nullable */,
                                         int64_t* out_copies /* [n_gangs][n_inst], nullable */,
                                         int32_t* out_limiting /* [n_gangs][n_inst], nullable */,
                                         int64_t* out_blocker /* [n_gangs][n_inst], nullable */);

/* Development aid: the engine reads its A/B switches (KT_NO_* / KT_SYNC_INGEST ... environment variables, all off by default)
 * once, at kt_engine_create; a tool that flips one on a live engine calls this afterwards. */
int32_t kt_debug_reload_env(kt_engine* e);

/* Development aid: a copy of the match cache as the last cached scan left it, for tests of what its two copies owe each other
 * (the view's words of record j are the table's words of pod row out_rows[j], in every plane, zeroes past a list's end included).
 *   which = 0: the table.               n = the pod rows ever fed; out[k * cap + r] = word k of pod row r.
 *   which = 1: the countable scan view. n = its records (the appended ones included); out[k * cap + j] = word k of record j,
 *                                       out_rows[j] (nullable) = the pod row of record j.
 * *out_n and *out_planes are always set; with cap = 0 nothing else is written (the sizing call), otherwise cap >= n is required
 * (KT_ERR_OUT_OF_RANGE).  KT_ERR_NOT_READY where there is nothing current to copy: no table built for this program, rows still
 * waiting for their refresh, or (which = 1) a view whose planes were not gathered.  Waits for the engine's last launch. */
int32_t kt_debug_match_planes(kt_engine* e, int32_t which, int64_t cap, uint64_t* out, int64_t* out_rows, int64_t* out_n, int32_t* out_planes);

/* Development aid: the match-code records beside that table (one 16-byte record per pod row: byte 0 the count 0..15 or 0xFF for
 * "more than 15: read the planes", bytes 1..15 the codes k << 6 | bit in ascending order — the terms of plane k the PreFilter
 * sweep's run rule leaves), for tests that decode them against the planes.  Same protocol as kt_debug_match_planes:
 *   which = 0: out[2 * r], out[2 * r + 1] = the low and high eight bytes of the record of pod row r; out_rows is not written.
 *   which = 1: the countable scan view's records (what the cached aggregate replays), record j of pod row out_rows[j] (nullable).
 * KT_ERR_NOT_READY also where the table has more planes than a record can name (no records are kept). */
int32_t kt_debug_match_codes(kt_engine* e, int32_t which, int64_t cap, uint64_t* out, int64_t* out_rows, int64_t* out_n);
/* Development aid, host side only: what plane k means for the pods of namespace row ns_row in the compiled single-chunk program —
 * *out_word = the word of term numbers at position k of the namespace's list (-1: the list is shorter), *out_lo / *out_hi = the
 * run masks of that word the records are cut with (all ones where no throttle of the program has several terms: the rule
 * x & ~((x | hi) - lo) then keeps everything).  KT_ERR_NOT_READY without a current single-chunk program. */
int32_t kt_debug_match_runs(kt_engine* e, int32_t ns_row, int32_t k, int32_t* out_word, uint64_t* out_lo, uint64_t* out_hi);

#ifdef __cplusplus
}
#endif
#endif /* KT_ENGINE_H */
