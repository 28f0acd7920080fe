// kt_engine_check.cpp — KubeThrottler.PreFilter (plugin.go:148-215) behind the C-ABI: the sweep over every pod, checks of a few
// pods (kt_check: the scheduler's call), admission queues with reservation, affected pods, and the paged forms for more than
// 16 resource names.
#include "kt_engine_impl.h"

// ---------------------------------------------------------------------------------------------------
// check
// ---------------------------------------------------------------------------------------------------
// The CheckRecs only depend on (stored status, reserved amounts, isThrottledOnEqual): rebuilt when one of them changed
// since they were last built (by kt_prepare_check or by kt_finalize with APPLY)
static int32_t ensure_check_recs(kt_engine* e, int32_t on_equal, int DT, hipStream_t s) {
  if (e->recs_valid && e->recs_eq == (on_equal != 0) && e->recs_DT == DT) return KT_OK;
  recs_invalidate_and_drain(e);  // rebuilt in place
  {
    TimedLaunch tl(e, KT_KERNEL_PREPARE, s);
    kt::launch_prepare_check(e->tt, e->thr_rows_hi, e->D, DT, on_equal != 0, e->recs_ptr(), req_bound(e), s);
  }
  if (e->few_ready) KT_HIP(e, hipEventRecord(e->recs_ev[e->recs_cur], s));
  std::lock_guard<std::mutex> g(e->recs_mu);
  e->recs_ev_pending[e->recs_cur] = e->few_ready;
  e->recs_prev_valid = false;  // records of an older status / other on_equal: not a substitute any more
  ++e->recs_seq[e->recs_cur];
  e->recs_valid = true;
  e->recs_eq = on_equal != 0;
  e->recs_DT = DT;
  return KT_OK;
}

// The match cache (kt_engine_impl.h), made current for a scan that will be enqueued on s right behind this call: built by one
// launch over every row when the program was compiled or the tables cleared since, else the rows pod events upserted since are
// refreshed by one launch of the list form.  Either launch writes through to the planes of the countable scan view where those
// are valid (ScanView::mx_valid) — also the full build: a table that went void under a valid view (more than kPatchBatchMax
// pending rows) comes back with the view's planes current, no second gather.
// Stream order of the write-through: the row -> record table and the appended records are written by kt_patch_scan_views on the
// FEED's stream, this launch runs on the SCAN's.  The pair is ordered as the atom rows this launch reads always were — they are
// written by the same feed launches: every launch-side call settles the feed on the host first (LaunchLock: settle_ingest) and
// order_behind_ingest puts s behind the feed kernel's event on the device while that kernel may not have retired; the other way
// round, the caller leaves s in last_stream and a feed call synchronises a last_stream that is not its own before it writes.  mc.mw stays nullptr where there is no table: the switch, a program the cache does
// not take (several chunks, slow shapes, overflow pods, more than 8 dimensions, a namespace word list longer than kMatchReplay, a
// check footprint that does not fit one CU twice), nothing fed yet.
int32_t match_cache_for_scan(kt_engine* e, hipStream_t s, kt::MatchCacheArgs& mc) {
  mc = kt::MatchCacheArgs();
  if (e->sw[kSw_NO_MATCH_CACHE] || e->cfg.kernel_variant != 0 || e->incremental || e->program_dirty || e->pod_rows_hi <= 0) return KT_OK;
  if (!kt::match_cache_fits(e->dindex) || e->hindex.has_slow || e->n_overflow != 0 || e->pods.LA > 8 || !e->pods.latom) return KT_OK;
  if (e->mc_planes_gen != e->program_gen) {  // the longest namespace word list of the (single) chunk: the planes a pod needs
    const kt::BmChunk& ch = e->dindex.h_chunks[0];
    const uint32_t* rng = (const uint32_t*)(e->hindex.bm_images.data() + ch.img_off + ch.off_nsl_rng);
    uint32_t longest = 0;
    for (uint32_t n = 0; n < e->hindex.n_ns; ++n) longest = std::max(longest, rng[2 * n + 1] - rng[2 * n]);
    e->mc_planes = longest, e->mc_planes_gen = e->program_gen;
    e->ctr_mc_planes.store((int64_t)longest, std::memory_order_relaxed);
  }
  const uint32_t planes = e->mc_planes;
  // (the dispatch's own predicate: a table the sweep would not replay is neither built nor refreshed)
  if (!kt::check_replays_match_cache(e->pods, e->sp, e->dindex, planes, e->n_overflow != 0, e->sw[kSw_CHECK_ONE_PER_CU])) return KT_OK;
  const uint64_t stride = (uint64_t)e->cfg.pod_capacity;
  ScanView& cv = e->views.countable;
  kt::MatchViewPlanes vp;
  const bool recs = kt::match_codes_fit(e->dindex, planes);  // does the table keep match-code records for this program
  if (cv.valid && cv.mx_valid && cv.mx.p && cv.pos.p && cv.mx_planes == planes && e->mc_gen == e->program_gen &&
      (!recs || (cv.mc_there && cv.mc.cap >= (size_t)cv.cap + 1)))
    vp.mx = cv.mx.p, vp.pos = cv.pos.p, vp.stride = (uint64_t)cv.cap + 1u, vp.mc = recs ? cv.mc.p : nullptr;
  else
    cv.mx_valid = false;  // (this call may write words the view's planes do not get: gathered again before they are replayed)
  if (!e->mc_valid || e->mc_gen != e->program_gen) {
    // (with vp set — the write-through of a FULL build — only in views of more than 2^20 records: the table goes void under a
    //  valid view when more than kPatchBatchMax rows are pending in batches that all fit the view's headroom, cv.extra grows at
    //  least as fast as the pending list, and the headroom passes kPatchBatchMax only as n / 16.  A compile voids the view too.)
    if (e->d_mc.cap < (size_t)planes * stride || (recs && e->d_mcodes.cap < (size_t)stride)) {
      if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));  // an earlier scan may still read the old table
      KT_HIP(e, e->d_mc.reserve((size_t)planes * stride));
      if (recs) KT_HIP(e, e->d_mcodes.reserve((size_t)stride));
    }
    order_behind_ingest(e, s);
    if (!kt::launch_build_match_cache(e->pods, e->pod_rows_hi, nullptr, e->dindex, e->d_mc.p, stride, planes, s, &vp, recs ? e->d_mcodes.p : nullptr)) {
      cv.mx_valid = false;
      return KT_OK;
    }
    KT_HIP(e, hipGetLastError());
    e->mc_valid = true, e->mc_gen = e->program_gen;
    e->mc_pending.clear();
    e->ctr_mc_builds.fetch_add(1, std::memory_order_relaxed);
  } else if (!e->mc_pending.empty()) {
    const size_t n = e->mc_pending.size();
    // the kernel reads the list where it lies, in a pinned buffer of its own, as the feed kernels read their event slots: no
    // copy and no host wait — the launch is all the first sweep after a pod event pays (a copy engine's trip in front of it
    // cost 7 us where the launch costs 3.5: profiles/match_cache.txt); an event behind the refresh says when the buffer of the
    // previous one is free again — long ago, as a rule
    if (!e->h_mc_rows) {
      KT_HIP(e, hipHostMalloc((void**)&e->h_mc_rows, (size_t)kPatchBatchMax * 8, hipHostMallocDefault));
      KT_HIP(e, hipEventCreateWithFlags(&e->mc_rows_ev, hipEventDisableTiming));
    } else if (e->mc_rows_ev_used) {
      KT_HIP(e, hipEventSynchronize(e->mc_rows_ev));
    }
    memcpy(e->h_mc_rows, e->mc_pending.data(), n * 8);
    order_behind_ingest(e, s);
    if (!kt::launch_build_match_cache(e->pods, (int64_t)n, e->h_mc_rows, e->dindex, e->d_mc.p, stride, planes, s, &vp, recs ? e->d_mcodes.p : nullptr)) {
      e->mc_valid = false, cv.mx_valid = false;
      e->mc_pending.clear();
      return KT_OK;
    }
    KT_HIP(e, hipGetLastError());
    KT_HIP(e, hipEventRecord(e->mc_rows_ev, s));
    e->mc_rows_ev_used = true;
    e->mc_pending.clear();
  }
  mc.mw = e->d_mc.p, mc.stride = stride, mc.planes = planes;
  // (the refresh path found the records' buffer as the build left it: both are reserved together, for the same capacity)
  if (recs && e->d_mcodes.p && e->d_mcodes.cap >= (size_t)stride) mc.codes = e->d_mcodes.p;
  return KT_OK;
}

// allow_small: false for callers that go on working on the device-side rows / summaries (kt_admit_launch)
static int32_t check_launch_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                                   hipStream_t s, bool allow_small = true) {
  e->headroom_ready = false;  // the one check slot is taken: a pending kt_headroom_launch is gone
  e->preempt_ready = false;   // ... and a pending kt_preempt_launch
  e->forecast_ready = false;  // ... and a pending kt_forecast_launch
  if (pod_rows) {
    for (int64_t i = 0; i < n; ++i)
      if (pod_rows[i] < 0 || pod_rows[i] >= e->cfg.pod_capacity)
        return e->fail(KT_ERR_OUT_OF_RANGE, "pod row %lld", (long long)pod_rows[i]);
  } else if (n > e->cfg.pod_capacity) {
    return e->fail(KT_ERR_OUT_OF_RANGE, "n=%lld > pod_capacity", (long long)n);
  }
  int32_t rc = ensure_ready(e, s);
  if (rc != KT_OK) return rc;
  const bool want_status = (flags & KT_CHECK_STATUS_MATRIX) != 0;
  const size_t T = (size_t)e->thr_rows_hi;
  if (e->d_summary.cap < (size_t)n + 1 || (want_status && e->d_status.cap < (size_t)n * T + 64) ||
      (pod_rows && e->d_rows.cap < (size_t)n + 1)) {
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));  // buffers may still be in use
    KT_HIP(e, e->d_summary.reserve((size_t)n + 1));
    if (want_status) KT_HIP(e, e->d_status.reserve((size_t)n * T + 64));  // slack: kt_admit reads rows 16 bytes at a time
    if (pod_rows) KT_HIP(e, e->d_rows.reserve((size_t)n + 1));
  }
  // a handful of pods (one PreFilter call): rows by value, one workgroup per index chunk, summaries to pinned memory
  const bool small = allow_small && e->cfg.kernel_variant != 1 && n > 0 && n <= kt::kCheckSmallMax;
  kt::CheckSmall sm{};
  if (small) {
    if (!e->h_small) {
      KT_HIP(e, hipHostMalloc((void**)&e->h_small, (size_t)kt::kCheckSmallMax * 8, hipHostMallocMapped));
      KT_HIP(e, e->d_ticket.reserve(16));
      KT_HIP(e, hipMemsetAsync(e->d_ticket.p, 0, 16 * 4, s));
    }
    sm.ticket = e->d_ticket.p;
    sm.host_summary = e->h_small;
    if (pod_rows && n <= 8) {
      sm.n_inline = (uint32_t)n;
      for (int64_t k = 0; k < 8; ++k) sm.inline_rows[k] = pod_rows[k < n ? k : n - 1];
    }
  }
  if (pod_rows && n && !sm.n_inline) {
    KT_HIP(e, hipMemcpyAsync(e->d_rows.p, pod_rows, (size_t)n * 8, hipMemcpyHostToDevice, s));
    KT_HIP(e, hipStreamSynchronize(s));  // caller memory must not be referenced after return
  }
  // the record layout follows the scan kernel that will read it
  const int DT = e->cfg.kernel_variant == 1 ? kt::dt_bucket(e->D) : kt::dt_bucket_ix(e->D);
  if ((rc = ensure_check_recs(e, on_equal, DT, s)) != KT_OK) return rc;
  // the sweep of every row of a single-chunk program replays the match cache (the few-pod, small, row-subset and status-matrix
  // forms neither read nor refresh it: the path from a pod event to its PreFilter stays as short as it was); a build or a
  // refresh of the table is enqueued here, ahead of the check's timed launch
  kt::MatchCacheArgs mc;
  if (e->cfg.kernel_variant != 1 && !pod_rows && !small && !want_status && n > 0 && n <= e->cfg.pod_capacity && e->dindex.n_chunks == 1 &&
      !e->sw[kSw_FORCE_NS_ORDER] && !e->sw[kSw_CHECK_ONE_PER_CU]) {
    if ((rc = match_cache_for_scan(e, s, mc)) != KT_OK) return rc;
    if (e->sw[kSw_NO_MATCH_CODES]) mc.codes = nullptr;  // (the records stay current; the sweep replays the planes)
    mc.tile_pairs = !e->sw[kSw_NO_TILE_PAIRS_CHECK];
  }
  {
    TimedLaunch tl(e, KT_KERNEL_CHECK, s);
    if (e->cfg.kernel_variant == 1)
      kt::launch_check_dense(e->pods, n, pod_rows ? e->d_rows.p : nullptr, e->sp, e->uses_keys, e->recs_ptr(),
                             e->d_summary.p, want_status ? e->d_status.p : nullptr, s),
          e->last_kernel[KT_KERNEL_CHECK] = "kt_check_dense";
    else {
      // a sweep over every row of a multi-chunk index runs in namespace order (results stay indexed by pod row)
      const bool by_ns = !pod_rows && !small && n == e->pod_rows_hi && (e->dindex.n_chunks > 1 || e->sw[kSw_FORCE_NS_ORDER]) && !e->sw[kSw_NO_NS_ORDER];
      if (by_ns && (rc = settle_view_patches(e, s)) != KT_OK) return rc;
      ScanView& av = e->views.all_rows;
      if (by_ns && (!av.valid || (int64_t)av.n != e->pod_rows_hi)) {  // every row is listed: the view holds pod_rows_hi records
        const ViewSpec spec{/*countable_only=*/false, /*by_ns=*/true, kt::check_sweep_blocks, e->pod_rows_hi, /*requests=*/false};
        KT_HIP(e, e->d_carry.reserve((size_t)e->pod_rows_hi + 1));
        if ((rc = list_view_rows(e, av, spec, s)) != KT_OK) return rc;
        if ((rc = copy_view_records(e, av, spec, /*headroom=*/0, s)) != KT_OK) return rc;
        av.valid = true;
      }
      kt::CheckByNs view{av.meta.p, av.latom.p, e->d_carry.p};
      if (by_ns && av.range_G) view.wg_range = av.range.p, view.wg_range_G = av.range_G;
      if (by_ns && !want_status && e->dindex.n_slow == 0 && e->n_overflow == 0 && e->dindex.n_chunks > 1 && !e->sw[kSw_NO_VERDICT_IMAGES]) {
        // the lean sweep of a multi-chunk program: TermInfo + WordVerdict of every word once per generation of CheckRecs
        // (one small launch) instead of once per (workgroup, chunk) — 256 x ~15 rebuilds of the same words
        const int b = e->recs_cur;
        if (e->wvimg_seq[b] != e->recs_seq[b] || e->wvimg_gen[b] != e->program_gen || e->wvimg_DT[b] != DT) {
          KT_HIP(e, e->d_wvimg[b].reserve(kt::verdict_images_bytes(e->dindex.bm_words, e->D)));
          TimedLaunch tl2(e, KT_KERNEL_PREPARE, s);
          kt::launch_build_verdict_images(e->dindex, e->dindex.bm_words, e->recs_ptr(), e->thr_rows_hi, e->D, e->d_wvimg[b].p, s);
          e->wvimg_seq[b] = e->recs_seq[b], e->wvimg_gen[b] = e->program_gen, e->wvimg_DT[b] = DT;
        }
        view.wv_img = e->d_wvimg[b].p, view.wv_total_words = e->dindex.bm_words;
      }
      const char* k = kt::launch_check_indexed(e->pods, n, by_ns ? av.rows.p : pod_rows ? e->d_rows.p : nullptr, e->sp, e->d_sp.p, e->dindex,
                                               e->recs_ptr(), e->d_summary.p, want_status ? e->d_status.p : nullptr, s,
                                               small ? &sm : nullptr, e->n_overflow != 0, by_ns ? &view : nullptr, e->sw[kSw_CHECK_ONE_PER_CU],
                                               mc.mw ? &mc : nullptr);
      if (mc.used) e->ctr_mc_scans.fetch_add(1, std::memory_order_relaxed);
      if (!k) return e->fail(KT_ERR_UNSUPPORTED, "%d throttle rows exceed the indexed check kernel's LDS budget (use kernel_variant 1)", e->thr_rows_hi);
      e->last_kernel[KT_KERNEL_CHECK] = k;
    }
  }
  KT_HIP(e, hipGetLastError());
  e->check_n = n;
  e->check_in_h_small = small;
  e->check_T = e->thr_rows_hi;
  e->check_has_status = want_status;
  e->check_ready = true;
  e->last_stream = s;
  return KT_OK;
}

int32_t kt_check_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  return check_launch_locked(e, n, pod_rows, on_equal, flags, pick_stream(e, stream));
}

// kt_sweep_launch — the PreFilter sweep of every pod row against the STORED status and the reconcile of every throttle
// as one pass over the pod tables (kt_check_bitmap's AGG instantiation: one chunk prologue and one selector scan per pod
// where kt_check_launch + kt_reconcile_launch make two), then kt_reduce_finalize_packed.  Results are read with
// kt_check_fetch / kt_reconcile_fetch and are bit for bit those of kt_check_launch(all rows) followed by
// kt_reconcile_launch — which is also what runs when the fused kernel does not apply (several index chunks, a slow list,
// pods whose atoms overflow their row, requests that do not pack, wide sums, an incremental engine, the dense variant).
int32_t kt_sweep_launch(kt_engine* e, int64_t now_s, int32_t now_ns, uint32_t flags, int32_t on_equal, void* stream) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  int32_t rc = ensure_ready(e, s);
  if (rc != KT_OK) return rc;
  const int64_t n = e->pod_rows_hi;
  auto one_after_the_other = [&]() -> int32_t {
    int32_t r = check_launch_locked(e, n, nullptr, on_equal, 0u, s);
    if (r != KT_OK) return r;
    if ((r = aggregate_locked(e, s, /*allow_fused=*/true)) != KT_OK) return r;
    return finalize_locked(e, now_s, now_ns, flags, s, /*consume=*/!e->incremental);
  };
  bool fused = e->cfg.kernel_variant != 1 && !e->incremental && e->dindex.n_chunks == 1 && e->dindex.n_slow == 0 && !e->hindex.has_slow && !e->dindex.has_long &&
               e->n_overflow == 0 && e->thr_rows_hi > 0 && n > 0 && kt::dt_bucket_ix(e->D) == 8 && !e->sw[kSw_NO_SWEEP] &&
               !e->sw[kSw_NO_FUSED] && !e->sw[kSw_NO_PACK];
  if (!fused) return one_after_the_other();
  if ((rc = request_sums_in_range(e, s)) != KT_OK) return rc;
  if (e->wide) return one_after_the_other();
  // the packed fold's plan for THIS scan: every row of [0, n) in row order, aggregate_blocks(n) workgroups
  const int nb = kt::aggregate_blocks(n);
  kt::PackPlan plan = kt::make_pack_plan(e->D, e->max_abs, e->or_abs, e->neg_seen, kt::aggregate_slab_pods(n, nb), /*pad_odd=*/true, /*max_words=*/4);
  if (!plan.nw || plan.rec_bytes > kt::agg_rec_bytes(e->D, false)) return one_after_the_other();  // (slab areas hold plain records)
  const size_t words = (size_t)e->thr_rows_hi * kt::partial_stride(e->D);
  if (e->ext_partial && (int64_t)words > e->ext_partial_words)
    return e->fail(KT_ERR_OUT_OF_RANGE, "caller partial buffer holds %lld words, %lld needed", (long long)e->ext_partial_words, (long long)words);
  if (e->d_summary.cap < (size_t)n + 1) {
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));  // the buffer may still be in use
    KT_HIP(e, e->d_summary.reserve((size_t)n + 1));
  }
  const int DT = kt::dt_bucket_ix(e->D);
  if ((rc = ensure_check_recs(e, on_equal, DT, s)) != KT_OK) return rc;
  e->fused_pending = false;
  e->agg_wide = false;
  if (words && e->clean_partial != (const void*)e->partial()) KT_HIP(e, hipMemsetAsync(e->partial(), 0, words * 8, s));
  e->clean_partial = nullptr;
  kt::AggScan sc;
  if ((rc = slab_tags(e, sc, s)) != KT_OK) return rc;
  int launched = 0;
  const char* k;
  {
    TimedLaunch tl(e, KT_KERNEL_CHECK, s);
    k = kt::launch_sweep_indexed(e->pods, n, e->sp, e->d_sp.p, e->dindex, e->recs_ptr(), e->d_summary.p, plan, e->d_slab.p, sc.slab_tag, sc.epoch,
                                 &launched, s);
  }
  if (!k) return one_after_the_other();  // (LDS: check tables + fold tables of this program do not fit one workgroup)
  if (launched != nb) return e->fail(KT_ERR_DEVICE, "kt_sweep_launch: %d workgroups launched, the packed fields were planned for %d", launched, nb);
  KT_HIP(e, hipGetLastError());
  e->last_kernel[KT_KERNEL_CHECK] = k;
  e->last_kernel[KT_KERNEL_AGGREGATE] = "(in kt_sweep_bitmap)";
  e->last_kernel[KT_KERNEL_REDUCE] = "(in kt_reduce_finalize_packed)";
  e->check_n = n, e->check_in_h_small = false, e->check_T = e->thr_rows_hi, e->check_has_status = false, e->check_ready = true;
  e->headroom_ready = false, e->preempt_ready = false, e->forecast_ready = false;
  e->fused_pending = true, e->fused_nb = launched, e->fused_epoch = sc.epoch, e->fused_pack = plan;
  e->agg_pending = true, e->agg_words = words, e->agg_gen = e->program_gen;
  e->last_stream = s;
  return finalize_locked(e, now_s, now_ns, flags, s, /*consume=*/true);
}

// ---------------------------------------------------------------------------------------------------
// sequential admission with reservation
// ---------------------------------------------------------------------------------------------------
// The queue in order over n_pages >= 1 page engines (one page: the engine itself), on page 0's stream s: one status-matrix check
// of page 0, then one kt_admit launch.  The caller holds every page's launch lock and has set the device; the results stay on the
// device behind page 0's check slot (kt_check_fetch).
// Gangs (n_gangs >= 0 with gang_off, else -1: the plain queue): validated by the caller (gangs_valid); page 0 keeps the offsets and the
// gang bytes on the device (kt_admit_gangs_fetch).
static int32_t admit_locked(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                            hipStream_t s, int64_t n_gangs = -1, const int64_t* gang_off = nullptr) {
  kt_engine* e0 = pages[0];
  const int32_t T = e0->thr_rows_hi;
  const bool gangs = n_gangs >= 0;
  e0->gang_ready = false;
  for (int32_t k = 0; k < n_pages; ++k)
    if (pages[k]->wide)
      return pages[k]->fail(KT_ERR_UNSUPPORTED, "admit queue: the stored `used` of page %d is wider than int64 (kt_admit reads int64 tables)", k);
  if ((double)n * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "admit queue: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  // (a) who affects whom, for the whole queue in parallel, from page 0 (selectors, namespaces and responsibility are the same
  //     in every page; statuses against the current reserved amounts)
  if (gangs && n_gangs > 0) {
    // the offsets go up in front of the check launch: the caller's memory is not referenced after return
    if (e0->d_gang_off.cap < (size_t)n_gangs + 1 || e0->d_gang_out.cap < (size_t)n_gangs) {
      if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));  // the buffers may still be in use
      KT_HIP(e0, e0->d_gang_off.reserve((size_t)n_gangs + 1));
      KT_HIP(e0, e0->d_gang_out.reserve((size_t)n_gangs));
    }
    KT_HIP(e0, hipMemcpyAsync(e0->d_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s));
    KT_HIP(e0, hipStreamSynchronize(s));
    e0->h_gang_off.assign(gang_off, gang_off + n_gangs + 1);
  }
  int32_t rc = check_launch_locked(e0, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  if (rc == KT_OK && gangs) e0->gang_ready = true, e0->gang_n = n_gangs, e0->gang_on_device = n > 0 && T > 0;
  if (rc != KT_OK || n == 0 || T == 0) return rc;  // (no throttle rows: a gang is admitted iff no member's PreFilter is an error)
  // (b) the queue in order, one wave, every page's reserved amounts side by side in LDS
  if (!e0->admit_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->admit_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->admit_pages_ev));  // the previous launch's copy has read h_admit_pages
  e0->h_admit_pages.resize((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) {
    const kt_engine* e = pages[k];
    e0->h_admit_pages[(size_t)k] = kt::AdmitPage{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  }
  const bool commit = (flags & KT_ADMIT_COMMIT) != 0;
  KT_HIP(e0, e0->d_admit.reserve(kt::admit_paged_state_bytes(T, e0->h_admit_pages.data(), n_pages) + (gangs ? kt::admit_gang_extra_bytes(T, n_pages) : 0) + 64));
  KT_HIP(e0, e0->d_admit_pages.reserve(sizeof(kt::AdmitPage) * (size_t)n_pages));
  static const bool force_global = getenv("KT_ADMIT_FORCE_GLOBAL") != nullptr;  // test hook: HBM-resident state
  hipError_t herr = hipSuccess;
  const kt::AdmitGangs ga{e0->d_gang_off.p, n_gangs, e0->d_gang_out.p};
  const bool launched = kt::launch_admit(e0->h_admit_pages.data(), n_pages, (kt::AdmitPage*)e0->d_admit_pages.p, e0->admit_pages_ev, n,
                                         pod_rows ? e0->d_rows.p : nullptr, T, on_equal != 0, commit, e0->d_status.p, e0->d_summary.p,
                                         e0->d_admit.p, force_global, s, &herr, gangs ? &ga : nullptr);
  if (herr != hipSuccess || !launched) e0->gang_ready = false;
  if (herr != hipSuccess) return e0->fail(KT_ERR_DEVICE, "admit queue: copy of the page descriptors: %s", hipGetErrorString(herr));
  if (!launched) return e0->fail(KT_ERR_UNSUPPORTED, "admit queue: %d throttle rows exceed the kernel's LDS list", T);
  KT_HIP(e0, hipGetLastError());
  if (commit)
    for (int32_t k = 0; k < n_pages; ++k) {
      kt_engine* e = pages[k];
      e->reserved_dev_newer = true;
      std::lock_guard<std::mutex> g(e->recs_mu);
      e->recs_valid = false;
    }
  return KT_OK;
}

int32_t kt_admit_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  return admit_locked(&e, 1, n, pod_rows, on_equal, flags, pick_stream(e, stream));
}

// gang_off[0] == 0, gang_off[n_gangs] == n, strictly increasing (no empty gang); n_gangs == 0 only with n == 0
static int32_t gangs_valid(kt_engine* e, int64_t n, int64_t n_gangs, const int64_t* gang_off) {
  if (n_gangs == 0) {
    if (n != 0) return e->fail(KT_ERR_INVALID_ARGUMENT, "admit gangs: no gangs for a queue of %lld pods", (long long)n);
    if (gang_off && gang_off[0] != 0) return e->fail(KT_ERR_INVALID_ARGUMENT, "admit gangs: gang_off[0] = %lld, not 0", (long long)gang_off[0]);
    return KT_OK;
  }
  if (!gang_off) return e->fail(KT_ERR_INVALID_ARGUMENT, "admit gangs: gang_off is NULL");
  if (gang_off[0] != 0) return e->fail(KT_ERR_INVALID_ARGUMENT, "admit gangs: gang_off[0] = %lld, not 0", (long long)gang_off[0]);
  for (int64_t g = 0; g < n_gangs; ++g) {
    if (gang_off[g + 1] == gang_off[g])
      return e->fail(KT_ERR_INVALID_ARGUMENT, "admit gangs: gang %lld is empty (gang_off[%lld] = gang_off[%lld] = %lld)", (long long)g, (long long)g,
                     (long long)(g + 1), (long long)gang_off[g]);
    if (gang_off[g + 1] < gang_off[g])
      return e->fail(KT_ERR_INVALID_ARGUMENT, "admit gangs: gang_off[%lld] = %lld is below gang_off[%lld] = %lld", (long long)(g + 1),
                     (long long)gang_off[g + 1], (long long)g, (long long)gang_off[g]);
  }
  if (gang_off[n_gangs] != n)
    return e->fail(KT_ERR_INVALID_ARGUMENT, "admit gangs: gang_off[%lld] = %lld, not n = %lld", (long long)n_gangs, (long long)gang_off[n_gangs], (long long)n);
  return KT_OK;
}

int32_t kt_admit_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int32_t on_equal,
                              uint32_t flags, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  int32_t rc = gangs_valid(e, n, n_gangs, gang_off);
  if (rc != KT_OK) return rc;
  KT_HIP(e, hipSetDevice(e->device));
  return admit_locked(&e, 1, n, pod_rows, on_equal, flags, pick_stream(e, stream), n_gangs, gang_off);
}

// the gang bytes of the last gang launch, under the launch lock; out nullable
static int32_t gangs_fetch_locked(kt_engine* e, int64_t n_gangs, uint8_t* out) {
  if (!e->gang_ready) return e->fail(KT_ERR_NOT_READY, "kt_admit_gangs_fetch before kt_admit_gangs_launch");
  if (n_gangs < 0 || n_gangs > e->gang_n)
    return e->fail(KT_ERR_OUT_OF_RANGE, "n_gangs=%lld, the last gang launch had %lld gangs", (long long)n_gangs, (long long)e->gang_n);
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  if (e->gang_on_device) {
    if (n_gangs && out) KT_HIP(e, hipMemcpyAsync(out, e->d_gang_out.p, (size_t)n_gangs, hipMemcpyDeviceToHost, s));
    KT_HIP(e, hipStreamSynchronize(s));
    return KT_OK;
  }
  // no throttle rows: nothing was reserved; a gang is admitted iff every member's PreFilter answered Success
  std::vector<uint64_t> sm((size_t)e->check_n + 1);
  if (e->check_n) KT_HIP(e, hipMemcpyAsync(sm.data(), e->d_summary.p, (size_t)e->check_n * 8, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  for (int64_t g = 0; g < n_gangs && out; ++g) {
    out[g] = 1;
    for (int64_t i = e->h_gang_off[(size_t)g]; i < e->h_gang_off[(size_t)g + 1]; ++i)
      if (sm[(size_t)i] != 0) out[g] = 0;
  }
  return KT_OK;
}

int32_t kt_admit_gangs_fetch(kt_engine* e, int64_t n_gangs, uint8_t* out_admitted) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  return gangs_fetch_locked(e, n_gangs, out_admitted);
}

int32_t kt_fetch_reserved(kt_engine* e, int32_t n, const int32_t* rows, const kt_amounts* out) {
  if (!e || !out || n < 0 || (n > 0 && !rows)) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  for (int32_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= e->thr_rows_hi) return e->fail(KT_ERR_OUT_OF_RANGE, "throttle row %d", rows[i]);
  int32_t rc = sync_status_to_host(e);
  if (rc != KT_OK) return rc;
  for (int32_t i = 0; i < n; ++i) amount_to_table(e->thr[(size_t)rows[i]].reserved, *out, (size_t)i, e->D);
  return KT_OK;
}

static int32_t check_fetch_locked(kt_engine* e, int64_t n, uint64_t* out_summary, uint8_t* out_status);

int32_t kt_check_fetch(kt_engine* e, int64_t n, uint64_t* out_summary, uint8_t* out_status) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  return check_fetch_locked(e, n, out_summary, out_status);
}

// ---- the few-pod path: what the scheduler's PreFilter actually calls (one pod per call, plugin.go:148-215)
static int32_t few_setup(kt_engine* e) {  // under the exclusive lock
  if (e->few_ready) return KT_OK;
  if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));  // CheckRecs written so far carry no event: let them land
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi = numerically lowest = highest priority
  KT_HIP(e, hipStreamCreateWithPriority(&e->small_stream, hipStreamNonBlocking, hi));
  for (auto& ev : e->recs_ev) KT_HIP(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  KT_HIP(e, e->d_few_acc.reserve(8));
  KT_HIP(e, e->d_few_ticket.reserve(4));
  KT_HIP(e, hipMemsetAsync(e->d_few_acc.p, 0, 8 * 8, e->small_stream));
  KT_HIP(e, hipMemsetAsync(e->d_few_ticket.p, 0, 4 * 4, e->small_stream));
  KT_HIP(e, hipHostMalloc((void**)&e->h_few, 16 * 8, hipHostMallocMapped));
  memset(e->h_few, 0, 16 * 8);
  KT_HIP(e, hipStreamSynchronize(e->small_stream));
  e->few_ready = true;
  return KT_OK;
}

static inline bool few_shape_ok(const kt_engine* e, int64_t n, const int64_t* pod_rows, const uint64_t* out_summary, const uint8_t* out_status) {
  static const bool disabled = getenv("KT_NO_FEW") != nullptr;  // A/B runs: every kt_check through the staged small launch
  return !disabled && n >= 1 && n <= 8 && pod_rows && out_summary && !out_status && e->cfg.kernel_variant == 0;
}

// Under the SHARED lock (+ small_mu): nothing of the engine's host state is modified except the fields only this path
// touches.  Returns 1 when served, 0 when the caller has to take the exclusive path, < 0 on error.
static int32_t check_few_shared(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint64_t* out_summary) {
  if (!e->few_ready || e->program_dirty || e->status_host_dirty || e->hindex.has_slow || e->dindex.has_long || e->dindex.n_slow != 0 || e->n_overflow != 0 ||
      e->thr_rows_hi <= 0 || e->dindex.n_chunks == 0)
    return 0;
  for (int64_t i = 0; i < n; ++i)
    if (pod_rows[i] < 0 || pod_rows[i] >= e->cfg.pod_capacity) return e->fail(KT_ERR_OUT_OF_RANGE, "pod row %lld", (long long)pod_rows[i]);
  // which generation of CheckRecs: the current one once the kernel that writes it has completed, else the previous one
  int b;
  bool wait_cur = false;
  {
    std::lock_guard<std::mutex> g(e->recs_mu);
    if (!e->recs_valid || e->recs_eq != (on_equal != 0) || e->recs_DT != kt::dt_bucket_ix(e->D)) return 0;
    b = e->recs_cur;
    if (e->recs_ev_pending[b] && hipEventQuery(e->recs_ev[b]) == hipSuccess) e->recs_ev_pending[b] = false;
    if (e->recs_ev_pending[b]) {
      const int pb = 1 - b;
      if (e->recs_prev_valid && e->recs_ev_pending[pb] && hipEventQuery(e->recs_ev[pb]) == hipSuccess) e->recs_ev_pending[pb] = false;
      if (e->recs_prev_valid && !e->recs_ev_pending[pb]) b = pb;
      else wait_cur = true;  // two reconciles in flight: wait for the newer one
    }
  }
  if (wait_cur) KT_HIP(e, hipStreamWaitEvent(e->small_stream, e->recs_ev[b], 0));
  order_behind_ingest(e, e->small_stream);  // (a pod event right before this PreFilter: behind its kernel on the device)
  const uint64_t seq = ++e->few_seq;
  if (!kt::launch_check_few(e->pods, (int)n, pod_rows, e->sp, e->dindex, e->d_recs2[b].p, e->d_few_acc.p, e->d_few_ticket.p, e->h_few, e->h_few + 8,
                            seq, e->small_stream))
    return 0;
  KT_HIP(e, hipGetLastError());
  // the last workgroup writes the words and then the sequence number into pinned memory: spin on it
  volatile uint64_t* seqp = (volatile uint64_t*)(e->h_few + 8);
  bool done = false;
  for (uint32_t spin = 0; spin < (1u << 22); ++spin) {
    if (*seqp == seq) {
      done = true;
      break;
    }
    __builtin_ia32_pause();
  }
  if (!done) {  // far beyond any plausible latency: let the runtime report what happened
    KT_HIP(e, hipStreamSynchronize(e->small_stream));
    if (*seqp != seq) return e->fail(KT_ERR_DEVICE, "kt_check_few: no completion signal");
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  for (int64_t i = 0; i < n; ++i) out_summary[i] = e->h_few[i];
  e->few_served.fetch_add(1, std::memory_order_relaxed);
  return 1;
}

// launch + fetch as ONE critical section: what a caller needs when other threads use the engine at the same time
// (Unreserve from binding goroutines, reconcile workers) — a kt_check_launch / kt_check_fetch pair can be interleaved
int32_t kt_check(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint64_t* out_summary, uint8_t* out_status) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  const bool few = few_shape_ok(e, n, pod_rows, out_summary, out_status);
  if (few) {
    std::shared_lock<std::shared_mutex> rd(e->mu);
    std::lock_guard<std::mutex> sl(e->small_mu);
    KT_HIP(e, hipSetDevice(e->device));
    settle_ingest(e);  // a pod event fed just before: PreFilter sees it
    const int32_t rc = check_few_shared(e, n, pod_rows, on_equal, out_summary);
    if (rc != 0) return rc < 0 ? rc : KT_OK;
  }
  LaunchLock lk(e, few && !e->few_ready);  // the one-time set-up of the few-pod path changes what those checks read
  KT_HIP(e, hipSetDevice(e->device));
  if (few && !e->few_ready) {
    int32_t rc0 = few_setup(e);
    if (rc0 != KT_OK) return rc0;
  }
  int32_t rc = check_launch_locked(e, n, pod_rows, on_equal, out_status ? KT_CHECK_STATUS_MATRIX : 0u, e->own_stream);
  if (rc != KT_OK) return rc;
  return check_fetch_locked(e, n, out_summary, out_status);
}

static int32_t check_fetch_locked(kt_engine* e, int64_t n, uint64_t* out_summary, uint8_t* out_status) {
  if (!e->check_ready) return e->fail(KT_ERR_NOT_READY, "kt_check_fetch before kt_check_launch");
  if (n < 0 || n > e->check_n) return e->fail(KT_ERR_OUT_OF_RANGE, "n=%lld, last check had %lld pods", (long long)n, (long long)e->check_n);
  if (out_status && !e->check_has_status) return e->fail(KT_ERR_NOT_READY, "status matrix was not requested at launch");
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  const bool from_pinned = e->check_in_h_small && e->h_small;  // the kernel already wrote the words to host memory
  if (n && out_summary && !from_pinned) KT_HIP(e, hipMemcpyAsync(out_summary, e->d_summary.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (n && out_status && e->check_T)  // the matrix was written with the row stride in effect at launch
    KT_HIP(e, hipMemcpyAsync(out_status, e->d_status.p, (size_t)n * (size_t)e->check_T, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  if (n && out_summary && from_pinned) memcpy(out_summary, e->h_small, (size_t)n * 8);
  return KT_OK;
}

// affectedPods restricted to the pods a caller names (throttle_controller.go:221-246 / clusterthrottle_controller.go:224-270):
// for each of the n pod rows and each of the m throttle rows — does the throttle's selector (namespace side included) match
// the pod as the engine holds it NOW.  What unreserveAffectedPods (throttle_controller.go:135-155) needs: a reservation is
// released behind a reconcile only for a pod that is IN the reconciled throttle's affected set — one whose labels moved on
// after Reserve is not.  One status-matrix check of those rows (a small launch), read by column.
int32_t kt_affected_pods(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t m, const int32_t* throttle_rows, uint8_t* out) {
  if (!e || n < 0 || m < 0 || (n > 0 && !pod_rows) || (m > 0 && !throttle_rows) || (n > 0 && m > 0 && !out)) return KT_ERR_INVALID_ARGUMENT;
  if (n == 0 || m == 0) return KT_OK;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  int32_t rc = ensure_ready(e, e->own_stream);
  if (rc != KT_OK) return rc;
  const int32_t T = e->thr_rows_hi;
  for (int32_t j = 0; j < m; ++j)
    if (throttle_rows[j] < 0 || throttle_rows[j] >= T) return e->fail(KT_ERR_OUT_OF_RANGE, "throttle row %d", throttle_rows[j]);
  if ((rc = check_launch_locked(e, n, pod_rows, 0, KT_CHECK_STATUS_MATRIX, e->own_stream)) != KT_OK) return rc;
  std::vector<uint8_t> st((size_t)n * (size_t)T);
  if ((rc = check_fetch_locked(e, n, nullptr, st.data())) != KT_OK) return rc;
  // the call used the engine's ONE check slot: a kt_check_launch of the caller that was pending is gone — its kt_check_fetch must
  // answer KT_ERR_NOT_READY instead of handing out these pods' results
  e->check_ready = false;
  for (int64_t i = 0; i < n; ++i)
    for (int32_t j = 0; j < m; ++j) {
      const uint8_t v = st[(size_t)i * (size_t)T + (size_t)throttle_rows[j]];
      out[(size_t)i * (size_t)m + (size_t)j] = v == KT_STATUS_ERROR ? (uint8_t)KT_STATUS_ERROR : v != KT_STATUS_NOT_AFFECTED ? 1 : 0;
    }
  return KT_OK;
}


int32_t kt_paged_check(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal,
                       uint64_t* out_summary, uint8_t* out_status) {
  if (!pages || n_pages < 1 || n < 0) return KT_ERR_INVALID_ARGUMENT;
  for (int32_t k = 0; k < n_pages; ++k)
    if (!pages[k]) return KT_ERR_INVALID_ARGUMENT;
  int32_t T = 0;
  int32_t rc = kt_throttle_rows(pages[0], &T);
  if (rc != KT_OK) return rc;
  for (int32_t k = 1; k < n_pages; ++k) {
    int32_t Tk = 0;
    if ((rc = kt_throttle_rows(pages[k], &Tk)) != KT_OK) return rc;
    if (Tk != T) return pages[k]->fail(KT_ERR_INVALID_ARGUMENT, "page %d holds %d throttle rows, page 0 %d: every page holds every throttle", k, Tk, T);
  }
  if (n == 0) return KT_OK;
  // CheckThrottleStatus precedence (first hit wins, throttle_types.go:128-153): exceeds > active > insufficient > not throttled
  auto rank = [](uint8_t v) -> uint8_t {
    return v == KT_STATUS_ERROR ? 5 : v == KT_STATUS_POD_REQUESTS_EXCEEDS_THRESHOLD ? 4 : v == KT_STATUS_ACTIVE ? 3 : v == KT_STATUS_INSUFFICIENT ? 2 : v == KT_STATUS_NOT_THROTTLED ? 1 : 0;
  };
  static const uint8_t code[6] = {KT_STATUS_NOT_AFFECTED, KT_STATUS_NOT_THROTTLED, KT_STATUS_INSUFFICIENT, KT_STATUS_ACTIVE, KT_STATUS_POD_REQUESTS_EXCEEDS_THRESHOLD, KT_STATUS_ERROR};
  const size_t cells = (size_t)n * (size_t)(T > 0 ? T : 1);
  std::vector<uint8_t> acc(cells, 0), page(cells);
  for (int32_t k = 0; k < n_pages; ++k) {
    if ((rc = kt_check(pages[k], n, pod_rows, on_equal, nullptr, page.data())) != KT_OK) return rc;
    for (size_t i = 0; i < (size_t)n * (size_t)T; ++i) acc[i] = std::max(acc[i], rank(page[i]));
  }
  for (int64_t i = 0; i < n; ++i) {
    uint64_t n_exc = 0, n_act = 0, n_ins = 0;
    bool err = false;
    for (int32_t t = 0; t < T; ++t) {
      const uint8_t r = acc[(size_t)i * T + t];
      err |= r == 5, n_exc += r == 4, n_act += r == 3, n_ins += r == 2;
      if (out_status) out_status[(size_t)i * T + t] = code[r];
    }
    if (out_summary) out_summary[i] = err ? 2ull : ((n_exc | n_act | n_ins) ? 1ull : 0ull) | n_exc << 4 | n_act << 24 | n_ins << 44;
  }
  return KT_OK;
}

// What the calls over several page engines share (kt_paged_admit, kt_paged_admit_gangs, kt_paged_headroom; `what` words the errors).
// paged_lock: every page exclusively, in address order — two paged calls over overlapping pages cannot deadlock
typedef std::vector<std::unique_ptr<LaunchLock>> PageLocks;
static int32_t paged_lock(const char* what, kt_engine* const* pages, int32_t n_pages, int64_t n, PageLocks& locks) {
  if (!pages || n_pages < 1 || n < 0) return KT_ERR_INVALID_ARGUMENT;
  for (int32_t k = 0; k < n_pages; ++k) {
    if (!pages[k]) return KT_ERR_INVALID_ARGUMENT;
    for (int32_t j = 0; j < k; ++j)
      if (pages[j] == pages[k]) return pages[k]->fail(KT_ERR_INVALID_ARGUMENT, "%s: the engine of page %d is also page %d", what, k, j);
  }
  std::vector<kt_engine*> by_addr(pages, pages + n_pages);
  std::sort(by_addr.begin(), by_addr.end(), std::less<kt_engine*>());
  for (kt_engine* e : by_addr) locks.emplace_back(new LaunchLock(e, /*force_exclusive=*/true));
  return KT_OK;
}
// paged_same_cluster: every page holds every throttle row and every pod row of the queue, on one device
static int32_t paged_same_cluster(const char* what, kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows) {
  kt_engine* e0 = pages[0];
  const int32_t T = e0->thr_rows_hi;
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if (e->thr_rows_hi != T) return e->fail(KT_ERR_INVALID_ARGUMENT, "page %d holds %d throttle rows, page 0 %d: every page holds every throttle", k, e->thr_rows_hi, T);
    if (e->device != e0->device) return e->fail(KT_ERR_UNSUPPORTED, "%s: page %d is on device %d, page 0 on %d", what, k, e->device, e0->device);
    if (pod_rows) {
      for (int64_t i = 0; i < n; ++i)
        if (pod_rows[i] < 0 || pod_rows[i] >= e->cfg.pod_capacity) return e->fail(KT_ERR_OUT_OF_RANGE, "page %d: pod row %lld", k, (long long)pod_rows[i]);
    } else if (n > e->cfg.pod_capacity) {
      return e->fail(KT_ERR_OUT_OF_RANGE, "page %d: n=%lld > pod_capacity", k, (long long)n);
    }
  }
  return KT_OK;
}
// paged_order: the kernel reads every page's tables on page 0's stream *s.  Uploads of host-side status / reserved rows
// (ensure_ready) and earlier launches of page k ran on page k's streams: they are SYNCHRONISED here (the calls are synchronous
// anyway); the newest feed kernel of page k is ordered before the launch on the device (order_behind_ingest).
static int32_t paged_order(kt_engine* const* pages, int32_t n_pages, hipStream_t* s) {
  kt_engine* e0 = pages[0];
  KT_HIP(e0, hipSetDevice(e0->device));
  *s = pick_stream(e0, nullptr);
  for (int32_t k = 1; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    int32_t rc = ensure_ready(e, e->own_stream);
    if (rc != KT_OK) return rc;
    KT_HIP(e, hipStreamSynchronize(e->own_stream));
    if (e->last_stream && e->last_stream != e->own_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
    order_behind_ingest(e, *s);
  }
  return KT_OK;
}

// kt_admit_launch / kt_admit_gangs_launch (n_gangs >= 0) over several engines, synchronous: what is specific to more than one engine,
// then admit_locked
static int32_t paged_admit(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                           uint64_t* out_summary, uint8_t* out_status, int64_t n_gangs, const int64_t* gang_off, uint8_t* out_gang_admitted) {
  PageLocks locks;
  int32_t rc = paged_lock("paged admit", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  const int32_t T = e0->thr_rows_hi;
  if (n_gangs >= 0) {
    const int32_t rcg = gangs_valid(e0, n, n_gangs, gang_off);
    if (rcg != KT_OK) return rcg;
  }
  if ((rc = paged_same_cluster("paged admit", pages, n_pages, n, pod_rows)) != KT_OK) return rc;
  if (n == 0) return KT_OK;
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  rc = admit_locked(pages, n_pages, n, pod_rows, on_equal, flags, s, n_gangs, gang_off);
  e0->check_ready = false;  // the call used page 0's check slot (as kt_affected_pods): a pending kt_check_launch is gone
  if (rc != KT_OK) return rc;
  if (out_summary) KT_HIP(e0, hipMemcpyAsync(out_summary, e0->d_summary.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (out_status && T > 0) KT_HIP(e0, hipMemcpyAsync(out_status, e0->d_status.p, (size_t)n * (size_t)T, hipMemcpyDeviceToHost, s));
  if (n_gangs >= 0) {
    rc = gangs_fetch_locked(e0, n_gangs, out_gang_admitted);  // (synchronises s)
    e0->gang_ready = false;  // the results have been handed out
    return rc;
  }
  KT_HIP(e0, hipStreamSynchronize(s));
  return KT_OK;
}

int32_t kt_paged_admit(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                       uint64_t* out_summary, uint8_t* out_status) {
  return paged_admit(pages, n_pages, n, pod_rows, on_equal, flags, out_summary, out_status, -1, nullptr, nullptr);
}

int32_t kt_paged_admit_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                             int32_t on_equal, uint32_t flags, uint64_t* out_summary, uint8_t* out_status, uint8_t* out_gang_admitted) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  return paged_admit(pages, n_pages, n, pod_rows, on_equal, flags, out_summary, out_status, n_gangs, gang_off, out_gang_admitted);
}

// ---------------------------------------------------------------------------------------------------
// headroom: how many copies of a pod the throttles still admit (kt_kernels_headroom.hip)
// ---------------------------------------------------------------------------------------------------
// Over n_pages >= 1 page engines (one page: the engine itself) on page 0's stream s: one status-matrix check of page 0 (who
// affects whom), then one kt_headroom launch over the page descriptors kt_admit reads.  The caller holds every page's launch lock
// and has set the device; the results stay on the device behind page 0 (kt_headroom_fetch).  Nothing of any page is changed.
static int32_t headroom_locked(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, int64_t cap,
                               hipStream_t s) {
  kt_engine* e0 = pages[0];
  const int32_t T = e0->thr_rows_hi;
  e0->headroom_ready = false, e0->headroom_gangs = false;
  for (int32_t k = 0; k < n_pages; ++k)
    if (pages[k]->wide)
      return pages[k]->fail(KT_ERR_UNSUPPORTED, "headroom: the stored `used` of page %d is wider than int64 (kt_headroom reads int64 tables)", k);
  if ((double)n * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "headroom: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  if (n == 0) {  // nothing is launched
    e0->headroom_ready = true, e0->headroom_n = 0;
    return KT_OK;
  }
  if (e0->d_headroom_copies.cap < (size_t)n || e0->d_headroom_limiting.cap < (size_t)n) {
    // a launch that was never fetched may still be writing the old buffers, on the stream it was given: that is last_stream
    // until the check below replaces it (admit_locked does the same before it reallocates)
    if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));
    KT_HIP(e0, e0->d_headroom_copies.reserve((size_t)n));
    KT_HIP(e0, e0->d_headroom_limiting.reserve((size_t)n));
  }
  int32_t rc = check_launch_locked(e0, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e0->check_ready = false;  // the slot holds this call's rows (as with kt_affected_pods): a pending kt_check_launch is gone
  if (rc != KT_OK) return rc;
  if (!e0->admit_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->admit_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->admit_pages_ev));  // the previous launch's copy has read h_admit_pages
  e0->h_admit_pages.resize((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) {
    const kt_engine* e = pages[k];
    e0->h_admit_pages[(size_t)k] = kt::AdmitPage{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  }
  KT_HIP(e0, e0->d_admit_pages.reserve(sizeof(kt::AdmitPage) * (size_t)n_pages));
  hipError_t herr = hipSuccess;
  if (!kt::launch_headroom(e0->h_admit_pages.data(), n_pages, (kt::AdmitPage*)e0->d_admit_pages.p, e0->admit_pages_ev, n,
                           pod_rows ? e0->d_rows.p : nullptr, T, on_equal != 0, (uint32_t)cap, e0->d_status.p, e0->d_summary.p,
                           e0->d_headroom_copies.p, e0->d_headroom_limiting.p, s, &herr))
    return e0->fail(KT_ERR_DEVICE, "headroom: copy of the page descriptors: %s", hipGetErrorString(herr));
  KT_HIP(e0, hipGetLastError());
  e0->headroom_ready = true, e0->headroom_n = n;
  return KT_OK;
}

static inline bool headroom_cap_ok(int64_t cap) { return cap >= 1 && cap <= (int64_t)KT_HEADROOM_MAX_CAP; }

int32_t kt_headroom_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, int64_t cap, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  if (!headroom_cap_ok(cap)) return e->fail(KT_ERR_INVALID_ARGUMENT, "headroom: cap = %lld, not in [1, %d]", (long long)cap, KT_HEADROOM_MAX_CAP);
  KT_HIP(e, hipSetDevice(e->device));
  return headroom_locked(&e, 1, n, pod_rows, on_equal, cap, pick_stream(e, stream));
}

// the results of the last headroom launch, under the launch lock; both outputs nullable
static int32_t headroom_fetch_locked(kt_engine* e, int64_t n, int64_t* out_copies, int32_t* out_limiting) {
  if (!e->headroom_ready || e->headroom_gangs) return e->fail(KT_ERR_NOT_READY, "kt_headroom_fetch before kt_headroom_launch");
  if (n < 0 || n > e->headroom_n) return e->fail(KT_ERR_OUT_OF_RANGE, "n=%lld, the last headroom launch had %lld pods", (long long)n, (long long)e->headroom_n);
  if (n == 0) return KT_OK;
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  if (out_copies) KT_HIP(e, hipMemcpyAsync(out_copies, e->d_headroom_copies.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (out_limiting) KT_HIP(e, hipMemcpyAsync(out_limiting, e->d_headroom_limiting.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

int32_t kt_headroom_fetch(kt_engine* e, int64_t n, int64_t* out_copies, int32_t* out_limiting) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  return headroom_fetch_locked(e, n, out_copies, out_limiting);
}

int32_t kt_paged_headroom(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, int64_t cap,
                          int64_t* out_copies, int32_t* out_limiting) {
  PageLocks locks;
  int32_t rc = paged_lock("paged headroom", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  if (!headroom_cap_ok(cap)) return e0->fail(KT_ERR_INVALID_ARGUMENT, "headroom: cap = %lld, not in [1, %d]", (long long)cap, KT_HEADROOM_MAX_CAP);
  if ((rc = paged_same_cluster("paged headroom", pages, n_pages, n, pod_rows)) != KT_OK) return rc;
  if (n == 0) return KT_OK;
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  if ((rc = headroom_locked(pages, n_pages, n, pod_rows, on_equal, cap, s)) != KT_OK) return rc;
  rc = headroom_fetch_locked(e0, n, out_copies, out_limiting);  // (synchronises s)
  e0->headroom_ready = false;  // the results have been handed out
  return rc;
}

// ---------------------------------------------------------------------------------------------------
// headroom, for gangs: how many copies of a whole gang the throttles still admit (kt_kernels_headroom_gangs.hip)
// ---------------------------------------------------------------------------------------------------
// The gang defects of kt_admit_gangs_launch and "a pod twice" asked per gang (as the gang forecast), then headroom_locked's
// refusals and its two launches with kt_headroom_gangs in kt_headroom's place.  The result shares the one pending headroom
// result; headroom_gangs tells the fetches apart.
int32_t kt_headroom_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int32_t on_equal,
                                 int64_t cap, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  if (n > 0 && !pod_rows) return e->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: pod_rows missing");
  int32_t rc = gangs_valid(e, n, n_gangs, gang_off);
  if (rc != KT_OK) return rc;
  {
    // gangs are judged independently: a pod may be in several of them, but not twice in one (it would reserve twice)
    std::vector<int64_t> sorted;
    for (int64_t g = 0; g < n_gangs; ++g) {
      sorted.assign(pod_rows + gang_off[g], pod_rows + gang_off[g + 1]);
      std::sort(sorted.begin(), sorted.end());
      for (size_t j = 1; j < sorted.size(); ++j)
        if (sorted[j] == sorted[j - 1])
          return e->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: pod row %lld is in gang %lld twice", (long long)sorted[j], (long long)g);
    }
  }
  for (int64_t i = 0; i < n; ++i)
    if (pod_rows[i] < 0 || pod_rows[i] >= e->cfg.pod_capacity)
      return e->fail(KT_ERR_OUT_OF_RANGE, "headroom gangs: pod row %lld", (long long)pod_rows[i]);
  if (!headroom_cap_ok(cap))
    return e->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: cap = %lld, not in [1, %d]", (long long)cap, KT_HEADROOM_MAX_CAP);
  const int32_t T = e->thr_rows_hi;
  if ((double)n * (double)T > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "headroom gangs: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "headroom gangs: the stored `used` is wider than int64 (kt_headroom_gangs reads int64 tables)");
  if (e->neg_seen)
    return e->fail(KT_ERR_UNSUPPORTED,
                   "headroom gangs: the engine has been fed a negative request; the search over the copies rests on sums that only grow "
                   "(kt_headroom_launch serves such an engine pod by pod)");
  e->headroom_ready = false, e->headroom_gangs = false;
  if (n == 0) {  // (no gangs) nothing is launched
    e->headroom_ready = true, e->headroom_gangs = true, e->headroom_n = 0;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  if (e->d_headroom_copies.cap < (size_t)n_gangs || e->d_headroom_limiting.cap < (size_t)n_gangs || e->d_headroom_blocker.cap < (size_t)n_gangs ||
      e->d_headroom_gang_off.cap < (size_t)n_gangs + 1) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_headroom_launch)
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
    KT_HIP(e, e->d_headroom_copies.reserve((size_t)n_gangs));
    KT_HIP(e, e->d_headroom_limiting.reserve((size_t)n_gangs));
    KT_HIP(e, e->d_headroom_blocker.reserve((size_t)n_gangs));
    KT_HIP(e, e->d_headroom_gang_off.reserve((size_t)n_gangs + 1));
  }
  // the offsets travel on the launch's stream, behind an earlier launch's kernel; the caller's memory is not referenced after return
  KT_HIP(e, hipMemcpyAsync(e->d_headroom_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  // ONE check over the members of all gangs: which throttles affect which pod, and the error rows
  rc = check_launch_locked(e, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e->check_ready = false;  // the slot holds this call's rows (as with kt_headroom_launch): a pending kt_check_launch is gone
  if (rc != KT_OK) return rc;
  const kt::AdmitPage pg{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  kt::launch_headroom_gangs(pg, n_gangs, e->d_rows.p, e->d_headroom_gang_off.p, T, on_equal != 0, (uint32_t)cap, e->d_status.p, e->d_summary.p,
                            e->d_headroom_copies.p, e->d_headroom_limiting.p, e->d_headroom_blocker.p, s);
  KT_HIP(e, hipGetLastError());
  e->last_stream = s;
  e->headroom_ready = true, e->headroom_gangs = true, e->headroom_n = n_gangs;
  return KT_OK;
}

int32_t kt_headroom_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_copies, int32_t* out_limiting, int64_t* out_blocker) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (!e->headroom_ready || !e->headroom_gangs) return e->fail(KT_ERR_NOT_READY, "kt_headroom_gangs_fetch before kt_headroom_gangs_launch");
  if (n_gangs < 0 || n_gangs > e->headroom_n)
    return e->fail(KT_ERR_OUT_OF_RANGE, "n_gangs=%lld, the last headroom gangs launch had %lld gangs", (long long)n_gangs, (long long)e->headroom_n);
  if (n_gangs == 0) return KT_OK;
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  if (out_copies) KT_HIP(e, hipMemcpyAsync(out_copies, e->d_headroom_copies.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
  if (out_limiting) KT_HIP(e, hipMemcpyAsync(out_limiting, e->d_headroom_limiting.p, (size_t)n_gangs * 4, hipMemcpyDeviceToHost, s));
  if (out_blocker) KT_HIP(e, hipMemcpyAsync(out_blocker, e->d_headroom_blocker.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// headroom, for gangs, over pages: kt_headroom_gangs_launch on the cluster of all names (kt_kernels_headroom_gangs_paged.hip)
// ---------------------------------------------------------------------------------------------------
// kt_paged_headroom's scaffolding with kt_headroom_gangs_launch's gang arguments: the gang defects and "a pod twice" asked per
// gang, then the page set and every page's engine; one check of page 0, ONE kernel over the descriptors kt_admit reads, the
// results through page 0's headroom buffers and out.
int32_t kt_paged_headroom_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                const int64_t* gang_off, int32_t on_equal, int64_t cap, int64_t* out_copies, int32_t* out_limiting,
                                int64_t* out_blocker) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  PageLocks locks;
  int32_t rc = paged_lock("paged headroom gangs", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  // ---- refusals: nothing is launched and no slot or pending result of any page is touched before the last of them
  if (n > 0 && !pod_rows) return e0->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: pod_rows missing");
  if ((rc = gangs_valid(e0, n, n_gangs, gang_off)) != KT_OK) return rc;
  {
    // gangs are judged independently: a pod may be in several of them, but not twice in one (it would reserve twice)
    std::vector<int64_t> sorted;
    for (int64_t g = 0; g < n_gangs; ++g) {
      sorted.assign(pod_rows + gang_off[g], pod_rows + gang_off[g + 1]);
      std::sort(sorted.begin(), sorted.end());
      for (size_t j = 1; j < sorted.size(); ++j)
        if (sorted[j] == sorted[j - 1])
          return e0->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: pod row %lld is in gang %lld twice", (long long)sorted[j], (long long)g);
    }
  }
  if (!headroom_cap_ok(cap))
    return e0->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: cap = %lld, not in [1, %d]", (long long)cap, KT_HEADROOM_MAX_CAP);
  if ((rc = paged_same_cluster("paged headroom gangs", pages, n_pages, n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((double)n * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "headroom gangs: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if (e->wide)
      return e->fail(KT_ERR_UNSUPPORTED, "headroom gangs: the stored `used` of page %d is wider than int64 (kt_headroom_gangs_paged reads int64 tables)",
                     k);
    if (e->neg_seen)
      return e->fail(KT_ERR_UNSUPPORTED,
                     "headroom gangs: page %d has been fed a negative request; the search over the copies rests on sums that only grow "
                     "(kt_paged_headroom serves such pages pod by pod)",
                     k);
  }
  if (n == 0) return KT_OK;  // (no gangs) nothing is launched
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  // ---- from here on the call owns page 0's check slot and headroom result
  e0->headroom_ready = false, e0->headroom_gangs = false;
  if (e0->d_headroom_copies.cap < (size_t)n_gangs || e0->d_headroom_limiting.cap < (size_t)n_gangs ||
      e0->d_headroom_blocker.cap < (size_t)n_gangs || e0->d_headroom_gang_off.cap < (size_t)n_gangs + 1) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_headroom_gangs_launch)
    if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));
    KT_HIP(e0, e0->d_headroom_copies.reserve((size_t)n_gangs));
    KT_HIP(e0, e0->d_headroom_limiting.reserve((size_t)n_gangs));
    KT_HIP(e0, e0->d_headroom_blocker.reserve((size_t)n_gangs));
    KT_HIP(e0, e0->d_headroom_gang_off.reserve((size_t)n_gangs + 1));
  }
  // the offsets travel on the launch's stream, behind an earlier launch's kernel (the call is synchronous: the caller's memory is
  // not referenced after return)
  KT_HIP(e0, hipMemcpyAsync(e0->d_headroom_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s));
  // ONE check of page 0 over the members of all gangs: which throttles affect which pod, and the error rows
  rc = check_launch_locked(e0, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e0->check_ready = false;  // the slot holds this call's rows (as with kt_paged_headroom): a pending kt_check_launch is gone
  if (rc != KT_OK) {
    (void)hipStreamSynchronize(s);  // the copy of the offsets reads the caller's memory
    return rc;
  }
  if (!e0->admit_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->admit_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->admit_pages_ev));  // the previous launch's copy has read h_admit_pages
  e0->h_admit_pages.resize((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) {
    const kt_engine* e = pages[k];
    e0->h_admit_pages[(size_t)k] = kt::AdmitPage{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  }
  KT_HIP(e0, e0->d_admit_pages.reserve(sizeof(kt::AdmitPage) * (size_t)n_pages));
  hipError_t herr = hipSuccess;
  if (!kt::launch_headroom_gangs_paged(e0->h_admit_pages.data(), n_pages, (kt::AdmitPage*)e0->d_admit_pages.p, e0->admit_pages_ev, n_gangs,
                                       e0->d_rows.p, e0->d_headroom_gang_off.p, T, on_equal != 0, (uint32_t)cap, e0->d_status.p, e0->d_summary.p,
                                       e0->d_headroom_copies.p, e0->d_headroom_limiting.p, e0->d_headroom_blocker.p, s, &herr)) {
    (void)hipStreamSynchronize(s);
    return e0->fail(KT_ERR_DEVICE, "paged headroom gangs: copy of the page descriptors: %s", hipGetErrorString(herr));
  }
  KT_HIP(e0, hipGetLastError());
  e0->last_stream = s;
  if (out_copies) KT_HIP(e0, hipMemcpyAsync(out_copies, e0->d_headroom_copies.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
  if (out_limiting) KT_HIP(e0, hipMemcpyAsync(out_limiting, e0->d_headroom_limiting.p, (size_t)n_gangs * 4, hipMemcpyDeviceToHost, s));
  if (out_blocker) KT_HIP(e0, hipMemcpyAsync(out_blocker, e0->d_headroom_blocker.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
  KT_HIP(e0, hipStreamSynchronize(s));
  e0->headroom_ready = false;  // the results have been handed out: no headroom result of either kind is pending on page 0
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// preempt: the shortest victim prefix that lets a blocked pod through (kt_kernels_preempt.hip), and the reprieve pass that shrinks
// its victim mask to a minimal set (kt_kernels_reprieve.hip)
// ---------------------------------------------------------------------------------------------------
// kt_preempt_launch and, with `reprieve`, kt_preempt_reprieve_launch: the same refusals, the same launches, and behind them on the
// same stream the one launch of kt_preempt_reprieve that rewrites the victim bytes in place.  The caller holds the launch lock.
static int32_t preempt_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows, int64_t now_s,
                              int32_t now_ns, int32_t on_equal, void* stream, bool reprieve) {
  if (n_cand < 0) return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt: n_cand = %lld", (long long)n_cand);
  if ((n > 0 && !pod_rows) || (n_cand > 0 && !cand_rows)) return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt: pod_rows / cand_rows missing");
  for (int64_t i = 0; i < n + n_cand; ++i) {
    const int64_t r = i < n ? pod_rows[i] : cand_rows[i - n];
    if (r < 0 || r >= e->cfg.pod_capacity) return e->fail(KT_ERR_OUT_OF_RANGE, "preempt: pod row %lld", (long long)r);
  }
  {
    std::vector<int64_t> sorted(cand_rows, cand_rows + n_cand);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t j = 1; j < n_cand; ++j)
      if (sorted[(size_t)j] == sorted[(size_t)j - 1])
        return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt: pod row %lld is a candidate twice", (long long)sorted[(size_t)j]);
    for (int64_t i = 0; i < n; ++i)
      if (std::binary_search(sorted.begin(), sorted.end(), pod_rows[i]))
        return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt: pod row %lld is a preemptor and a candidate", (long long)pod_rows[i]);
  }
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  // the issue's two products, and their sum: the one matrix this call launches holds (n + n_cand) x throttle_rows bytes
  if ((double)n * (double)T > 2147483648.0 || (double)n_cand * (double)T > 2147483648.0 || ((double)n + (double)n_cand) * (double)T > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "preempt: (n + n_cand) x throttle_rows = (%lld + %lld) x %d exceeds 2^31 matrix bytes", (long long)n,
                   (long long)n_cand, T);
  if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "preempt: not for KT_VARIANT_INCREMENTAL engines");
  if (e->exchange_world > 1) return e->fail(KT_ERR_UNSUPPORTED, "preempt: the engine exchanges partials with %d ranks (one rank only)", e->exchange_world);
  if (e->wide && e->req_sums_valid) return e->fail(KT_ERR_UNSUPPORTED, "preempt: `used` is wider than int64 (kt_preempt reads int64 sums)");
  e->preempt_ready = false;
  if (n == 0) {  // nothing is launched
    e->preempt_ready = true, e->preempt_gangs = false, e->preempt_n = 0, e->preempt_m = n_cand;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  // pod batches since the last aggregate may have pushed the sums beyond int64: found out here (the |request| sums kernel, when
  // they are not known), before the check slot or any result buffer is touched
  int32_t rc = ensure_ready(e, s);
  if (rc == KT_OK) rc = request_sums_in_range(e, s);
  if (rc != KT_OK) return rc;
  if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "preempt: `used` is wider than int64 (kt_preempt reads int64 sums)");
  const size_t vic = (size_t)n * (size_t)n_cand;
  // the reprieve kernel's list state where it can outgrow LDS (0 bytes: it cannot, or nothing is walked)
  const size_t ws = reprieve && n_cand > 0 ? kt::reprieve_ws_bytes(T, e->D, n, e->reprieve_lds_cap_limit) : 0;
  if (e->d_preempt_prefix.cap < (size_t)n || e->d_preempt_victims.cap < vic + 1 || (ws != 0 && e->d_reprieve_ws.cap < ws)) {
    // a launch that was never fetched may still be writing the old buffers, on the stream it was given (as kt_headroom_launch)
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
    KT_HIP(e, e->d_preempt_prefix.reserve((size_t)n));
    KT_HIP(e, e->d_preempt_victims.reserve(vic + 1));
    if (ws != 0) KT_HIP(e, e->d_reprieve_ws.reserve(ws));
  }
  // ONE check over preemptors ++ candidates: which throttles match which pod, and the error rows
  std::vector<int64_t> rows((size_t)(n + n_cand));
  std::copy(pod_rows, pod_rows + n, rows.begin());
  std::copy(cand_rows, cand_rows + n_cand, rows.begin() + n);
  const bool forecast_was_ready = e->forecast_ready;  // its result lives in buffers this call does not write: it stays fetchable
  rc = check_launch_locked(e, n + n_cand, rows.data(), on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e->check_ready = false;  // the slot holds this call's rows (as with kt_affected_pods): a pending kt_check_launch is gone
  e->forecast_ready = forecast_was_ready;
  if (rc != KT_OK) return rc;
  if ((rc = preempt_reconcile_locked(e, now_s, now_ns, s)) != KT_OK) return rc;
  const kt::AdmitPage pg{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  kt::launch_preempt(pg, n, n_cand, e->d_rows.p, e->thr_rows_hi, on_equal != 0, e->d_status.p, e->d_summary.p, e->d_preempt_partial.p,
                     e->d_out_calc.tab(), e->d_out_calc_updated.p, e->d_out_error.p, e->d_preempt_prefix.p, e->d_preempt_victims.p, s);
  KT_HIP(e, hipGetLastError());
  if (reprieve) {
    kt::launch_preempt_reprieve(pg, n, n_cand, e->d_rows.p, e->thr_rows_hi, on_equal != 0, e->d_status.p, e->d_preempt_partial.p,
                                e->d_out_calc.tab(), e->d_out_calc_updated.p, e->d_out_error.p, e->d_preempt_prefix.p, e->d_preempt_victims.p,
                                ws != 0 ? e->d_reprieve_ws.p : nullptr, e->reprieve_lds_cap_limit, s);
    KT_HIP(e, hipGetLastError());
  }
  e->last_stream = s;
  e->preempt_ready = true, e->preempt_gangs = false, e->preempt_n = n, e->preempt_m = n_cand;
  return KT_OK;
}

int32_t kt_preempt_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows, int64_t now_s,
                          int32_t now_ns, int32_t on_equal, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return preempt_locked(e, n, pod_rows, n_cand, cand_rows, now_s, now_ns, on_equal, stream, /*reprieve=*/false);
}

int32_t kt_preempt_reprieve_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows, int64_t now_s,
                                   int32_t now_ns, int32_t on_equal, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return preempt_locked(e, n, pod_rows, n_cand, cand_rows, now_s, now_ns, on_equal, stream, /*reprieve=*/true);
}

int32_t kt_preempt_fetch(kt_engine* e, int64_t n, int64_t* out_prefix, uint8_t* out_victims) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (!e->preempt_ready || e->preempt_gangs) return e->fail(KT_ERR_NOT_READY, "kt_preempt_fetch before kt_preempt_launch");
  if (n < 0 || n > e->preempt_n) return e->fail(KT_ERR_OUT_OF_RANGE, "n=%lld, the last preempt launch had %lld pods", (long long)n, (long long)e->preempt_n);
  if (n == 0) return KT_OK;
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  if (out_prefix) KT_HIP(e, hipMemcpyAsync(out_prefix, e->d_preempt_prefix.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (out_victims && e->preempt_m)
    KT_HIP(e, hipMemcpyAsync(out_victims, e->d_preempt_victims.p, (size_t)n * (size_t)e->preempt_m, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// preempt over pages: kt_preempt_launch / kt_preempt_reprieve_launch on the cluster of all names (kt_kernels_preempt_paged.hip)
// ---------------------------------------------------------------------------------------------------
// How a synchronous paged call (kt_paged_preempt, kt_paged_preempt_gangs, kt_paged_forecast) ends once it has launched on page 0's stream s: the stream is
// drained, pages 1.. get back the last_stream they came with (`last`: nothing of the call stays pending on any page), and a
// device error that shows only now is returned in KT_OK's place
static int32_t paged_finish(const char* what, kt_engine* const* pages, int32_t n_pages, hipStream_t s, const std::vector<hipStream_t>& last,
                            int32_t code) {
  const hipError_t herr = hipStreamSynchronize(s);
  for (int32_t k = 1; k < n_pages; ++k) pages[k]->last_stream = last[(size_t)k];
  if (code == KT_OK && herr != hipSuccess) return pages[0]->fail(KT_ERR_DEVICE, "%s: %s", what, hipGetErrorString(herr));
  return code;
}

int32_t kt_paged_preempt(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows,
                         int64_t now_s, int32_t now_ns, int32_t on_equal, uint32_t flags, int64_t* out_prefix, uint8_t* out_victims) {
  PageLocks locks;
  int32_t rc = paged_lock("paged preempt", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if (flags & ~KT_PREEMPT_REPRIEVE) return e0->fail(KT_ERR_INVALID_ARGUMENT, "paged preempt: flags = 0x%x", flags);
  const bool reprieve = (flags & KT_PREEMPT_REPRIEVE) != 0;
  if (n_cand < 0) return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt: n_cand = %lld", (long long)n_cand);
  if ((n > 0 && !pod_rows) || (n_cand > 0 && !cand_rows)) return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt: pod_rows / cand_rows missing");
  if ((rc = paged_same_cluster("paged preempt", pages, n_pages, n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place:
  if ((rc = paged_same_cluster("paged preempt", pages, n_pages, n_cand, cand_rows)) != KT_OK) return rc;  //  nothing is allocated yet)
  const int32_t T = e0->thr_rows_hi;
  if ((double)n * (double)T > 2147483648.0 || (double)n_cand * (double)T > 2147483648.0 || ((double)n + (double)n_cand) * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "preempt: (n + n_cand) x throttle_rows = (%lld + %lld) x %d exceeds 2^31 matrix bytes", (long long)n,
                    (long long)n_cand, T);
  {
    std::vector<int64_t> sorted(cand_rows, cand_rows + n_cand);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t j = 1; j < n_cand; ++j)
      if (sorted[(size_t)j] == sorted[(size_t)j - 1])
        return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt: pod row %lld is a candidate twice", (long long)sorted[(size_t)j]);
    for (int64_t i = 0; i < n; ++i)
      if (std::binary_search(sorted.begin(), sorted.end(), pod_rows[i]))
        return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt: pod row %lld is a preemptor and a candidate", (long long)pod_rows[i]);
  }
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "preempt: page %d: not for KT_VARIANT_INCREMENTAL engines", k);
    if (e->exchange_world > 1)
      return e->fail(KT_ERR_UNSUPPORTED, "preempt: page %d exchanges partials with %d ranks (one rank only)", k, e->exchange_world);
    if (e->wide && e->req_sums_valid)
      return e->fail(KT_ERR_UNSUPPORTED, "preempt: `used` of page %d is wider than int64 (kt_preempt_paged reads int64 sums)", k);
  }
  if (n == 0) return KT_OK;  // nothing is launched
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  if ((rc = ensure_ready(e0, s)) != KT_OK) return rc;
  // pod batches since a page's last aggregate may have pushed its sums beyond int64: found out here (the |request| sums kernel of
  // that page, where they are not known), before the check slot, a reconcile report or a result buffer of any page is touched
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = request_sums_in_range(e, s)) != KT_OK) return rc;
    if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "preempt: `used` of page %d is wider than int64 (kt_preempt_paged reads int64 sums)", k);
  }
  // ---- from here on the call owns page 0's check slot and preempt result and every page's reconcile report
  e0->preempt_ready = false;
  if (!e0->preempt_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->preempt_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->preempt_pages_ev));  // the previous call's copy has read h_preempt_pages
  e0->h_preempt_pages.resize((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k)  // (D alone is read before the launches below fill in the rest)
    e0->h_preempt_pages[(size_t)k].pg = kt::AdmitPage{pages[k]->pods.flags, pages[k]->pods.req, pages[k]->tt, pages[k]->D, pages[k]->pods.DS, 0u, 0u, 0u};
  const size_t vic = (size_t)n * (size_t)n_cand;
  const size_t ws = reprieve && n_cand > 0 ? kt::reprieve_paged_ws_bytes(T, e0->h_preempt_pages.data(), n_pages, n, e0->reprieve_lds_cap_limit) : 0;
  if (e0->d_preempt_prefix.cap < (size_t)n || e0->d_preempt_victims.cap < vic + 1 || (ws != 0 && e0->d_reprieve_ws.cap < ws)) {
    // a launch that was never fetched may still be writing the old buffers, on the stream it was given (as kt_preempt_launch)
    if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));
    KT_HIP(e0, e0->d_preempt_prefix.reserve((size_t)n));
    KT_HIP(e0, e0->d_preempt_victims.reserve(vic + 1));
    if (ws != 0) KT_HIP(e0, e0->d_reprieve_ws.reserve(ws));
  }
  KT_HIP(e0, e0->d_preempt_pages.reserve(sizeof(kt::PreemptPage) * (size_t)n_pages));
  // Everything below runs on page 0's stream.  A failure after the first launch drains that stream before it is returned, and
  // pages 1.. get their own stream back as last_stream: nothing of this call stays pending on any page.
  std::vector<hipStream_t> last((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) last[(size_t)k] = pages[k]->last_stream;
  auto finish = [&](int32_t code) -> int32_t { return paged_finish("paged preempt", pages, n_pages, s, last, code); };
  // ONE check of page 0 over preemptors ++ candidates: which throttles match which pod, and the error rows
  std::vector<int64_t> rows((size_t)(n + n_cand));
  std::copy(pod_rows, pod_rows + n, rows.begin());
  std::copy(cand_rows, cand_rows + n_cand, rows.begin() + n);
  const bool forecast_was_ready = e0->forecast_ready;  // its result lives in buffers this call does not write: it stays fetchable
  rc = check_launch_locked(e0, n + n_cand, rows.data(), on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e0->check_ready = false;  // the slot holds this call's rows (as with kt_affected_pods): a pending kt_check_launch is gone
  e0->forecast_ready = forecast_was_ready;
  if (rc != KT_OK) return finish(rc);
  // every page: its dense aggregate beside its partial buffer and its dry finalize at `now` (its reconcile report is dropped)
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = preempt_reconcile_locked(e, now_s, now_ns, s)) != KT_OK) return finish(rc);
    kt::PreemptPage& pp = e0->h_preempt_pages[(size_t)k];
    pp.partial = e->d_preempt_partial.p, pp.calc = e->d_out_calc.tab(), pp.calc_updated = e->d_out_calc_updated.p, pp.error = e->d_out_error.p;
  }
  hipError_t herr = hipSuccess;
  if (!kt::launch_preempt_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n, n_cand,
                                e0->d_rows.p, T, on_equal != 0, e0->d_status.p, e0->d_summary.p, e0->d_preempt_prefix.p, e0->d_preempt_victims.p, s,
                                &herr))
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt: copy of the page descriptors: %s", hipGetErrorString(herr)));
  if ((herr = hipGetLastError()) != hipSuccess) return finish(e0->fail(KT_ERR_DEVICE, "paged preempt: %s", hipGetErrorString(herr)));
  if (reprieve) {
    kt::launch_preempt_reprieve_paged(e0->h_preempt_pages.data(), n_pages, (const kt::PreemptPage*)e0->d_preempt_pages.p, n, n_cand, e0->d_rows.p, T,
                                      on_equal != 0, e0->d_status.p, e0->d_preempt_prefix.p, e0->d_preempt_victims.p,
                                      ws != 0 ? e0->d_reprieve_ws.p : nullptr, e0->reprieve_lds_cap_limit, s);
    if ((herr = hipGetLastError()) != hipSuccess) return finish(e0->fail(KT_ERR_DEVICE, "paged preempt: %s", hipGetErrorString(herr)));
  }
  e0->last_stream = s;
  if (out_prefix && (herr = hipMemcpyAsync(out_prefix, e0->d_preempt_prefix.p, (size_t)n * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt: %s", hipGetErrorString(herr)));
  if (out_victims && n_cand && (herr = hipMemcpyAsync(out_victims, e0->d_preempt_victims.p, vic, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt: %s", hipGetErrorString(herr)));
  return finish(KT_OK);  // (synchronises s; the results have been handed out: no preempt result is pending on page 0)
}

// ---------------------------------------------------------------------------------------------------
// preempt, for gangs: the shortest victim prefix that lets a whole gang through (kt_kernels_preempt_gangs.hip), and the reprieve
// pass that shrinks its victim mask to a minimal set (kt_kernels_preempt_gangs_reprieve.hip)
// ---------------------------------------------------------------------------------------------------
// kt_preempt_gangs_launch: the refusals of preempt_locked in its order (with the gang defects in front, and "a pod twice" asked
// per gang), then the same launches with kt_preempt_gangs in kt_preempt's place.  The result shares the one pending preempt result;
// preempt_gangs tells the fetches apart.  With `reprieve` (kt_preempt_gangs_reprieve_launch): behind them on the same stream the one
// launch of kt_preempt_gangs_reprieve that rewrites the victim bytes in place.  The caller holds the launch lock.
static int32_t preempt_gangs_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_cand,
                                    const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, void* stream, bool reprieve) {
  int32_t rc = gangs_valid(e, n, n_gangs, gang_off);
  if (rc != KT_OK) return rc;
  if (n_cand < 0) return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: n_cand = %lld", (long long)n_cand);
  if ((n > 0 && !pod_rows) || (n_cand > 0 && !cand_rows)) return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod_rows / cand_rows missing");
  for (int64_t i = 0; i < n + n_cand; ++i) {
    const int64_t r = i < n ? pod_rows[i] : cand_rows[i - n];
    if (r < 0 || r >= e->cfg.pod_capacity) return e->fail(KT_ERR_OUT_OF_RANGE, "preempt gangs: pod row %lld", (long long)r);
  }
  {
    std::vector<int64_t> sorted(cand_rows, cand_rows + n_cand);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t j = 1; j < n_cand; ++j)
      if (sorted[(size_t)j] == sorted[(size_t)j - 1])
        return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod row %lld is a candidate twice", (long long)sorted[(size_t)j]);
    for (int64_t i = 0; i < n; ++i)
      if (std::binary_search(sorted.begin(), sorted.end(), pod_rows[i]))
        return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod row %lld is a member and a candidate", (long long)pod_rows[i]);
    // gangs are alternatives: a pod may be in several of them, but not twice in one (it would reserve twice)
    for (int64_t g = 0; g < n_gangs; ++g) {
      sorted.assign(pod_rows + gang_off[g], pod_rows + gang_off[g + 1]);
      std::sort(sorted.begin(), sorted.end());
      for (size_t j = 1; j < sorted.size(); ++j)
        if (sorted[j] == sorted[j - 1])
          return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod row %lld is in gang %lld twice", (long long)sorted[j], (long long)g);
    }
  }
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  if ((double)n * (double)T > 2147483648.0 || (double)n_cand * (double)T > 2147483648.0 || ((double)n + (double)n_cand) * (double)T > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "preempt gangs: (n + n_cand) x throttle_rows = (%lld + %lld) x %d exceeds 2^31 matrix bytes", (long long)n,
                   (long long)n_cand, T);
  if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: not for KT_VARIANT_INCREMENTAL engines");
  if (e->exchange_world > 1)
    return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: the engine exchanges partials with %d ranks (one rank only)", e->exchange_world);
  if (e->wide && e->req_sums_valid) return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: `used` is wider than int64 (kt_preempt_gangs reads int64 sums)");
  if (n == 0) {  // (no gangs) nothing is launched
    e->preempt_ready = true, e->preempt_gangs = true, e->preempt_n = 0, e->preempt_m = n_cand;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  // the |request| sums probe where the sums are unknown, before the check slot or any result buffer is touched (as preempt_locked)
  rc = ensure_ready(e, s);
  if (rc == KT_OK) rc = request_sums_in_range(e, s);
  if (rc != KT_OK) return rc;
  if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: `used` is wider than int64 (kt_preempt_gangs reads int64 sums)");
  const size_t vic = (size_t)n_gangs * (size_t)n_cand;
  // the reprieve kernel's list state where it can outgrow LDS (0 bytes: it cannot, or nothing is walked)
  const size_t ws = reprieve && n_cand > 0 ? kt::reprieve_ws_bytes(T, e->D, n_gangs, e->reprieve_lds_cap_limit) : 0;
  if (e->d_preempt_prefix.cap < (size_t)n_gangs || e->d_preempt_victims.cap < vic + 1 || e->d_preempt_blocker.cap < (size_t)n_gangs ||
      e->d_preempt_gang_off.cap < (size_t)n_gangs + 1 || (ws != 0 && e->d_reprieve_ws.cap < ws)) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_preempt_launch)
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
    KT_HIP(e, e->d_preempt_prefix.reserve((size_t)n_gangs));
    KT_HIP(e, e->d_preempt_victims.reserve(vic + 1));
    KT_HIP(e, e->d_preempt_blocker.reserve((size_t)n_gangs));
    KT_HIP(e, e->d_preempt_gang_off.reserve((size_t)n_gangs + 1));
    if (ws != 0) KT_HIP(e, e->d_reprieve_ws.reserve(ws));
  }
  // the offsets travel on the launch's stream, behind an earlier launch's kernel; the caller's memory is not referenced after return
  KT_HIP(e, hipMemcpyAsync(e->d_preempt_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  // ONE check over members ++ candidates: which throttles match which pod, and the error rows
  std::vector<int64_t> rows((size_t)(n + n_cand));
  std::copy(pod_rows, pod_rows + n, rows.begin());
  std::copy(cand_rows, cand_rows + n_cand, rows.begin() + n);
  const bool forecast_was_ready = e->forecast_ready;  // its result lives in buffers this call does not write: it stays fetchable
  rc = check_launch_locked(e, n + n_cand, rows.data(), on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e->check_ready = false;  // the slot holds this call's rows (as with kt_preempt_launch): a pending kt_check_launch is gone
  e->forecast_ready = forecast_was_ready;
  if (rc != KT_OK) return rc;
  if ((rc = preempt_reconcile_locked(e, now_s, now_ns, s)) != KT_OK) return rc;
  const kt::AdmitPage pg{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  kt::launch_preempt_gangs(pg, n, n_cand, e->d_rows.p, n_gangs, e->d_preempt_gang_off.p, e->thr_rows_hi, on_equal != 0, e->d_status.p, e->d_summary.p,
                           e->d_preempt_partial.p, e->d_out_calc.tab(), e->d_out_calc_updated.p, e->d_out_error.p, e->d_preempt_prefix.p,
                           e->d_preempt_victims.p, e->d_preempt_blocker.p, s);
  KT_HIP(e, hipGetLastError());
  if (reprieve) {
    kt::launch_preempt_gangs_reprieve(pg, n, n_cand, e->d_rows.p, n_gangs, e->d_preempt_gang_off.p, e->thr_rows_hi, on_equal != 0, e->d_status.p,
                                      e->d_preempt_partial.p, e->d_out_calc.tab(), e->d_out_calc_updated.p, e->d_out_error.p, e->d_preempt_prefix.p,
                                      e->d_preempt_victims.p, ws != 0 ? e->d_reprieve_ws.p : nullptr, e->reprieve_lds_cap_limit, s);
    KT_HIP(e, hipGetLastError());
  }
  e->last_stream = s;
  e->preempt_ready = true, e->preempt_gangs = true, e->preempt_n = n_gangs, e->preempt_m = n_cand;
  return KT_OK;
}

int32_t kt_preempt_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_cand,
                                const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return preempt_gangs_locked(e, n, pod_rows, n_gangs, gang_off, n_cand, cand_rows, now_s, now_ns, on_equal, stream, /*reprieve=*/false);
}

int32_t kt_preempt_gangs_reprieve_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_cand,
                                         const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return preempt_gangs_locked(e, n, pod_rows, n_gangs, gang_off, n_cand, cand_rows, now_s, now_ns, on_equal, stream, /*reprieve=*/true);
}

int32_t kt_preempt_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_prefix, uint8_t* out_victims, int64_t* out_blocker) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (!e->preempt_ready || !e->preempt_gangs) return e->fail(KT_ERR_NOT_READY, "kt_preempt_gangs_fetch before kt_preempt_gangs_launch");
  if (n_gangs < 0 || n_gangs > e->preempt_n)
    return e->fail(KT_ERR_OUT_OF_RANGE, "n_gangs=%lld, the last preempt gangs launch had %lld gangs", (long long)n_gangs, (long long)e->preempt_n);
  if (n_gangs == 0) return KT_OK;
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  if (out_prefix) KT_HIP(e, hipMemcpyAsync(out_prefix, e->d_preempt_prefix.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
  if (out_victims && e->preempt_m)
    KT_HIP(e, hipMemcpyAsync(out_victims, e->d_preempt_victims.p, (size_t)n_gangs * (size_t)e->preempt_m, hipMemcpyDeviceToHost, s));
  if (out_blocker) KT_HIP(e, hipMemcpyAsync(out_blocker, e->d_preempt_blocker.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// preempt, for gangs, over pages: kt_preempt_gangs_launch / kt_preempt_gangs_reprieve_launch on the cluster of all names
// (kt_kernels_preempt_gangs_paged.hip)
// ---------------------------------------------------------------------------------------------------
int32_t kt_paged_preempt_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                               int64_t n_cand, const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, uint32_t flags,
                               int64_t* out_prefix, uint8_t* out_victims, int64_t* out_blocker) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  PageLocks locks;
  int32_t rc = paged_lock("paged preempt gangs", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  // ---- refusals: nothing is allocated or launched and no slot of any page is touched before the last of them
  if (flags & ~KT_PREEMPT_REPRIEVE) return e0->fail(KT_ERR_INVALID_ARGUMENT, "paged preempt gangs: flags = 0x%x", flags);
  const bool reprieve = (flags & KT_PREEMPT_REPRIEVE) != 0;
  if ((rc = gangs_valid(e0, n, n_gangs, gang_off)) != KT_OK) return rc;
  if (n_cand < 0) return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: n_cand = %lld", (long long)n_cand);
  if ((n > 0 && !pod_rows) || (n_cand > 0 && !cand_rows)) return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod_rows / cand_rows missing");
  if ((rc = paged_same_cluster("paged preempt gangs", pages, n_pages, n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked
  if ((rc = paged_same_cluster("paged preempt gangs", pages, n_pages, n_cand, cand_rows)) != KT_OK) return rc;  //  in place)
  {
    std::vector<int64_t> sorted(cand_rows, cand_rows + n_cand);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t j = 1; j < n_cand; ++j)
      if (sorted[(size_t)j] == sorted[(size_t)j - 1])
        return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod row %lld is a candidate twice", (long long)sorted[(size_t)j]);
    for (int64_t i = 0; i < n; ++i)
      if (std::binary_search(sorted.begin(), sorted.end(), pod_rows[i]))
        return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod row %lld is a member and a candidate", (long long)pod_rows[i]);
    // gangs are alternatives: a pod may be in several of them, but not twice in one (it would reserve twice)
    for (int64_t g = 0; g < n_gangs; ++g) {
      sorted.assign(pod_rows + gang_off[g], pod_rows + gang_off[g + 1]);
      std::sort(sorted.begin(), sorted.end());
      for (size_t j = 1; j < sorted.size(); ++j)
        if (sorted[j] == sorted[j - 1])
          return e0->fail(KT_ERR_INVALID_ARGUMENT, "preempt gangs: pod row %lld is in gang %lld twice", (long long)sorted[j], (long long)g);
    }
  }
  const int32_t T = e0->thr_rows_hi;
  if ((double)n * (double)T > 2147483648.0 || (double)n_cand * (double)T > 2147483648.0 || ((double)n + (double)n_cand) * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "preempt gangs: (n + n_cand) x throttle_rows = (%lld + %lld) x %d exceeds 2^31 matrix bytes", (long long)n,
                    (long long)n_cand, T);
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: page %d: not for KT_VARIANT_INCREMENTAL engines", k);
    if (e->exchange_world > 1)
      return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: page %d exchanges partials with %d ranks (one rank only)", k, e->exchange_world);
    if (e->wide && e->req_sums_valid)
      return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: `used` of page %d is wider than int64 (kt_preempt_gangs_paged reads int64 sums)", k);
  }
  if (n == 0) return KT_OK;  // (no gangs) nothing is launched
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  if ((rc = ensure_ready(e0, s)) != KT_OK) return rc;
  // the |request| sums probe of every page where the sums are not known, before the check slot, a reconcile report or a result
  // buffer of any page is touched (as kt_paged_preempt)
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = request_sums_in_range(e, s)) != KT_OK) return rc;
    if (e->wide)
      return e->fail(KT_ERR_UNSUPPORTED, "preempt gangs: `used` of page %d is wider than int64 (kt_preempt_gangs_paged reads int64 sums)", k);
  }
  // ---- from here on the call owns page 0's check slot and preempt result and every page's reconcile report
  e0->preempt_ready = false;
  if (!e0->preempt_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->preempt_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->preempt_pages_ev));  // the previous call's copy has read h_preempt_pages
  e0->h_preempt_pages.resize((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k)  // (D alone is read before the launches below fill in the rest)
    e0->h_preempt_pages[(size_t)k].pg = kt::AdmitPage{pages[k]->pods.flags, pages[k]->pods.req, pages[k]->tt, pages[k]->D, pages[k]->pods.DS, 0u, 0u, 0u};
  const size_t vic = (size_t)n_gangs * (size_t)n_cand;
  const size_t ws =
      reprieve && n_cand > 0 ? kt::reprieve_paged_ws_bytes(T, e0->h_preempt_pages.data(), n_pages, n_gangs, e0->reprieve_lds_cap_limit) : 0;
  if (e0->d_preempt_prefix.cap < (size_t)n_gangs || e0->d_preempt_victims.cap < vic + 1 || e0->d_preempt_blocker.cap < (size_t)n_gangs ||
      e0->d_preempt_gang_off.cap < (size_t)n_gangs + 1 || (ws != 0 && e0->d_reprieve_ws.cap < ws)) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_preempt_gangs_launch)
    if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));
    KT_HIP(e0, e0->d_preempt_prefix.reserve((size_t)n_gangs));
    KT_HIP(e0, e0->d_preempt_victims.reserve(vic + 1));
    KT_HIP(e0, e0->d_preempt_blocker.reserve((size_t)n_gangs));
    KT_HIP(e0, e0->d_preempt_gang_off.reserve((size_t)n_gangs + 1));
    if (ws != 0) KT_HIP(e0, e0->d_reprieve_ws.reserve(ws));
  }
  KT_HIP(e0, e0->d_preempt_pages.reserve(sizeof(kt::PreemptPage) * (size_t)n_pages));
  // Everything below runs on page 0's stream.  A failure after the first launch drains that stream before it is returned, and
  // pages 1.. get their own stream back as last_stream: nothing of this call stays pending on any page.
  std::vector<hipStream_t> last((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) last[(size_t)k] = pages[k]->last_stream;
  auto finish = [&](int32_t code) -> int32_t { return paged_finish("paged preempt gangs", pages, n_pages, s, last, code); };
  // ONE check of page 0 over members ++ candidates: which throttles match which pod, and the error rows
  std::vector<int64_t> rows((size_t)(n + n_cand));
  std::copy(pod_rows, pod_rows + n, rows.begin());
  std::copy(cand_rows, cand_rows + n_cand, rows.begin() + n);
  const bool forecast_was_ready = e0->forecast_ready;  // its result lives in buffers this call does not write: it stays fetchable
  rc = check_launch_locked(e0, n + n_cand, rows.data(), on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e0->check_ready = false;  // the slot holds this call's rows (as with kt_affected_pods): a pending kt_check_launch is gone
  e0->forecast_ready = forecast_was_ready;
  if (rc != KT_OK) return finish(rc);
  // every page: its dense aggregate beside its partial buffer and its dry finalize at `now` (its reconcile report is dropped)
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = preempt_reconcile_locked(e, now_s, now_ns, s)) != KT_OK) return finish(rc);
    kt::PreemptPage& pp = e0->h_preempt_pages[(size_t)k];
    pp.partial = e->d_preempt_partial.p, pp.calc = e->d_out_calc.tab(), pp.calc_updated = e->d_out_calc_updated.p, pp.error = e->d_out_error.p;
  }
  hipError_t herr = hipSuccess;
  // the offsets travel on the same stream (the call is synchronous: the caller's memory outlives the copy)
  if ((herr = hipMemcpyAsync(e0->d_preempt_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt gangs: copy of the gang offsets: %s", hipGetErrorString(herr)));
  if (!kt::launch_preempt_gangs_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n, n_cand,
                                      e0->d_rows.p, n_gangs, e0->d_preempt_gang_off.p, T, on_equal != 0, e0->d_status.p, e0->d_summary.p,
                                      e0->d_preempt_prefix.p, e0->d_preempt_victims.p, e0->d_preempt_blocker.p, s, &herr))
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt gangs: copy of the page descriptors: %s", hipGetErrorString(herr)));
  if ((herr = hipGetLastError()) != hipSuccess) return finish(e0->fail(KT_ERR_DEVICE, "paged preempt gangs: %s", hipGetErrorString(herr)));
  if (reprieve) {
    kt::launch_preempt_gangs_reprieve_paged(e0->h_preempt_pages.data(), n_pages, (const kt::PreemptPage*)e0->d_preempt_pages.p, n, n_cand, e0->d_rows.p,
                                            n_gangs, e0->d_preempt_gang_off.p, T, on_equal != 0, e0->d_status.p, e0->d_preempt_prefix.p,
                                            e0->d_preempt_victims.p, ws != 0 ? e0->d_reprieve_ws.p : nullptr, e0->reprieve_lds_cap_limit, s);
    if ((herr = hipGetLastError()) != hipSuccess) return finish(e0->fail(KT_ERR_DEVICE, "paged preempt gangs: %s", hipGetErrorString(herr)));
  }
  e0->last_stream = s;
  if (out_prefix && (herr = hipMemcpyAsync(out_prefix, e0->d_preempt_prefix.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt gangs: %s", hipGetErrorString(herr)));
  if (out_victims && n_cand && (herr = hipMemcpyAsync(out_victims, e0->d_preempt_victims.p, vic, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt gangs: %s", hipGetErrorString(herr)));
  if (out_blocker && (herr = hipMemcpyAsync(out_blocker, e0->d_preempt_blocker.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged preempt gangs: %s", hipGetErrorString(herr)));
  return finish(KT_OK);  // (synchronises s; the results have been handed out: no preempt result is pending on page 0)
}

// ---------------------------------------------------------------------------------------------------
// forecast: the first instant at which a blocked pod passes (kt_kernels_forecast.hip)
// ---------------------------------------------------------------------------------------------------
// what kt_forecast_launch, kt_forecast_gangs_launch and kt_paged_forecast_gangs refuse about their instants (and a missing array), in
// front of everything else
static int32_t forecast_instants_valid(kt_engine* e, bool rows_missing, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns) {
  if (n_inst < 1) return e->fail(KT_ERR_INVALID_ARGUMENT, "forecast: n_inst = %lld", (long long)n_inst);
  if (rows_missing || !inst_s || !inst_ns) return e->fail(KT_ERR_INVALID_ARGUMENT, "forecast: pod_rows / inst_s / inst_ns missing");
  for (int64_t k = 0; k < n_inst; ++k) {
    if (inst_ns[k] < 0 || inst_ns[k] >= 1000000000) return e->fail(KT_ERR_INVALID_ARGUMENT, "forecast: inst_ns[%lld] = %d", (long long)k, inst_ns[k]);
    if (k && !(inst_s[k - 1] < inst_s[k] || (inst_s[k - 1] == inst_s[k] && inst_ns[k - 1] < inst_ns[k])))
      return e->fail(KT_ERR_INVALID_ARGUMENT, "forecast: the instants are not strictly ascending at position %lld", (long long)k);
  }
  return KT_OK;
}

// The caller holds the launch lock.  Every refusal comes before the check slot, the reconcile report or a result buffer is touched.
static int32_t forecast_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns,
                               int32_t on_equal, void* stream) {
  if (int32_t bad = forecast_instants_valid(e, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) return bad;
  for (int64_t i = 0; i < n; ++i)
    if (pod_rows[i] < 0 || pod_rows[i] >= e->cfg.pod_capacity) return e->fail(KT_ERR_OUT_OF_RANGE, "forecast: pod row %lld", (long long)pod_rows[i]);
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  if ((double)n * (double)T > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "forecast: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  if ((double)n * (double)n_inst > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "forecast: n x n_inst = %lld x %lld exceeds 2^31 verdict bytes", (long long)n, (long long)n_inst);
  if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "forecast: not for KT_VARIANT_INCREMENTAL engines");
  if (e->exchange_world > 1) return e->fail(KT_ERR_UNSUPPORTED, "forecast: the engine exchanges partials with %d ranks (one rank only)", e->exchange_world);
  if (e->wide && e->req_sums_valid) return e->fail(KT_ERR_UNSUPPORTED, "forecast: `used` is wider than int64 (kt_forecast reads int64 sums)");
  if (n == 0) {  // nothing is launched
    e->forecast_ready = true, e->forecast_kind = kForecastPods, e->forecast_n = 0, e->forecast_m = n_inst;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  // pod batches since the last aggregate may have pushed the sums beyond int64: found out here (the |request| sums kernel, when
  // they are not known), before the check slot or any result buffer is touched
  int32_t rc = ensure_ready(e, s);
  if (rc == KT_OK) rc = request_sums_in_range(e, s);
  if (rc != KT_OK) return rc;
  if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "forecast: `used` is wider than int64 (kt_forecast reads int64 sums)");
  e->forecast_ready = false;
  const size_t ver = (size_t)n * (size_t)n_inst;
  if (e->d_forecast_first.cap < (size_t)n || e->d_forecast_verdicts.cap < ver + 1 || e->d_forecast_inst_s.cap < (size_t)n_inst ||
      e->d_forecast_inst_ns.cap < (size_t)n_inst) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_preempt_launch)
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
    KT_HIP(e, e->d_forecast_first.reserve((size_t)n));
    KT_HIP(e, e->d_forecast_verdicts.reserve(ver + 1));
    KT_HIP(e, e->d_forecast_inst_s.reserve((size_t)n_inst));
    KT_HIP(e, e->d_forecast_inst_ns.reserve((size_t)n_inst));
  }
  // the instants travel on the launch's stream, behind an earlier forecast's kernel; the caller's memory is not referenced after
  // return (the synchronisation is the one behind the check's row copy, and one of the call's own for safety)
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_s.p, inst_s, (size_t)n_inst * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_ns.p, inst_ns, (size_t)n_inst * 4, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  // ONE check over the pods: which throttles affect which pod, and the error rows.  The preempt result lives in buffers this
  // call does not write: it stays fetchable
  const bool preempt_was_ready = e->preempt_ready;
  rc = check_launch_locked(e, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e->check_ready = false;  // the slot holds this call's rows (as with kt_preempt_launch): a pending kt_check_launch is gone
  e->preempt_ready = preempt_was_ready;
  if (rc != KT_OK) return rc;
  // the aggregate with exact contributor counts and the error bytes; the dry finalize runs at t_0
  if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return rc;
  const kt::AdmitPage pg{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  kt::launch_forecast(pg, n, n_inst, e->d_rows.p, e->d_forecast_inst_s.p, e->d_forecast_inst_ns.p, T, on_equal != 0, e->d_status.p, e->d_summary.p,
                      e->d_preempt_partial.p, e->d_out_error.p, e->d_forecast_first.p, e->d_forecast_verdicts.p, s);
  KT_HIP(e, hipGetLastError());
  e->last_stream = s;
  e->forecast_ready = true, e->forecast_kind = kForecastPods, e->forecast_n = n, e->forecast_m = n_inst;
  return KT_OK;
}

int32_t kt_forecast_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns,
                           int32_t on_equal, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return forecast_locked(e, n, pod_rows, n_inst, inst_s, inst_ns, on_equal, stream);
}

int32_t kt_forecast_fetch(kt_engine* e, int64_t n, int64_t* out_first, uint8_t* out_verdicts) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (!e->forecast_ready || e->forecast_kind != kForecastPods) return e->fail(KT_ERR_NOT_READY, "kt_forecast_fetch before kt_forecast_launch");
  if (n < 0 || n > e->forecast_n) return e->fail(KT_ERR_OUT_OF_RANGE, "n=%lld, the last forecast launch had %lld pods", (long long)n, (long long)e->forecast_n);
  if (n == 0) return KT_OK;
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  if (out_first) KT_HIP(e, hipMemcpyAsync(out_first, e->d_forecast_first.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (out_verdicts) KT_HIP(e, hipMemcpyAsync(out_verdicts, e->d_forecast_verdicts.p, (size_t)n * (size_t)e->forecast_m, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// headroom forecast: how many copies of a pod the throttles admit at each instant (kt_kernels_headroom_forecast.hip)
// ---------------------------------------------------------------------------------------------------
// forecast_locked's sequence with kt_headroom_forecast in kt_forecast's place: the refusals in its order (cap and want behind the
// instants), the |request| sums probe, ONE check, the dry aggregate and finalize at t_0, the kernel.  The result shares the one
// pending forecast result as its third kind.  The caller holds the launch lock.
static int32_t headroom_forecast_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s,
                                        const int32_t* inst_ns, int32_t on_equal, int64_t cap, int64_t want, void* stream) {
  if (int32_t bad = forecast_instants_valid(e, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) return bad;
  if (!headroom_cap_ok(cap))
    return e->fail(KT_ERR_INVALID_ARGUMENT, "headroom forecast: cap = %lld, not in [1, %d]", (long long)cap, KT_HEADROOM_MAX_CAP);
  if (want < 1 || want > cap)
    return e->fail(KT_ERR_INVALID_ARGUMENT, "headroom forecast: want = %lld, not in [1, cap = %lld]", (long long)want, (long long)cap);
  for (int64_t i = 0; i < n; ++i)
    if (pod_rows[i] < 0 || pod_rows[i] >= e->cfg.pod_capacity)
      return e->fail(KT_ERR_OUT_OF_RANGE, "headroom forecast: pod row %lld", (long long)pod_rows[i]);
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  if ((double)n * (double)T > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "headroom forecast: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  if ((double)n * (double)n_inst > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "headroom forecast: n x n_inst = %lld x %lld exceeds 2^31 results", (long long)n, (long long)n_inst);
  if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "headroom forecast: not for KT_VARIANT_INCREMENTAL engines");
  if (e->exchange_world > 1)
    return e->fail(KT_ERR_UNSUPPORTED, "headroom forecast: the engine exchanges partials with %d ranks (one rank only)", e->exchange_world);
  if (e->wide && e->req_sums_valid)
    return e->fail(KT_ERR_UNSUPPORTED, "headroom forecast: `used` is wider than int64 (kt_headroom_forecast reads int64 sums)");
  if (n == 0) {  // nothing is launched
    e->forecast_ready = true, e->forecast_kind = kForecastHeadroom, e->forecast_n = 0, e->forecast_m = n_inst;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  // the |request| sums probe where the sums are unknown, before the check slot or any result buffer is touched (as forecast_locked)
  int32_t rc = ensure_ready(e, s);
  if (rc == KT_OK) rc = request_sums_in_range(e, s);
  if (rc != KT_OK) return rc;
  if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "headroom forecast: `used` is wider than int64 (kt_headroom_forecast reads int64 sums)");
  e->forecast_ready = false;
  const size_t cells = (size_t)n * (size_t)n_inst;
  if (e->d_forecast_first.cap < (size_t)n || e->d_forecast_copies.cap < cells || e->d_forecast_limiting.cap < cells ||
      e->d_forecast_inst_s.cap < (size_t)n_inst || e->d_forecast_inst_ns.cap < (size_t)n_inst) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_forecast_launch)
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
    KT_HIP(e, e->d_forecast_first.reserve((size_t)n));
    KT_HIP(e, e->d_forecast_copies.reserve(cells));
    KT_HIP(e, e->d_forecast_limiting.reserve(cells));
    KT_HIP(e, e->d_forecast_inst_s.reserve((size_t)n_inst));
    KT_HIP(e, e->d_forecast_inst_ns.reserve((size_t)n_inst));
  }
  // the instants travel on the launch's stream, behind an earlier forecast's kernel; the caller's memory is not referenced after
  // return
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_s.p, inst_s, (size_t)n_inst * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_ns.p, inst_ns, (size_t)n_inst * 4, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  // ONE check over the pods: which throttles affect which pod, and the error rows.  The preempt result lives in buffers this
  // call does not write: it stays fetchable
  const bool preempt_was_ready = e->preempt_ready;
  rc = check_launch_locked(e, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e->check_ready = false;  // the slot holds this call's rows (as with kt_forecast_launch): a pending kt_check_launch is gone
  e->preempt_ready = preempt_was_ready;
  if (rc != KT_OK) return rc;
  // the aggregate with exact contributor counts and the error bytes; the dry finalize runs at t_0
  if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return rc;
  const kt::AdmitPage pg{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  kt::launch_headroom_forecast(pg, n, n_inst, e->d_rows.p, e->d_forecast_inst_s.p, e->d_forecast_inst_ns.p, T, on_equal != 0, (uint32_t)cap,
                               (uint32_t)want, e->d_status.p, e->d_summary.p, e->d_preempt_partial.p, e->d_out_error.p, e->d_forecast_first.p,
                               e->d_forecast_copies.p, e->d_forecast_limiting.p, s);
  KT_HIP(e, hipGetLastError());
  e->last_stream = s;
  e->forecast_ready = true, e->forecast_kind = kForecastHeadroom, e->forecast_n = n, e->forecast_m = n_inst;
  return KT_OK;
}

int32_t kt_headroom_forecast_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns,
                                    int32_t on_equal, int64_t cap, int64_t want, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return headroom_forecast_locked(e, n, pod_rows, n_inst, inst_s, inst_ns, on_equal, cap, want, stream);
}

int32_t kt_headroom_forecast_fetch(kt_engine* e, int64_t n, int64_t* out_first, int64_t* out_copies, int32_t* out_limiting) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (!e->forecast_ready || e->forecast_kind != kForecastHeadroom)
    return e->fail(KT_ERR_NOT_READY, "kt_headroom_forecast_fetch before kt_headroom_forecast_launch");
  if (n < 0 || n > e->forecast_n)
    return e->fail(KT_ERR_OUT_OF_RANGE, "n=%lld, the last headroom forecast launch had %lld pods", (long long)n, (long long)e->forecast_n);
  if (n == 0) return KT_OK;
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  const size_t cells = (size_t)n * (size_t)e->forecast_m;
  if (out_first) KT_HIP(e, hipMemcpyAsync(out_first, e->d_forecast_first.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (out_copies) KT_HIP(e, hipMemcpyAsync(out_copies, e->d_forecast_copies.p, cells * 8, hipMemcpyDeviceToHost, s));
  if (out_limiting) KT_HIP(e, hipMemcpyAsync(out_limiting, e->d_forecast_limiting.p, cells * 4, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// forecast, for gangs: the first instant at which a whole gang is admitted (kt_kernels_forecast_gangs.hip)
// ---------------------------------------------------------------------------------------------------
// The refusals of forecast_locked in its order (the instants first, then the gang defects and "a pod twice" asked per gang), then
// the same launches with kt_forecast_gangs in kt_forecast's place.  The result shares the one pending forecast result;
// forecast_kind tells the fetches apart.  The caller holds the launch lock.
static int32_t forecast_gangs_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_inst,
                                     const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, void* stream) {
  if (int32_t bad = forecast_instants_valid(e, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) return bad;
  int32_t rc = gangs_valid(e, n, n_gangs, gang_off);
  if (rc != KT_OK) return rc;
  {
    // gangs are judged independently: a pod may be in several of them, but not twice in one (it would reserve twice)
    std::vector<int64_t> sorted;
    for (int64_t g = 0; g < n_gangs; ++g) {
      sorted.assign(pod_rows + gang_off[g], pod_rows + gang_off[g + 1]);
      std::sort(sorted.begin(), sorted.end());
      for (size_t j = 1; j < sorted.size(); ++j)
        if (sorted[j] == sorted[j - 1])
          return e->fail(KT_ERR_INVALID_ARGUMENT, "forecast gangs: pod row %lld is in gang %lld twice", (long long)sorted[j], (long long)g);
    }
  }
  for (int64_t i = 0; i < n; ++i)
    if (pod_rows[i] < 0 || pod_rows[i] >= e->cfg.pod_capacity)
      return e->fail(KT_ERR_OUT_OF_RANGE, "forecast gangs: pod row %lld", (long long)pod_rows[i]);
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  if ((double)n * (double)T > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "forecast gangs: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  if ((double)n_gangs * (double)n_inst > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "forecast gangs: n_gangs x n_inst = %lld x %lld exceeds 2^31 verdict bytes", (long long)n_gangs,
                   (long long)n_inst);
  if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: not for KT_VARIANT_INCREMENTAL engines");
  if (e->exchange_world > 1)
    return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: the engine exchanges partials with %d ranks (one rank only)", e->exchange_world);
  if (e->wide && e->req_sums_valid)
    return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: `used` is wider than int64 (kt_forecast_gangs reads int64 sums)");
  if (n == 0) {  // (no gangs) nothing is launched
    e->forecast_ready = true, e->forecast_kind = kForecastGangs, e->forecast_n = 0, e->forecast_m = n_inst;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  // the |request| sums probe where the sums are unknown, before the check slot or any result buffer is touched (as forecast_locked)
  rc = ensure_ready(e, s);
  if (rc == KT_OK) rc = request_sums_in_range(e, s);
  if (rc != KT_OK) return rc;
  if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: `used` is wider than int64 (kt_forecast_gangs reads int64 sums)");
  e->forecast_ready = false;
  const size_t ver = (size_t)n_gangs * (size_t)n_inst;
  if (e->d_forecast_first.cap < (size_t)n_gangs || e->d_forecast_verdicts.cap < ver + 1 || e->d_forecast_blocker.cap < ver ||
      e->d_forecast_inst_s.cap < (size_t)n_inst || e->d_forecast_inst_ns.cap < (size_t)n_inst || e->d_forecast_gang_off.cap < (size_t)n_gangs + 1) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_forecast_launch)
    if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
    KT_HIP(e, e->d_forecast_first.reserve((size_t)n_gangs));
    KT_HIP(e, e->d_forecast_verdicts.reserve(ver + 1));
    KT_HIP(e, e->d_forecast_blocker.reserve(ver));
    KT_HIP(e, e->d_forecast_inst_s.reserve((size_t)n_inst));
    KT_HIP(e, e->d_forecast_inst_ns.reserve((size_t)n_inst));
    KT_HIP(e, e->d_forecast_gang_off.reserve((size_t)n_gangs + 1));
  }
  // the instants and the offsets travel on the launch's stream, behind an earlier forecast's kernel; the caller's memory is not
  // referenced after return
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_s.p, inst_s, (size_t)n_inst * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_ns.p, inst_ns, (size_t)n_inst * 4, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  // ONE check over the members of all gangs: which throttles affect which pod, and the error rows.  The preempt result lives in
  // buffers this call does not write: it stays fetchable
  const bool preempt_was_ready = e->preempt_ready;
  rc = check_launch_locked(e, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e->check_ready = false;  // the slot holds this call's rows (as with kt_forecast_launch): a pending kt_check_launch is gone
  e->preempt_ready = preempt_was_ready;
  if (rc != KT_OK) return rc;
  // the aggregate with exact contributor counts and the error bytes; the dry finalize runs at t_0
  if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return rc;
  const kt::AdmitPage pg{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
  kt::launch_forecast_gangs(pg, n_gangs, n_inst, e->d_rows.p, e->d_forecast_gang_off.p, e->d_forecast_inst_s.p, e->d_forecast_inst_ns.p, T,
                            on_equal != 0, e->d_status.p, e->d_summary.p, e->d_preempt_partial.p, e->d_out_error.p, e->d_forecast_first.p,
                            e->d_forecast_verdicts.p, e->d_forecast_blocker.p, s);
  KT_HIP(e, hipGetLastError());
  e->last_stream = s;
  e->forecast_ready = true, e->forecast_kind = kForecastGangs, e->forecast_n = n_gangs, e->forecast_m = n_inst;
  return KT_OK;
}

int32_t kt_forecast_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_inst,
                                 const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return forecast_gangs_locked(e, n, pod_rows, n_gangs, gang_off, n_inst, inst_s, inst_ns, on_equal, stream);
}

int32_t kt_forecast_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_first, uint8_t* out_verdicts, int64_t* out_blocker) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (!e->forecast_ready || e->forecast_kind != kForecastGangs) return e->fail(KT_ERR_NOT_READY, "kt_forecast_gangs_fetch before kt_forecast_gangs_launch");
  if (n_gangs < 0 || n_gangs > e->forecast_n)
    return e->fail(KT_ERR_OUT_OF_RANGE, "n_gangs=%lld, the last forecast gangs launch had %lld gangs", (long long)n_gangs, (long long)e->forecast_n);
  if (n_gangs == 0) return KT_OK;
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  const size_t ver = (size_t)n_gangs * (size_t)e->forecast_m;
  if (out_first) KT_HIP(e, hipMemcpyAsync(out_first, e->d_forecast_first.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
  if (out_verdicts) KT_HIP(e, hipMemcpyAsync(out_verdicts, e->d_forecast_verdicts.p, ver, hipMemcpyDeviceToHost, s));
  if (out_blocker) KT_HIP(e, hipMemcpyAsync(out_blocker, e->d_forecast_blocker.p, ver * 8, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// forecast over pages: kt_forecast_launch + kt_forecast_fetch on the cluster of all names (kt_kernels_forecast_paged.hip)
// ---------------------------------------------------------------------------------------------------
int32_t kt_paged_forecast(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s,
                          const int32_t* inst_ns, int32_t on_equal, int64_t* out_first, uint8_t* out_verdicts) {
  PageLocks locks;
  int32_t rc = paged_lock("paged forecast", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if (n_inst < 1) return e0->fail(KT_ERR_INVALID_ARGUMENT, "forecast: n_inst = %lld", (long long)n_inst);
  if ((n > 0 && !pod_rows) || !inst_s || !inst_ns) return e0->fail(KT_ERR_INVALID_ARGUMENT, "forecast: pod_rows / inst_s / inst_ns missing");
  for (int64_t k = 0; k < n_inst; ++k) {
    if (inst_ns[k] < 0 || inst_ns[k] >= 1000000000) return e0->fail(KT_ERR_INVALID_ARGUMENT, "forecast: inst_ns[%lld] = %d", (long long)k, inst_ns[k]);
    if (k && !(inst_s[k - 1] < inst_s[k] || (inst_s[k - 1] == inst_s[k] && inst_ns[k - 1] < inst_ns[k])))
      return e0->fail(KT_ERR_INVALID_ARGUMENT, "forecast: the instants are not strictly ascending at position %lld", (long long)k);
  }
  if ((rc = paged_same_cluster("paged forecast", pages, n_pages, n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((double)n * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "forecast: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  if ((double)n * (double)n_inst > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "forecast: n x n_inst = %lld x %lld exceeds 2^31 verdict bytes", (long long)n, (long long)n_inst);
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "forecast: page %d: not for KT_VARIANT_INCREMENTAL engines", k);
    if (e->exchange_world > 1)
      return e->fail(KT_ERR_UNSUPPORTED, "forecast: page %d exchanges partials with %d ranks (one rank only)", k, e->exchange_world);
    if (e->wide && e->req_sums_valid)
      return e->fail(KT_ERR_UNSUPPORTED, "forecast: `used` of page %d is wider than int64 (kt_forecast_paged reads int64 sums)", k);
  }
  if (n == 0) return KT_OK;  // nothing is launched
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  if ((rc = ensure_ready(e0, s)) != KT_OK) return rc;
  // pod batches since a page's last aggregate may have pushed its sums beyond int64: found out here (the |request| sums kernel of
  // that page, where they are not known), before the check slot, a reconcile report or a result buffer of any page is touched
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = request_sums_in_range(e, s)) != KT_OK) return rc;
    if (e->wide) return e->fail(KT_ERR_UNSUPPORTED, "forecast: `used` of page %d is wider than int64 (kt_forecast_paged reads int64 sums)", k);
  }
  // ---- from here on the call owns page 0's check slot and forecast result and every page's reconcile report
  e0->forecast_ready = false, e0->forecast_kind = kForecastPods;
  if (!e0->preempt_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->preempt_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->preempt_pages_ev));  // the previous call's copy has read h_preempt_pages
  e0->h_preempt_pages.assign((size_t)n_pages, kt::PreemptPage{});
  const size_t ver = (size_t)n * (size_t)n_inst;
  if (e0->d_forecast_first.cap < (size_t)n || e0->d_forecast_verdicts.cap < ver + 1 || e0->d_forecast_inst_s.cap < (size_t)n_inst ||
      e0->d_forecast_inst_ns.cap < (size_t)n_inst) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_forecast_launch)
    if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));
    KT_HIP(e0, e0->d_forecast_first.reserve((size_t)n));
    KT_HIP(e0, e0->d_forecast_verdicts.reserve(ver + 1));
    KT_HIP(e0, e0->d_forecast_inst_s.reserve((size_t)n_inst));
    KT_HIP(e0, e0->d_forecast_inst_ns.reserve((size_t)n_inst));
  }
  KT_HIP(e0, e0->d_preempt_pages.reserve(sizeof(kt::PreemptPage) * (size_t)n_pages));
  // Everything below runs on page 0's stream.  A failure after the first launch drains that stream before it is returned, and
  // pages 1.. get their own stream back as last_stream: nothing of this call stays pending on any page.
  std::vector<hipStream_t> last((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) last[(size_t)k] = pages[k]->last_stream;
  auto finish = [&](int32_t code) -> int32_t { return paged_finish("paged forecast", pages, n_pages, s, last, code); };
  hipError_t herr = hipSuccess;
  // the instants travel on the same stream, behind an earlier forecast's kernel (the call returns behind finish: the caller's
  // memory is not referenced afterwards)
  if ((herr = hipMemcpyAsync(e0->d_forecast_inst_s.p, inst_s, (size_t)n_inst * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
      (herr = hipMemcpyAsync(e0->d_forecast_inst_ns.p, inst_ns, (size_t)n_inst * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast: %s", hipGetErrorString(herr)));
  // ONE check of page 0 over the pods: which throttles affect which pod, and the error rows.  The preempt result lives in buffers
  // this call does not write: it stays fetchable
  const bool preempt_was_ready = e0->preempt_ready;
  rc = check_launch_locked(e0, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e0->check_ready = false;  // the slot holds this call's rows (as with kt_forecast_launch): a pending kt_check_launch is gone
  e0->preempt_ready = preempt_was_ready;
  if (rc != KT_OK) return finish(rc);
  // every page: its dense aggregate beside its partial buffer and its dry finalize at t_0 (its reconcile report is dropped)
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return finish(rc);
    kt::PreemptPage& pp = e0->h_preempt_pages[(size_t)k];
    pp.pg = kt::AdmitPage{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
    pp.partial = e->d_preempt_partial.p, pp.calc = e->d_out_calc.tab(), pp.calc_updated = e->d_out_calc_updated.p, pp.error = e->d_out_error.p;
  }
  if (!kt::launch_forecast_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n, n_inst,
                                 e0->d_rows.p, e0->d_forecast_inst_s.p, e0->d_forecast_inst_ns.p, T, on_equal != 0, e0->d_status.p,
                                 e0->d_summary.p, e0->d_forecast_first.p, e0->d_forecast_verdicts.p, s, &herr))
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast: copy of the page descriptors: %s", hipGetErrorString(herr)));
  if ((herr = hipGetLastError()) != hipSuccess) return finish(e0->fail(KT_ERR_DEVICE, "paged forecast: %s", hipGetErrorString(herr)));
  e0->last_stream = s;
  if (out_first && (herr = hipMemcpyAsync(out_first, e0->d_forecast_first.p, (size_t)n * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast: %s", hipGetErrorString(herr)));
  if (out_verdicts && (herr = hipMemcpyAsync(out_verdicts, e0->d_forecast_verdicts.p, ver, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast: %s", hipGetErrorString(herr)));
  return finish(KT_OK);  // (synchronises s; the results have been handed out: no forecast result is pending on page 0)
}

// ---------------------------------------------------------------------------------------------------
// forecast for gangs over pages: kt_forecast_gangs_launch + kt_forecast_gangs_fetch on the cluster of all names
// (kt_kernels_forecast_gangs_paged.hip)
// ---------------------------------------------------------------------------------------------------
// kt_paged_forecast's scaffolding with forecast_gangs_locked's gang arguments: the instants first, then the gang defects and "a pod
// twice" asked per gang, then the page set and every page's engine.
int32_t kt_paged_forecast_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                const int64_t* gang_off, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal,
                                int64_t* out_first, uint8_t* out_verdicts, int64_t* out_blocker) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  PageLocks locks;
  int32_t rc = paged_lock("paged forecast gangs", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if (int32_t bad = forecast_instants_valid(e0, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) return bad;
  if ((rc = gangs_valid(e0, n, n_gangs, gang_off)) != KT_OK) return rc;
  {
    // gangs are judged independently: a pod may be in several of them, but not twice in one (it would reserve twice)
    std::vector<int64_t> sorted;
    for (int64_t g = 0; g < n_gangs; ++g) {
      sorted.assign(pod_rows + gang_off[g], pod_rows + gang_off[g + 1]);
      std::sort(sorted.begin(), sorted.end());
      for (size_t j = 1; j < sorted.size(); ++j)
        if (sorted[j] == sorted[j - 1])
          return e0->fail(KT_ERR_INVALID_ARGUMENT, "forecast gangs: pod row %lld is in gang %lld twice", (long long)sorted[j], (long long)g);
    }
  }
  if ((rc = paged_same_cluster("paged forecast gangs", pages, n_pages, n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((double)n * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "forecast gangs: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  if ((double)n_gangs * (double)n_inst > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "forecast gangs: n_gangs x n_inst = %lld x %lld exceeds 2^31 verdict bytes", (long long)n_gangs,
                    (long long)n_inst);
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if (e->incremental) return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: page %d: not for KT_VARIANT_INCREMENTAL engines", k);
    if (e->exchange_world > 1)
      return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: page %d exchanges partials with %d ranks (one rank only)", k, e->exchange_world);
    if (e->wide && e->req_sums_valid)
      return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: `used` of page %d is wider than int64 (kt_forecast_gangs_paged reads int64 sums)", k);
  }
  if (n == 0) return KT_OK;  // (no gangs) nothing is launched
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  if ((rc = ensure_ready(e0, s)) != KT_OK) return rc;
  // the |request| sums probe of every page where the sums are not known, before the check slot, a reconcile report or a result
  // buffer of any page is touched (as kt_paged_forecast)
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = request_sums_in_range(e, s)) != KT_OK) return rc;
    if (e->wide)
      return e->fail(KT_ERR_UNSUPPORTED, "forecast gangs: `used` of page %d is wider than int64 (kt_forecast_gangs_paged reads int64 sums)", k);
  }
  // ---- from here on the call owns page 0's check slot and forecast result and every page's reconcile report
  e0->forecast_ready = false, e0->forecast_kind = kForecastPods;
  if (!e0->preempt_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->preempt_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->preempt_pages_ev));  // the previous call's copy has read h_preempt_pages
  e0->h_preempt_pages.assign((size_t)n_pages, kt::PreemptPage{});
  const size_t ver = (size_t)n_gangs * (size_t)n_inst;
  if (e0->d_forecast_first.cap < (size_t)n_gangs || e0->d_forecast_verdicts.cap < ver + 1 || e0->d_forecast_blocker.cap < ver ||
      e0->d_forecast_inst_s.cap < (size_t)n_inst || e0->d_forecast_inst_ns.cap < (size_t)n_inst ||
      e0->d_forecast_gang_off.cap < (size_t)n_gangs + 1) {
    // a launch that was never fetched may still be using the old buffers, on the stream it was given (as kt_forecast_gangs_launch)
    if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));
    KT_HIP(e0, e0->d_forecast_first.reserve((size_t)n_gangs));
    KT_HIP(e0, e0->d_forecast_verdicts.reserve(ver + 1));
    KT_HIP(e0, e0->d_forecast_blocker.reserve(ver));
    KT_HIP(e0, e0->d_forecast_inst_s.reserve((size_t)n_inst));
    KT_HIP(e0, e0->d_forecast_inst_ns.reserve((size_t)n_inst));
    KT_HIP(e0, e0->d_forecast_gang_off.reserve((size_t)n_gangs + 1));
  }
  KT_HIP(e0, e0->d_preempt_pages.reserve(sizeof(kt::PreemptPage) * (size_t)n_pages));
  // Everything below runs on page 0's stream.  A failure after the first launch drains that stream before it is returned, and
  // pages 1.. get their own stream back as last_stream: nothing of this call stays pending on any page.
  std::vector<hipStream_t> last((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) last[(size_t)k] = pages[k]->last_stream;
  auto finish = [&](int32_t code) -> int32_t { return paged_finish("paged forecast gangs", pages, n_pages, s, last, code); };
  hipError_t herr = hipSuccess;
  // the instants and the offsets travel on the same stream, behind an earlier forecast's kernel (the call returns behind finish:
  // the caller's memory is not referenced afterwards)
  if ((herr = hipMemcpyAsync(e0->d_forecast_inst_s.p, inst_s, (size_t)n_inst * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
      (herr = hipMemcpyAsync(e0->d_forecast_inst_ns.p, inst_ns, (size_t)n_inst * 4, hipMemcpyHostToDevice, s)) != hipSuccess ||
      (herr = hipMemcpyAsync(e0->d_forecast_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast gangs: %s", hipGetErrorString(herr)));
  // ONE check of page 0 over the members of all gangs: which throttles affect which pod, and the error rows.  The preempt result
  // lives in buffers this call does not write: it stays fetchable
  const bool preempt_was_ready = e0->preempt_ready;
  rc = check_launch_locked(e0, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e0->check_ready = false;  // the slot holds this call's rows (as with kt_paged_forecast): a pending kt_check_launch is gone
  e0->preempt_ready = preempt_was_ready;
  if (rc != KT_OK) return finish(rc);
  // every page: its dense aggregate beside its partial buffer and its dry finalize at t_0 (its reconcile report is dropped)
  for (int32_t k = 0; k < n_pages; ++k) {
    kt_engine* e = pages[k];
    if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return finish(rc);
    kt::PreemptPage& pp = e0->h_preempt_pages[(size_t)k];
    pp.pg = kt::AdmitPage{e->pods.flags, e->pods.req, e->tt, e->D, e->pods.DS, 0u, 0u, 0u};
    pp.partial = e->d_preempt_partial.p, pp.calc = e->d_out_calc.tab(), pp.calc_updated = e->d_out_calc_updated.p, pp.error = e->d_out_error.p;
  }
  if (!kt::launch_forecast_gangs_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n_gangs,
                                       n_inst, e0->d_rows.p, e0->d_forecast_gang_off.p, e0->d_forecast_inst_s.p, e0->d_forecast_inst_ns.p, T,
                                       on_equal != 0, e0->d_status.p, e0->d_summary.p, e0->d_forecast_first.p, e0->d_forecast_verdicts.p,
                                       e0->d_forecast_blocker.p, s, &herr))
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast gangs: copy of the page descriptors: %s", hipGetErrorString(herr)));
  if ((herr = hipGetLastError()) != hipSuccess) return finish(e0->fail(KT_ERR_DEVICE, "paged forecast gangs: %s", hipGetErrorString(herr)));
  e0->last_stream = s;
  if (out_first && (herr = hipMemcpyAsync(out_first, e0->d_forecast_first.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast gangs: %s", hipGetErrorString(herr)));
  if (out_verdicts && (herr = hipMemcpyAsync(out_verdicts, e0->d_forecast_verdicts.p, ver, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast gangs: %s", hipGetErrorString(herr)));
  if (out_blocker && (herr = hipMemcpyAsync(out_blocker, e0->d_forecast_blocker.p, ver * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return finish(e0->fail(KT_ERR_DEVICE, "paged forecast gangs: %s", hipGetErrorString(herr)));
  return finish(KT_OK);  // (synchronises s; the results have been handed out: no forecast result of either kind is pending on page 0)
}

// Host-only: the instants in (from, until] at which some valid and responsible throttle's CalculateThreshold can change — every
// parsed non-zero begin, and end + 1 ns for every parsed non-zero end: the first instant at which IsActive is false (at `end`
// itself, the instant NextOverrideHappensIn reports, the override is still active)
int32_t kt_override_instants(kt_engine* e, int64_t from_s, int32_t from_ns, int64_t until_s, int32_t until_ns, int64_t cap, int64_t* out_s,
                             int32_t* out_ns, int64_t* out_total) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  if (cap < 0 || (cap > 0 && (!out_s || !out_ns)) || !out_total) return e->fail(KT_ERR_INVALID_ARGUMENT, "override_instants: cap = %lld, arrays missing", (long long)cap);
  typedef std::pair<int64_t, int32_t> Inst;
  const Inst from(from_s, from_ns), until(until_s, until_ns);
  std::vector<Inst> v;
  auto add = [&](int64_t s_, int32_t ns_) {
    const Inst t(s_, ns_);
    if (from < t && !(until < t)) v.push_back(t);
  };
  const uint32_t need = KT_THR_VALID | KT_THR_RESPONSIBLE;
  for (int32_t t = 0; t < e->thr_rows_hi; ++t) {
    const HostThrottle& h = e->thr[(size_t)t];
    if ((h.flags & need) != need) continue;
    for (const Override& ov : h.ovr) {
      if (ov.flags & kt::kOvrParseError) continue;
      if (!(ov.begin_s == kt::kZeroTimeS && ov.begin_ns == 0)) add(ov.begin_s, ov.begin_ns);
      if (!(ov.end_s == kt::kZeroTimeS && ov.end_ns == 0)) {
        if (ov.end_ns == 999999999) add(ov.end_s + 1, 0);
        else add(ov.end_s, ov.end_ns + 1);
      }
    }
  }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  *out_total = (int64_t)v.size();
  const int64_t w = std::min<int64_t>((int64_t)v.size(), cap);
  for (int64_t k = 0; k < w; ++k) out_s[k] = v[(size_t)k].first, out_ns[k] = v[(size_t)k].second;
  return KT_OK;
}

int32_t kt_paged_reconcile(kt_engine* const* pages, int32_t n_pages, int64_t now_s, int32_t now_ns, uint32_t flags, int32_t n,
                           const kt_status* page_out, uint8_t* replaced_any, uint8_t* error_any) {
  if (!pages || n_pages < 1 || n < 0 || !page_out) return KT_ERR_INVALID_ARGUMENT;
  for (int32_t k = 0; k < n_pages; ++k)
    if (!pages[k]) return KT_ERR_INVALID_ARGUMENT;
  // With APPLY a page that has reconciled holds the NEW status; a failure on a later page must not leave the pages disagreeing
  // about calculatedThreshold / throttled without the caller knowing which did what.  So: every page is first
  // reconciled WITHOUT apply (a dry run that can fail — LDS budgets, sums out of range — on any page before anything is stored),
  // and only when all succeeded is the step run again with the caller's flags; a failure in that second pass (device errors only:
  // the same launches just succeeded) still drains every launched page's result and is reported after the last page.
  int32_t rc;
  if (flags & KT_RECONCILE_APPLY)
    for (int32_t k = 0; k < n_pages; ++k)
      if ((rc = kt_reconcile_launch(pages[k], now_s, now_ns, flags & ~KT_RECONCILE_APPLY, nullptr)) != KT_OK) return rc;
  int32_t launched = 0, first_err = KT_OK;
  for (; launched < n_pages; ++launched)  // (enqueued on every page's own stream: the pages run side by side on the device)
    if ((rc = kt_reconcile_launch(pages[launched], now_s, now_ns, flags, nullptr)) != KT_OK) { first_err = rc; break; }
  if (replaced_any) memset(replaced_any, 0, (size_t)n);
  if (error_any) memset(error_any, 0, (size_t)n);
  for (int32_t k = 0; k < launched; ++k) {
    if ((rc = kt_reconcile_fetch(pages[k], n, &page_out[k])) != KT_OK) {
      if (first_err == KT_OK) first_err = rc;
      continue;
    }
    for (int32_t i = 0; i < n; ++i) {
      if (replaced_any && page_out[k].calc_at_nonzero) replaced_any[i] |= page_out[k].calc_at_nonzero[i] != 0;
      if (error_any && page_out[k].error) error_any[i] |= page_out[k].error[i] != 0;
    }
  }
  return first_err;
}

