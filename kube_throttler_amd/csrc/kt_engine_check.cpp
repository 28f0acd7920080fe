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
int32_t check_launch_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags, hipStream_t s, bool allow_small) {
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
// Elastic gangs (min_members set, member_flags nullable; validated by the caller: elastic_valid): page 0 keeps the quorums, the flag
// bytes and the kept members per gang beside them (kt_admit_gangs_elastic_fetch).
static int32_t admit_locked(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, uint32_t flags,
                            hipStream_t s, int64_t n_gangs = -1, const int64_t* gang_off = nullptr, const int64_t* min_members = nullptr,
                            const uint8_t* member_flags = nullptr) {
  kt_engine* e0 = pages[0];
  const int32_t T = e0->thr_rows_hi;
  const bool gangs = n_gangs >= 0;
  const bool elastic = gangs && min_members != nullptr;
  e0->gang_ready = false;
  e0->gang_elastic = false;
  for (int32_t k = 0; k < n_pages; ++k)
    if (pages[k]->wide)
      return pages[k]->fail(KT_ERR_UNSUPPORTED, "admit queue: the stored `used` of page %d is wider than int64 (kt_admit reads int64 tables)", k);
  if ((double)n * (double)T > 2147483648.0)
    return e0->fail(KT_ERR_OUT_OF_RANGE, "admit queue: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", (long long)n, T);
  // (a) who affects whom, for the whole queue in parallel, from page 0 (selectors, namespaces and responsibility are the same
  //     in every page; statuses against the current reserved amounts)
  if (gangs && n_gangs > 0) {
    // the offsets go up in front of the check launch: the caller's memory is not referenced after return
    const bool grow_elastic = elastic && (e0->d_gang_min.cap < (size_t)n_gangs || e0->d_gang_members.cap < (size_t)n_gangs ||
                                          (member_flags && e0->d_gang_flags.cap < (size_t)n));
    if (e0->d_gang_off.cap < (size_t)n_gangs + 1 || e0->d_gang_out.cap < (size_t)n_gangs || grow_elastic) {
      if (e0->last_stream) KT_HIP(e0, hipStreamSynchronize(e0->last_stream));  // the buffers may still be in use
      KT_HIP(e0, e0->d_gang_off.reserve((size_t)n_gangs + 1));
      KT_HIP(e0, e0->d_gang_out.reserve((size_t)n_gangs));
      if (elastic) {
        KT_HIP(e0, e0->d_gang_min.reserve((size_t)n_gangs));
        KT_HIP(e0, e0->d_gang_members.reserve((size_t)n_gangs));
        if (member_flags) KT_HIP(e0, e0->d_gang_flags.reserve((size_t)n));
      }
    }
    KT_HIP(e0, hipMemcpyAsync(e0->d_gang_off.p, gang_off, ((size_t)n_gangs + 1) * 8, hipMemcpyHostToDevice, s));
    if (elastic) {
      KT_HIP(e0, hipMemcpyAsync(e0->d_gang_min.p, min_members, (size_t)n_gangs * 8, hipMemcpyHostToDevice, s));
      if (member_flags) KT_HIP(e0, hipMemcpyAsync(e0->d_gang_flags.p, member_flags, (size_t)n, hipMemcpyHostToDevice, s));
    }
    KT_HIP(e0, hipStreamSynchronize(s));
    e0->h_gang_off.assign(gang_off, gang_off + n_gangs + 1);
    if (elastic) {
      e0->h_gang_min.assign(min_members, min_members + n_gangs);
      if (member_flags) e0->h_gang_flags.assign(member_flags, member_flags + n);
      else e0->h_gang_flags.clear();
    }
  }
  int32_t rc = check_launch_locked(e0, n, pod_rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  if (rc == KT_OK && gangs) e0->gang_ready = true, e0->gang_n = n_gangs, e0->gang_on_device = n > 0 && T > 0, e0->gang_elastic = elastic;
  if (rc != KT_OK || n == 0 || T == 0) return rc;  // (no throttle rows: a gang is admitted iff no member's PreFilter is an error)
  // (b) the queue in order, one wave, every page's reserved amounts side by side in LDS
  if (!e0->admit_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->admit_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->admit_pages_ev));  // the previous launch's copy has read h_admit_pages
  e0->h_admit_pages.resize((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) e0->h_admit_pages[(size_t)k] = admit_page_of(pages[k]);
  const bool commit = (flags & KT_ADMIT_COMMIT) != 0;
  KT_HIP(e0, e0->d_admit.reserve(kt::admit_paged_state_bytes(T, e0->h_admit_pages.data(), n_pages) + (gangs ? kt::admit_gang_extra_bytes(T, n_pages) : 0) + 64));
  KT_HIP(e0, e0->d_admit_pages.reserve(sizeof(kt::AdmitPage) * (size_t)n_pages));
  static const bool force_global = getenv("KT_ADMIT_FORCE_GLOBAL") != nullptr;  // test hook: HBM-resident state
  hipError_t herr = hipSuccess;
  kt::AdmitGangs ga{e0->d_gang_off.p, n_gangs, e0->d_gang_out.p};
  if (elastic) ga.min_dev = e0->d_gang_min.p, ga.flags_dev = member_flags ? e0->d_gang_flags.p : nullptr, ga.members_dev = e0->d_gang_members.p;
  const bool launched = kt::launch_admit(e0->h_admit_pages.data(), n_pages, (kt::AdmitPage*)e0->d_admit_pages.p, e0->admit_pages_ev, n,
                                         pod_rows ? e0->d_rows.p : nullptr, T, on_equal != 0, commit, e0->d_status.p, e0->d_summary.p,
                                         e0->d_admit.p, force_global, s, &herr, gangs ? &ga : nullptr);
  if (herr != hipSuccess || !launched) e0->gang_ready = false, e0->gang_elastic = false;
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
int32_t gangs_valid(kt_engine* e, int64_t n, int64_t n_gangs, const int64_t* gang_off) {
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

// the gang bytes of the last gang launch, under the launch lock; out nullable.  out_members (nullable): the kept members per gang of
// an elastic launch, beside the bytes
static int32_t gangs_fetch_locked(kt_engine* e, int64_t n_gangs, uint8_t* out, int64_t* out_members = nullptr) {
  if (!e->gang_ready) return e->fail(KT_ERR_NOT_READY, "kt_admit_gangs_fetch before kt_admit_gangs_launch");
  if (n_gangs < 0 || n_gangs > e->gang_n)
    return e->fail(KT_ERR_OUT_OF_RANGE, "n_gangs=%lld, the last gang launch had %lld gangs", (long long)n_gangs, (long long)e->gang_n);
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  if (e->gang_on_device) {
    if (n_gangs && out) KT_HIP(e, hipMemcpyAsync(out, e->d_gang_out.p, (size_t)n_gangs, hipMemcpyDeviceToHost, s));
    if (n_gangs && out_members) KT_HIP(e, hipMemcpyAsync(out_members, e->d_gang_members.p, (size_t)n_gangs * 8, hipMemcpyDeviceToHost, s));
    KT_HIP(e, hipStreamSynchronize(s));
    return KT_OK;
  }
  // no throttle rows: nothing was reserved; a gang is admitted iff every member's PreFilter answered Success — an elastic one iff
  // its quorum of members and every required one did
  std::vector<uint64_t> sm((size_t)e->check_n + 1);
  if (e->check_n) KT_HIP(e, hipMemcpyAsync(sm.data(), e->d_summary.p, (size_t)e->check_n * 8, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  for (int64_t g = 0; g < n_gangs && (out || out_members); ++g) {
    bool all = true, required_out = false;
    int64_t n_in = 0;
    for (int64_t i = e->h_gang_off[(size_t)g]; i < e->h_gang_off[(size_t)g + 1]; ++i) {
      const bool ok = sm[(size_t)i] == 0;
      all &= ok, n_in += ok ? 1 : 0;
      if (!ok && e->gang_elastic && !e->h_gang_flags.empty() && (e->h_gang_flags[(size_t)i] & KT_GANG_MEMBER_REQUIRED)) required_out = true;
    }
    const bool kept = e->gang_elastic ? n_in >= e->h_gang_min[(size_t)g] && !required_out : all;
    if (out) out[g] = kept ? 1 : 0;
    if (out_members) out_members[g] = kept ? n_in : 0;
  }
  return KT_OK;
}

// what the elastic gang calls refuse behind gangs_valid: a missing quorum array, a quorum outside [1, size of the gang], a flag byte
// with a bit other than KT_GANG_MEMBER_REQUIRED (the wording names the admission, as gangs_valid's does, for every caller)
int32_t elastic_valid(kt_engine* e, int64_t n, int64_t n_gangs, const int64_t* gang_off, const int64_t* min_members, const uint8_t* member_flags) {
  if (n_gangs > 0 && !min_members) return e->fail(KT_ERR_INVALID_ARGUMENT, "admit elastic gangs: min_members is NULL");
  for (int64_t g = 0; g < n_gangs; ++g) {
    const int64_t size = gang_off[g + 1] - gang_off[g];
    if (min_members[g] < 1 || min_members[g] > size)
      return e->fail(KT_ERR_INVALID_ARGUMENT, "admit elastic gangs: min_members[%lld] = %lld of gang %lld is outside [1, %lld], the gang's size",
                     (long long)g, (long long)min_members[g], (long long)g, (long long)size);
  }
  for (int64_t i = 0; member_flags && i < n; ++i)
    if (member_flags[i] & ~(uint8_t)KT_GANG_MEMBER_REQUIRED)
      return e->fail(KT_ERR_INVALID_ARGUMENT, "admit elastic gangs: member_flags[%lld] = 0x%02x at queue position %lld has a bit other than KT_GANG_MEMBER_REQUIRED",
                     (long long)i, (unsigned)member_flags[i], (long long)i);
  return KT_OK;
}

int32_t kt_admit_gangs_elastic_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                      const int64_t* min_members, const uint8_t* member_flags, int32_t on_equal, uint32_t flags, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  int32_t rc = gangs_valid(e, n, n_gangs, gang_off);
  if (rc == KT_OK) rc = elastic_valid(e, n, n_gangs, gang_off, min_members, member_flags);
  if (rc != KT_OK) return rc;
  KT_HIP(e, hipSetDevice(e->device));
  static const int64_t no_quorum = 0;  // (n_gangs == 0: the elastic form with nothing to read)
  return admit_locked(&e, 1, n, pod_rows, on_equal, flags, pick_stream(e, stream), n_gangs, gang_off, min_members ? min_members : &no_quorum, member_flags);
}

int32_t kt_admit_gangs_elastic_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_members) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (e->gang_ready && !e->gang_elastic)
    return e->fail(KT_ERR_NOT_READY, "kt_admit_gangs_elastic_fetch: the pending gang launch is kt_admit_gangs_launch, which keeps no counts");
  return gangs_fetch_locked(e, n_gangs, nullptr, out_members);
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

// What the calls over several page engines share (kt_paged_admit, kt_paged_admit_gangs and the paged queries of
// kt_engine_queries.cpp; `what` words the errors).
// paged_lock: every page exclusively, in address order — two paged calls over overlapping pages cannot deadlock
int32_t paged_lock(const char* what, kt_engine* const* pages, int32_t n_pages, int64_t n, PageLocks& locks) {
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
int32_t paged_same_cluster(const char* what, kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows) {
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
int32_t paged_order(kt_engine* const* pages, int32_t n_pages, hipStream_t* s) {
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
                           uint64_t* out_summary, uint8_t* out_status, int64_t n_gangs, const int64_t* gang_off, uint8_t* out_gang_admitted,
                           bool elastic = false, const int64_t* min_members = nullptr, const uint8_t* member_flags = nullptr,
                           int64_t* out_members = nullptr) {
  PageLocks locks;
  int32_t rc = paged_lock("paged admit", pages, n_pages, n, locks);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = pages[0];
  const int32_t T = e0->thr_rows_hi;
  if (n_gangs >= 0) {
    int32_t rcg = gangs_valid(e0, n, n_gangs, gang_off);
    if (rcg == KT_OK && elastic) rcg = elastic_valid(e0, n, n_gangs, gang_off, min_members, member_flags);
    if (rcg != KT_OK) return rcg;
  }
  if ((rc = paged_same_cluster("paged admit", pages, n_pages, n, pod_rows)) != KT_OK) return rc;
  if (n == 0) return KT_OK;
  hipStream_t s = nullptr;
  if ((rc = paged_order(pages, n_pages, &s)) != KT_OK) return rc;
  rc = admit_locked(pages, n_pages, n, pod_rows, on_equal, flags, s, n_gangs, gang_off, elastic ? min_members : nullptr, member_flags);
  e0->check_ready = false;  // the call used page 0's check slot (as kt_affected_pods): a pending kt_check_launch is gone
  if (rc != KT_OK) return rc;
  if (out_summary) KT_HIP(e0, hipMemcpyAsync(out_summary, e0->d_summary.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (out_status && T > 0) KT_HIP(e0, hipMemcpyAsync(out_status, e0->d_status.p, (size_t)n * (size_t)T, hipMemcpyDeviceToHost, s));
  if (n_gangs >= 0) {
    rc = gangs_fetch_locked(e0, n_gangs, out_gang_admitted, elastic ? out_members : nullptr);  // (synchronises s)
    e0->gang_ready = false, e0->gang_elastic = false;  // the results have been handed out
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

int32_t kt_paged_admit_gangs_elastic(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                     const int64_t* gang_off, const int64_t* min_members, const uint8_t* member_flags, int32_t on_equal, uint32_t flags,
                                     uint64_t* out_summary, uint8_t* out_status, int64_t* out_members) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  return paged_admit(pages, n_pages, n, pod_rows, on_equal, flags, out_summary, out_status, n_gangs, gang_off, nullptr, /*elastic=*/true, min_members,
                     member_flags, out_members);
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

