// kt_engine_views.cpp — the scan views (ScanView, kt_engine_impl.h): the builder of both and the pod events applied to them in place.
#include "kt_engine_impl.h"

// ---- build, step 1: which rows, in which order, and the record ranges of the scan's workgroups.  Leaves v.n on the host:
// the countable view's headroom and pack plan follow from it (aggregate_locked decides them between the steps).
int32_t list_view_rows(kt_engine* e, ScanView& v, const ViewSpec& spec, hipStream_t s) {
  ScanViews& vs = e->views;
  const uint32_t n_ns = (uint32_t)e->sp.n_ns;
  e->ctr_view_builds.fetch_add(1, std::memory_order_relaxed);
  v.valid = false;
  v.by_ns = spec.by_ns;
  KT_HIP(e, v.rows.reserve((size_t)spec.rows_cap + 1));
  KT_HIP(e, v.d_n.reserve(1));
  if (spec.by_ns) {
    KT_HIP(e, vs.d_ns_cursor.reserve((size_t)n_ns + 1));
    kt::launch_order_rows_by_ns(e->pods, e->pod_rows_hi, spec.countable_only, n_ns, vs.d_ns_cursor.p, v.rows.p, v.d_n.p, s);
  } else {  // (ascending rows: the countable pods only — a scan of every row in row order needs no list)
    KT_HIP(e, hipMemsetAsync(v.d_n.p, 0, 8, s));
    kt::launch_compact_countable(e->pods, e->pod_rows_hi, v.rows.p, v.d_n.p, s);
  }
  KT_HIP(e, hipGetLastError());
  // The ranges are planned on the host from a copy of the namespace ends, which travels with the row count (known without
  // asking when every row is listed): a view build is not a per-step cost, and one GPU thread took 388 us for the plan.
  const bool plan_ranges = spec.by_ns && !e->sw[kSw_NO_WG_RANGES];
  if (spec.countable_only) KT_HIP(e, hipMemcpyAsync(&v.n, v.d_n.p, 8, hipMemcpyDeviceToHost, s));
  else v.n = (unsigned long long)e->pod_rows_hi;
  if (plan_ranges) {
    vs.h_ns_end.resize((size_t)n_ns + 1);
    KT_HIP(e, hipMemcpyAsync(vs.h_ns_end.data(), vs.d_ns_cursor.p, (size_t)n_ns * 8, hipMemcpyDeviceToHost, s));
  }
  if (spec.countable_only || plan_ranges) KT_HIP(e, hipStreamSynchronize(s));
  v.range_G = 0;
  if (plan_ranges && v.n > 0) {
    v.range_G = spec.grid((int64_t)v.n);
    KT_HIP(e, v.range.reserve((size_t)v.range_G + 2));
    vs.h_range.resize((size_t)v.range_G + 2);
    kt::plan_wg_ranges(vs.h_ns_end.data(), n_ns, (int64_t)v.n, v.range_G, vs.h_range.data());
    KT_HIP(e, hipMemcpyAsync(v.range.p, vs.h_range.data(), vs.h_range.size() * 4, hipMemcpyHostToDevice, s));
    KT_HIP(e, hipStreamSynchronize(s));  // (1 KB; h_range is reused)
  }
  return KT_OK;
}

// ---- build, step 2: scan-ordered copies of the listed pods' records (the scan streams them instead of gathering through the
// list), `headroom` free records behind them, and the row -> record table.  Requests are copied packed when v.pack says so.
int32_t copy_view_records(kt_engine* e, ScanView& v, const ViewSpec& spec, int64_t headroom, hipStream_t s) {
  ScanViews& vs = e->views;
  v.cap = (int64_t)v.n + headroom;
  v.extra = 0;
  v.mx_valid = false;  // (the aggregate gathers the planes of the new records where it will replay them: aggregate_locked)
  const size_t nc = (size_t)v.cap + 1, np = (size_t)spec.rows_cap + 1;
  KT_HIP(e, v.meta.reserve(nc));
  KT_HIP(e, v.latom.reserve(nc * (size_t)e->pods.LA));
  if (spec.requests) KT_HIP(e, v.pack.nw ? v.pk.reserve(nc * (size_t)v.pack.stride) : v.req.reserve(nc * (size_t)e->pods.DS));
  KT_HIP(e, v.pos.reserve(np));
  KT_HIP(e, vs.d_dirty.reserve(4));
  KT_HIP(e, hipMemsetAsync(v.pos.p, 0xFF, np * 4, s));
  if (spec.countable_only) {  // the records past the listed ones are "no pod" until something is appended there
    KT_HIP(e, hipMemsetAsync(v.meta.p + v.n, 0, (size_t)(headroom + 1) * 8, s));
    KT_HIP(e, hipMemsetAsync(v.rows.p + v.n, 0, (size_t)(headroom + 1) * 8, s));
  }
  if (!vs.check_dirty) KT_HIP(e, hipMemsetAsync(vs.d_dirty.p, 0, 4, s));
  kt::launch_build_scan_view(e->pods, (int64_t)v.n, v.rows.p, v.meta.p, v.latom.p, spec.requests && !v.pack.nw ? v.req.p : nullptr, s,
                             v.pack.nw ? &v.pack : nullptr, v.pk.p, v.pos.p);
  KT_HIP(e, hipGetLastError());
  return KT_OK;
}

// ---- pod events applied to the views in place
// can a batch of n pod rows (largest |request| per dimension batch_max, OR of the values batch_or, a negative value seen)
// be applied to the current views?  The packed request words only hold what their plan was proved for.
bool views_patchable(const kt_engine* e, int64_t n, const unsigned __int128* batch_max, const uint64_t* batch_or, bool batch_neg) {
  const ScanView& c = e->views.countable;
  if (e->incremental || e->cfg.kernel_variant != 0 || e->program_dirty || n > kPatchBatchMax) return false;
  if (!c.valid && !e->views.all_rows.valid) return false;  // nothing to patch: the next scan builds anyway
  if (e->sw[kSw_NO_VIEW_PATCH]) return false;
  if (c.valid) {
    if (c.meta.p == nullptr || c.pos.p == nullptr) return false;
    if (c.extra + n > c.cap - (int64_t)c.n) return false;
    if (c.pack.nw) {
      if (batch_neg) return false;
      for (int d = 0; d < e->D; ++d) {
        if (batch_max[d] > e->max_abs[d]) return false;  // a field may be too narrow
        if (c.pack.shift[d] && (batch_or[d] & ((1ull << c.pack.shift[d]) - 1ull))) return false;  // fewer common trailing zeros
      }
    }
    // (an unpacked view of an engine that could pack stays: a rebuild decides again)
  }
  return true;
}
// the views a pod event batch of n rows has to be applied to (host bookkeeping included: call once per batch)
kt::ViewPatch view_patch_of(kt_engine* e, int64_t n) {
  ScanView& c = e->views.countable;
  const ScanView& a = e->views.all_rows;
  kt::ViewPatch v{};
  if (c.valid) {
    v.vc_meta = c.meta.p, v.vc_latom = c.latom.p, v.vc_req = c.pack.nw ? nullptr : c.req.p, v.vc_pk = c.pack.nw ? c.pk.p : nullptr;
    v.vc_rows = c.rows.p, v.pos_c = c.pos.p, v.n_c = c.d_n.p, v.cap_c = c.cap;
    v.by_ns = c.by_ns ? 1u : 0u;
    v.pk = c.pack;
    if (!c.by_ns) c.extra += n;  // at most n appended
  }
  if (a.valid) v.va_meta = a.meta.p, v.va_latom = a.latom.p, v.pos_a = a.pos.p, v.rows_a = (int64_t)a.n;
  v.dirty = e->views.d_dirty.p;
  if ((c.valid && c.by_ns) || a.valid) e->views.check_dirty = true;
  return v;
}
int32_t patch_views(kt_engine* e, int64_t n, const int64_t* rows_dev, int64_t row0, hipStream_t s) {
  const kt::ViewPatch v = view_patch_of(e, n);
  kt::launch_patch_scan_views(e->pods, n, rows_dev, row0, v, s);
  KT_HIP(e, hipGetLastError());
  return KT_OK;
}
// before a scan uses a namespace-ordered view that was patched: did an entry have to move?
int32_t settle_view_patches(kt_engine* e, hipStream_t s) {
  ScanViews& vs = e->views;
  if (!vs.check_dirty) return KT_OK;
  uint32_t dirty = 0;
  KT_HIP(e, hipMemcpyAsync(&dirty, vs.d_dirty.p, 4, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  if (dirty) {
    vs.invalidate();
    KT_HIP(e, hipMemsetAsync(vs.d_dirty.p, 0, 4, s));
  }
  vs.check_dirty = false;
  return KT_OK;
}
