// kt_engine_queries.cpp — the admission queries behind the C-ABI: headroom, preempt (with reprieve), forecast and headroom forecast,
// their gang forms and their paged forms for more than 16 resource names, and kt_override_instants.  Every query is one
// status-matrix check of its rows (check_launch_locked, kt_engine_check.cpp) and one kernel behind it; the steps they share are the
// helpers below, and every entry point calls them in its own order — the order of its refusals is part of its contract.
#include "kt_engine_impl.h"

namespace {  // (the helpers' types too stay out of the library's symbol table)

// ---------------------------------------------------------------------------------------------------
// refusals: `what` words the message; page >= 0: the wording of a paged call about that page, recorded on that page's engine.
// A refusal comes before any state change of the call: no ready flag, no page descriptor, no buffer, no check slot.
// ---------------------------------------------------------------------------------------------------
static int32_t rows_in_range(kt_engine* e, const char* what, int64_t n, const int64_t* rows) {
  for (int64_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= e->cfg.pod_capacity) return e->fail(KT_ERR_OUT_OF_RANGE, "%s: pod row %lld", what, (long long)rows[i]);
  return KT_OK;
}

// gangs are judged independently: a pod may be in several of them, but not twice in one (it would reserve twice)
static int32_t no_row_twice_in_a_gang(kt_engine* e, const char* what, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off) {
  std::vector<int64_t> sorted;
  for (int64_t g = 0; g < n_gangs; ++g) {
    sorted.assign(pod_rows + gang_off[g], pod_rows + gang_off[g + 1]);
    std::sort(sorted.begin(), sorted.end());
    for (size_t j = 1; j < sorted.size(); ++j)
      if (sorted[j] == sorted[j - 1])
        return e->fail(KT_ERR_INVALID_ARGUMENT, "%s: pod row %lld is in gang %lld twice", what, (long long)sorted[j], (long long)g);
  }
  return KT_OK;
}

static int32_t preempt_arrays_present(kt_engine* e, const char* what, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows) {
  if (n_cand < 0) return e->fail(KT_ERR_INVALID_ARGUMENT, "%s: n_cand = %lld", what, (long long)n_cand);
  if ((n > 0 && !pod_rows) || (n_cand > 0 && !cand_rows)) return e->fail(KT_ERR_INVALID_ARGUMENT, "%s: pod_rows / cand_rows missing", what);
  return KT_OK;
}

// no candidate twice, and none that is also a preemptor (gangs: a member)
static int32_t candidates_distinct_from_preemptors(kt_engine* e, const char* what, int64_t n, const int64_t* pod_rows, int64_t n_cand,
                                                   const int64_t* cand_rows, bool gangs) {
  std::vector<int64_t> sorted(cand_rows, cand_rows + n_cand);
  std::sort(sorted.begin(), sorted.end());
  for (int64_t j = 1; j < n_cand; ++j)
    if (sorted[(size_t)j] == sorted[(size_t)j - 1])
      return e->fail(KT_ERR_INVALID_ARGUMENT, "%s: pod row %lld is a candidate twice", what, (long long)sorted[(size_t)j]);
  for (int64_t i = 0; i < n; ++i)
    if (std::binary_search(sorted.begin(), sorted.end(), pod_rows[i]))
      return e->fail(KT_ERR_INVALID_ARGUMENT, gangs ? "%s: pod row %lld is a member and a candidate" : "%s: pod row %lld is a preemptor and a candidate",
                     what, (long long)pod_rows[i]);
  return KT_OK;
}

// the status matrix of the call's one check holds n x throttle_rows bytes; with candidates (n_cand >= 0) (n + n_cand) x throttle_rows
static int32_t matrix_fits(kt_engine* e, const char* what, int32_t T, int64_t n, int64_t n_cand = -1) {
  const double lim = 2147483648.0;
  if (n_cand < 0) {
    if ((double)n * (double)T > lim) return e->fail(KT_ERR_OUT_OF_RANGE, "%s: n x throttle_rows = %lld x %d exceeds 2^31 matrix bytes", what, (long long)n, T);
  } else if ((double)n * (double)T > lim || (double)n_cand * (double)T > lim || ((double)n + (double)n_cand) * (double)T > lim) {
    return e->fail(KT_ERR_OUT_OF_RANGE, "%s: (n + n_cand) x throttle_rows = (%lld + %lld) x %d exceeds 2^31 matrix bytes", what, (long long)n,
                   (long long)n_cand, T);
  }
  return KT_OK;
}

// one result per (pod or gang, instant)
static int32_t verdicts_fit(kt_engine* e, const char* what, int64_t n, int64_t n_inst, const char* n_name = "n", const char* unit = "verdict bytes") {
  if ((double)n * (double)n_inst > 2147483648.0)
    return e->fail(KT_ERR_OUT_OF_RANGE, "%s: %s x n_inst = %lld x %lld exceeds 2^31 %s", what, n_name, (long long)n, (long long)n_inst, unit);
  return KT_OK;
}

static int32_t used_is_wide(kt_engine* e, const char* what, int page, const char* kernel) {
  if (page < 0) return e->fail(KT_ERR_UNSUPPORTED, "%s: `used` is wider than int64 (%s reads int64 sums)", what, kernel);
  return e->fail(KT_ERR_UNSUPPORTED, "%s: `used` of page %d is wider than int64 (%s reads int64 sums)", what, page, kernel);
}

// the queries that reconcile dryly (preempt_reconcile_locked): a rescanning engine of one rank whose sums are known to fit int64
static int32_t serves_dry_reconcile(kt_engine* e, const char* what, int page, const char* kernel) {
  if (e->incremental)
    return page < 0 ? e->fail(KT_ERR_UNSUPPORTED, "%s: not for KT_VARIANT_INCREMENTAL engines", what)
                    : e->fail(KT_ERR_UNSUPPORTED, "%s: page %d: not for KT_VARIANT_INCREMENTAL engines", what, page);
  if (e->exchange_world > 1)
    return page < 0 ? e->fail(KT_ERR_UNSUPPORTED, "%s: the engine exchanges partials with %d ranks (one rank only)", what, e->exchange_world)
                    : e->fail(KT_ERR_UNSUPPORTED, "%s: page %d exchanges partials with %d ranks (one rank only)", what, page, e->exchange_world);
  if (e->wide && e->req_sums_valid) return used_is_wide(e, what, page, kernel);
  return KT_OK;
}

// Pod batches since the last aggregate may have pushed the sums beyond int64: found out here (the |request| sums kernel, where they
// are not known).  With ensure_ready the one thing that runs before the last refusal of a call.
static int32_t sums_fit_int64(kt_engine* e, const char* what, int page, const char* kernel, hipStream_t s) {
  int32_t rc = request_sums_in_range(e, s);
  if (rc != KT_OK) return rc;
  return e->wide ? used_is_wide(e, what, page, kernel) : KT_OK;
}

// the headroom kernels read the STORED `used` (no reconcile of their own) ...
static int32_t stored_used_fits(kt_engine* e, const char* what, int page, const char* kernel) {
  if (!e->wide) return KT_OK;
  if (page < 0) return e->fail(KT_ERR_UNSUPPORTED, "%s: the stored `used` is wider than int64 (%s reads int64 tables)", what, kernel);
  return e->fail(KT_ERR_UNSUPPORTED, "%s: the stored `used` of page %d is wider than int64 (%s reads int64 tables)", what, page, kernel);
}
// ... and the gang forms search over the copies, which takes sums that only grow
static int32_t sums_only_grow(kt_engine* e, const char* what, int page, const char* pod_by_pod = nullptr) {
  if (!e->neg_seen) return KT_OK;
  if (page < 0)
    return e->fail(KT_ERR_UNSUPPORTED,
                   "%s: the engine has been fed a negative request; the search over the copies rests on sums that only grow "
                   "(%s serves such an engine pod by pod)",
                   what, pod_by_pod ? pod_by_pod : "kt_headroom_launch");
  return e->fail(KT_ERR_UNSUPPORTED,
                 "%s: page %d has been fed a negative request; the search over the copies rests on sums that only grow "
                 "(%s serves such pages pod by pod)",
                 what, page, pod_by_pod ? pod_by_pod : "kt_paged_headroom");
}

static int32_t cap_in_range(kt_engine* e, const char* what, int64_t cap) {
  if (cap >= 1 && cap <= (int64_t)KT_HEADROOM_MAX_CAP) return KT_OK;
  return e->fail(KT_ERR_INVALID_ARGUMENT, "%s: cap = %lld, not in [1, %d]", what, (long long)cap, KT_HEADROOM_MAX_CAP);
}

// the copies a headroom forecast's `first` asks for
static int32_t want_in_range(kt_engine* e, const char* what, int64_t want, int64_t cap) {
  if (want >= 1 && want <= cap) return KT_OK;
  return e->fail(KT_ERR_INVALID_ARGUMENT, "%s: want = %lld, not in [1, cap = %lld]", what, (long long)want, (long long)cap);
}

// what every forecast refuses about its instants (and a missing array), in front of everything else
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

// ---------------------------------------------------------------------------------------------------
// device-side steps
// ---------------------------------------------------------------------------------------------------
// Result buffers of at least so many elements each (0: that buffer is not needed).  A launch that was never fetched may still be
// using the old buffers, on the stream it was given — that is last_stream until the call's check replaces it: when any buffer is
// short that stream is synchronised, once, before the first of them is reallocated.
struct Need {
  void* buf;
  size_t n, cap;
  hipError_t (*reserve)(void*, size_t);
  template <class T>
  Need(DevBuf<T>& b, size_t n_) : buf(&b), n(n_), cap(b.cap), reserve([](void* p, size_t k) { return ((DevBuf<T>*)p)->reserve(k); }) {}
};
static int32_t reserve_behind_last_stream(kt_engine* e, std::initializer_list<Need> needs) {
  if (std::none_of(needs.begin(), needs.end(), [](const Need& w) { return w.n != 0 && w.cap < w.n; })) return KT_OK;
  if (e->last_stream) KT_HIP(e, hipStreamSynchronize(e->last_stream));
  for (const Need& w : needs)
    if (w.n != 0) KT_HIP(e, w.reserve(w.buf, w.n));
  return KT_OK;
}

// The ONE check of a query: which throttles affect which of its rows, and the error rows, as a status matrix behind e's check slot.
// The slot then holds this call's rows (as with kt_affected_pods): a pending kt_check_launch is gone, and so are the pending query
// results check_launch_locked clears — except `keep` (preempt_ready / forecast_ready, or none): that result lives in buffers the
// calling query does not write and stays fetchable.
static int32_t query_check(kt_engine* e, int64_t n, const int64_t* rows, int32_t on_equal, hipStream_t s, bool kt_engine::*keep) {
  const bool kept = keep && e->*keep;
  const int32_t rc = check_launch_locked(e, n, rows, on_equal, KT_CHECK_STATUS_MATRIX, s, /*allow_small=*/false);
  e->check_ready = false;
  if (keep) e->*keep = kept;
  return rc;
}

// preemptors (or members) ++ candidates: the rows of a preempt query's one check
static std::vector<int64_t> joined_rows(int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows) {
  std::vector<int64_t> rows(pod_rows, pod_rows + n);
  rows.insert(rows.end(), cand_rows, cand_rows + n_cand);
  return rows;
}

// The page descriptors kt_admit reads, for a headroom kernel over `pages`: page 0's host copy is the source of an asynchronous copy,
// rewritten only once admit_pages_ev says the previous launch's copy has read it (kt_engine_impl.h: h_admit_pages).
static int32_t take_admit_pages(kt_engine* const* pages, int32_t n_pages) {
  kt_engine* e0 = pages[0];
  if (!e0->admit_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->admit_pages_ev, hipEventDisableTiming));
  KT_HIP(e0, hipEventSynchronize(e0->admit_pages_ev));
  e0->h_admit_pages.resize((size_t)n_pages);
  for (int32_t k = 0; k < n_pages; ++k) e0->h_admit_pages[(size_t)k] = admit_page_of(pages[k]);
  KT_HIP(e0, e0->d_admit_pages.reserve(sizeof(kt::AdmitPage) * (size_t)n_pages));
  return KT_OK;
}

// What a *_fetch refuses: nothing of its kind pending, n beyond the launch (name: the calls' infix, what: the query in words)
static int32_t fetch_ready(kt_engine* e, bool ready, const char* name, const char* what, bool gangs, int64_t n, int64_t had) {
  if (!ready) return e->fail(KT_ERR_NOT_READY, "kt_%s_fetch before kt_%s_launch", name, name);
  if (n < 0 || n > had)
    return e->fail(KT_ERR_OUT_OF_RANGE, gangs ? "n_gangs=%lld, the last %s launch had %lld gangs" : "n=%lld, the last %s launch had %lld pods",
                   (long long)n, what, (long long)had);
  return KT_OK;
}
// ... and how it hands out: every destination the caller gave, on the stream of the launch, then ONE synchronisation
struct Out {
  void* dst;
  const void* src;
  size_t bytes;
};
static int32_t fetch_out(kt_engine* e, std::initializer_list<Out> outs) {
  hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
  for (const Out& o : outs)
    if (o.dst && o.bytes) KT_HIP(e, hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, s));
  KT_HIP(e, hipStreamSynchronize(s));
  return KT_OK;
}

// ---------------------------------------------------------------------------------------------------
// A synchronous call over several page engines: every page locked (in address order), launches on page 0's stream s, results handed
// out by the call itself.  From take_preempt_pages on the call ends through finish(): the stream is drained — every copy that reads
// the caller's memory has landed — and pages 1.. get back the last_stream they came with, on every path: nothing of the call stays
// pending on any page.
// ---------------------------------------------------------------------------------------------------
struct PagedCall {
  const char* what;  // words paged_lock's, paged_same_cluster's and the device errors
  kt_engine* const* pages;
  int32_t n_pages;
  PageLocks locks;
  kt_engine* e0 = nullptr;
  hipStream_t s = nullptr;
  std::vector<hipStream_t> last;

  int32_t lock(int64_t n) {
    const int32_t rc = paged_lock(what, pages, n_pages, n, locks);
    if (rc == KT_OK) e0 = pages[0];
    return rc;
  }
  int32_t same_cluster(int64_t n, const int64_t* rows) { return paged_same_cluster(what, pages, n_pages, n, rows); }
  int32_t order() { return paged_order(pages, n_pages, &s); }
  // The descriptors of the paged preempt and forecast kernels, on page 0 under the rule of h_admit_pages with preempt_pages_ev;
  // reconcile_pages fills in the rest.  The call owns every page's reconcile report from here on.
  int32_t take_preempt_pages() {
    if (!e0->preempt_pages_ev) KT_HIP(e0, hipEventCreateWithFlags(&e0->preempt_pages_ev, hipEventDisableTiming));
    KT_HIP(e0, hipEventSynchronize(e0->preempt_pages_ev));  // the previous call's copy has read h_preempt_pages
    e0->h_preempt_pages.resize((size_t)n_pages);
    for (int32_t k = 0; k < n_pages; ++k) e0->h_preempt_pages[(size_t)k].pg = admit_page_of(pages[k]);
    KT_HIP(e0, e0->d_preempt_pages.reserve(sizeof(kt::PreemptPage) * (size_t)n_pages));
    last.resize((size_t)n_pages);
    for (int32_t k = 0; k < n_pages; ++k) last[(size_t)k] = pages[k]->last_stream;
    return KT_OK;
  }
  // a device error that shows only at the drain is returned in KT_OK's place
  int32_t finish(int32_t code) {
    const hipError_t herr = hipStreamSynchronize(s);
    for (int32_t k = 1; k < n_pages; ++k) pages[k]->last_stream = last[(size_t)k];
    if (code == KT_OK && herr != hipSuccess) return e0->fail(KT_ERR_DEVICE, "%s: %s", what, hipGetErrorString(herr));
    return code;
  }
  int32_t device_error(hipError_t herr, const char* doing = "") { return finish(e0->fail(KT_ERR_DEVICE, "%s: %s%s", what, doing, hipGetErrorString(herr))); }
  // a copy on s in either direction (a null end or no bytes: nothing) -> KT_OK, or the code of a call that HAS finished
  int32_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!dst || !src || !bytes) return KT_OK;
    const hipError_t herr = hipMemcpyAsync(dst, src, bytes, kind, s);
    return herr == hipSuccess ? KT_OK : device_error(herr);
  }
  int32_t in(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyHostToDevice); }
  int32_t out(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToHost); }
  int32_t launched() {  // behind a kernel launch
    const hipError_t herr = hipGetLastError();
    return herr == hipSuccess ? KT_OK : device_error(herr);
  }
};

// every page: its dense aggregate beside its partial buffer and its dry finalize at the instant (its reconcile report is dropped),
// and where the paged kernel finds their results -> KT_OK, or the code of a call that HAS finished
static int32_t reconcile_pages(PagedCall& c, int64_t now_s, int32_t now_ns) {
  for (int32_t k = 0; k < c.n_pages; ++k) {
    kt_engine* e = c.pages[k];
    const int32_t rc = preempt_reconcile_locked(e, now_s, now_ns, c.s);
    if (rc != KT_OK) return c.finish(rc);
    kt::PreemptPage& pp = c.e0->h_preempt_pages[(size_t)k];
    pp.partial = e->d_preempt_partial.p, pp.calc = e->d_out_calc.tab(), pp.calc_updated = e->d_out_calc_updated.p, pp.error = e->d_out_error.p;
  }
  return KT_OK;
}

}  // namespace

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
  int32_t rc;
  e0->headroom_ready = false, e0->headroom_gangs = false;
  for (int32_t k = 0; k < n_pages; ++k)
    if ((rc = stored_used_fits(pages[k], "headroom", k, "kt_headroom")) != KT_OK) return rc;
  if ((rc = matrix_fits(e0, "headroom", T, n)) != KT_OK) return rc;
  if (n == 0) {  // nothing is launched
    e0->headroom_ready = true, e0->headroom_n = 0;
    return KT_OK;
  }
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_headroom_copies, (size_t)n}, {e0->d_headroom_limiting, (size_t)n}})) != KT_OK) return rc;
  if ((rc = query_check(e0, n, pod_rows, on_equal, s, nullptr)) != KT_OK) return rc;
  if ((rc = take_admit_pages(pages, n_pages)) != KT_OK) return rc;
  hipError_t herr = hipSuccess;
  if (!kt::launch_headroom(e0->h_admit_pages.data(), n_pages, (kt::AdmitPage*)e0->d_admit_pages.p, e0->admit_pages_ev, n,
                           pod_rows ? e0->d_rows.p : nullptr, T, on_equal != 0, (uint32_t)cap, e0->d_status.p, e0->d_summary.p,
                           e0->d_headroom_copies.p, e0->d_headroom_limiting.p, s, &herr))
    return e0->fail(KT_ERR_DEVICE, "headroom: copy of the page descriptors: %s", hipGetErrorString(herr));
  KT_HIP(e0, hipGetLastError());
  e0->headroom_ready = true, e0->headroom_n = n;
  return KT_OK;
}

int32_t kt_headroom_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int32_t on_equal, int64_t cap, void* stream) {
  if (!e || n < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  if (int32_t bad = cap_in_range(e, "headroom", cap)) return bad;
  KT_HIP(e, hipSetDevice(e->device));
  return headroom_locked(&e, 1, n, pod_rows, on_equal, cap, pick_stream(e, stream));
}

// the results of the last headroom launch, under the launch lock; both outputs nullable
static int32_t headroom_fetch_locked(kt_engine* e, int64_t n, int64_t* out_copies, int32_t* out_limiting) {
  if (int32_t bad = fetch_ready(e, e->headroom_ready && !e->headroom_gangs, "headroom", "headroom", false, n, e->headroom_n)) return bad;
  if (n == 0) return KT_OK;
  return fetch_out(e, {{out_copies, e->d_headroom_copies.p, (size_t)n * 8}, {out_limiting, e->d_headroom_limiting.p, (size_t)n * 4}});
}

int32_t kt_headroom_fetch(kt_engine* e, int64_t n, int64_t* out_copies, int32_t* out_limiting) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  return headroom_fetch_locked(e, n, out_copies, out_limiting);
}

int32_t kt_paged_headroom(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int32_t on_equal, int64_t cap,
                          int64_t* out_copies, int32_t* out_limiting) {
  PagedCall c{"paged headroom", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  if ((rc = cap_in_range(e0, "headroom", cap)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK) return rc;
  if (n == 0) return KT_OK;
  if ((rc = c.order()) != KT_OK) return rc;
  if ((rc = headroom_locked(pages, n_pages, n, pod_rows, on_equal, cap, c.s)) != KT_OK) return rc;
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
  const char* what = "headroom gangs";
  const int32_t T = e->thr_rows_hi;
  int32_t rc;
  if (n > 0 && !pod_rows) return e->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: pod_rows missing");
  if ((rc = gangs_valid(e, n, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = rows_in_range(e, what, n, pod_rows)) != KT_OK) return rc;
  if ((rc = cap_in_range(e, what, cap)) != KT_OK) return rc;
  if ((rc = matrix_fits(e, what, T, n)) != KT_OK) return rc;
  if ((rc = stored_used_fits(e, what, -1, "kt_headroom_gangs")) != KT_OK) return rc;
  if ((rc = sums_only_grow(e, what, -1)) != KT_OK) return rc;
  e->headroom_ready = false, e->headroom_gangs = false;
  if (n == 0) {  // (no gangs) nothing is launched
    e->headroom_ready = true, e->headroom_gangs = true, e->headroom_n = 0;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  const size_t ng = (size_t)n_gangs;
  if ((rc = reserve_behind_last_stream(e, {{e->d_headroom_copies, ng}, {e->d_headroom_limiting, ng}, {e->d_headroom_blocker, ng}, {e->d_headroom_gang_off, ng + 1}})) != KT_OK)
    return rc;
  // the offsets travel on the launch's stream, behind an earlier launch's kernel; the caller's memory is not referenced after return
  KT_HIP(e, hipMemcpyAsync(e->d_headroom_gang_off.p, gang_off, (ng + 1) * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  if ((rc = query_check(e, n, pod_rows, on_equal, s, nullptr)) != KT_OK) return rc;  // over the members of all gangs
  kt::launch_headroom_gangs(admit_page_of(e), n_gangs, e->d_rows.p, e->d_headroom_gang_off.p, T, on_equal != 0, (uint32_t)cap, e->d_status.p,
                            e->d_summary.p, e->d_headroom_copies.p, e->d_headroom_limiting.p, e->d_headroom_blocker.p, s);
  KT_HIP(e, hipGetLastError());
  e->last_stream = s;
  e->headroom_ready = true, e->headroom_gangs = true, e->headroom_n = n_gangs;
  return KT_OK;
}

int32_t kt_headroom_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_copies, int32_t* out_limiting, int64_t* out_blocker) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (int32_t bad = fetch_ready(e, e->headroom_ready && e->headroom_gangs, "headroom_gangs", "headroom gangs", true, n_gangs, e->headroom_n)) return bad;
  if (n_gangs == 0) return KT_OK;
  const size_t ng = (size_t)n_gangs;
  return fetch_out(e, {{out_copies, e->d_headroom_copies.p, ng * 8}, {out_limiting, e->d_headroom_limiting.p, ng * 4}, {out_blocker, e->d_headroom_blocker.p, ng * 8}});
}

// ---------------------------------------------------------------------------------------------------
// headroom, for gangs, over pages: kt_headroom_gangs_launch on the cluster of all names (kt_kernels_headroom_gangs_paged.hip)
// ---------------------------------------------------------------------------------------------------
// kt_paged_headroom's scaffolding with kt_headroom_gangs_launch's gang arguments: the gang defects and "a pod twice" asked per
// gang, then the page set and every page's engine; one check of page 0, ONE kernel over the descriptors kt_admit reads, the
// results through page 0's headroom buffers and out.  Nothing it calls changes a page's last_stream: there is none to hand back,
// and the one thing an error path has to wait for is the copy of the offsets.
int32_t kt_paged_headroom_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                const int64_t* gang_off, int32_t on_equal, int64_t cap, int64_t* out_copies, int32_t* out_limiting,
                                int64_t* out_blocker) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  PagedCall c{"paged headroom gangs", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  const char* what = "headroom gangs";
  // ---- refusals: nothing is launched and no slot or pending result of any page is touched before the last of them
  if (n > 0 && !pod_rows) return e0->fail(KT_ERR_INVALID_ARGUMENT, "headroom gangs: pod_rows missing");
  if ((rc = gangs_valid(e0, n, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e0, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = cap_in_range(e0, what, cap)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((rc = matrix_fits(e0, what, T, n)) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k) {
    if ((rc = stored_used_fits(pages[k], what, k, "kt_headroom_gangs_paged")) != KT_OK) return rc;
    if ((rc = sums_only_grow(pages[k], what, k)) != KT_OK) return rc;
  }
  if (n == 0) return KT_OK;  // (no gangs) nothing is launched
  if ((rc = c.order()) != KT_OK) return rc;
  hipStream_t s = c.s;
  // ---- from here on the call owns page 0's check slot and headroom result
  e0->headroom_ready = false, e0->headroom_gangs = false;
  const size_t ng = (size_t)n_gangs;
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_headroom_copies, ng}, {e0->d_headroom_limiting, ng}, {e0->d_headroom_blocker, ng}, {e0->d_headroom_gang_off, ng + 1}})) != KT_OK)
    return rc;
  // the offsets travel on the launch's stream, behind an earlier launch's kernel (the call is synchronous: the caller's memory is
  // not referenced after return)
  KT_HIP(e0, hipMemcpyAsync(e0->d_headroom_gang_off.p, gang_off, (ng + 1) * 8, hipMemcpyHostToDevice, s));
  if ((rc = query_check(e0, n, pod_rows, on_equal, s, nullptr)) != KT_OK) {  // over the members of all gangs
    (void)hipStreamSynchronize(s);  // the copy of the offsets reads the caller's memory
    return rc;
  }
  if ((rc = take_admit_pages(pages, n_pages)) != KT_OK) return rc;
  hipError_t herr = hipSuccess;
  if (!kt::launch_headroom_gangs_paged(e0->h_admit_pages.data(), n_pages, (kt::AdmitPage*)e0->d_admit_pages.p, e0->admit_pages_ev, n_gangs,
                                       e0->d_rows.p, e0->d_headroom_gang_off.p, T, on_equal != 0, (uint32_t)cap, e0->d_status.p, e0->d_summary.p,
                                       e0->d_headroom_copies.p, e0->d_headroom_limiting.p, e0->d_headroom_blocker.p, s, &herr)) {
    (void)hipStreamSynchronize(s);
    return e0->fail(KT_ERR_DEVICE, "paged headroom gangs: copy of the page descriptors: %s", hipGetErrorString(herr));
  }
  KT_HIP(e0, hipGetLastError());
  e0->last_stream = s;
  rc = fetch_out(e0, {{out_copies, e0->d_headroom_copies.p, ng * 8}, {out_limiting, e0->d_headroom_limiting.p, ng * 4}, {out_blocker, e0->d_headroom_blocker.p, ng * 8}});
  if (rc != KT_OK) return rc;
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
  const char* what = "preempt";
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  int32_t rc;
  if ((rc = preempt_arrays_present(e, what, n, pod_rows, n_cand, cand_rows)) != KT_OK) return rc;
  if ((rc = rows_in_range(e, what, n, pod_rows)) != KT_OK || (rc = rows_in_range(e, what, n_cand, cand_rows)) != KT_OK) return rc;
  if ((rc = candidates_distinct_from_preemptors(e, what, n, pod_rows, n_cand, cand_rows, /*gangs=*/false)) != KT_OK) return rc;
  if ((rc = matrix_fits(e, what, T, n, n_cand)) != KT_OK) return rc;
  if ((rc = serves_dry_reconcile(e, what, -1, "kt_preempt")) != KT_OK) return rc;
  e->preempt_ready = false;
  if (n == 0) {  // nothing is launched
    e->preempt_ready = true, e->preempt_kind = kPreemptPods, e->preempt_n = 0, e->preempt_m = n_cand;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  if ((rc = ensure_ready(e, s)) != KT_OK || (rc = sums_fit_int64(e, what, -1, "kt_preempt", s)) != KT_OK) return rc;
  const size_t vic = (size_t)n * (size_t)n_cand;
  // the reprieve kernel's list state where it can outgrow LDS (0 bytes: it cannot, or nothing is walked)
  const size_t ws = reprieve && n_cand > 0 ? kt::reprieve_ws_bytes(T, e->D, n, e->reprieve_lds_cap_limit) : 0;
  if ((rc = reserve_behind_last_stream(e, {{e->d_preempt_prefix, (size_t)n}, {e->d_preempt_victims, vic + 1}, {e->d_reprieve_ws, ws}})) != KT_OK) return rc;
  const std::vector<int64_t> rows = joined_rows(n, pod_rows, n_cand, cand_rows);
  if ((rc = query_check(e, n + n_cand, rows.data(), on_equal, s, &kt_engine::forecast_ready)) != KT_OK) return rc;
  if ((rc = preempt_reconcile_locked(e, now_s, now_ns, s)) != KT_OK) return rc;
  const kt::AdmitPage pg = admit_page_of(e);
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
  e->preempt_ready = true, e->preempt_kind = kPreemptPods, e->preempt_n = n, e->preempt_m = n_cand;
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
  if (int32_t bad = fetch_ready(e, e->preempt_ready && e->preempt_kind == kPreemptPods, "preempt", "preempt", false, n, e->preempt_n)) return bad;
  if (n == 0) return KT_OK;
  return fetch_out(e, {{out_prefix, e->d_preempt_prefix.p, (size_t)n * 8}, {out_victims, e->d_preempt_victims.p, (size_t)n * (size_t)e->preempt_m}});
}

// ---------------------------------------------------------------------------------------------------
// preempt over pages: kt_preempt_launch / kt_preempt_reprieve_launch on the cluster of all names (kt_kernels_preempt_paged.hip)
// ---------------------------------------------------------------------------------------------------
int32_t kt_paged_preempt(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_cand, const int64_t* cand_rows,
                         int64_t now_s, int32_t now_ns, int32_t on_equal, uint32_t flags, int64_t* out_prefix, uint8_t* out_victims) {
  PagedCall c{"paged preempt", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  const char *what = "preempt", *kernel = "kt_preempt_paged";
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if (flags & ~KT_PREEMPT_REPRIEVE) return e0->fail(KT_ERR_INVALID_ARGUMENT, "paged preempt: flags = 0x%x", flags);
  const bool reprieve = (flags & KT_PREEMPT_REPRIEVE) != 0;
  if ((rc = preempt_arrays_present(e0, what, n, pod_rows, n_cand, cand_rows)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK || (rc = c.same_cluster(n_cand, cand_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((rc = matrix_fits(e0, what, T, n, n_cand)) != KT_OK) return rc;
  if ((rc = candidates_distinct_from_preemptors(e0, what, n, pod_rows, n_cand, cand_rows, /*gangs=*/false)) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k)
    if ((rc = serves_dry_reconcile(pages[k], what, k, kernel)) != KT_OK) return rc;
  if (n == 0) return KT_OK;  // nothing is launched
  if ((rc = c.order()) != KT_OK || (rc = ensure_ready(e0, c.s)) != KT_OK) return rc;
  hipStream_t s = c.s;
  for (int32_t k = 0; k < n_pages; ++k)  // (before the check slot, a reconcile report or a result buffer of any page is touched)
    if ((rc = sums_fit_int64(pages[k], what, k, kernel, s)) != KT_OK) return rc;
  // ---- from here on the call owns page 0's check slot and preempt result and every page's reconcile report
  e0->preempt_ready = false;
  if ((rc = c.take_preempt_pages()) != KT_OK) return rc;
  const size_t vic = (size_t)n * (size_t)n_cand;
  const size_t ws = reprieve && n_cand > 0 ? kt::reprieve_paged_ws_bytes(T, e0->h_preempt_pages.data(), n_pages, n, e0->reprieve_lds_cap_limit) : 0;
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_preempt_prefix, (size_t)n}, {e0->d_preempt_victims, vic + 1}, {e0->d_reprieve_ws, ws}})) != KT_OK) return rc;
  const std::vector<int64_t> rows = joined_rows(n, pod_rows, n_cand, cand_rows);
  if ((rc = query_check(e0, n + n_cand, rows.data(), on_equal, s, &kt_engine::forecast_ready)) != KT_OK) return c.finish(rc);
  if ((rc = reconcile_pages(c, now_s, now_ns)) != KT_OK) return rc;
  hipError_t herr = hipSuccess;
  if (!kt::launch_preempt_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n, n_cand,
                                e0->d_rows.p, T, on_equal != 0, e0->d_status.p, e0->d_summary.p, e0->d_preempt_prefix.p, e0->d_preempt_victims.p, s,
                                &herr))
    return c.device_error(herr, "copy of the page descriptors: ");
  if ((rc = c.launched()) != KT_OK) return rc;
  if (reprieve) {
    kt::launch_preempt_reprieve_paged(e0->h_preempt_pages.data(), n_pages, (const kt::PreemptPage*)e0->d_preempt_pages.p, n, n_cand, e0->d_rows.p, T,
                                      on_equal != 0, e0->d_status.p, e0->d_preempt_prefix.p, e0->d_preempt_victims.p,
                                      ws != 0 ? e0->d_reprieve_ws.p : nullptr, e0->reprieve_lds_cap_limit, s);
    if ((rc = c.launched()) != KT_OK) return rc;
  }
  e0->last_stream = s;
  if ((rc = c.out(out_prefix, e0->d_preempt_prefix.p, (size_t)n * 8)) != KT_OK || (rc = c.out(out_victims, e0->d_preempt_victims.p, vic)) != KT_OK) return rc;
  return c.finish(KT_OK);  // (synchronises s; the results have been handed out: no preempt result is pending on page 0)
}

// ---------------------------------------------------------------------------------------------------
// preempt, for gangs: the shortest victim prefix that lets a whole gang through (kt_kernels_preempt_gangs.hip), and the reprieve
// pass that shrinks its victim mask to a minimal set (kt_kernels_preempt_gangs_reprieve.hip)
// ---------------------------------------------------------------------------------------------------
// kt_preempt_gangs_launch: the refusals of preempt_locked in its order (with the gang defects in front, and "a pod twice" asked
// per gang), then the same launches with kt_preempt_gangs in kt_preempt's place.  The result shares the one pending preempt result;
// preempt_kind tells the fetches apart.  With `reprieve` (kt_preempt_gangs_reprieve_launch): behind them on the same stream the one
// launch of kt_preempt_gangs_reprieve that rewrites the victim bytes in place.  The caller holds the launch lock.
// `rule` (kt_preempt_gangs_elastic_launch, which has refused the rule's own defects): the quorum per gang and the flag byte per
// member.  The arrays travel on the launch's stream beside the offsets; the kernel is kt_preempt_gangs_elastic, which walks the
// victims back itself when `reprieve` is set, and the result is the kind of its own.
struct ElasticRule {
  const int64_t* min_members;   // [n_gangs]
  const uint8_t* member_flags;  // [n], nullable
};
static int32_t preempt_gangs_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_cand,
                                    const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, void* stream, bool reprieve,
                                    const ElasticRule* rule = nullptr) {
  const char* what = rule ? "preempt elastic gangs" : "preempt gangs";
  const char* kernel = rule ? "kt_preempt_gangs_elastic" : "kt_preempt_gangs";
  const PreemptKind kind = rule ? kPreemptGangsElastic : kPreemptGangs;
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  int32_t rc;
  if ((rc = gangs_valid(e, n, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = preempt_arrays_present(e, what, n, pod_rows, n_cand, cand_rows)) != KT_OK) return rc;
  if ((rc = rows_in_range(e, what, n, pod_rows)) != KT_OK || (rc = rows_in_range(e, what, n_cand, cand_rows)) != KT_OK) return rc;
  if ((rc = candidates_distinct_from_preemptors(e, what, n, pod_rows, n_cand, cand_rows, /*gangs=*/true)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = matrix_fits(e, what, T, n, n_cand)) != KT_OK) return rc;
  if ((rc = serves_dry_reconcile(e, what, -1, kernel)) != KT_OK) return rc;
  if (n == 0) {  // (no gangs) nothing is launched
    e->preempt_ready = true, e->preempt_kind = kind, e->preempt_n = 0, e->preempt_m = n_cand;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  if ((rc = ensure_ready(e, s)) != KT_OK || (rc = sums_fit_int64(e, what, -1, kernel, s)) != KT_OK) return rc;
  const size_t ng = (size_t)n_gangs, vic = ng * (size_t)n_cand;
  // the reprieve kernel's list state where it can outgrow LDS (0 bytes: it cannot, or nothing is walked)
  const size_t ws = rule ? 0 : reprieve && n_cand > 0 ? kt::reprieve_ws_bytes(T, e->D, n_gangs, e->reprieve_lds_cap_limit) : 0;
  // ... and the elastic kernel's state of a union (it builds it for every gang, whatever the list holds)
  const size_t ews = rule ? kt::preempt_gangs_elastic_ws_bytes(T, e->D, n_gangs, e->preempt_elastic_lds_cap_limit) : 0;
  const bool flagged = rule && rule->member_flags;
  if ((rc = reserve_behind_last_stream(e, {{e->d_preempt_prefix, ng}, {e->d_preempt_victims, vic + 1}, {e->d_preempt_blocker, ng}, {e->d_preempt_gang_off, ng + 1}, {e->d_reprieve_ws, ws},
                                           {e->d_preempt_members, rule ? ng : 0}, {e->d_preempt_min, rule ? ng : 0}, {e->d_preempt_flags, flagged ? (size_t)n : 0}, {e->d_preempt_elastic_ws, ews}})) != KT_OK)
    return rc;
  // the offsets travel on the launch's stream, behind an earlier launch's kernel; the caller's memory is not referenced after return
  KT_HIP(e, hipMemcpyAsync(e->d_preempt_gang_off.p, gang_off, (ng + 1) * 8, hipMemcpyHostToDevice, s));
  if (rule) KT_HIP(e, hipMemcpyAsync(e->d_preempt_min.p, rule->min_members, ng * 8, hipMemcpyHostToDevice, s));
  if (flagged) KT_HIP(e, hipMemcpyAsync(e->d_preempt_flags.p, rule->member_flags, (size_t)n, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  const std::vector<int64_t> rows = joined_rows(n, pod_rows, n_cand, cand_rows);
  if ((rc = query_check(e, n + n_cand, rows.data(), on_equal, s, &kt_engine::forecast_ready)) != KT_OK) return rc;
  if ((rc = preempt_reconcile_locked(e, now_s, now_ns, s)) != KT_OK) return rc;
  const kt::AdmitPage pg = admit_page_of(e);
  if (rule)
    kt::launch_preempt_gangs_elastic(pg, n, n_cand, e->d_rows.p, n_gangs, e->d_preempt_gang_off.p, e->d_preempt_min.p,
                                     flagged ? e->d_preempt_flags.p : nullptr, e->thr_rows_hi, on_equal != 0, reprieve, e->d_status.p, e->d_summary.p,
                                     e->d_preempt_partial.p, e->d_out_calc.tab(), e->d_out_calc_updated.p, e->d_out_error.p, e->d_preempt_prefix.p,
                                     e->d_preempt_victims.p, e->d_preempt_members.p, e->d_preempt_blocker.p,
                                     ews != 0 ? e->d_preempt_elastic_ws.p : nullptr, e->preempt_elastic_lds_cap_limit, s);
  else
    kt::launch_preempt_gangs(pg, n, n_cand, e->d_rows.p, n_gangs, e->d_preempt_gang_off.p, e->thr_rows_hi, on_equal != 0, e->d_status.p, e->d_summary.p,
                             e->d_preempt_partial.p, e->d_out_calc.tab(), e->d_out_calc_updated.p, e->d_out_error.p, e->d_preempt_prefix.p,
                             e->d_preempt_victims.p, e->d_preempt_blocker.p, s);
  KT_HIP(e, hipGetLastError());
  if (reprieve && !rule) {
    kt::launch_preempt_gangs_reprieve(pg, n, n_cand, e->d_rows.p, n_gangs, e->d_preempt_gang_off.p, e->thr_rows_hi, on_equal != 0, e->d_status.p,
                                      e->d_preempt_partial.p, e->d_out_calc.tab(), e->d_out_calc_updated.p, e->d_out_error.p, e->d_preempt_prefix.p,
                                      e->d_preempt_victims.p, ws != 0 ? e->d_reprieve_ws.p : nullptr, e->reprieve_lds_cap_limit, s);
    KT_HIP(e, hipGetLastError());
  }
  e->last_stream = s;
  e->preempt_ready = true, e->preempt_kind = kind, e->preempt_n = n_gangs, e->preempt_m = n_cand;
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
  if (int32_t bad = fetch_ready(e, e->preempt_ready && e->preempt_kind == kPreemptGangs, "preempt_gangs", "preempt gangs", true, n_gangs, e->preempt_n)) return bad;
  if (n_gangs == 0) return KT_OK;
  const size_t ng = (size_t)n_gangs;
  return fetch_out(e, {{out_prefix, e->d_preempt_prefix.p, ng * 8}, {out_victims, e->d_preempt_victims.p, ng * (size_t)e->preempt_m}, {out_blocker, e->d_preempt_blocker.p, ng * 8}});
}

// ---------------------------------------------------------------------------------------------------
// preempt, for elastic gangs: the shortest victim prefix that lets a gang's quorum in (kt_kernels_preempt_gangs_elastic.hip)
// ---------------------------------------------------------------------------------------------------
// The refusals: every gang_off defect, the rule's (elastic_valid, worded as kt_admit_gangs_elastic_launch words them), a flag bit
// other than KT_PREEMPT_REPRIEVE, then everything preempt_gangs_locked refuses in its order.
int32_t kt_preempt_gangs_elastic_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                        const int64_t* min_members, const uint8_t* member_flags, int64_t n_cand, const int64_t* cand_rows,
                                        int64_t now_s, int32_t now_ns, int32_t on_equal, uint32_t flags, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  int32_t rc = gangs_valid(e, n, n_gangs, gang_off);
  if (rc == KT_OK) rc = elastic_valid(e, n, n_gangs, gang_off, min_members, member_flags);
  if (rc != KT_OK) return rc;
  if (flags & ~KT_PREEMPT_REPRIEVE) return e->fail(KT_ERR_INVALID_ARGUMENT, "preempt elastic gangs: flags = 0x%x", flags);
  const ElasticRule rule{min_members, member_flags};
  return preempt_gangs_locked(e, n, pod_rows, n_gangs, gang_off, n_cand, cand_rows, now_s, now_ns, on_equal, stream,
                              (flags & KT_PREEMPT_REPRIEVE) != 0, &rule);
}

int32_t kt_preempt_gangs_elastic_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_prefix, uint8_t* out_victims, int64_t* out_members,
                                       int64_t* out_blocker) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (int32_t bad = fetch_ready(e, e->preempt_ready && e->preempt_kind == kPreemptGangsElastic, "preempt_gangs_elastic", "preempt elastic gangs", true,
                                n_gangs, e->preempt_n))
    return bad;
  if (n_gangs == 0) return KT_OK;
  const size_t ng = (size_t)n_gangs;
  return fetch_out(e, {{out_prefix, e->d_preempt_prefix.p, ng * 8}, {out_victims, e->d_preempt_victims.p, ng * (size_t)e->preempt_m}, {out_members, e->d_preempt_members.p, ng * 8}, {out_blocker, e->d_preempt_blocker.p, ng * 8}});
}

// ---------------------------------------------------------------------------------------------------
// preempt, for gangs, over pages: kt_preempt_gangs_launch / kt_preempt_gangs_reprieve_launch on the cluster of all names
// (kt_kernels_preempt_gangs_paged.hip)
// ---------------------------------------------------------------------------------------------------
int32_t kt_paged_preempt_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                               int64_t n_cand, const int64_t* cand_rows, int64_t now_s, int32_t now_ns, int32_t on_equal, uint32_t flags,
                               int64_t* out_prefix, uint8_t* out_victims, int64_t* out_blocker) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  PagedCall c{"paged preempt gangs", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  const char *what = "preempt gangs", *kernel = "kt_preempt_gangs_paged";
  // ---- refusals: nothing is allocated or launched and no slot of any page is touched before the last of them
  if (flags & ~KT_PREEMPT_REPRIEVE) return e0->fail(KT_ERR_INVALID_ARGUMENT, "paged preempt gangs: flags = 0x%x", flags);
  const bool reprieve = (flags & KT_PREEMPT_REPRIEVE) != 0;
  if ((rc = gangs_valid(e0, n, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = preempt_arrays_present(e0, what, n, pod_rows, n_cand, cand_rows)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK || (rc = c.same_cluster(n_cand, cand_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  if ((rc = candidates_distinct_from_preemptors(e0, what, n, pod_rows, n_cand, cand_rows, /*gangs=*/true)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e0, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  const int32_t T = e0->thr_rows_hi;
  if ((rc = matrix_fits(e0, what, T, n, n_cand)) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k)
    if ((rc = serves_dry_reconcile(pages[k], what, k, kernel)) != KT_OK) return rc;
  if (n == 0) return KT_OK;  // (no gangs) nothing is launched
  if ((rc = c.order()) != KT_OK || (rc = ensure_ready(e0, c.s)) != KT_OK) return rc;
  hipStream_t s = c.s;
  for (int32_t k = 0; k < n_pages; ++k)  // (before the check slot, a reconcile report or a result buffer of any page is touched)
    if ((rc = sums_fit_int64(pages[k], what, k, kernel, s)) != KT_OK) return rc;
  // ---- from here on the call owns page 0's check slot and preempt result and every page's reconcile report
  e0->preempt_ready = false;
  if ((rc = c.take_preempt_pages()) != KT_OK) return rc;
  const size_t ng = (size_t)n_gangs, vic = ng * (size_t)n_cand;
  const size_t ws =
      reprieve && n_cand > 0 ? kt::reprieve_paged_ws_bytes(T, e0->h_preempt_pages.data(), n_pages, n_gangs, e0->reprieve_lds_cap_limit) : 0;
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_preempt_prefix, ng}, {e0->d_preempt_victims, vic + 1}, {e0->d_preempt_blocker, ng}, {e0->d_preempt_gang_off, ng + 1}, {e0->d_reprieve_ws, ws}})) != KT_OK)
    return rc;
  const std::vector<int64_t> rows = joined_rows(n, pod_rows, n_cand, cand_rows);
  if ((rc = query_check(e0, n + n_cand, rows.data(), on_equal, s, &kt_engine::forecast_ready)) != KT_OK) return c.finish(rc);
  if ((rc = reconcile_pages(c, now_s, now_ns)) != KT_OK) return rc;
  hipError_t herr = hipSuccess;
  // the offsets travel on the same stream (the call is synchronous: the caller's memory outlives the copy)
  if ((herr = hipMemcpyAsync(e0->d_preempt_gang_off.p, gang_off, (ng + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c.device_error(herr, "copy of the gang offsets: ");
  if (!kt::launch_preempt_gangs_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n, n_cand,
                                      e0->d_rows.p, n_gangs, e0->d_preempt_gang_off.p, T, on_equal != 0, e0->d_status.p, e0->d_summary.p,
                                      e0->d_preempt_prefix.p, e0->d_preempt_victims.p, e0->d_preempt_blocker.p, s, &herr))
    return c.device_error(herr, "copy of the page descriptors: ");
  if ((rc = c.launched()) != KT_OK) return rc;
  if (reprieve) {
    kt::launch_preempt_gangs_reprieve_paged(e0->h_preempt_pages.data(), n_pages, (const kt::PreemptPage*)e0->d_preempt_pages.p, n, n_cand, e0->d_rows.p,
                                            n_gangs, e0->d_preempt_gang_off.p, T, on_equal != 0, e0->d_status.p, e0->d_preempt_prefix.p,
                                            e0->d_preempt_victims.p, ws != 0 ? e0->d_reprieve_ws.p : nullptr, e0->reprieve_lds_cap_limit, s);
    if ((rc = c.launched()) != KT_OK) return rc;
  }
  e0->last_stream = s;
  if ((rc = c.out(out_prefix, e0->d_preempt_prefix.p, ng * 8)) != KT_OK || (rc = c.out(out_victims, e0->d_preempt_victims.p, vic)) != KT_OK ||
      (rc = c.out(out_blocker, e0->d_preempt_blocker.p, ng * 8)) != KT_OK)
    return rc;
  return c.finish(KT_OK);  // (synchronises s; the results have been handed out: no preempt result is pending on page 0)
}

// ---------------------------------------------------------------------------------------------------
// forecast: the first instant at which a blocked pod passes (kt_kernels_forecast.hip)
// ---------------------------------------------------------------------------------------------------
// The caller holds the launch lock.  Every refusal comes before the check slot, the reconcile report or a result buffer is touched.
static int32_t forecast_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns,
                               int32_t on_equal, void* stream) {
  const char *what = "forecast", *kernel = "kt_forecast";
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  int32_t rc;
  if ((rc = forecast_instants_valid(e, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = rows_in_range(e, what, n, pod_rows)) != KT_OK) return rc;
  if ((rc = matrix_fits(e, what, T, n)) != KT_OK || (rc = verdicts_fit(e, what, n, n_inst)) != KT_OK) return rc;
  if ((rc = serves_dry_reconcile(e, what, -1, kernel)) != KT_OK) return rc;
  if (n == 0) {  // nothing is launched
    e->forecast_ready = true, e->forecast_kind = kForecastPods, e->forecast_n = 0, e->forecast_m = n_inst;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  if ((rc = ensure_ready(e, s)) != KT_OK || (rc = sums_fit_int64(e, what, -1, kernel, s)) != KT_OK) return rc;
  e->forecast_ready = false;
  const size_t ver = (size_t)n * (size_t)n_inst, m = (size_t)n_inst;
  if ((rc = reserve_behind_last_stream(e, {{e->d_forecast_first, (size_t)n}, {e->d_forecast_verdicts, ver + 1}, {e->d_forecast_inst_s, m}, {e->d_forecast_inst_ns, m}})) != KT_OK)
    return rc;
  // the instants travel on the launch's stream, behind an earlier forecast's kernel; the caller's memory is not referenced after
  // return
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_s.p, inst_s, m * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_ns.p, inst_ns, m * 4, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  if ((rc = query_check(e, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return rc;
  // the aggregate with exact contributor counts and the error bytes; the dry finalize runs at t_0
  if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return rc;
  kt::launch_forecast(admit_page_of(e), n, n_inst, e->d_rows.p, e->d_forecast_inst_s.p, e->d_forecast_inst_ns.p, T, on_equal != 0, e->d_status.p,
                      e->d_summary.p, e->d_preempt_partial.p, e->d_out_error.p, e->d_forecast_first.p, e->d_forecast_verdicts.p, s);
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
  if (int32_t bad = fetch_ready(e, e->forecast_ready && e->forecast_kind == kForecastPods, "forecast", "forecast", false, n, e->forecast_n)) return bad;
  if (n == 0) return KT_OK;
  return fetch_out(e, {{out_first, e->d_forecast_first.p, (size_t)n * 8}, {out_verdicts, e->d_forecast_verdicts.p, (size_t)n * (size_t)e->forecast_m}});
}

// ---------------------------------------------------------------------------------------------------
// headroom forecast: how many copies of a pod the throttles admit at each instant (kt_kernels_headroom_forecast.hip)
// ---------------------------------------------------------------------------------------------------
// forecast_locked's sequence with kt_headroom_forecast in kt_forecast's place: the refusals in its order (cap and want behind the
// instants), the |request| sums probe, ONE check, the dry aggregate and finalize at t_0, the kernel.  The result shares the one
// pending forecast result as its third kind.  The caller holds the launch lock.
static int32_t headroom_forecast_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s,
                                        const int32_t* inst_ns, int32_t on_equal, int64_t cap, int64_t want, void* stream) {
  const char *what = "headroom forecast", *kernel = "kt_headroom_forecast";
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  int32_t rc;
  if ((rc = forecast_instants_valid(e, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = cap_in_range(e, what, cap)) != KT_OK) return rc;
  if ((rc = want_in_range(e, what, want, cap)) != KT_OK) return rc;
  if ((rc = rows_in_range(e, what, n, pod_rows)) != KT_OK) return rc;
  if ((rc = matrix_fits(e, what, T, n)) != KT_OK || (rc = verdicts_fit(e, what, n, n_inst, "n", "results")) != KT_OK) return rc;
  if ((rc = serves_dry_reconcile(e, what, -1, kernel)) != KT_OK) return rc;
  if (n == 0) {  // nothing is launched
    e->forecast_ready = true, e->forecast_kind = kForecastHeadroom, e->forecast_n = 0, e->forecast_m = n_inst;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  if ((rc = ensure_ready(e, s)) != KT_OK || (rc = sums_fit_int64(e, what, -1, kernel, s)) != KT_OK) return rc;
  e->forecast_ready = false;
  const size_t cells = (size_t)n * (size_t)n_inst, m = (size_t)n_inst;
  if ((rc = reserve_behind_last_stream(e, {{e->d_forecast_first, (size_t)n}, {e->d_forecast_copies, cells}, {e->d_forecast_limiting, cells}, {e->d_forecast_inst_s, m}, {e->d_forecast_inst_ns, m}})) != KT_OK)
    return rc;
  // the instants travel on the launch's stream, behind an earlier forecast's kernel; the caller's memory is not referenced after
  // return
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_s.p, inst_s, m * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_ns.p, inst_ns, m * 4, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  if ((rc = query_check(e, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return rc;
  // the aggregate with exact contributor counts and the error bytes; the dry finalize runs at t_0
  if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return rc;
  kt::launch_headroom_forecast(admit_page_of(e), n, n_inst, e->d_rows.p, e->d_forecast_inst_s.p, e->d_forecast_inst_ns.p, T, on_equal != 0, (uint32_t)cap,
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
  if (int32_t bad = fetch_ready(e, e->forecast_ready && e->forecast_kind == kForecastHeadroom, "headroom_forecast", "headroom forecast", false, n, e->forecast_n))
    return bad;
  if (n == 0) return KT_OK;
  const size_t cells = (size_t)n * (size_t)e->forecast_m;
  return fetch_out(e, {{out_first, e->d_forecast_first.p, (size_t)n * 8}, {out_copies, e->d_forecast_copies.p, cells * 8}, {out_limiting, e->d_forecast_limiting.p, cells * 4}});
}

// ---------------------------------------------------------------------------------------------------
// forecast, for gangs: the first instant at which a whole gang is admitted (kt_kernels_forecast_gangs.hip)
// ---------------------------------------------------------------------------------------------------
// The refusals of forecast_locked in its order (the instants first, then the gang defects and "a pod twice" asked per gang), then
// the same launches with kt_forecast_gangs in kt_forecast's place.  The result shares the one pending forecast result;
// forecast_kind tells the fetches apart.  The caller holds the launch lock.
// `rule` (kt_forecast_gangs_elastic_launch): the quorum per gang and the flag byte per member.  Its refusals come behind the gang
// defects (they read the sizes) and before the rest; the arrays travel on the launch's stream beside the offsets; the kernel is
// kt_forecast_gangs_elastic with the small launch for `first` behind it, and the result is the kind of its own.
static int32_t forecast_gangs_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_inst,
                                     const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, void* stream,
                                     const ElasticRule* rule = nullptr) {
  const char* what = rule ? "forecast elastic gangs" : "forecast gangs";
  const char* kernel = rule ? "kt_forecast_gangs_elastic" : "kt_forecast_gangs";
  const ForecastKind kind = rule ? kForecastGangsElastic : kForecastGangs;
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  int32_t rc;
  if ((rc = forecast_instants_valid(e, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = gangs_valid(e, n, n_gangs, gang_off)) != KT_OK) return rc;
  if (rule && (rc = elastic_valid(e, n, n_gangs, gang_off, rule->min_members, rule->member_flags)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = rows_in_range(e, what, n, pod_rows)) != KT_OK) return rc;
  if ((rc = matrix_fits(e, what, T, n)) != KT_OK || (rc = verdicts_fit(e, what, n_gangs, n_inst, "n_gangs")) != KT_OK) return rc;
  if ((rc = serves_dry_reconcile(e, what, -1, kernel)) != KT_OK) return rc;
  if (n == 0) {  // (no gangs) nothing is launched
    e->forecast_ready = true, e->forecast_kind = kind, e->forecast_n = 0, e->forecast_m = n_inst;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  if ((rc = ensure_ready(e, s)) != KT_OK || (rc = sums_fit_int64(e, what, -1, kernel, s)) != KT_OK) return rc;
  e->forecast_ready = false;
  const size_t ng = (size_t)n_gangs, m = (size_t)n_inst, ver = ng * m;
  const bool flagged = rule && rule->member_flags;
  const size_t ws = rule ? kt::forecast_gangs_elastic_ws_bytes(T, e->D, n_gangs, n_inst, e->forecast_elastic_lds_cap_limit) : 0;
  if ((rc = reserve_behind_last_stream(e, {{e->d_forecast_first, ng}, {e->d_forecast_verdicts, ver + 1}, {e->d_forecast_blocker, ver}, {e->d_forecast_inst_s, m}, {e->d_forecast_inst_ns, m}, {e->d_forecast_gang_off, ng + 1},
                                           {e->d_forecast_members, rule ? ver : 0}, {e->d_forecast_min, rule ? ng : 0}, {e->d_forecast_flags, flagged ? (size_t)n : 0}, {e->d_forecast_elastic_ws, ws}})) != KT_OK)
    return rc;
  // the instants and the offsets travel on the launch's stream, behind an earlier forecast's kernel; the caller's memory is not
  // referenced after return
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_s.p, inst_s, m * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_ns.p, inst_ns, m * 4, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_gang_off.p, gang_off, (ng + 1) * 8, hipMemcpyHostToDevice, s));
  if (rule) KT_HIP(e, hipMemcpyAsync(e->d_forecast_min.p, rule->min_members, ng * 8, hipMemcpyHostToDevice, s));
  if (flagged) KT_HIP(e, hipMemcpyAsync(e->d_forecast_flags.p, rule->member_flags, (size_t)n, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  if ((rc = query_check(e, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return rc;  // over the members of all gangs
  // the aggregate with exact contributor counts and the error bytes; the dry finalize runs at t_0
  if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return rc;
  if (rule)
    kt::launch_forecast_gangs_elastic(admit_page_of(e), n_gangs, n_inst, e->d_rows.p, e->d_forecast_gang_off.p, e->d_forecast_min.p,
                                      flagged ? e->d_forecast_flags.p : nullptr, e->d_forecast_inst_s.p, e->d_forecast_inst_ns.p, T, on_equal != 0,
                                      e->d_status.p, e->d_summary.p, e->d_preempt_partial.p, e->d_out_error.p, e->d_forecast_first.p,
                                      e->d_forecast_verdicts.p, e->d_forecast_members.p, e->d_forecast_blocker.p,
                                      ws != 0 ? e->d_forecast_elastic_ws.p : nullptr, e->forecast_elastic_lds_cap_limit, s);
  else
    kt::launch_forecast_gangs(admit_page_of(e), n_gangs, n_inst, e->d_rows.p, e->d_forecast_gang_off.p, e->d_forecast_inst_s.p, e->d_forecast_inst_ns.p, T,
                              on_equal != 0, e->d_status.p, e->d_summary.p, e->d_preempt_partial.p, e->d_out_error.p, e->d_forecast_first.p,
                              e->d_forecast_verdicts.p, e->d_forecast_blocker.p, s);
  KT_HIP(e, hipGetLastError());
  e->last_stream = s;
  e->forecast_ready = true, e->forecast_kind = kind, e->forecast_n = n_gangs, e->forecast_m = n_inst;
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
  if (int32_t bad = fetch_ready(e, e->forecast_ready && e->forecast_kind == kForecastGangs, "forecast_gangs", "forecast gangs", true, n_gangs, e->forecast_n))
    return bad;
  if (n_gangs == 0) return KT_OK;
  const size_t ng = (size_t)n_gangs, ver = ng * (size_t)e->forecast_m;
  return fetch_out(e, {{out_first, e->d_forecast_first.p, ng * 8}, {out_verdicts, e->d_forecast_verdicts.p, ver}, {out_blocker, e->d_forecast_blocker.p, ver * 8}});
}

// ---------------------------------------------------------------------------------------------------
// forecast, for elastic gangs: the first instant at which a gang's quorum fits (kt_kernels_forecast_gangs_elastic.hip)
// ---------------------------------------------------------------------------------------------------
int32_t kt_forecast_gangs_elastic_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                         const int64_t* min_members, const uint8_t* member_flags, int64_t n_inst, const int64_t* inst_s,
                                         const int32_t* inst_ns, int32_t on_equal, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  const ElasticRule rule{min_members, member_flags};
  return forecast_gangs_locked(e, n, pod_rows, n_gangs, gang_off, n_inst, inst_s, inst_ns, on_equal, stream, &rule);
}

int32_t kt_forecast_gangs_elastic_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_first, uint8_t* out_verdicts, int64_t* out_members,
                                        int64_t* out_blocker) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (int32_t bad = fetch_ready(e, e->forecast_ready && e->forecast_kind == kForecastGangsElastic, "forecast_gangs_elastic", "forecast elastic gangs", true,
                                n_gangs, e->forecast_n))
    return bad;
  if (n_gangs == 0) return KT_OK;
  const size_t ng = (size_t)n_gangs, ver = ng * (size_t)e->forecast_m;
  return fetch_out(e, {{out_first, e->d_forecast_first.p, ng * 8}, {out_verdicts, e->d_forecast_verdicts.p, ver}, {out_members, e->d_forecast_members.p, ver * 8}, {out_blocker, e->d_forecast_blocker.p, ver * 8}});
}

// ---------------------------------------------------------------------------------------------------
// headroom forecast, for gangs: how many copies of a whole gang the throttles admit at each instant
// (kt_kernels_headroom_forecast_gangs.hip)
// ---------------------------------------------------------------------------------------------------
// forecast_gangs_locked's sequence with kt_headroom_forecast_gangs in kt_forecast_gangs' place: the refusals in its order (cap and
// want behind the instants, as the headroom forecast), the |request| sums probe, and behind it the last refusal — the search over
// the copies takes sums that only grow; then ONE check, the dry aggregate and finalize at t_0, the kernel.  The result shares the
// one pending forecast result as its fourth kind.  The caller holds the launch lock.
static int32_t headroom_forecast_gangs_locked(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off,
                                              int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, int64_t cap,
                                              int64_t want, void* stream) {
  const char *what = "headroom forecast gangs", *kernel = "kt_headroom_forecast_gangs";
  const int32_t T = e->thr_rows_hi;  // (moved by throttle batches only, under this lock: ensure_ready below does not change it)
  int32_t rc;
  if ((rc = forecast_instants_valid(e, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = cap_in_range(e, what, cap)) != KT_OK) return rc;
  if ((rc = want_in_range(e, what, want, cap)) != KT_OK) return rc;
  if ((rc = gangs_valid(e, n, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = rows_in_range(e, what, n, pod_rows)) != KT_OK) return rc;
  if ((rc = matrix_fits(e, what, T, n)) != KT_OK || (rc = verdicts_fit(e, what, n_gangs, n_inst, "n_gangs", "results")) != KT_OK) return rc;
  if ((rc = serves_dry_reconcile(e, what, -1, kernel)) != KT_OK) return rc;
  if (n == 0) {  // (no gangs) nothing is launched
    e->forecast_ready = true, e->forecast_kind = kForecastHeadroomGangs, e->forecast_n = 0, e->forecast_m = n_inst;
    return KT_OK;
  }
  KT_HIP(e, hipSetDevice(e->device));
  hipStream_t s = pick_stream(e, stream);
  if ((rc = ensure_ready(e, s)) != KT_OK || (rc = sums_fit_int64(e, what, -1, kernel, s)) != KT_OK) return rc;
  if ((rc = sums_only_grow(e, what, -1, "kt_headroom_forecast_launch")) != KT_OK) return rc;
  e->forecast_ready = false;
  const size_t ng = (size_t)n_gangs, m = (size_t)n_inst, cells = ng * m;
  if ((rc = reserve_behind_last_stream(e, {{e->d_forecast_first, ng}, {e->d_forecast_copies, cells}, {e->d_forecast_limiting, cells}, {e->d_forecast_blocker, cells}, {e->d_forecast_inst_s, m}, {e->d_forecast_inst_ns, m}, {e->d_forecast_gang_off, ng + 1}})) != KT_OK)
    return rc;
  // the instants and the offsets travel on the launch's stream, behind an earlier forecast's kernel; the caller's memory is not
  // referenced after return
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_s.p, inst_s, m * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_inst_ns.p, inst_ns, m * 4, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipMemcpyAsync(e->d_forecast_gang_off.p, gang_off, (ng + 1) * 8, hipMemcpyHostToDevice, s));
  KT_HIP(e, hipStreamSynchronize(s));
  if ((rc = query_check(e, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return rc;  // over the members of all gangs
  // the aggregate with exact contributor counts and the error bytes; the dry finalize runs at t_0
  if ((rc = preempt_reconcile_locked(e, inst_s[0], inst_ns[0], s)) != KT_OK) return rc;
  kt::launch_headroom_forecast_gangs(admit_page_of(e), n_gangs, n_inst, e->d_rows.p, e->d_forecast_gang_off.p, e->d_forecast_inst_s.p,
                                     e->d_forecast_inst_ns.p, T, on_equal != 0, (uint32_t)cap, (uint32_t)want, e->d_status.p, e->d_summary.p,
                                     e->d_preempt_partial.p, e->d_out_error.p, e->d_forecast_first.p, e->d_forecast_copies.p,
                                     e->d_forecast_limiting.p, e->d_forecast_blocker.p, s);
  KT_HIP(e, hipGetLastError());
  e->last_stream = s;
  e->forecast_ready = true, e->forecast_kind = kForecastHeadroomGangs, e->forecast_n = n_gangs, e->forecast_m = n_inst;
  return KT_OK;
}

int32_t kt_headroom_forecast_gangs_launch(kt_engine* e, int64_t n, const int64_t* pod_rows, int64_t n_gangs, const int64_t* gang_off, int64_t n_inst,
                                          const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, int64_t cap, int64_t want, void* stream) {
  if (!e || n < 0 || n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  return headroom_forecast_gangs_locked(e, n, pod_rows, n_gangs, gang_off, n_inst, inst_s, inst_ns, on_equal, cap, want, stream);
}

int32_t kt_headroom_forecast_gangs_fetch(kt_engine* e, int64_t n_gangs, int64_t* out_first, int64_t* out_copies, int32_t* out_limiting,
                                         int64_t* out_blocker) {
  if (!e) return KT_ERR_INVALID_ARGUMENT;
  LaunchLock lk(e);
  KT_HIP(e, hipSetDevice(e->device));
  if (int32_t bad = fetch_ready(e, e->forecast_ready && e->forecast_kind == kForecastHeadroomGangs, "headroom_forecast_gangs", "headroom forecast gangs",
                                true, n_gangs, e->forecast_n))
    return bad;
  if (n_gangs == 0) return KT_OK;
  const size_t ng = (size_t)n_gangs, cells = ng * (size_t)e->forecast_m;
  return fetch_out(e, {{out_first, e->d_forecast_first.p, ng * 8}, {out_copies, e->d_forecast_copies.p, cells * 8}, {out_limiting, e->d_forecast_limiting.p, cells * 4}, {out_blocker, e->d_forecast_blocker.p, cells * 8}});
}

// ---------------------------------------------------------------------------------------------------
// forecast over pages: kt_forecast_launch + kt_forecast_fetch on the cluster of all names (kt_kernels_forecast_paged.hip)
// ---------------------------------------------------------------------------------------------------
int32_t kt_paged_forecast(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_inst, const int64_t* inst_s,
                          const int32_t* inst_ns, int32_t on_equal, int64_t* out_first, uint8_t* out_verdicts) {
  PagedCall c{"paged forecast", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  const char *what = "forecast", *kernel = "kt_forecast_paged";
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if ((rc = forecast_instants_valid(e0, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((rc = matrix_fits(e0, what, T, n)) != KT_OK || (rc = verdicts_fit(e0, what, n, n_inst)) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k)
    if ((rc = serves_dry_reconcile(pages[k], what, k, kernel)) != KT_OK) return rc;
  if (n == 0) return KT_OK;  // nothing is launched
  if ((rc = c.order()) != KT_OK || (rc = ensure_ready(e0, c.s)) != KT_OK) return rc;
  hipStream_t s = c.s;
  for (int32_t k = 0; k < n_pages; ++k)  // (before the check slot, a reconcile report or a result buffer of any page is touched)
    if ((rc = sums_fit_int64(pages[k], what, k, kernel, s)) != KT_OK) return rc;
  // ---- from here on the call owns page 0's check slot and forecast result and every page's reconcile report
  e0->forecast_ready = false, e0->forecast_kind = kForecastPods;
  if ((rc = c.take_preempt_pages()) != KT_OK) return rc;
  const size_t ver = (size_t)n * (size_t)n_inst, m = (size_t)n_inst;
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_forecast_first, (size_t)n}, {e0->d_forecast_verdicts, ver + 1}, {e0->d_forecast_inst_s, m}, {e0->d_forecast_inst_ns, m}})) != KT_OK)
    return rc;
  // the instants travel on the same stream, behind an earlier forecast's kernel (the call returns behind finish: the caller's
  // memory is not referenced afterwards)
  if ((rc = c.in(e0->d_forecast_inst_s.p, inst_s, m * 8)) != KT_OK || (rc = c.in(e0->d_forecast_inst_ns.p, inst_ns, m * 4)) != KT_OK) return rc;
  if ((rc = query_check(e0, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return c.finish(rc);
  if ((rc = reconcile_pages(c, inst_s[0], inst_ns[0])) != KT_OK) return rc;  // (the dry finalize runs at t_0)
  hipError_t herr = hipSuccess;
  if (!kt::launch_forecast_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n, n_inst,
                                 e0->d_rows.p, e0->d_forecast_inst_s.p, e0->d_forecast_inst_ns.p, T, on_equal != 0, e0->d_status.p,
                                 e0->d_summary.p, e0->d_forecast_first.p, e0->d_forecast_verdicts.p, s, &herr))
    return c.device_error(herr, "copy of the page descriptors: ");
  if ((rc = c.launched()) != KT_OK) return rc;
  e0->last_stream = s;
  if ((rc = c.out(out_first, e0->d_forecast_first.p, (size_t)n * 8)) != KT_OK || (rc = c.out(out_verdicts, e0->d_forecast_verdicts.p, ver)) != KT_OK) return rc;
  return c.finish(KT_OK);  // (synchronises s; the results have been handed out: no forecast result is pending on page 0)
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
  PagedCall c{"paged forecast gangs", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  const char *what = "forecast gangs", *kernel = "kt_forecast_gangs_paged";
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if ((rc = forecast_instants_valid(e0, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = gangs_valid(e0, n, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e0, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((rc = matrix_fits(e0, what, T, n)) != KT_OK || (rc = verdicts_fit(e0, what, n_gangs, n_inst, "n_gangs")) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k)
    if ((rc = serves_dry_reconcile(pages[k], what, k, kernel)) != KT_OK) return rc;
  if (n == 0) return KT_OK;  // (no gangs) nothing is launched
  if ((rc = c.order()) != KT_OK || (rc = ensure_ready(e0, c.s)) != KT_OK) return rc;
  hipStream_t s = c.s;
  for (int32_t k = 0; k < n_pages; ++k)  // (before the check slot, a reconcile report or a result buffer of any page is touched)
    if ((rc = sums_fit_int64(pages[k], what, k, kernel, s)) != KT_OK) return rc;
  // ---- from here on the call owns page 0's check slot and forecast result and every page's reconcile report
  e0->forecast_ready = false, e0->forecast_kind = kForecastPods;
  if ((rc = c.take_preempt_pages()) != KT_OK) return rc;
  const size_t ng = (size_t)n_gangs, m = (size_t)n_inst, ver = ng * m;
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_forecast_first, ng}, {e0->d_forecast_verdicts, ver + 1}, {e0->d_forecast_blocker, ver}, {e0->d_forecast_inst_s, m}, {e0->d_forecast_inst_ns, m}, {e0->d_forecast_gang_off, ng + 1}})) != KT_OK)
    return rc;
  // the instants and the offsets travel on the same stream, behind an earlier forecast's kernel (the call returns behind finish:
  // the caller's memory is not referenced afterwards)
  if ((rc = c.in(e0->d_forecast_inst_s.p, inst_s, m * 8)) != KT_OK || (rc = c.in(e0->d_forecast_inst_ns.p, inst_ns, m * 4)) != KT_OK ||
      (rc = c.in(e0->d_forecast_gang_off.p, gang_off, (ng + 1) * 8)) != KT_OK)
    return rc;
  if ((rc = query_check(e0, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return c.finish(rc);  // over the members of all gangs
  if ((rc = reconcile_pages(c, inst_s[0], inst_ns[0])) != KT_OK) return rc;  // (the dry finalize runs at t_0)
  hipError_t herr = hipSuccess;
  if (!kt::launch_forecast_gangs_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n_gangs,
                                       n_inst, e0->d_rows.p, e0->d_forecast_gang_off.p, e0->d_forecast_inst_s.p, e0->d_forecast_inst_ns.p, T,
                                       on_equal != 0, e0->d_status.p, e0->d_summary.p, e0->d_forecast_first.p, e0->d_forecast_verdicts.p,
                                       e0->d_forecast_blocker.p, s, &herr))
    return c.device_error(herr, "copy of the page descriptors: ");
  if ((rc = c.launched()) != KT_OK) return rc;
  e0->last_stream = s;
  if ((rc = c.out(out_first, e0->d_forecast_first.p, ng * 8)) != KT_OK || (rc = c.out(out_verdicts, e0->d_forecast_verdicts.p, ver)) != KT_OK ||
      (rc = c.out(out_blocker, e0->d_forecast_blocker.p, ver * 8)) != KT_OK)
    return rc;
  return c.finish(KT_OK);  // (synchronises s; the results have been handed out: no forecast result of either kind is pending on page 0)
}

// ---------------------------------------------------------------------------------------------------
// headroom forecast over pages: kt_headroom_forecast_launch + kt_headroom_forecast_fetch on the cluster of all names
// (kt_kernels_headroom_forecast_paged.hip)
// ---------------------------------------------------------------------------------------------------
// kt_paged_forecast's body with cap and want behind the instants, as headroom_forecast_locked orders them, and the copies and
// limiting rows in the verdict bytes' place.
int32_t kt_paged_headroom_forecast(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_inst,
                                   const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal, int64_t cap, int64_t want,
                                   int64_t* out_first, int64_t* out_copies, int32_t* out_limiting) {
  PagedCall c{"paged headroom forecast", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  const char *what = "headroom forecast", *kernel = "kt_headroom_forecast_paged";
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if ((rc = forecast_instants_valid(e0, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = cap_in_range(e0, c.what, cap)) != KT_OK || (rc = want_in_range(e0, c.what, want, cap)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((rc = matrix_fits(e0, what, T, n)) != KT_OK || (rc = verdicts_fit(e0, what, n, n_inst, "n", "results")) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k)
    if ((rc = serves_dry_reconcile(pages[k], what, k, kernel)) != KT_OK) return rc;
  if (n == 0) return KT_OK;  // nothing is launched
  if ((rc = c.order()) != KT_OK || (rc = ensure_ready(e0, c.s)) != KT_OK) return rc;
  hipStream_t s = c.s;
  for (int32_t k = 0; k < n_pages; ++k)  // (before the check slot, a reconcile report or a result buffer of any page is touched)
    if ((rc = sums_fit_int64(pages[k], what, k, kernel, s)) != KT_OK) return rc;
  // ---- from here on the call owns page 0's check slot and forecast result and every page's reconcile report
  e0->forecast_ready = false, e0->forecast_kind = kForecastPods;
  if ((rc = c.take_preempt_pages()) != KT_OK) return rc;
  const size_t cells = (size_t)n * (size_t)n_inst, m = (size_t)n_inst;
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_forecast_first, (size_t)n}, {e0->d_forecast_copies, cells}, {e0->d_forecast_limiting, cells}, {e0->d_forecast_inst_s, m}, {e0->d_forecast_inst_ns, m}})) != KT_OK)
    return rc;
  // the instants travel on the same stream, behind an earlier forecast's kernel (the call returns behind finish: the caller's
  // memory is not referenced afterwards)
  if ((rc = c.in(e0->d_forecast_inst_s.p, inst_s, m * 8)) != KT_OK || (rc = c.in(e0->d_forecast_inst_ns.p, inst_ns, m * 4)) != KT_OK) return rc;
  if ((rc = query_check(e0, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return c.finish(rc);
  if ((rc = reconcile_pages(c, inst_s[0], inst_ns[0])) != KT_OK) return rc;  // (the dry finalize runs at t_0)
  hipError_t herr = hipSuccess;
  if (!kt::launch_headroom_forecast_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev, n, n_inst,
                                          e0->d_rows.p, e0->d_forecast_inst_s.p, e0->d_forecast_inst_ns.p, T, on_equal != 0, (uint32_t)cap,
                                          (uint32_t)want, e0->d_status.p, e0->d_summary.p, e0->d_forecast_first.p, e0->d_forecast_copies.p,
                                          e0->d_forecast_limiting.p, s, &herr))
    return c.device_error(herr, "copy of the page descriptors: ");
  if ((rc = c.launched()) != KT_OK) return rc;
  e0->last_stream = s;
  if ((rc = c.out(out_first, e0->d_forecast_first.p, (size_t)n * 8)) != KT_OK || (rc = c.out(out_copies, e0->d_forecast_copies.p, cells * 8)) != KT_OK ||
      (rc = c.out(out_limiting, e0->d_forecast_limiting.p, cells * 4)) != KT_OK)
    return rc;
  return c.finish(KT_OK);  // (synchronises s; the results have been handed out: no forecast result of any kind is pending on page 0)
}

// ---------------------------------------------------------------------------------------------------
// headroom forecast for gangs over pages: kt_headroom_forecast_gangs_launch + kt_headroom_forecast_gangs_fetch on the cluster of
// all names (kt_kernels_headroom_forecast_gangs_paged.hip)
// ---------------------------------------------------------------------------------------------------
// kt_paged_forecast_gangs' body with cap and want behind the instants, as headroom_forecast_gangs_locked orders them, the last
// refusal of that call asked of every page, and the copies, limiting rows and blockers in the verdict bytes' place.
int32_t kt_paged_headroom_forecast_gangs(kt_engine* const* pages, int32_t n_pages, int64_t n, const int64_t* pod_rows, int64_t n_gangs,
                                         const int64_t* gang_off, int64_t n_inst, const int64_t* inst_s, const int32_t* inst_ns, int32_t on_equal,
                                         int64_t cap, int64_t want, int64_t* out_first, int64_t* out_copies, int32_t* out_limiting,
                                         int64_t* out_blocker) {
  if (n_gangs < 0) return KT_ERR_INVALID_ARGUMENT;
  PagedCall c{"paged headroom forecast gangs", pages, n_pages};
  int32_t rc = c.lock(n);
  if (rc != KT_OK) return rc;
  kt_engine* e0 = c.e0;
  const char *what = "headroom forecast gangs", *kernel = "kt_headroom_forecast_gangs_paged";
  // ---- refusals: nothing is launched and no slot of any page is touched before the last of them
  if ((rc = forecast_instants_valid(e0, n > 0 && !pod_rows, n_inst, inst_s, inst_ns)) != KT_OK) return rc;
  if ((rc = cap_in_range(e0, c.what, cap)) != KT_OK || (rc = want_in_range(e0, c.what, want, cap)) != KT_OK) return rc;
  if ((rc = gangs_valid(e0, n, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = no_row_twice_in_a_gang(e0, what, pod_rows, n_gangs, gang_off)) != KT_OK) return rc;
  if ((rc = c.same_cluster(n, pod_rows)) != KT_OK) return rc;  // (the rows are range-checked in place)
  const int32_t T = e0->thr_rows_hi;
  if ((rc = matrix_fits(e0, what, T, n)) != KT_OK || (rc = verdicts_fit(e0, what, n_gangs, n_inst, "n_gangs", "results")) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k)
    if ((rc = serves_dry_reconcile(pages[k], what, k, kernel)) != KT_OK) return rc;
  if (n == 0) return KT_OK;  // (no gangs) nothing is launched
  if ((rc = c.order()) != KT_OK || (rc = ensure_ready(e0, c.s)) != KT_OK) return rc;
  hipStream_t s = c.s;
  for (int32_t k = 0; k < n_pages; ++k)  // (before the check slot, a reconcile report or a result buffer of any page is touched)
    if ((rc = sums_fit_int64(pages[k], what, k, kernel, s)) != KT_OK) return rc;
  for (int32_t k = 0; k < n_pages; ++k)  // the search over the copies takes sums that only grow, on every page
    if ((rc = sums_only_grow(pages[k], what, k, "kt_paged_headroom_forecast")) != KT_OK) return rc;
  // ---- from here on the call owns page 0's check slot and forecast result and every page's reconcile report
  e0->forecast_ready = false, e0->forecast_kind = kForecastPods;
  if ((rc = c.take_preempt_pages()) != KT_OK) return rc;
  const size_t ng = (size_t)n_gangs, m = (size_t)n_inst, cells = ng * m;
  if ((rc = reserve_behind_last_stream(e0, {{e0->d_forecast_first, ng}, {e0->d_forecast_copies, cells}, {e0->d_forecast_limiting, cells}, {e0->d_forecast_blocker, cells}, {e0->d_forecast_inst_s, m}, {e0->d_forecast_inst_ns, m}, {e0->d_forecast_gang_off, ng + 1}})) != KT_OK)
    return rc;
  // the instants and the offsets travel on the same stream, behind an earlier forecast's kernel (the call returns behind finish:
  // the caller's memory is not referenced afterwards)
  if ((rc = c.in(e0->d_forecast_inst_s.p, inst_s, m * 8)) != KT_OK || (rc = c.in(e0->d_forecast_inst_ns.p, inst_ns, m * 4)) != KT_OK ||
      (rc = c.in(e0->d_forecast_gang_off.p, gang_off, (ng + 1) * 8)) != KT_OK)
    return rc;
  if ((rc = query_check(e0, n, pod_rows, on_equal, s, &kt_engine::preempt_ready)) != KT_OK) return c.finish(rc);  // over the members of all gangs
  if ((rc = reconcile_pages(c, inst_s[0], inst_ns[0])) != KT_OK) return rc;  // (the dry finalize runs at t_0)
  hipError_t herr = hipSuccess;
  if (!kt::launch_headroom_forecast_gangs_paged(e0->h_preempt_pages.data(), n_pages, (kt::PreemptPage*)e0->d_preempt_pages.p, e0->preempt_pages_ev,
                                                n_gangs, n_inst, e0->d_rows.p, e0->d_forecast_gang_off.p, e0->d_forecast_inst_s.p,
                                                e0->d_forecast_inst_ns.p, T, on_equal != 0, (uint32_t)cap, (uint32_t)want, e0->d_status.p,
                                                e0->d_summary.p, e0->d_forecast_first.p, e0->d_forecast_copies.p, e0->d_forecast_limiting.p,
                                                e0->d_forecast_blocker.p, s, &herr))
    return c.device_error(herr, "copy of the page descriptors: ");
  if ((rc = c.launched()) != KT_OK) return rc;
  e0->last_stream = s;
  if ((rc = c.out(out_first, e0->d_forecast_first.p, ng * 8)) != KT_OK || (rc = c.out(out_copies, e0->d_forecast_copies.p, cells * 8)) != KT_OK ||
      (rc = c.out(out_limiting, e0->d_forecast_limiting.p, cells * 4)) != KT_OK || (rc = c.out(out_blocker, e0->d_forecast_blocker.p, cells * 8)) != KT_OK)
    return rc;
  return c.finish(KT_OK);  // (synchronises s; the results have been handed out: no forecast result of any kind is pending on page 0)
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
