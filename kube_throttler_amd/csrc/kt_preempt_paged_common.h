// kt_preempt_paged_common.h — what the preemption kernels over PAGES share (kt_kernels_preempt_paged.hip: kt_preempt_paged,
// kt_preempt_reprieve_paged; kt_kernels_preempt_gangs_paged.hip: kt_preempt_gangs_paged, kt_preempt_gangs_reprieve_paged), gfx950:
// the arguments of the prefix and of the reprieve kernel, a page seen through kt_preempt's helpers, the facts that hold for a
// throttle as a whole (the OR over the pages), and the reprieve list over the flat name index, counted and gathered, generic in
// whose matrix rows are listed.  And what the gang kernels over pages share: a page as gang_walk sees it, the names a gang requests
// of a page, and — for the two gang forecasts — the throttle's state on one page and CalculateThreshold at a lane's instant.
#pragma once
#include "kt_admit_common.h"

namespace kt {

struct PreemptPagedArgs {
  const PreemptPage* pages;  // [n_pages] in device memory
  int32_t n_pages;
  const int64_t* rows;       // [n + m] pod table rows (the same in every page): the preemptors, then the candidates
  int64_t n, m;
  const uint8_t* status;     // [n + m][T] page 0's check
  const uint64_t* summary;   // [n + m]
  int64_t* prefix;           // [n] out
  uint8_t* victims;          // [n][m] out (and the per-position verdict bits while the kernel runs)
  int32_t T, on_equal;
};

// what kt_preempt's helpers read, for page k
__device__ __forceinline__ PreemptArgs preempt_page_args(const PreemptPagedArgs& a, int k) {
  const PreemptPage pp = preempt_page(a.pages, k);
  PreemptArgs r;
  r.pg = pp.pg, r.rows = a.rows, r.n = a.n, r.m = a.m, r.status = a.status, r.summary = a.summary, r.partial = pp.partial, r.calc = pp.calc;
  r.calc_updated = pp.calc_updated, r.error = pp.error, r.prefix = a.prefix, r.victims = a.victims, r.T = a.T, r.on_equal = a.on_equal;
  return r;
}

// the facts of throttle t that hold for the throttle as a whole: the OR over the pages
__device__ __forceinline__ void paged_thr_facts(const PreemptPage* pages, int n_pages, uint32_t t, bool* stored, bool* use_calc) {
  bool st = false, uc = false;
  for (int k = 0; k < n_pages; ++k) {
    const PreemptPage pp = preempt_page(pages, k);
    const uint32_t tf = pp.pg.tt.flags[t];
    st |= preempt_row_stored(tf, pp.error[t]);
    uc |= (tf & kThrCalcAtNonzero) != 0 || pp.calc_updated[t] != 0;
  }
  *stored = st, *use_calc = uc;
}

// ---- what the gang kernels over pages share (kt_kernels_preempt_gangs_paged.hip, kt_kernels_forecast_gangs_paged.hip) ------------------
// what gang_walk reads of one page
struct GangPageView {
  AdmitPage pg;
  const int64_t* rows;
  const uint8_t* status;
  int32_t T;
};

// the names of page `pg` some member of [i0, i1) that throttle t affects requests with a non-zero value (wave-uniform loads)
__device__ __forceinline__ uint32_t gang_page_requested(const AdmitPage& pg, const int64_t* rows, const uint8_t* status, int T, uint32_t t, int64_t i0,
                                                        int64_t i1) {
  uint32_t need = 0;
  for (int64_t i = i0; i < i1; ++i) {
    if (status[i * (int64_t)T + t] == 0) continue;
    const int64_t p = rows[i];
    for (int d = 0; d < pg.D; ++d) need |= pg.req[p * pg.DS + d] != 0 ? 1u << d : 0u;
  }
  return need;
}

// ---- what the gang forecasts over pages share (kt_kernels_forecast_gangs_paged.hip, kt_kernels_headroom_forecast_gangs_paged.hip) ----
// what does not depend on the instant of throttle t on one page: one batch of wave-uniform loads
template <int DT>
struct ForecastPageThr {
  uint32_t ovr0, ovr1, s_p, k_p, names;  // names: those some threshold of the throttle can name on this page
  bool fp_differs, spec_diff;            // the messages fingerprint differs; spec against the stored calculated threshold, by value
  int64_t sv[DT], kv[DT];
};

template <int DT>
__device__ __forceinline__ ForecastPageThr<DT> forecast_page_thr(const ThrTables& tt, int D, uint32_t t) {
  ForecastPageThr<DT> r;
  r.ovr0 = tt.ovr_off[t], r.ovr1 = tt.ovr_off[t + 1];
  const uint64_t status_fp = tt.status_msgs_fp[t], spec_fp = tt.spec_msgs_fp[t];
  r.s_p = tt.spec.present[t], r.k_p = tt.calc.present[t];
  // whether an override has a parse error (the messages of CalculateThreshold: they do not depend on the instant)
  r.names = r.s_p | r.k_p;
  bool any_err = false;
  for (uint32_t o = r.ovr0; o < r.ovr1; ++o) {
    if (tt.ovr_flags[o] & kOvrParseError) any_err = true;
    else r.names |= tt.ovr_thr.present[o];
  }
  r.fp_differs = status_fp != (any_err ? spec_fp : 0ull);
  r.spec_diff = false;
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    r.sv[d] = r.kv[d] = 0;
    if (d >= D) continue;
    r.sv[d] = tt.spec.v[(size_t)t * D + d], r.kv[d] = tt.calc.v[(size_t)t * D + d];
    r.spec_diff |= ((r.s_p >> d) & 1u) && r.sv[d] != r.kv[d];
  }
  return r;
}

// CalculateThreshold of the throttle on one page at the lane's instant: first active override wins, per name and for the count;
// no active override: spec.threshold, otherwise the merged override REPLACES it.  *diff: it differs by value from the stored
// calculated threshold over the names it has.  The whole wave arrives (one ballot per override).
template <int DT>
__device__ __forceinline__ void forecast_page_calc(const ThrTables& tt, int D, uint32_t t, const ForecastPageThr<DT>& pt, int64_t ts, int32_t tn,
                                                   bool* c_hc_out, int64_t* c_c_out, uint32_t* c_p_out, int64_t (&c_v)[DT], bool* diff_out) {
  bool active_found = false, c_hc = false, diff = false;
  int64_t c_c = 0;
  uint32_t c_p = 0;
#pragma unroll
  for (int d = 0; d < DT; ++d) c_v[d] = 0;
  for (uint32_t o = pt.ovr0; o < pt.ovr1; ++o) {
    // one batch of loads per override (wave-uniform)
    const uint8_t of = tt.ovr_flags[o];
    const int64_t ob_s = tt.ovr_begin_s[o], oe_s = tt.ovr_end_s[o];
    const int32_t ob_ns = tt.ovr_begin_ns[o], oe_ns = tt.ovr_end_ns[o];
    const bool o_hc = tt.ovr_thr.has_count[o] != 0;
    const int64_t o_c = tt.ovr_thr.count[o];
    const uint32_t op = tt.ovr_thr.present[o];
    if (of & kOvrParseError) continue;
    const bool end_zero = oe_s == kZeroTimeS && oe_ns == 0;
    const bool active = forecast_le(ob_s, ob_ns, ts, tn) && (end_zero || forecast_le(ts, tn, oe_s, oe_ns));
    if (__ballot(active) == 0ull) continue;
    active_found |= active;
    if (active && !c_hc && o_hc) c_hc = true, c_c = o_c;
    const uint32_t take = active ? op & ~c_p : 0u;  // the names this override decides at this lane's instant
    c_p |= take;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      if (d >= D || !((op >> d) & 1u)) continue;  // (wave-uniform)
      const int64_t o_v = tt.ovr_thr.v[(size_t)o * D + d];
      if ((take >> d) & 1u) {
        diff |= o_v != pt.kv[d];
        c_v[d] = o_v;
      }
    }
  }
  if (!active_found) {
    c_p = pt.s_p, c_hc = tt.spec.has_count[t] != 0, c_c = tt.spec.count[t], diff = pt.spec_diff;
#pragma unroll
    for (int d = 0; d < DT; ++d) c_v[d] = pt.sv[d];
  }
  *c_hc_out = c_hc, *c_c_out = c_c, *c_p_out = c_p, *diff_out = diff;
}

// ---- the reprieve pass -------------------------------------------------------------------------------------------------------
struct ReprievePagedArgs {
  const PreemptPage* pages;  // [n_pages] in device memory, as the prefix kernel read them
  int32_t n_pages, F;        // F: the flat name count, the sum of the pages' D
  const int64_t* rows;       // [n + m]
  int64_t n, m;
  const uint8_t* status;     // [n + m][T]
  const int64_t* prefix;     // [n] ([n_gangs]) as the prefix kernel left it
  uint8_t* victims;          // [n][m] ([n_gangs][m]) in: the prefix mask, out: the reprieved set
  unsigned char* ws;         // gridDim.x slots of ws_slot bytes (nullptr: T <= lds_cap)
  size_t ws_slot;
  int32_t T, on_equal;
  uint32_t lds_cap;          // entries the LDS state holds
};

constexpr uint32_t kPagedUseCalc = 0x80000000u;  // bit 31 of a list entry's throttle row: it reads the calculated threshold

// The affecting throttles that are reconciled on every page — chunk(c0, list, &err) appends one chunk of the matrix row (of the
// union of the members' rows) to the chunk list: counted (GATHER = false) or gathered into the state with every page's totals;
// returns the wave-uniform list length
template <int DT, bool GATHER, class ST, class CHUNK>
__device__ __forceinline__ uint32_t reprieve_paged_list(const ReprievePagedArgs& a, const CHUNK& chunk, lds_u32wp list, ST* st, uint32_t lane) {
  const int T = a.T;
  uint32_t n_list = 0;
  for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
    bool err_c = false;  // (prefix > 0: the row holds no error byte)
    const uint32_t n_c = chunk(c0, list, &err_c);
    __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
    for (uint32_t a0 = 0; a0 < n_c; a0 += kWave) {
      const uint32_t ai = a0 + lane;
      const uint32_t t = ai < n_c ? list[ai] : 0u;
      bool stored = false, use_calc = false;
      if (ai < n_c) paged_thr_facts(a.pages, a.n_pages, t, &stored, &use_calc);
      const bool keep = ai < n_c && !stored;
      const uint64_t mk = __ballot(keep);
      if constexpr (GATHER) {
        const uint32_t e = n_list + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (keep && e < st->cap) {
          st->tl[e] = t | (use_calc ? kPagedUseCalc : 0u);
          uint32_t fb = 0;  // the page's first flat name
          for (int k = 0; k < a.n_pages; ++k) {
            const PreemptPage pp = preempt_page(a.pages, k);
            const int D = pp.pg.D;
            const unsigned long long* prow = pp.partial + (size_t)t * partial_stride(D);
            if (k == 0) st->pods[e] = (int64_t)prow[partial_off_pods(D)];
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d >= D) continue;
              st->uv[(size_t)(fb + d) * st->cap + e] = (int64_t)prow[d];
              st->uc[(size_t)(fb + d) * st->cap + e] = (uint32_t)prow[partial_off_presence(D) + d];
            }
            fb += (uint32_t)D;
          }
        }
      }
      n_list += (uint32_t)__popcll(mk);
    }
    __syncthreads();  // the next chunk rewrites the chunk list
  }
  return n_list;
}

// the flat name count F of a page set (host side)
inline int preempt_paged_names(const PreemptPage* pages, int n_pages) {
  int F = 0;
  for (int k = 0; k < n_pages; ++k) F += pages[k].pg.D;
  return F > 0 ? F : 1;
}

}  // namespace kt
