// kt_preempt_paged_common.h — what the preemption kernels over PAGES share (kt_kernels_preempt_paged.hip: kt_preempt_paged,
// kt_preempt_reprieve_paged; kt_kernels_preempt_gangs_paged.hip: kt_preempt_gangs_paged, kt_preempt_gangs_reprieve_paged), gfx950:
// the arguments of the prefix and of the reprieve kernel, a page seen through kt_preempt's helpers, the facts that hold for a
// throttle as a whole (the OR over the pages), and the reprieve list over the flat name index, counted and gathered, generic in
// whose matrix rows are listed.
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
