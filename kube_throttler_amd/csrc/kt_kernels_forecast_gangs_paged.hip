// kt_kernels_forecast_gangs_paged.hip — the first instant at which a whole gang is admitted, over PAGES of resource names
// (kt_paged_forecast_gangs), gfx950.
//
// The definition is kt_kernels_forecast_gangs.hip's on the cluster of all names; a page is an engine of <= 16 names that holds
// every pod row and every throttle row (kt_engine.h, "PAGES").  Two things keep the answer from being put together out of the
// existing calls: an admitted member reserves against the throttles the later members meet (the members' own paged forecasts do
// not compose), and status.calculatedThreshold is compared and replaced AS A WHOLE, so whether a throttle reads its calculated
// threshold or spec.threshold at instant t is ONE fact for all pages that changes from instant to instant (the pages' own gang
// forecasts do not compose either).
//
// kt_forecast_gangs_paged<DT> (DT: the bucket of the widest page): kt_forecast_gangs (one wave per gang, the grid strides, lane =
// instant position, 64 instants per block) crossed with kt_forecast_paged (the whole-throttle facts as an OR over the pages), the
// member walk page by page as kt_preempt_gangs_paged does it.
//   per gang      the first member whose PreFilter is an error (page 0's summary) or whose row is invalid (page 0's pod_flags) by a
//                 ballot over member blocks of 64; the UNION of the members' affecting throttles chunk by chunk through the 4 KiB
//                 LDS list, from page 0's matrix.
//   per throttle  stored (preempt_row_stored on some page) and calc_at_any (calculatedAt set on some page), wave-uniform.
//     a stored throttle is walked once per page, wave-uniform: that page's stored `used`, throttled flags and reserved row against
//       tt.calc where calc_at_any holds and tt.spec otherwise.  The pod count is page 0's: the other pages hand gang_walk a
//       threshold that does not name the count and a count flag of false (kt_preempt_gangs_paged's way; gang_walk is untouched).
//       The minimum first stopped position over the pages holds at every instant.
//     otherwise, per block of 64 instants, TWO passes over the pages:
//       1. `differs`, the lane's own: each page's CalculateThreshold at the lane's instant differs by value from that page's
//          stored one over its names, or that page's messages fingerprint differs; page 0 adds the comparison of the count.  EVERY
//          page takes part, also one none of whose names any member requests: it can replace the threshold for all the others.
//          Only the overrides are walked: wave-uniform loads.  The pass is skipped where calc_at_any holds (wave-uniform).
//       2. reads_calc = calc_at_any || differs.  Per page the overrides again, then GangThr from the calculated threshold if
//          reads_calc, else from spec; GangUsed from the fresh sums of that page's partial row; the throttled bits by IsThrottled
//          against the CALCULATED threshold either way; the count part on page 0 only; ONE gang_walk over that page's view.  A page
//          k != 0 is skipped here when no affected member requests a name of it that some threshold of the throttle on that page
//          can name.  gang_walk reloads the member rows through dependent trips and is the expensive part: it runs once per page
//          and block, not once per threshold candidate.
//     The lane keeps the minimum first stopped position over throttles and pages in its own blocker word, as kt_forecast_gangs.
//   output        kt_forecast_gangs': verdicts[g][k], blocker[g][k] (the first queue position that is not Success at t_k, -1:
//                 none), first[g] (ballot over the blocks in order).  With one page the kernel computes what kt_forecast_gangs
//                 computes.
// Every __ballot, __syncthreads and readfirstlane sits where the whole wave arrives: the loops over chunks, throttles, pages,
// blocks, overrides and members are wave-uniform.
#include "kt_preempt_paged_common.h"

namespace kt {

struct ForecastGangsPagedArgs {
  const PreemptPage* pages;  // [n_pages] in device memory (calc / calc_updated of the dry finalize are not read: every instant is computed)
  int32_t n_pages;
  const int64_t* rows;       // [n] pod table rows (the same in every page): the members of all gangs
  const int64_t* gang_off;   // [n_gangs + 1] queue positions
  int64_t n_gangs, m;        // gangs, instants
  const int64_t* inst_s;     // [m] strictly ascending
  const int32_t* inst_ns;    // [m]
  const uint8_t* status;     // [n][T] page 0's check
  const uint64_t* summary;   // [n]
  int64_t* first;            // [n_gangs] out
  uint8_t* verdicts;         // [n_gangs][m] out
  int64_t* blocker;          // [n_gangs][m] out
  int32_t T, on_equal;
};

template <int DT>
__global__ __launch_bounds__(kWave) void kt_forecast_gangs_paged(const ForecastGangsPagedArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, n_pages = a.n_pages;
  const bool eq = a.on_equal != 0;
  const int64_t m = a.m;
  const uint32_t* pod_flags0 = preempt_page(a.pages, 0).pg.pod_flags;
  for (int64_t gi = blockIdx.x; gi < a.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
    uint8_t* ver = a.verdicts + gi * m;
    int64_t* blk = a.blocker + gi * m;
    // the first member whose PreFilter is an error or whose row is invalid: it is not Success at any instant
    int64_t bad = i1;
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(pod_flags0[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        bad = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    // while the kernel runs blk[q] holds the first stopped position over the throttles and pages so far, i1: none
    for (int64_t q = lane; q < m; q += kWave) ver[q] = 0, blk[q] = bad;
    bool err = bad < i1;
    int64_t stored_first = i1;  // the first member a throttle that keeps its stored status stops: at every instant
    for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      err |= __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        // ---- the facts of the throttle as a whole: the OR over the pages
        bool stored = false, calc_at_any = false;
        for (int k = 0; k < n_pages; ++k) {
          const PreemptPage pp = preempt_page(a.pages, k);
          const uint32_t tf = pp.pg.tt.flags[t];
          stored |= preempt_row_stored(tf, pp.error[t]);
          calc_at_any |= (tf & kThrCalcAtNonzero) != 0;
        }
        if (stored) {  // the stored status of every page: nothing of it depends on the instant
          for (int k = 0; k < n_pages; ++k) {
            const PreemptPage pp = preempt_page(a.pages, k);
            const GangPageView view{pp.pg, a.rows, a.status, T};
            const int D = pp.pg.D;
            const ThrTables& tt = pp.pg.tt;
            const bool first_page = k == 0;
            // (page 0 carries the pod count; elsewhere a page none of whose names an affected member requests stops nobody)
            if (!first_page && gang_page_requested(pp.pg, a.rows, a.status, T, t, i0, i1) == 0u) continue;
            const uint32_t tf = tt.flags[t];
            const AmountTab& th = calc_at_any ? tt.calc : tt.spec;
            GangThr<DT> g;
            g.eq = eq, g.eq3 = admit_eq3(tf, eq);
            // the pod count is page 0's: elsewhere the threshold does not name it
            g.th_hc = first_page && th.has_count[t] != 0, g.th_c = th.count[t], g.th_p = th.present[t];
            g.r_hc = tt.reserved.has_count[t] != 0, g.r_c = tt.reserved.count[t], g.r_p = tt.reserved.present[t];
            GangUsed<DT> u;
            u.c_flag = first_page && (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
            u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              g.tv[d] = g.rv[d] = u.u_v[d] = 0;
              if (d >= D) continue;
              g.tv[d] = th.v[(size_t)t * D + d], g.rv[d] = tt.reserved.v[(size_t)t * D + d], u.u_v[d] = tt.used.v[(size_t)t * D + d];
            }
            const int64_t first = gang_walk<DT>(view, t, i0, i1, g, u);
            stored_first = first < stored_first ? first : stored_first;
          }
          continue;
        }
        for (int64_t q0 = 0; q0 < m; q0 += kWave) {
          const int64_t q = q0 + lane;
          const bool in = q < m;
          const int64_t ts = a.inst_s[in ? q : m - 1];
          const int32_t tn = a.inst_ns[in ? q : m - 1];
          // ---- pass 1: does some page see a threshold (or messages) that differ from what it stores, at the lane's instant
          bool differs = false;
          if (!calc_at_any) {  // (wave-uniform; where calculatedAt is set the calculated threshold is read whatever this says)
            for (int k = 0; k < n_pages; ++k) {
              const PreemptPage pp = preempt_page(a.pages, k);
              const ThrTables& tt = pp.pg.tt;
              const ForecastPageThr<DT> pt = forecast_page_thr<DT>(tt, pp.pg.D, t);
              bool c_hc, diff;
              int64_t c_c, c_v[DT];
              uint32_t c_p;
              forecast_page_calc<DT>(tt, pp.pg.D, t, pt, ts, tn, &c_hc, &c_c, &c_p, c_v, &diff);
              differs |= c_p != pt.k_p || diff || pt.fp_differs;
              if (k == 0) {  // the count: the same in every page, compared once
                const bool k_hc = tt.calc.has_count[t] != 0;
                differs |= c_hc != k_hc || (c_hc && c_c != tt.calc.count[t]);
              }
            }
          }
          // ---- the threshold the check reads behind this reconcile, on every page: calculatedThreshold once calculatedAt is set
          //      or some page replaces it, else spec
          const bool reads_calc = calc_at_any || differs;
          // ---- pass 2: the members on every page
          int64_t lane_first = i1;
          for (int k = 0; k < n_pages; ++k) {
            const PreemptPage pp = preempt_page(a.pages, k);
            const int D = pp.pg.D;
            const ThrTables& tt = pp.pg.tt;
            const bool first_page = k == 0;
            const ForecastPageThr<DT> pt = forecast_page_thr<DT>(tt, D, t);
            // the names some affected member requests and some threshold can name: the others pass every step of every member
            const uint32_t need = gang_page_requested(pp.pg, a.rows, a.status, T, t, i0, i1) & pt.names;
            if (!first_page && need == 0u) continue;  // (wave-uniform; page 0 carries the pod count)
            const uint32_t tf = tt.flags[t];
            bool c_hc, diff;
            int64_t c_c, c_v[DT];
            uint32_t c_p;
            forecast_page_calc<DT>(tt, D, t, pt, ts, tn, &c_hc, &c_c, &c_p, c_v, &diff);
            const unsigned long long* prow = pp.partial + (size_t)t * partial_stride(D);
            const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
            GangThr<DT> g;
            g.eq = eq, g.eq3 = admit_eq3(tf, eq);
            // the pod count is page 0's: elsewhere the threshold does not name it
            g.th_hc = first_page && (reads_calc ? c_hc : tt.spec.has_count[t] != 0);
            g.th_c = reads_calc ? c_c : tt.spec.count[t];
            g.th_p = reads_calc ? c_p : pt.s_p;
            g.r_hc = tt.reserved.has_count[t] != 0, g.r_c = tt.reserved.count[t], g.r_p = tt.reserved.present[t];
            GangUsed<DT> u;
            u.u_hc = pods_total > 0, u.u_c = pods_total;
            // ---- throttled = calculatedThreshold.IsThrottled(used, true): the lane's own flag bits
            u.c_flag = first_page && c_hc && u.u_hc && pods_total >= c_c;
            u.flag_m = u.pr_m = 0u;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              g.tv[d] = g.rv[d] = u.u_v[d] = 0;
              if (d >= D) continue;
              g.tv[d] = reads_calc ? c_v[d] : pt.sv[d];
              g.rv[d] = tt.reserved.v[(size_t)t * D + d];  // (every name: Reserve adds to it whoever reads it)
              if (!((need >> d) & 1u)) continue;          // (wave-uniform)
              u.u_v[d] = (int64_t)prow[d];
              // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
              const bool u_pr = prow[partial_off_presence(D) + d] != 0ull || u.u_v[d] != 0;
              u.pr_m |= u_pr ? 1u << d : 0u;
              if (((c_p >> d) & 1u) && u_pr && u.u_v[d] >= c_v[d]) u.flag_m |= 1u << d;
            }
            const GangPageView view{pp.pg, a.rows, a.status, T};
            const int64_t first = gang_walk<DT>(view, t, i0, i1, g, u);
            lane_first = first < lane_first ? first : lane_first;
          }
          if (in && lane_first < blk[q]) blk[q] = lane_first;  // the lane's own word
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    int64_t ans = -1;
    for (int64_t q0 = 0; q0 < m; q0 += kWave) {
      const int64_t q = q0 + lane;
      bool pass = false;
      if (q < m) {
        int64_t b = blk[q];
        b = stored_first < b ? stored_first : b;
        pass = !err && b >= i1;
        ver[q] = err ? (uint8_t)2 : pass ? (uint8_t)0 : (uint8_t)1;
        blk[q] = b < i1 ? b : -1;
      }
      const uint64_t mk = __ballot(pass);
      if (mk != 0ull && ans < 0) ans = q0 + (__ffsll((long long)mk) - 1);  // the first passing position
    }
    if (lane == 0) a.first[gi] = ans;
  }
}

bool launch_forecast_gangs_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n_gangs, int64_t m,
                                 const int64_t* rows_dev, const int64_t* gang_off_dev, const int64_t* inst_s, const int32_t* inst_ns, int T,
                                 bool on_equal, const uint8_t* status, const uint64_t* summary, int64_t* first, uint8_t* verdicts, int64_t* blocker,
                                 hipStream_t s, hipError_t* hip_err) {
  *hip_err = hipSuccess;
  if (n_gangs <= 0 || m <= 0) return true;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  ForecastGangsPagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.m = m, a.inst_s = inst_s;
  a.inst_ns = inst_ns, a.status = status, a.summary = summary, a.first = first, a.verdicts = verdicts, a.blocker = blocker;
  a.T = T, a.on_equal = on_equal ? 1 : 0;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(PreemptPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_forecast_gangs_paged<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_forecast_gangs_paged<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_forecast_gangs_paged<16>, dim3(blocks), dim3(kWave), 0, s, a);
  return true;
}

}  // namespace kt
