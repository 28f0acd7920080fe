// kt_kernels_forecast_paged.hip — the first instant at which a blocked pod passes, over PAGES of resource names
// (kt_paged_forecast), gfx950.
//
// The definition is kt_kernels_forecast.hip's on the cluster of all names; a page is an engine of <= 16 names that holds every pod
// row and every throttle row (kt_engine.h, "PAGES").  status.calculatedThreshold is compared and replaced AS A WHOLE
// (throttle_controller.go:116-133), so whether a throttle reads its calculated threshold or spec.threshold at instant t is ONE
// fact for all pages, and it changes from instant to instant: the answer cannot be put together from per-page forecasts.
//
// kt_forecast_paged<DT> (DT: the bucket of the widest page): one wave per pod (the grid strides), lane = instant position, 64
// instants per block; the affecting throttles come chunk by chunk from PAGE 0's status matrix (the selector side is the same in
// every page, a pod-level error shows in every page).  Per affecting throttle:
//   whole-throttle facts, wave-uniform, an OR over the pages:
//     stored       the dry reconcile is an error on some page, or the throttle is not valid and responsible: the stored status is
//                  read on every page at every instant;
//     calc_at_any  calculatedAt is set on some page (between a paged reconcile that applies and the host's write-back the pages'
//                  stored flags may disagree: the throttle has been replaced once some page says so).
//   a stored throttle is judged once over every page: the count part on page 0, every page's name part, against tt.calc where
//     calc_at_any holds and tt.spec otherwise.  A failure makes the pod `never` pass.
//   otherwise, per block of 64 instants, the lane keeps `differs`, `f_calc` and `f_spec` across the pages.  For each page it walks
//     that page's overrides exactly as kt_forecast does (activity is decided by the instants, the same on every page; the first
//     active override wins per name of that page; the per-name register arrays belong to one page at a time), then
//       differs |= the page's calculated threshold at the lane's instant differs by value from the page's stored one over its names
//                  (c_p != k_p || diff) or the page's messages fingerprint differs; page 0 adds the comparison of the count (the
//                  count is the same in every page);
//       f_calc  |= the page's name part of the four steps against the calculated threshold;
//       f_spec  |= the same against spec.threshold;
//     the `flagged` term (c_p has the name, the used sum is present and at least c_v) is the same in both; the count part goes into
//     both accumulators on page 0 only.  After the last page reads_calc = calc_at_any || differs, f = reads_calc ? f_calc : f_spec,
//     and the lane stores 1 into its own verdict byte if f.  One walk per page and block: no second pass once reads_calc is known.
//   Judging skips the names the pod does not request or no threshold of the page names (`need`) — on a page that holds none, nothing
//   is judged — but `differs` is formed on EVERY page: a page that holds nothing the pod asks for can still replace the threshold
//   for all the others.
// first[i], the error rows (summary == 2 or an invalid pod row on page 0: every byte 2, first = -1) and the `never` rows are
// kt_forecast's.  With one page the kernel computes what kt_forecast computes.  Every __ballot sits where the whole wave arrives:
// the loops over chunks, throttles, pages, blocks and overrides are wave-uniform.
#include "kt_admit_common.h"

namespace kt {

struct ForecastPagedArgs {
  const PreemptPage* pages;  // [n_pages] in device memory (calc / calc_updated of the dry finalize are not read: every instant is computed)
  int32_t n_pages;
  const int64_t* rows;       // [n] pod table rows (the same in every page)
  int64_t n, m;              // pods, instants
  const int64_t* inst_s;     // [m] strictly ascending
  const int32_t* inst_ns;    // [m]
  const uint8_t* status;     // [n][T] page 0's check
  const uint64_t* summary;   // [n]
  int64_t* first;            // [n] out
  uint8_t* verdicts;         // [n][m] out
  int32_t T, on_equal;
};

template <int DT>
__global__ __launch_bounds__(kWave) void kt_forecast_paged(const ForecastPagedArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, n_pages = a.n_pages;
  const bool eq = a.on_equal != 0;
  const int64_t n = a.n, m = a.m;
  const uint32_t* pod_flags0 = preempt_page(a.pages, 0).pg.pod_flags;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {  // (wave-uniform: one pod per wave and turn)
    const int64_t p = a.rows[i];
    uint8_t* ver = a.verdicts + i * m;
    for (int64_t q = lane; q < m; q += kWave) ver[q] = 0;
    const uint8_t* row = a.status + i * T;
    bool err = a.summary[i] == 2ull || !(pod_flags0[p] & kPodValid);
    bool never = false;  // a throttle that keeps its stored status stops the pod: at every instant
    for (int c0 = 0; c0 < T && !err && !never; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      err = __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c && !err && !never; ++ai) {
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
          bool f = false;
          for (int k = 0; k < n_pages; ++k) {
            const PreemptPage pp = preempt_page(a.pages, k);
            const int D = pp.pg.D, DS = pp.pg.DS;
            const ThrTables& tt = pp.pg.tt;
            const uint32_t tf = tt.flags[t];
            const AmountTab& th = calc_at_any ? tt.calc : tt.spec;
            const bool eq3 = admit_eq3(tf, eq);
            if (k == 0)
              f |= preempt_fails(1, th.has_count[t] != 0, th.count[t], (tf & kThrThrottledPod) != 0, tt.used.has_count[t] != 0, tt.used.count[t],
                                 tt.reserved.has_count[t] != 0, tt.reserved.count[t], eq3, eq);
            const uint32_t th_p = th.present[t], u_p = tt.used.present[t], r_p = tt.reserved.present[t], flg = tt.thrl_flag[t] & tt.thrl_has[t];
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d >= D) continue;
              const int64_t vpd = pp.pg.req[p * DS + d];
              if (vpd == 0) continue;
              f |= preempt_fails(vpd, (th_p >> d) & 1u, th.v[(size_t)t * D + d], (flg >> d) & 1u, (u_p >> d) & 1u, tt.used.v[(size_t)t * D + d],
                                 (r_p >> d) & 1u, tt.reserved.v[(size_t)t * D + d], eq3, eq);
            }
          }
          never = f;
          continue;
        }
        for (int64_t q0 = 0; q0 < m; q0 += kWave) {
          const int64_t q = q0 + lane;
          const bool in = q < m;
          const int64_t ts = a.inst_s[in ? q : m - 1];
          const int32_t tn = a.inst_ns[in ? q : m - 1];
          bool differs = false, f_calc = false, f_spec = false;  // the lane's own, across the pages
          for (int k = 0; k < n_pages; ++k) {
            // ---- the throttle's own state on page k: one batch of wave-uniform loads
            const PreemptPage pp = preempt_page(a.pages, k);
            const int D = pp.pg.D, DS = pp.pg.DS;
            const ThrTables& tt = pp.pg.tt;
            const uint32_t tf = tt.flags[t];
            const bool eq3 = admit_eq3(tf, eq);
            const uint32_t ovr0 = tt.ovr_off[t], ovr1 = tt.ovr_off[t + 1];
            const uint64_t status_fp = tt.status_msgs_fp[t], spec_fp = tt.spec_msgs_fp[t];
            const uint32_t s_p = tt.spec.present[t], k_p = tt.calc.present[t], r_p = tt.reserved.present[t];
            const unsigned long long* prow = pp.partial + (size_t)t * partial_stride(D);
            // the names some threshold of this throttle can name on this page, and whether an override has a parse error (the
            // messages of CalculateThreshold: they do not depend on the instant)
            uint32_t names = s_p | k_p;
            bool any_err = false;
            for (uint32_t o = ovr0; o < ovr1; ++o) {
              if (tt.ovr_flags[o] & kOvrParseError) any_err = true;
              else names |= tt.ovr_thr.present[o];
            }
            const bool fp_differs = status_fp != (any_err ? spec_fp : 0ull);
            int64_t vp[DT], sv[DT], kv[DT], rv[DT], tot_v[DT];
            bool need[DT], u_pr[DT];
            bool spec_diff = false;  // spec.threshold against the stored calculatedThreshold, by value, over the names spec has
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              need[d] = u_pr[d] = false, vp[d] = sv[d] = kv[d] = rv[d] = tot_v[d] = 0;
              if (d >= D) continue;
              sv[d] = tt.spec.v[(size_t)t * D + d], kv[d] = tt.calc.v[(size_t)t * D + d];
              spec_diff |= ((s_p >> d) & 1u) && sv[d] != kv[d];
              vp[d] = pp.pg.req[p * DS + d];
              // a name the pod does not request passes every step, and so does one that no threshold names
              need[d] = vp[d] != 0 && ((names >> d) & 1u);
              if (!need[d]) continue;
              rv[d] = tt.reserved.v[(size_t)t * D + d];
              tot_v[d] = (int64_t)prow[d];
              // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
              u_pr[d] = prow[partial_off_presence(D) + d] != 0ull || tot_v[d] != 0;
            }
            // ---- CalculateThreshold(t) on this page: first active override wins, per name and for the count
            bool active_found = false, c_hc = false, diff = false;
            int64_t c_c = 0, c_v[DT];
            uint32_t c_p = 0;
#pragma unroll
            for (int d = 0; d < DT; ++d) c_v[d] = 0;
            for (uint32_t o = ovr0; o < ovr1; ++o) {
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
                  diff |= o_v != kv[d];
                  c_v[d] = o_v;
                }
              }
            }
            if (!active_found) {  // no active override: spec.threshold; otherwise the merged override REPLACES it
              c_p = s_p, diff = spec_diff;
#pragma unroll
              for (int d = 0; d < DT; ++d) c_v[d] = sv[d];
            }
            // ---- does this page see a threshold (or messages) that differ from what it stores
            differs |= c_p != k_p || diff || fp_differs;
            if (k == 0) {  // the count: the same in every page, compared and judged once
              const bool s_hc = tt.spec.has_count[t] != 0, k_hc = tt.calc.has_count[t] != 0, r_hc = tt.reserved.has_count[t] != 0;
              const int64_t s_c = tt.spec.count[t], k_c = tt.calc.count[t], r_c = tt.reserved.count[t];
              const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
              const bool u_hc = pods_total > 0;
              if (!active_found) c_hc = s_hc, c_c = s_c;
              differs |= c_hc != k_hc || (c_hc && c_c != k_c);
              const bool flagged = c_hc && u_hc && pods_total >= c_c;
              f_calc |= preempt_fails(1, c_hc, c_c, flagged, u_hc, pods_total, r_hc, r_c, eq3, eq);
              f_spec |= preempt_fails(1, s_hc, s_c, flagged, u_hc, pods_total, r_hc, r_c, eq3, eq);
            }
            // ---- throttled = calculatedThreshold.IsThrottled(used, true), then the four steps against either threshold
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (!need[d]) continue;  // (wave-uniform)
              const bool flagged = ((c_p >> d) & 1u) && u_pr[d] && tot_v[d] >= c_v[d];
              f_calc |= preempt_fails(vp[d], (c_p >> d) & 1u, c_v[d], flagged, u_pr[d], tot_v[d], (r_p >> d) & 1u, rv[d], eq3, eq);
              f_spec |= preempt_fails(vp[d], (s_p >> d) & 1u, sv[d], flagged, u_pr[d], tot_v[d], (r_p >> d) & 1u, rv[d], eq3, eq);
            }
          }
          // ---- the threshold the check reads behind this reconcile, on every page: calculatedThreshold once calculatedAt is set
          //      or some page replaces it, else spec
          const bool reads_calc = calc_at_any || differs;
          if (in && (reads_calc ? f_calc : f_spec)) ver[q] = (uint8_t)1;  // KT_VERDICT_UNSCHEDULABLE; the lane's own byte
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    int64_t ans = -1;
    if (err || never) {
      for (int64_t q = lane; q < m; q += kWave) ver[q] = err ? (uint8_t)2 : (uint8_t)1;
    } else {
      for (int64_t q0 = 0; q0 < m; q0 += kWave) {
        const int64_t q = q0 + lane;
        const uint64_t mk = __ballot(q < m && ver[q] == 0);
        if (mk != 0ull) {
          ans = q0 + (__ffsll((long long)mk) - 1);  // the first passing position
          break;
        }
      }
    }
    if (lane == 0) a.first[i] = ans;
  }
}

bool launch_forecast_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                           const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, const uint8_t* status,
                           const uint64_t* summary, int64_t* first, uint8_t* verdicts, hipStream_t s, hipError_t* hip_err) {
  *hip_err = hipSuccess;
  if (n <= 0 || m <= 0) return true;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  ForecastPagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.n = n, a.m = m, a.inst_s = inst_s, a.inst_ns = inst_ns, a.status = status;
  a.summary = summary, a.first = first, a.verdicts = verdicts, a.T = T, a.on_equal = on_equal ? 1 : 0;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(PreemptPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_forecast_paged<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_forecast_paged<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_forecast_paged<16>, dim3(blocks), dim3(kWave), 0, s, a);
  return true;
}

}  // namespace kt
