// kt_kernels_headroom_forecast_paged.hip — how many copies of a pod the throttles admit at each of a list of instants, over PAGES
// of resource names (kt_paged_headroom_forecast), gfx950.
//
// The definition is kt_kernels_headroom_forecast.hip's on the cluster of all names; a page is an engine of <= 16 names that holds
// every pod row and every throttle row (kt_engine.h, "PAGES").  The page rules are kt_kernels_forecast_paged.hip's:
// status.calculatedThreshold is compared and replaced AS A WHOLE (throttle_controller.go:116-133), so whether a throttle reads its
// calculated threshold or spec.threshold at instant t is ONE fact for all pages, and it changes from instant to instant — the answer
// is not the minimum of the pages' own headroom forecasts.  The headroom rules are kt_headroom's over pages: the pod count is judged
// on page 0 only, each page judges its own names against its own reserved row and presence bits, the throttle's number is the
// minimum over the count and every needed name of every page.
//
// kt_headroom_forecast_paged<DT> (DT: the bucket of the widest page): one wave per pod (the grid strides), lane = instant position,
// 64 instants per block; the affecting throttles come chunk by chunk from PAGE 0's status matrix.  Per affecting throttle:
//   whole-throttle facts, wave-uniform, an OR over the pages: `stored` and `calc_at_any`, as kt_forecast_paged forms them.
//   a stored throttle is judged once over every page: the count term on page 0 and every requested name of every page through
//     headroom_of_term, against tt.calc where calc_at_any holds and tt.spec otherwise, from the stored used / reserved /
//     thrl_flag & thrl_has as the stored branch of kt_headroom_forecast reads them; its (h, row) goes into `kept`, the minimum that
//     holds at every instant.
//   otherwise, per block of 64 instants, the lane keeps `differs`, `h_calc` and `h_spec` across the pages: two running minima that
//     start at cap.  For each page it walks that page's overrides exactly as kt_forecast_paged does (the per-name register arrays
//     belong to one page at a time), forms `differs` on EVERY page, and reduces headroom_of_term of every needed name into h_calc
//     against the calculated threshold and into h_spec against spec.threshold; `flagged` (c_p has the name, the used sum is present
//     and at least c_v) is the same in both, the count term goes into both on page 0 only, `brings` is the page's own presence bit of
//     the pod.  After the last page reads_calc = calc_at_any || differs and h = reads_calc ? h_calc : h_spec.  One walk per page and
//     block: no second pass once reads_calc is known.
//   running answer: the lexicographic minimum of (h, throttle row) per position, in the lane's own cell of the copies buffer, as
//     kt_headroom_forecast keeps it (the chunk list is NOT in row order: the row is a key of the comparison); a lane lowers its cell
//     only where h < cap.
// Output and the error rows are kt_headroom_forecast's: copies = min(cap, h), limiting = the row where h < cap, else -1, first = the
// first position with copies >= want (ballot over the blocks in order), or -1; summary == 2 or an invalid pod row on page 0: 0, -1
// and -1.  With one page the kernel computes what kt_headroom_forecast computes.  Every __ballot sits where the whole wave arrives:
// the loops over chunks, throttles, pages, blocks and overrides are wave-uniform.
#include "kt_admit_common.h"

namespace kt {

struct HeadroomForecastPagedArgs {
  const PreemptPage* pages;  // [n_pages] in device memory (calc / calc_updated of the dry finalize are not read: every instant is computed)
  int32_t n_pages;
  const int64_t* rows;       // [n] pod table rows (the same in every page)
  int64_t n, m;              // pods, instants
  const int64_t* inst_s;     // [m] strictly ascending
  const int32_t* inst_ns;    // [m]
  const uint8_t* status;     // [n][T] page 0's check
  const uint64_t* summary;   // [n]
  int64_t* first;            // [n] out
  int64_t* copies;           // [n][m] out (and the running (h, row) pair of every position while the kernel runs)
  int32_t* limiting;         // [n][m] out
  int32_t T, on_equal;
  uint32_t cap, want;        // 1 <= want <= cap <= 2^31 - 1
};

__device__ __forceinline__ uint32_t hfp_min(uint32_t a, uint32_t b) { return b < a ? b : a; }
__device__ __forceinline__ unsigned long long hfp_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

template <int DT>
__global__ __launch_bounds__(kWave) void kt_headroom_forecast_paged(const HeadroomForecastPagedArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, n_pages = a.n_pages;
  const bool eq = a.on_equal != 0;
  const uint32_t cap = a.cap, want = a.want;
  const int64_t n = a.n, m = a.m;
  const unsigned long long none = (unsigned long long)cap << 32 | 0xFFFFFFFFull;  // (cap, no row)
  const uint32_t* pod_flags0 = preempt_page(a.pages, 0).pg.pod_flags;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {  // (wave-uniform: one pod per wave and turn)
    const int64_t p = a.rows[i];
    unsigned long long* run = (unsigned long long*)(a.copies + i * m);  // the lane's own cells: positions lane, lane + 64, ...
    int32_t* lim = a.limiting + i * m;
    for (int64_t q = lane; q < m; q += kWave) run[q] = none;
    const uint8_t* row = a.status + i * T;
    bool err = a.summary[i] == 2ull || !(pod_flags0[p] & kPodValid);
    unsigned long long kept = none;  // the minimum over the throttles that keep their stored status: it holds at every instant
    for (int c0 = 0; c0 < T && !err; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      err = __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c && !err; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        // ---- the facts of the throttle as a whole: the OR over the pages
        bool stored = false, calc_at_any = false;
        for (int k = 0; k < n_pages; ++k) {
          const PreemptPage pp = preempt_page(a.pages, k);
          const uint32_t tf = pp.pg.tt.flags[t];
          stored |= preempt_row_stored(tf, pp.error[t]);
          calc_at_any |= (tf & kThrCalcAtNonzero) != 0;
        }
        HeadroomTerm hm;
        hm.eq = eq;
        if (stored) {  // the stored status of every page: nothing of it depends on the instant
          uint32_t h = cap;
          for (int k = 0; k < n_pages; ++k) {
            const PreemptPage pp = preempt_page(a.pages, k);
            const int D = pp.pg.D, DS = pp.pg.DS;
            const ThrTables& tt = pp.pg.tt;
            const uint32_t tf = tt.flags[t];
            const AmountTab& th = calc_at_any ? tt.calc : tt.spec;
            hm.eq3 = admit_eq3(tf, eq);
            if (k == 0) {  // the pod count: the same in every page
              const bool u_hc = tt.used.has_count[t] != 0, r_hc = tt.reserved.has_count[t] != 0;
              hm.v = 1, hm.va = 1, hm.tv = th.count[t], hm.uv = u_hc ? tt.used.count[t] : 0, hm.rv = r_hc ? tt.reserved.count[t] : 0;
              hm.th_has = th.has_count[t] != 0, hm.present0 = u_hc || r_hc, hm.brings = true, hm.flagged = (tf & kThrThrottledPod) != 0;
              h = hfp_min(h, headroom_of_term(hm, h));
            }
            const uint32_t th_p = th.present[t], u_p = tt.used.present[t], r_p = tt.reserved.present[t], flg = tt.thrl_flag[t] & tt.thrl_has[t];
            const uint32_t brings = pp.pg.pod_flags[p] >> kPresentShift;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d >= D) continue;
              const int64_t vpd = pp.pg.req[p * DS + d];
              if (vpd == 0) continue;  // steps 1-4 of a name the pod does not request
              hm.brings = (brings >> d) & 1u;
              hm.v = vpd, hm.va = hm.brings ? vpd : 0;
              hm.th_has = (th_p >> d) & 1u;
              hm.tv = th.v[(size_t)t * D + d];
              hm.uv = ((u_p >> d) & 1u) ? tt.used.v[(size_t)t * D + d] : 0;
              hm.rv = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
              hm.present0 = ((u_p | r_p) >> d) & 1u;
              hm.flagged = (flg >> d) & 1u;
              h = hfp_min(h, headroom_of_term(hm, h));
            }
          }
          kept = hfp_min(kept, (unsigned long long)h << 32 | t);
          continue;
        }
        for (int64_t q0 = 0; q0 < m; q0 += kWave) {
          const int64_t q = q0 + lane;
          const bool in = q < m;
          const int64_t ts = a.inst_s[in ? q : m - 1];
          const int32_t tn = a.inst_ns[in ? q : m - 1];
          bool differs = false;  // the lane's own, across the pages
          uint32_t h_calc = cap, h_spec = cap;
          for (int k = 0; k < n_pages; ++k) {
            // ---- the throttle's own state on page k: one batch of wave-uniform loads
            const PreemptPage pp = preempt_page(a.pages, k);
            const int D = pp.pg.D, DS = pp.pg.DS;
            const ThrTables& tt = pp.pg.tt;
            const uint32_t tf = tt.flags[t];
            hm.eq3 = admit_eq3(tf, eq);
            const uint32_t ovr0 = tt.ovr_off[t], ovr1 = tt.ovr_off[t + 1];
            const uint64_t status_fp = tt.status_msgs_fp[t], spec_fp = tt.spec_msgs_fp[t];
            const uint32_t s_p = tt.spec.present[t], k_p = tt.calc.present[t], r_p = tt.reserved.present[t];
            const uint32_t brings = pp.pg.pod_flags[p] >> kPresentShift;
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
              rv[d] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
              // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
              const int64_t tot = (int64_t)prow[d];
              u_pr[d] = prow[partial_off_presence(D) + d] != 0ull || tot != 0;
              tot_v[d] = u_pr[d] ? tot : 0;
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
              const int64_t s_c = tt.spec.count[t], k_c = tt.calc.count[t];
              const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
              const bool u_hc = pods_total > 0;
              if (!active_found) c_hc = s_hc, c_c = s_c;
              differs |= c_hc != k_hc || (c_hc && c_c != k_c);
              hm.v = 1, hm.va = 1, hm.uv = u_hc ? pods_total : 0, hm.rv = r_hc ? tt.reserved.count[t] : 0;  // (a clear presence bit reads as 0)
              hm.present0 = u_hc || r_hc, hm.brings = true;
              hm.flagged = c_hc && u_hc && pods_total >= c_c;
              hm.th_has = c_hc, hm.tv = c_c;
              h_calc = hfp_min(h_calc, headroom_of_term(hm, h_calc));
              hm.th_has = s_hc, hm.tv = s_c;
              h_spec = hfp_min(h_spec, headroom_of_term(hm, h_spec));
            }
            // ---- throttled = calculatedThreshold.IsThrottled(used, true), then the closed form of the four steps against either
            //      threshold: the minimum so far is the term's cap (min(h, term) is the same number, and headroom_fit bisects below
            //      h only)
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (!need[d]) continue;  // (wave-uniform)
              hm.brings = (brings >> d) & 1u;
              hm.v = vp[d], hm.va = hm.brings ? vp[d] : 0;
              hm.uv = tot_v[d], hm.rv = rv[d];
              hm.present0 = u_pr[d] || ((r_p >> d) & 1u);
              hm.flagged = ((c_p >> d) & 1u) && u_pr[d] && tot_v[d] >= c_v[d];
              hm.th_has = (c_p >> d) & 1u, hm.tv = c_v[d];
              h_calc = hfp_min(h_calc, headroom_of_term(hm, h_calc));
              hm.th_has = (s_p >> d) & 1u, hm.tv = sv[d];
              h_spec = hfp_min(h_spec, headroom_of_term(hm, h_spec));
            }
          }
          // ---- the threshold the check reads behind this reconcile, on every page: calculatedThreshold once calculatedAt is set
          //      or some page replaces it, else spec
          const bool reads_calc = calc_at_any || differs;
          const uint32_t h = reads_calc ? h_calc : h_spec;
          // (cap, any row) lowers no answer: only a throttle that stops a copy below cap touches the lane's cell
          if (in && h < cap) run[q] = hfp_min(run[q], (unsigned long long)h << 32 | t);
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    int64_t ans = -1;
    for (int64_t q0 = 0; q0 < m; q0 += kWave) {
      const int64_t q = q0 + lane;
      const bool in = q < m;
      const unsigned long long best = in ? hfp_min(run[q], kept) : none;
      const uint32_t h = err ? 0u : (uint32_t)(best >> 32);
      if (in) {
        a.copies[i * m + q] = (int64_t)h;
        lim[q] = (err || h >= cap) ? -1 : (int32_t)(uint32_t)best;
      }
      const uint64_t mk = __ballot(in && !err && h >= want);
      if (mk != 0ull && ans < 0) ans = q0 + (__ffsll((long long)mk) - 1);  // the first position with `want` copies
    }
    if (lane == 0) a.first[i] = ans;
  }
}

bool launch_headroom_forecast_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                                    const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, uint32_t cap,
                                    uint32_t want, const uint8_t* status, const uint64_t* summary, int64_t* first, int64_t* copies,
                                    int32_t* limiting, hipStream_t s, hipError_t* hip_err) {
  *hip_err = hipSuccess;
  if (n <= 0 || m <= 0) return true;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  HeadroomForecastPagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.n = n, a.m = m, a.inst_s = inst_s, a.inst_ns = inst_ns, a.status = status;
  a.summary = summary, a.first = first, a.copies = copies, a.limiting = limiting, a.T = T, a.on_equal = on_equal ? 1 : 0;
  a.cap = cap, a.want = want;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(PreemptPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_headroom_forecast_paged<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_headroom_forecast_paged<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_headroom_forecast_paged<16>, dim3(blocks), dim3(kWave), 0, s, a);
  return true;
}

}  // namespace kt
