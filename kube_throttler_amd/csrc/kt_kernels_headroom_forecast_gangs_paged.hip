// kt_kernels_headroom_forecast_gangs_paged.hip — how many copies of a whole gang the throttles admit at each of a list of
// instants, over PAGES of resource names (kt_paged_headroom_forecast_gangs), gfx950.
//
// The definition is kt_kernels_headroom_forecast_gangs.hip's on the cluster of all names; a page is an engine of <= 16 names that
// holds every pod row and every throttle row (kt_engine.h, "PAGES").  copies[g][k] is the number of leading admitted gangs of a dry
// kt_paged_admit_gangs over `cap` consecutive copies of gang g, with R_k — every valid and responsible throttle reconciled at t_k
// on every page — as the stored status.  Two sets of rules meet:
//   thresholds  kt_kernels_forecast_gangs_paged.hip's: status.calculatedThreshold is compared and replaced AS A WHOLE, so whether a
//               throttle reads its calculated threshold or spec.threshold at instant t_k is ONE fact for all pages (`stored` and
//               `calc_at_any` are ORs over the pages, `differs` is the OR over EVERY page, also one none of whose names any member
//               requests, page 0 adds the comparison of the count) that changes from instant to instant: the minimum of the pages'
//               own gang headroom forecasts is wrong.  The throttled bits are IsThrottled(used, true) against the CALCULATED
//               threshold either way.  A throttle that keeps its stored status (its reconcile is an error, or it is not valid and
//               responsible, on some page) is read on every page against tt.calc where calc_at_any holds and tt.spec otherwise —
//               NOT admit_threshold of the page, which kt_headroom_gangs_paged uses.
//   copies      kt_kernels_headroom_gangs_paged.hip's: an admitted copy reserves on every page, each page its own names' values and
//               the presence of the names a member carries there; the pod count is judged and reserved once, on page 0 (the other
//               pages hand gang_walk a threshold that does not name the count and a count flag of false).  Copy j passes on throttle
//               t iff the in-order member walk passes on every page, each against its own reserved row plus j * A_t of that page:
//               an AND of monotone predicates.  So per instant every (throttle, page) pair is a throttle of its own, and the answer
//               is the lexicographic minimum over the pairs of (copies, first stopped position, throttle row).  A page k != 0 none
//               of whose names an affected member requests with a non-zero value stops nobody and is skipped in the walk — never in
//               `differs`.
//
// kt_headroom_forecast_gangs_paged<DT> (DT: the bucket of the widest page) is kt_headroom_forecast_gangs' body — one wave per gang,
// the grid strides, lane = instant position, 64 instants per block, the lane's own bisection with gang_walk (kt_admit_common.h,
// unchanged) as judge — with kt_forecast_gangs_paged's two passes over the pages inside the block loop:
//   per gang      the first member whose PreFilter is an error (page 0's summary) or whose row is invalid (page 0's pod_flags) by a
//                 ballot over member blocks of 64; the UNION of the members' affecting throttles chunk by chunk through the 4 KiB
//                 LDS list, from page 0's matrix.
//   per throttle  `stored` and `calc_at_any`, wave-uniform.  A stored throttle runs ONE block with every lane alike; any other one
//                 block per 64 instants:
//     pass 1      `differs`, the lane's own: forecast_page_thr + the override walk on every page (wave-uniform loads), page 0 adds
//                 the count.  Skipped where calc_at_any holds, and for a stored throttle.
//     pass 2      per page, reads_calc = calc_at_any || differs:
//       A_t       one pass over the members: what one admitted copy reserves on this page, over the names ANY threshold of the
//                 throttle can name here (masked per lane to the names the lane's threshold has), and the names an affected member
//                 requests with a non-zero value — which says whether the page is skipped;
//       state     the override walk again for the lane's GangThr; GangUsed from the page's partial row, presence by exact
//                 contributor counts; the throttled bits against the calculated threshold; the count part on page 0 only.  A
//                 stored throttle: that page's stored used, throttled flags and reserved row against tt.calc / tt.spec;
//       range     up to the lane's running minimum — it lives in the lane's own cells of the three [n_gangs][m] outputs and so
//                 carries across pages as well as throttles — and no further than every amount the lane's threshold names stays
//                 inside int64 (hfgp_fit; the count's cut on page 0 only);
//       search    the probe at the top of the range, then the lane's own bisection below it, 1 + 31 rounds at the most, while a
//                 ballot says some lane still searches; every probe is one gang_walk over the page's view (GangPageView) with the
//                 candidate's reserved row;
//       update    the strict lexicographic (h, first, t) update of the lane's cells — the row is a key: the chunk list is not in
//                 row order.  A stored throttle updates the kept triple, which runs over pages as well as throttles and is folded
//                 into every position at the end.
//                 A gang with an Error / invalid member: copy 0 alone, the walk ends in front of that member, per (throttle, page)
//                 with the lane's thresholds (the blocker may differ per instant).
//   output        kt_headroom_forecast_gangs': copies[g][k] = min(cap, h); blocker[g][k] / limiting[g][k] = first / t of the
//                 minimum, -1 where h >= cap (limiting also where the blocker is the Error member); first[g] = the first position
//                 with copies >= want (ballot over the blocks in order), or -1.  With one page the kernel computes what
//                 kt_headroom_forecast_gangs computes.
// Every __ballot, __syncthreads and readfirstlane sits where the whole wave arrives: the loops over chunks, throttles, pages,
// blocks, overrides, rounds and members are wave-uniform.  All writes are vector stores in plain C++.
#include "kt_preempt_paged_common.h"

namespace kt {

struct HeadroomForecastGangsPagedArgs {
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
  int64_t* copies;           // [n_gangs][m] out (and the running h of every position while the kernel runs)
  int32_t* limiting;         // [n_gangs][m] out (... its row)
  int64_t* blocker;          // [n_gangs][m] out (... its first stopped position)
  int32_t T, on_equal;
  uint32_t cap, want;        // 1 <= want <= cap <= 2^31 - 1
};

constexpr int64_t kHfgpInt64Max = 0x7FFFFFFFFFFFFFFFll;

// (private copies of kt_kernels_headroom_forecast_gangs.hip's hfg_fit / hfg_row: nothing of that file is lifted)
// the candidates of one amount end at (INT64_MAX - base) / per: beyond, reserved + (j + 1) per has left int64 (per > 0)
__device__ __forceinline__ int64_t hfgp_fit(int64_t base, int64_t per, int64_t top) {
  const uint64_t q = ((uint64_t)kHfgpInt64Max - (uint64_t)base) / (uint64_t)per;  // (base may be negative: the difference fits 64 bits)
  return q < (uint64_t)top ? (int64_t)q : top;
}
// base + j * per of a candidate inside its range (the result fits int64; formed modulo 2^64, which has no undefined corner)
__device__ __forceinline__ int64_t hfgp_row(int64_t base, int64_t j, int64_t per) { return (int64_t)((uint64_t)base + (uint64_t)j * (uint64_t)per); }

template <int DT>
__global__ __launch_bounds__(kWave) void kt_headroom_forecast_gangs_paged(const HeadroomForecastGangsPagedArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, n_pages = a.n_pages;
  const bool eq = a.on_equal != 0;
  const int64_t m = a.m, cap = (int64_t)a.cap, want = (int64_t)a.want;
  const uint32_t* pod_flags0 = preempt_page(a.pages, 0).pg.pod_flags;
  for (int64_t gi = blockIdx.x; gi < a.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
    int64_t* cop = a.copies + gi * m;  // the lane's own cells: positions lane, lane + 64, ...
    int32_t* lim = a.limiting + gi * m;
    int64_t* blk = a.blocker + gi * m;
    // the first member whose PreFilter is an error or whose row is invalid: copy 0 is not admitted, the walk ends in front of it
    int64_t bad = i1;
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(pod_flags0[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        bad = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    const bool err = bad < i1;
    const int64_t h0 = err ? 0 : cap;
    for (int64_t q = lane; q < m; q += kWave) cop[q] = h0, blk[q] = bad, lim[q] = -1;
    // the minimum over the (throttle, page) pairs that keep their stored status: it holds at every instant (every lane holds the same)
    int64_t kept_h = h0, kept_first = bad;
    int32_t kept_t = -1;
    for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
      bool err_c = false;  // (the error rows are the summary's: `bad` above)
      const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
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
        for (int64_t q0 = 0; q0 < (stored ? 1 : m); q0 += kWave) {
          const int64_t q = q0 + lane;
          const bool in = stored || q < m;
          const int64_t ts = a.inst_s[q < m ? q : m - 1];
          const int32_t tn = a.inst_ns[q < m ? q : m - 1];
          // ---- pass 1: does some page see a threshold (or messages) that differ from what it stores, at the lane's instant
          bool differs = false;
          if (!stored && !calc_at_any) {  // (wave-uniform; where calculatedAt is set the calculated threshold is read whatever this says)
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
          // ---- pass 2: the search, page by page
          for (int k = 0; k < n_pages; ++k) {
            const PreemptPage pp = preempt_page(a.pages, k);
            const GangPageView view{pp.pg, a.rows, a.status, T};
            const int D = pp.pg.D, DS = pp.pg.DS;
            const ThrTables& tt = pp.pg.tt;
            const bool first_page = k == 0;
            const uint32_t tf = tt.flags[t];
            const AmountTab& sth = calc_at_any ? tt.calc : tt.spec;  // what a stored throttle is read against
            ForecastPageThr<DT> pt;
            if (!stored) pt = forecast_page_thr<DT>(tt, D, t);
            // the names some threshold of the throttle can name on this page
            const uint32_t names = stored ? sth.present[t] : pt.names;
            // ---- A_t of this page: what one admitted copy reserves here, one pass over the members.  A name is summed where SOME
            //      threshold of the throttle can name it (the lane's own is not known yet); the lane masks below.  The same pass
            //      says which names an affected member requests with a non-zero value
            int64_t per[DT], per_c = 0;
            uint32_t per_p = 0, need = 0;
#pragma unroll
            for (int d = 0; d < DT; ++d) per[d] = 0;
            for (int64_t i = i0; i < i1; ++i) {
              if (a.status[i * (int64_t)T + t] == 0) continue;
              const int64_t p = a.rows[i];
              const uint32_t present = (pp.pg.pod_flags[p] >> kPresentShift) & ((1u << D) - 1u);
              per_c += 1, per_p |= present;
#pragma unroll
              for (int d = 0; d < DT; ++d) {
                if (d >= D) continue;
                const int64_t v = pp.pg.req[p * DS + d];
                need |= v != 0 ? 1u << d : 0u;
                if (!(((present & names) >> d) & 1u)) continue;
                per[d] = v > kHfgpInt64Max - per[d] ? kHfgpInt64Max : per[d] + v;  // (saturated: the range then ends at copy 0 or 1)
              }
            }
            // (page 0 carries the pod count; elsewhere a page none of whose names an affected member requests stops nobody.  A
            // stored throttle may flag a name its threshold does not name: only the reconciled ones are cut to `names`)
            if (!stored) need &= names;
            if (!first_page && need == 0u) continue;  // (wave-uniform)
            GangThr<DT> g;
            GangUsed<DT> u;
            g.eq = eq, g.eq3 = admit_eq3(tf, eq);
            const bool r_hc = tt.reserved.has_count[t] != 0;
            const int64_t r_c = r_hc ? tt.reserved.count[t] : 0;  // a reserved amount whose presence bit is clear reads as 0
            const uint32_t r_p = tt.reserved.present[t];
            int64_t base[DT];  // the page's stored reserved row (0 where absent)
            if (stored) {  // the stored tables of this page: every lane alike
              // the pod count is page 0's: elsewhere the threshold does not name it
              g.th_hc = first_page && sth.has_count[t] != 0, g.th_c = sth.count[t], g.th_p = sth.present[t];
              u.c_flag = first_page && (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
              u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
#pragma unroll
              for (int d = 0; d < DT; ++d) {
                base[d] = g.tv[d] = u.u_v[d] = 0;
                if (d >= D) continue;
                g.tv[d] = sth.v[(size_t)t * D + d], u.u_v[d] = tt.used.v[(size_t)t * D + d];
                base[d] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
              }
            } else {
              // ---- CalculateThreshold at the lane's instant on this page, the threshold the check reads, the throttled bits
              bool c_hc, diff;
              int64_t c_c, c_v[DT];
              uint32_t c_p;
              forecast_page_calc<DT>(tt, D, t, pt, ts, tn, &c_hc, &c_c, &c_p, c_v, &diff);
              const unsigned long long* prow = pp.partial + (size_t)t * partial_stride(D);
              const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
              g.th_hc = first_page && (reads_calc ? c_hc : tt.spec.has_count[t] != 0);
              g.th_c = reads_calc ? c_c : tt.spec.count[t];
              g.th_p = reads_calc ? c_p : pt.s_p;
              u.u_hc = pods_total > 0, u.u_c = pods_total;
              // throttled = calculatedThreshold.IsThrottled(used, true): the lane's own flag bits
              u.c_flag = first_page && c_hc && u.u_hc && pods_total >= c_c;
              u.flag_m = u.pr_m = 0u;
#pragma unroll
              for (int d = 0; d < DT; ++d) {
                base[d] = g.tv[d] = u.u_v[d] = 0;
                if (d >= D) continue;
                g.tv[d] = reads_calc ? c_v[d] : pt.sv[d];
                base[d] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
                if (!((need >> d) & 1u)) continue;  // (wave-uniform)
                u.u_v[d] = (int64_t)prow[d];
                // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
                const bool u_pr = prow[partial_off_presence(D) + d] != 0ull || u.u_v[d] != 0;
                u.pr_m |= u_pr ? 1u << d : 0u;
                if (((c_p >> d) & 1u) && u_pr && u.u_v[d] >= c_v[d]) u.flag_m |= 1u << d;
              }
            }
            int64_t h, first;
            if (err) {  // copy 0 alone, in front of the Error member
              g.r_hc = r_hc, g.r_c = r_c, g.r_p = r_p;
#pragma unroll
              for (int d = 0; d < DT; ++d) g.rv[d] = base[d];
              first = gang_walk<DT>(view, t, i0, bad, g, u), h = 0;
              if (first >= bad) first = i1;  // (nothing is stopped: no candidate for the minimum)
            } else {
              // ---- the range: up to the running minimum, and no further than every amount the lane's threshold names on this
              //      page stays inside int64 (the count's cut where the count is judged: g.th_hc is false off page 0)
              const int64_t run_h = stored ? kept_h : (q < m ? cop[q] : 0);
              const int64_t lim_h = run_h < kept_h ? run_h : kept_h;
              int64_t top = lim_h < cap ? lim_h : cap - 1;
              const int64_t pc = g.th_hc ? per_c : 0;
              if (pc > 0) top = hfgp_fit(r_c, pc, top);
#pragma unroll
              for (int d = 0; d < DT; ++d)
                if (((g.th_p >> d) & 1u) && per[d] > 0) top = hfgp_fit(base[d], per[d], top);
              // ---- the probe at top, then the bisection on [lo, hi): hi has been seen to fail, everything below lo passes
              int64_t lo = 0, hi = top, j = top;
              bool known = false, busy = in;
              first = i1;
              while (__ballot(busy) != 0ull) {
                // (an idle lane walks its last candidate again: its state fits too)
                g.r_hc = r_hc || j > 0, g.r_c = r_c + j * pc, g.r_p = j > 0 ? r_p | per_p : r_p;
#pragma unroll
                for (int d = 0; d < DT; ++d) g.rv[d] = ((g.th_p >> d) & 1u) ? hfgp_row(base[d], j, per[d]) : base[d];
                const int64_t f = gang_walk<DT>(view, t, i0, i1, g, u);
                if (busy) {
                  const bool fails = f < i1;
                  if (fails) hi = j, first = f, known = true;
                  else if (!known) busy = false;  // the pair passes at the running minimum: it changes nothing
                  else lo = j + 1;
                  if (lo >= hi) busy = false;
                  j = busy ? lo + (hi - lo) / 2 : j;
                }
              }
              h = hi;
              if (!known) first = i1;
            }
            // ---- the lexicographic minimum of (h, first, t)
            if (first >= i1) {  // (per lane: the pair stops nothing here)
            } else if (stored) {
              if (h < kept_h || (h == kept_h && (first < kept_first || (first == kept_first && (int32_t)t < kept_t))))
                kept_h = h, kept_first = first, kept_t = (int32_t)t;
            } else if (q < m) {
              const int64_t b_h = cop[q], b_first = blk[q];
              const int32_t b_t = lim[q];
              if (h < b_h || (h == b_h && (first < b_first || (first == b_first && (int32_t)t < b_t)))) cop[q] = h, blk[q] = first, lim[q] = (int32_t)t;
            }
          }
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    int64_t ans = -1;
    for (int64_t q0 = 0; q0 < m; q0 += kWave) {
      const int64_t q = q0 + lane;
      const bool in = q < m;
      int64_t h = 0;
      if (in) {
        h = cop[q];
        int64_t first = blk[q];
        int32_t t = lim[q];
        if (kept_h < h || (kept_h == h && (kept_first < first || (kept_first == first && kept_t < t)))) h = kept_h, first = kept_first, t = kept_t;
        const bool none = !err && h >= cap;  // all cap copies are admitted
        cop[q] = h, blk[q] = none ? -1 : first, lim[q] = none ? -1 : t;
      }
      const uint64_t mk = __ballot(in && h >= want);
      if (mk != 0ull && ans < 0) ans = q0 + (__ffsll((long long)mk) - 1);  // the first position with `want` copies
    }
    if (lane == 0) a.first[gi] = ans;
  }
}

// pages: the descriptors as launch_forecast_gangs_paged takes them; copied to pages_dev, pages_copied recorded behind the copy, as
// there.  false: *hip_err says why
bool launch_headroom_forecast_gangs_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n_gangs,
                                          int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev, const int64_t* inst_s,
                                          const int32_t* inst_ns, int T, bool on_equal, uint32_t cap, uint32_t want, const uint8_t* status,
                                          const uint64_t* summary, int64_t* first, int64_t* copies, int32_t* limiting, int64_t* blocker,
                                          hipStream_t s, hipError_t* hip_err) {
  *hip_err = hipSuccess;
  if (n_gangs <= 0 || m <= 0) return true;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  HeadroomForecastGangsPagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.m = m, a.inst_s = inst_s;
  a.inst_ns = inst_ns, a.status = status, a.summary = summary, a.first = first, a.copies = copies, a.limiting = limiting, a.blocker = blocker;
  a.T = T, a.on_equal = on_equal ? 1 : 0, a.cap = cap, a.want = want;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(PreemptPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_headroom_forecast_gangs_paged<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_headroom_forecast_gangs_paged<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_headroom_forecast_gangs_paged<16>, dim3(blocks), dim3(kWave), 0, s, a);
  return true;
}

}  // namespace kt
