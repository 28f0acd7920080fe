// kt_kernels_headroom_forecast_gangs.hip — how many copies of a whole gang the throttles admit at each of a list of instants
// (kt_headroom_forecast_gangs_launch), gfx950.
//
// kt_forecast_gangs (kt_kernels_forecast_gangs.hip) and kt_headroom_gangs (kt_kernels_headroom_gangs.hip) joined: the first has the
// threshold of state R_k at a lane's instant t_k, the second the search over the copies with gang_walk (kt_admit_common.h) as
// judge.  copies[g][k] is headroom(gang g, cap) with R_k as the stored status: the leading admitted gangs of a dry kt_admit_gangs
// over `cap` consecutive copies.  As in kt_headroom_gangs copy j meets on throttle t the stored reserved row plus j * A_t, the
// throttles are independent given that, and with non-negative requests passes_t(j) is monotone in j: h_t is found by search.  `used`
// and A_t do not depend on k; the threshold and the throttled flags are the lane's own, so the SEARCH is the lane's own too: lane =
// instant position, every lane bisects its own range, and the walks of one round run side by side (gang_walk's member loop is
// wave-uniform, the candidate's reserved row is the lane's).
//
//   input   that of kt_forecast_gangs (status matrix and summary words of ONE check over the members of all gangs, the partial rows
//           of an aggregate with exact contributor counts, the error bytes of a dry finalize, the stored tables, the instants, the
//           gang offsets), plus cap and want.  Read-only.
//   per gang (one wave, the grid strides) the first member whose PreFilter is an error or whose row is invalid by a ballot over
//           member blocks of 64; the UNION of the members' affecting throttles chunk by chunk through the 4 KiB LDS list; per
//           throttle one batch of wave-uniform loads (as kt_forecast_gangs) and A_t from one pass over the members (as
//           kt_headroom_gangs, over the names ANY threshold of the throttle can name); then the instants 64 at a time:
//     1     the lane computes CalculateThreshold at its instant, `replace`, the threshold the check reads and the throttled bits
//           from the fresh sums: a GangThr / GangUsed of its own;
//     2     its range: up to its running minimum for this position (cap - 1 while nothing binds), and no further than every amount
//           ITS threshold names stays inside int64 (hfg_fit; the bound is kt_headroom_gangs': a copy that passes has passed step 4
//           of a member that asks for the name, which takes a threshold that names it).  An amount the lane's threshold does not
//           name never decides: nothing is multiplied into its row;
//     3     the probe at the top of the range (it passes: the throttle changes nothing for the lane), then a bisection below it for
//           the first failing candidate, while a ballot says some lane still searches: 1 + 31 rounds at the most.  In every round
//           every searching lane fills the reserved row of its own candidate and calls gang_walk; `first` is kept from the probe
//           at j = h_t;
//     4     the lane's running answer is the lexicographic minimum of (h, first, t) — the row is a key: the chunk list is not in
//           row order.  It lives in the lane's own cells of the three [n_gangs][m] output buffers, written only where a throttle
//           lowers it.
//           A throttle that keeps its stored status (reconcile error, not valid or not responsible) is judged ONCE through the same
//           steps 2-3 from the stored tables as kt_headroom_gangs reads them, every lane alike; its triple is folded into every
//           position at the end.  A gang with an Error / invalid member: copy 0 alone, the walk ends in front of that member, with
//           the lane's thresholds (the blocker may differ per instant).
//   output  copies[g][k] = min(cap, h); blocker[g][k] / limiting[g][k] = first / t of the minimum, -1 where h >= cap (limiting
//           also where the blocker is the Error member); first[g] = the first position with copies >= want (ballot over the blocks
//           in order), or -1.
#include "kt_admit_common.h"

namespace kt {

struct HeadroomForecastGangArgs {
  AdmitPage pg;                       // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;                // [n] pod table rows: the members of all gangs
  const int64_t* gang_off;            // [n_gangs + 1] queue positions
  int64_t n_gangs, m;                 // gangs, instants
  const int64_t* inst_s;              // [m] strictly ascending
  const int32_t* inst_ns;             // [m]
  const uint8_t* status;              // [n][T]
  const uint64_t* summary;            // [n]
  const unsigned long long* partial;  // [T][partial_stride(D)], exact contributor counts
  const uint8_t* error;               // [T] the reconcile is an error: the stored status stays
  int64_t* first;                     // [n_gangs] out
  int64_t* copies;                    // [n_gangs][m] out (and the running h of every position while the kernel runs)
  int32_t* limiting;                  // [n_gangs][m] out (... its row)
  int64_t* blocker;                   // [n_gangs][m] out (... its first stopped position)
  int32_t T, on_equal;
  uint32_t cap, want;                 // 1 <= want <= cap <= 2^31 - 1
};

constexpr int64_t kHfgInt64Max = 0x7FFFFFFFFFFFFFFFll;

// the candidates of one amount end at (INT64_MAX - base) / per: beyond, reserved + (j + 1) per has left int64 (per > 0)
__device__ __forceinline__ int64_t hfg_fit(int64_t base, int64_t per, int64_t top) {
  const uint64_t q = ((uint64_t)kHfgInt64Max - (uint64_t)base) / (uint64_t)per;  // (base may be negative: the difference fits 64 bits)
  return q < (uint64_t)top ? (int64_t)q : top;
}
// base + j * per of a candidate inside its range (the result fits int64; formed modulo 2^64, which has no undefined corner)
__device__ __forceinline__ int64_t hfg_row(int64_t base, int64_t j, int64_t per) { return (int64_t)((uint64_t)base + (uint64_t)j * (uint64_t)per); }

template <int DT>
__global__ __launch_bounds__(kWave) void kt_headroom_forecast_gangs(const HeadroomForecastGangArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  const int stride = partial_stride(D);
  const int64_t m = a.m, cap = (int64_t)a.cap, want = (int64_t)a.want;
  for (int64_t gi = blockIdx.x; gi < a.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
    int64_t* cop = a.copies + gi * m;  // the lane's own cells: positions lane, lane + 64, ...
    int32_t* lim = a.limiting + gi * m;
    int64_t* blk = a.blocker + gi * m;
    // the first member whose PreFilter is an error or whose row is invalid: copy 0 is not admitted, the walk ends in front of it
    int64_t bad = i1;
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(a.pg.pod_flags[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        bad = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    const bool err = bad < i1;
    const int64_t h0 = err ? 0 : cap;
    for (int64_t q = lane; q < m; q += kWave) cop[q] = h0, blk[q] = bad, lim[q] = -1;
    // the minimum over the throttles that keep their stored status: it holds at every instant (every lane holds the same)
    int64_t kept_h = h0, kept_first = bad;
    int32_t kept_t = -1;
    for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
      bool err_c = false;  // (the error rows are the summary's: `bad` above)
      const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        const uint32_t tf = tt.flags[t];
        const bool stored = preempt_row_stored(tf, a.error[t]);
        GangThr<DT> g;
        GangUsed<DT> u;
        g.eq = eq, g.eq3 = admit_eq3(tf, eq);
        const bool r_hc = tt.reserved.has_count[t] != 0;
        const int64_t r_c = r_hc ? tt.reserved.count[t] : 0;  // a reserved amount whose presence bit is clear reads as 0
        const uint32_t r_p = tt.reserved.present[t];
        // ---- what does not depend on the instant: one batch of wave-uniform loads
        uint32_t ovr0 = 0, ovr1 = 0, s_p = 0, k_p = 0, names = 0, need = 0;
        bool s_hc = false, k_hc = false, fp_differs = false, spec_diff = false;
        int64_t s_c = 0, k_c = 0, pods_total = 0;
        int64_t sv[DT], kv[DT], base[DT], per[DT];  // spec / calc rows, the stored reserved row (0 where absent), A_t's values
        if (stored) {  // the stored tables as kt_headroom_gangs reads them
          const AmountTab& th = admit_threshold(tt, tf);
          g.th_hc = th.has_count[t] != 0, g.th_c = th.count[t], g.th_p = th.present[t];
          u.c_flag = (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
          u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
          names = g.th_p;
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            sv[d] = kv[d] = base[d] = per[d] = g.tv[d] = u.u_v[d] = 0;
            if (d >= D) continue;
            g.tv[d] = th.v[(size_t)t * D + d], u.u_v[d] = tt.used.v[(size_t)t * D + d];
            base[d] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
          }
        } else {
          ovr0 = tt.ovr_off[t], ovr1 = tt.ovr_off[t + 1];
          const uint64_t status_fp = tt.status_msgs_fp[t], spec_fp = tt.spec_msgs_fp[t];
          s_hc = tt.spec.has_count[t] != 0, k_hc = tt.calc.has_count[t] != 0;
          s_c = tt.spec.count[t], k_c = tt.calc.count[t];
          s_p = tt.spec.present[t], k_p = tt.calc.present[t];
          const unsigned long long* prow = a.partial + (size_t)t * stride;
          pods_total = (int64_t)prow[partial_off_pods(D)];
          u.u_hc = pods_total > 0, u.u_c = pods_total;
          // the names some threshold of this throttle can name, and whether an override has a parse error (the messages of
          // CalculateThreshold: they do not depend on the instant)
          names = s_p | k_p;
          bool any_err = false;
          for (uint32_t o = ovr0; o < ovr1; ++o) {
            if (tt.ovr_flags[o] & kOvrParseError) any_err = true;
            else names |= tt.ovr_thr.present[o];
          }
          fp_differs = status_fp != (any_err ? spec_fp : 0ull);
          // the names some affected member requests and some threshold can name: the others pass every step of every member
          for (int64_t i = i0; i < i1; ++i) {
            if (a.status[i * (int64_t)T + t] == 0) continue;
            const int64_t p = a.rows[i];
            for (int d = 0; d < D; ++d) need |= a.pg.req[p * DS + d] != 0 ? 1u << d : 0u;
          }
          need &= names;
          u.pr_m = 0u;
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            sv[d] = kv[d] = base[d] = per[d] = g.tv[d] = u.u_v[d] = 0;
            if (d >= D) continue;
            sv[d] = tt.spec.v[(size_t)t * D + d], kv[d] = tt.calc.v[(size_t)t * D + d];
            spec_diff |= ((s_p >> d) & 1u) && sv[d] != kv[d];
            base[d] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
            if (!((need >> d) & 1u)) continue;
            u.u_v[d] = (int64_t)prow[d];
            // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
            if (prow[partial_off_presence(D) + d] != 0ull || u.u_v[d] != 0) u.pr_m |= 1u << d;
          }
        }
        // ---- A_t: what one admitted copy reserves on t, one pass over the members.  A name is summed where SOME threshold of the
        //      throttle can name it (the lane's own is not known yet); the lane masks below
        int64_t per_c = 0;
        uint32_t per_p = 0;
        if (!err)
          for (int64_t i = i0; i < i1; ++i) {
            if (a.status[i * (int64_t)T + t] == 0) continue;
            const int64_t p = a.rows[i];
            const uint32_t present = (a.pg.pod_flags[p] >> kPresentShift) & ((1u << D) - 1u);
            per_c += 1, per_p |= present;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d >= D || !(((present & names) >> d) & 1u)) continue;
              const int64_t v = a.pg.req[p * DS + d];
              per[d] = v > kHfgInt64Max - per[d] ? kHfgInt64Max : per[d] + v;  // (saturated: the range then ends at copy 0 or 1)
            }
          }
        for (int64_t q0 = 0; q0 < (stored ? 1 : m); q0 += kWave) {
          const int64_t q = q0 + lane;
          const bool in = stored || q < m;
          if (!stored) {
            const int64_t ts = a.inst_s[q < m ? q : m - 1];
            const int32_t tn = a.inst_ns[q < m ? q : m - 1];
            // ---- step 1.  CalculateThreshold(t): first active override wins, per name and for the count
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
              c_p = s_p, c_hc = s_hc, c_c = s_c, diff = spec_diff;
#pragma unroll
              for (int d = 0; d < DT; ++d) c_v[d] = sv[d];
            }
            // ---- replace the stored calculatedThreshold only if threshold or messages differ by value
            const bool same = (c_hc == k_hc) && (!c_hc || c_c == k_c) && c_p == k_p && !diff;
            const bool replace = !same || fp_differs;
            // ---- the threshold the check reads behind this reconcile: calculatedThreshold once calculatedAt is set, else spec
            const bool reads_calc = (tf & kThrCalcAtNonzero) || replace;
            g.th_hc = reads_calc ? c_hc : s_hc;
            g.th_c = reads_calc ? c_c : s_c;
            g.th_p = reads_calc ? c_p : s_p;
            // ---- throttled = calculatedThreshold.IsThrottled(used, true): the lane's own flag bits
            u.c_flag = c_hc && u.u_hc && pods_total >= c_c;
            u.flag_m = 0u;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              g.tv[d] = reads_calc ? c_v[d] : sv[d];
              if (!((need >> d) & 1u)) continue;  // (wave-uniform)
              if (((c_p >> d) & 1u) && ((u.pr_m >> d) & 1u) && u.u_v[d] >= c_v[d]) u.flag_m |= 1u << d;
            }
          }
          int64_t h, first;
          if (err) {  // copy 0 alone, in front of the Error member
            g.r_hc = r_hc, g.r_c = r_c, g.r_p = r_p;
#pragma unroll
            for (int d = 0; d < DT; ++d) g.rv[d] = base[d];
            first = gang_walk<DT>(a, t, i0, bad, g, u), h = 0;
            if (first >= bad) first = i1;  // (nothing is stopped: no candidate for the minimum)
          } else {
            // ---- step 2.  The range: up to the running minimum, and no further than every amount the lane's threshold names
            //      stays inside int64
            const int64_t run_h = stored ? kept_h : (q < m ? cop[q] : 0);
            const int64_t lim_h = run_h < kept_h ? run_h : kept_h;
            int64_t top = lim_h < cap ? lim_h : cap - 1;
            const int64_t pc = g.th_hc ? per_c : 0;
            if (pc > 0) top = hfg_fit(r_c, pc, top);
#pragma unroll
            for (int d = 0; d < DT; ++d)
              if (((g.th_p >> d) & 1u) && per[d] > 0) top = hfg_fit(base[d], per[d], top);
            // ---- step 3.  The probe at top, then the bisection on [lo, hi): hi has been seen to fail, everything below lo passes
            int64_t lo = 0, hi = top, j = top;
            bool known = false, busy = in;
            first = i1;
            while (__ballot(busy) != 0ull) {
              // (an idle lane walks its last candidate again: its state fits too)
              g.r_hc = r_hc || j > 0, g.r_c = r_c + j * pc, g.r_p = j > 0 ? r_p | per_p : r_p;
#pragma unroll
              for (int d = 0; d < DT; ++d) g.rv[d] = ((g.th_p >> d) & 1u) ? hfg_row(base[d], j, per[d]) : base[d];
              const int64_t f = gang_walk<DT>(a, t, i0, i1, g, u);
              if (busy) {
                const bool fails = f < i1;
                if (fails) hi = j, first = f, known = true;
                else if (!known) busy = false;  // the throttle passes at the running minimum: it changes nothing
                else lo = j + 1;
                if (lo >= hi) busy = false;
                j = busy ? lo + (hi - lo) / 2 : j;
              }
            }
            h = hi;
            if (!known) first = i1;
          }
          // ---- step 4.  The lexicographic minimum of (h, first, t)
          if (first >= i1) {  // (per lane: the throttle stops nothing here)
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

void launch_headroom_forecast_gangs(const AdmitPage& pg, int64_t n_gangs, int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev,
                                    const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, uint32_t cap, uint32_t want,
                                    const uint8_t* status, const uint64_t* summary, const unsigned long long* partial, const uint8_t* error,
                                    int64_t* first, int64_t* copies, int32_t* limiting, int64_t* blocker, hipStream_t s) {
  if (n_gangs <= 0 || m <= 0) return;
  HeadroomForecastGangArgs a{};
  a.pg = pg, a.rows = rows_dev, a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.m = m, a.inst_s = inst_s, a.inst_ns = inst_ns;
  a.status = status, a.summary = summary, a.partial = partial, a.error = error, a.first = first, a.copies = copies, a.limiting = limiting;
  a.blocker = blocker, a.T = T, a.on_equal = on_equal ? 1 : 0, a.cap = cap, a.want = want;
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_headroom_forecast_gangs<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_headroom_forecast_gangs<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_headroom_forecast_gangs<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
