// kt_kernels_forecast_gangs.hip — the first instant at which a whole gang is admitted (kt_forecast_gangs_launch), gfx950.
//
// kt_forecast (kt_kernels_forecast.hip) and gang_walk (kt_admit_common.h) turned towards each other.  Gang g is the queue
// positions [gang_off[g], gang_off[g + 1]); in state R_k (every valid and responsible throttle reconciled at the caller's instant
// t_k) its members get PreFilter in order and every admitted member reserves on the throttles that affect it, exactly as
// kt_admit's Reserve does.  The gang passes at t_k iff every (member, affecting throttle, amount) passes its four steps against
// the threshold of R_k and the reserved prefix of that member.  `used` does not depend on k and the reserved prefix does not
// depend on k either (a member reserves whatever it asks): only the threshold values and the throttled flags are the lane's own.
//
//   input   as kt_forecast: status matrix and summary words of ONE check over the members of all gangs, the partial rows of an
//           aggregate with exact contributor counts, the error bytes of a dry finalize, the stored tables, the instants; and the
//           gang offsets.  All read-only.
//   per gang (one wave, the grid strides) the first member whose PreFilter is an error or whose row is invalid by a ballot over
//           member blocks of 64; the UNION of the members' affecting throttles chunk by chunk through the 4 KiB LDS list; per
//           throttle one batch of wave-uniform loads (as kt_forecast), then the instants 64 at a time: every lane computes
//           CalculateThreshold at its own instant, `replace`, the threshold the check reads and the throttled bits from the
//           fresh sums, fills a GangThr / GangUsed of its own and calls gang_walk — the member loop is wave-uniform.  A throttle
//           that keeps its stored status is walked once, wave-uniform: its result holds at every instant.
//   output  verdicts[g][k] = KT_VERDICT_*, blocker[g][k] = the first queue position that is not Success at t_k (-1: none), kept
//           by the lane in the bytes of its own positions while the kernel runs; first[g] = the first position whose verdict is
//           0 (ballot over the blocks in order), or -1.
#include "kt_admit_common.h"

namespace kt {

struct ForecastGangArgs {
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
  uint8_t* verdicts;                  // [n_gangs][m] out
  int64_t* blocker;                   // [n_gangs][m] out
  int32_t T, on_equal;
};

template <int DT>
__global__ __launch_bounds__(kWave) void kt_forecast_gangs(const ForecastGangArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  const int stride = partial_stride(D);
  const int64_t m = a.m;
  for (int64_t gi = blockIdx.x; gi < a.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
    uint8_t* ver = a.verdicts + gi * m;
    int64_t* blk = a.blocker + gi * m;
    // the first member whose PreFilter is an error or whose row is invalid: it is not Success at any instant
    int64_t bad = i1;
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(a.pg.pod_flags[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        bad = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    // while the kernel runs blk[q] holds the first stopped position over the throttles so far, i1: none
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
        const uint32_t tf = tt.flags[t];
        const bool stored = preempt_row_stored(tf, a.error[t]);
        GangThr<DT> g;
        g.eq = eq, g.eq3 = admit_eq3(tf, eq);
        g.r_hc = tt.reserved.has_count[t] != 0, g.r_c = tt.reserved.count[t], g.r_p = tt.reserved.present[t];
        GangUsed<DT> u;
        if (stored) {  // nothing of it depends on the instant
          const AmountTab& th = admit_threshold(tt, tf);
          g.th_hc = th.has_count[t] != 0, g.th_c = th.count[t], g.th_p = th.present[t];
          u.c_flag = (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
          u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            g.tv[d] = g.rv[d] = u.u_v[d] = 0;
            if (d >= D) continue;
            g.tv[d] = th.v[(size_t)t * D + d], g.rv[d] = tt.reserved.v[(size_t)t * D + d], u.u_v[d] = tt.used.v[(size_t)t * D + d];
          }
          const int64_t first = gang_walk<DT>(a, t, i0, i1, g, u);
          stored_first = first < stored_first ? first : stored_first;
          continue;
        }
        // ---- the throttle's own state: one batch of wave-uniform loads
        const uint32_t ovr0 = tt.ovr_off[t], ovr1 = tt.ovr_off[t + 1];
        const uint64_t status_fp = tt.status_msgs_fp[t], spec_fp = tt.spec_msgs_fp[t];
        const bool s_hc = tt.spec.has_count[t] != 0, k_hc = tt.calc.has_count[t] != 0;
        const int64_t s_c = tt.spec.count[t], k_c = tt.calc.count[t];
        const uint32_t s_p = tt.spec.present[t], k_p = tt.calc.present[t];
        const unsigned long long* prow = a.partial + (size_t)t * stride;
        const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
        u.u_hc = pods_total > 0, u.u_c = pods_total;
        // the names some threshold of this throttle can name, and whether an override has a parse error (the messages of
        // CalculateThreshold: they do not depend on the instant)
        uint32_t names = s_p | k_p;
        bool any_err = false;
        for (uint32_t o = ovr0; o < ovr1; ++o) {
          if (tt.ovr_flags[o] & kOvrParseError) any_err = true;
          else names |= tt.ovr_thr.present[o];
        }
        const bool fp_differs = status_fp != (any_err ? spec_fp : 0ull);
        // the names some affected member requests and some threshold can name: the others pass every step of every member
        uint32_t need = 0;
        for (int64_t i = i0; i < i1; ++i) {
          if (a.status[i * (int64_t)T + t] == 0) continue;
          const int64_t p = a.rows[i];
          for (int d = 0; d < D; ++d) need |= a.pg.req[p * DS + d] != 0 ? 1u << d : 0u;
        }
        need &= names;
        int64_t sv[DT], kv[DT];
        bool spec_diff = false;  // spec.threshold against the stored calculatedThreshold, by value, over the names spec has
        u.pr_m = 0u;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          sv[d] = kv[d] = g.rv[d] = u.u_v[d] = 0;
          if (d >= D) continue;
          sv[d] = tt.spec.v[(size_t)t * D + d], kv[d] = tt.calc.v[(size_t)t * D + d];
          spec_diff |= ((s_p >> d) & 1u) && sv[d] != kv[d];
          g.rv[d] = tt.reserved.v[(size_t)t * D + d];
          if (!((need >> d) & 1u)) continue;
          u.u_v[d] = (int64_t)prow[d];
          // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
          if (prow[partial_off_presence(D) + d] != 0ull || u.u_v[d] != 0) u.pr_m |= 1u << d;
        }
        for (int64_t q0 = 0; q0 < m; q0 += kWave) {
          const int64_t q = q0 + lane;
          const bool in = q < m;
          const int64_t ts = a.inst_s[in ? q : m - 1];
          const int32_t tn = a.inst_ns[in ? q : m - 1];
          // ---- CalculateThreshold(t): first active override wins, per name and for the count
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
          const int64_t first = gang_walk<DT>(a, t, i0, i1, g, u);
          if (in && first < blk[q]) blk[q] = first;  // the lane's own word
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

void launch_forecast_gangs(const AdmitPage& pg, int64_t n_gangs, int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev,
                           const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, const uint8_t* status, const uint64_t* summary,
                           const unsigned long long* partial, const uint8_t* error, int64_t* first, uint8_t* verdicts, int64_t* blocker,
                           hipStream_t s) {
  if (n_gangs <= 0 || m <= 0) return;
  ForecastGangArgs a{};
  a.pg = pg, a.rows = rows_dev, a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.m = m, a.inst_s = inst_s, a.inst_ns = inst_ns;
  a.status = status, a.summary = summary, a.partial = partial, a.error = error, a.first = first, a.verdicts = verdicts, a.blocker = blocker;
  a.T = T, a.on_equal = on_equal ? 1 : 0;
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_forecast_gangs<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_forecast_gangs<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_forecast_gangs<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
