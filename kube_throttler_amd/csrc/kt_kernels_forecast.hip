// kt_kernels_forecast.hip — the first instant at which a blocked pod passes (kt_forecast_launch), gfx950.
//
// For pod p and the caller's ascending instants t_0 .. t_{m-1}, state R_k is the cluster as the engine holds it, every valid and
// responsible throttle reconciled at t_k (throttle_controller.go:116-133: used = fold Add over the counted pods,
// CalculateThreshold(t_k), throttled = IsThrottled(used, true), calculatedThreshold replaced only where threshold or messages
// differ by value).  first(p) is the smallest k for which PreFilter(p) (plugin.go:148-215) is Success in R_k.  `used` does not
// depend on k, the threshold does not depend on the pod, and the four CheckThrottledFor steps (throttle_types.go:128-153) are
// independent per (affecting throttle, resource name or pod count): EVERY k is judged, in parallel, lane = instant position —
// kt_preempt turned by ninety degrees.
//
//   input   status matrix [n][T] and summary words of ONE check over the pods (which throttles match which pod; error rows), pod
//           flags and request rows, the partial rows of an aggregate with EXACT per-name contributor counts, the error bytes of a
//           dry finalize (they do not depend on the instant), the stored tables (spec, calc, used, throttled, reserved, both
//           message fingerprints, the override tables), the instants.  All read-only.
//   per pod (one wave, the grid strides) the affecting throttles chunk by chunk through a 4 KiB LDS list (as kt_preempt); per
//           throttle the instants 64 at a time: the throttle's overrides are walked in order with wave-uniform loads, every lane
//           decides activity at its own instant (begin <= t && (end is zero || t <= end), a parse error is never active) and merges
//           "first active override wins" per name and for the count; without an active override spec.threshold.  Then `replace`
//           (by value against the stored calculatedThreshold, plus the messages fingerprint, which depends on parse errors only),
//           the threshold the check reads (calculatedThreshold iff calculatedAt was non-zero or this reconcile replaces it, else
//           spec.threshold), throttled from the fresh sums against the calculated threshold, and the four steps.  A throttle
//           that keeps its stored status (reconcile error, not valid or not responsible) is judged once, wave-uniform.
//   output  verdicts[i][k] = KT_VERDICT_*: a lane stores 1 into the bytes of its own positions where some (throttle, amount)
//           pair stops the pod; first[i] = the first position whose byte is 0 (ballot over the blocks in order), or -1.
#include "kt_admit_common.h"

namespace kt {

struct ForecastArgs {
  AdmitPage pg;                       // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;                // [n] pod table rows
  int64_t n, m;                       // pods, instants
  const int64_t* inst_s;              // [m] strictly ascending
  const int32_t* inst_ns;             // [m]
  const uint8_t* status;              // [n][T]
  const uint64_t* summary;            // [n]
  const unsigned long long* partial;  // [T][partial_stride(D)], exact contributor counts
  const uint8_t* error;               // [T] the reconcile is an error: the stored status stays
  int64_t* first;                     // [n] out
  uint8_t* verdicts;                  // [n][m] out
  int32_t T, on_equal;
};

template <int DT>
__global__ __launch_bounds__(kWave) void kt_forecast(const ForecastArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  const int stride = partial_stride(D);
  const int64_t n = a.n, m = a.m;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {  // (wave-uniform: one pod per wave and turn)
    const int64_t p = a.rows[i];
    uint8_t* ver = a.verdicts + i * m;
    for (int64_t q = lane; q < m; q += kWave) ver[q] = 0;
    const uint8_t* row = a.status + i * T;
    bool err = a.summary[i] == 2ull || !(a.pg.pod_flags[p] & kPodValid);
    bool never = false;  // a throttle that keeps its stored status stops the pod: at every instant
    for (int c0 = 0; c0 < T && !err && !never; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      err = __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c && !err && !never; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        const uint32_t tf = tt.flags[t];
        const bool stored = a.error[t] != 0 || (tf & (kThrValid | kThrResponsible)) != (kThrValid | kThrResponsible);
        const bool eq3 = admit_eq3(tf, eq);
        const bool r_hc = tt.reserved.has_count[t] != 0;
        const int64_t r_c = tt.reserved.count[t];
        const uint32_t r_p = tt.reserved.present[t];
        if (stored) {  // nothing of it depends on the instant
          const AmountTab& th = admit_threshold(tt, tf);
          const uint32_t th_p = th.present[t], u_p = tt.used.present[t], flg = tt.thrl_flag[t] & tt.thrl_has[t];
          bool f = preempt_fails(1, th.has_count[t] != 0, th.count[t], (tf & kThrThrottledPod) != 0, tt.used.has_count[t] != 0, tt.used.count[t],
                                 r_hc, r_c, eq3, eq);
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (d >= D) continue;
            const int64_t vpd = a.pg.req[p * DS + d];
            if (vpd == 0) continue;
            f |= preempt_fails(vpd, (th_p >> d) & 1u, th.v[(size_t)t * D + d], (flg >> d) & 1u, (u_p >> d) & 1u, tt.used.v[(size_t)t * D + d],
                               (r_p >> d) & 1u, tt.reserved.v[(size_t)t * D + d], eq3, eq);
          }
          never = f;
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
        const bool u_hc = pods_total > 0;
        // the names some threshold of this throttle can name, and whether an override has a parse error (the messages of
        // CalculateThreshold: they do not depend on the instant)
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
          vp[d] = a.pg.req[p * DS + d];
          // a name the pod does not request passes every step, and so does one that no threshold names
          need[d] = vp[d] != 0 && ((names >> d) & 1u);
          if (!need[d]) continue;
          rv[d] = tt.reserved.v[(size_t)t * D + d];
          tot_v[d] = (int64_t)prow[d];
          // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
          u_pr[d] = prow[partial_off_presence(D) + d] != 0ull || tot_v[d] != 0;
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
          // ---- replace the stored calculatedThreshold only if threshold or messages differ by value (where they do not, the
          //      stored one equals the computed one by value: the lane goes on with its own)
          const bool same = (c_hc == k_hc) && (!c_hc || c_c == k_c) && c_p == k_p && !diff;
          const bool replace = !same || fp_differs;
          // ---- the threshold the check reads behind this reconcile: calculatedThreshold once calculatedAt is set, else spec
          const bool reads_calc = (tf & kThrCalcAtNonzero) || replace;
          const bool th_hc = reads_calc ? c_hc : s_hc;
          const int64_t th_c = reads_calc ? c_c : s_c;
          const uint32_t th_p = reads_calc ? c_p : s_p;
          // ---- throttled = calculatedThreshold.IsThrottled(used, true), then the four steps
          bool f = preempt_fails(1, th_hc, th_c, c_hc && u_hc && pods_total >= c_c, u_hc, pods_total, r_hc, r_c, eq3, eq);
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (!need[d]) continue;  // (wave-uniform)
            const bool flagged = ((c_p >> d) & 1u) && u_pr[d] && tot_v[d] >= c_v[d];
            f |= preempt_fails(vp[d], (th_p >> d) & 1u, reads_calc ? c_v[d] : sv[d], flagged, u_pr[d], tot_v[d], (r_p >> d) & 1u, rv[d], eq3, eq);
          }
          if (in && f) ver[q] = (uint8_t)1;  // KT_VERDICT_UNSCHEDULABLE; the lane's own byte
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

void launch_forecast(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns, int T,
                     bool on_equal, const uint8_t* status, const uint64_t* summary, const unsigned long long* partial, const uint8_t* error,
                     int64_t* first, uint8_t* verdicts, hipStream_t s) {
  if (n <= 0 || m <= 0) return;
  ForecastArgs a{};
  a.pg = pg, a.rows = rows_dev, a.n = n, a.m = m, a.inst_s = inst_s, a.inst_ns = inst_ns, a.status = status, a.summary = summary;
  a.partial = partial, a.error = error, a.first = first, a.verdicts = verdicts, a.T = T, a.on_equal = on_equal ? 1 : 0;
  const int blocks = (int)(n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_forecast<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_forecast<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_forecast<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
