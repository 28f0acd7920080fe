// kt_kernels_preempt.hip — the shortest victim prefix that lets a blocked pod through (kt_preempt_launch), gfx950.
//
// For preemptor p and the caller-ordered candidates c_0 .. c_{m-1}, state S_k is the cluster without c_0 .. c_{k-1}, every
// responsible throttle reconciled at `now` (throttle_controller.go:116-133: used = fold Add over the counted pods,
// CalculateThreshold(now), throttled = IsThrottled(used, true)).  prefix(p) is the smallest k for which PreFilter(p)
// (plugin.go:148-215) is Success in S_k.  Deleting a prefix lowers every `used` by a prefix sum of the candidates' amounts, the
// threshold does not depend on k, and the four CheckThrottledFor steps (throttle_types.go:128-153) of p are independent per
// (affecting throttle, resource name or pod count): EVERY k is judged, in parallel, lane = candidate position — nothing is
// walked and nothing is bisected, so requests of either sign cannot make the answer wrong.
//
//   input   status matrix [n + m][T] and summary words of ONE check over preemptors ++ candidates (which throttles match
//           which pod; error rows), pod flags and request rows, the partial rows of an aggregate with EXACT per-name
//           contributor counts (values, contributors, counted pods per throttle), the calculated threshold of a dry finalize at
//           `now` with its calc_updated / error bytes, the stored tables (spec, reserved; used and throttled for rows whose
//           reconcile is an error: they keep their stored status in every S_k).  All read-only.
//   per preemptor (one wave, the grid strides) the affected throttles chunk by chunk through a 4 KiB LDS list (as kt_headroom);
//           per throttle the candidates 64 at a time: a wave inclusive scan of the lane's contribution (value and contributor
//           bit per requested name, 1 for the pod count; zero unless the candidate is counted and matched) plus the carry of
//           the earlier blocks, then the four steps at the lane's prefix length.  The verdict bits of all (throttle, amount)
//           pairs meet in the preemptor's row of the victim buffer (bit 1: some pair fails at k = position + 1; bit 0: the
//           candidate is counted and matched by an affecting throttle) — a lane only ever touches the bytes of its own
//           positions.  k = 0 is judged once per pair, wave-uniform.
//   output  prefix[i]: 0, the first position whose fail bit is clear + 1, or -1; victims[i][j] = j < prefix && bit 0.
//           The list is cut (m_eff) before the first candidate whose own check row is an error or whose row is invalid.
#include "kt_admit_common.h"

namespace kt {

template <int DT>
__global__ __launch_bounds__(kWave) void kt_preempt(const PreemptArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  const int stride = partial_stride(D);
  const int64_t n = a.n, m = a.m;
  const int64_t m_eff = preempt_m_eff(a, lane);  // the list ends before the first candidate whose PreFilter is an error or whose row is invalid
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {  // (wave-uniform: one preemptor per wave and turn)
    const int64_t p = a.rows[i];
    uint8_t* vic = a.victims + i * m;
    for (int64_t q = lane; q < m; q += kWave) vic[q] = 0;
    const uint8_t* row = a.status + i * T;
    bool err = a.summary[i] == 2ull || !(a.pg.pod_flags[p] & kPodValid);
    bool fail0 = false;  // some (throttle, amount) stops the pod in S_0
    bool never = false;  // ... in every S_k: a row that keeps its stored status fails
    for (int c0 = 0; c0 < T && !err && !never; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      err = __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c && !err && !never; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        const uint32_t tf = tt.flags[t];
        const bool stored = preempt_row_stored(tf, a.error[t]);
        const AmountTab& th = preempt_threshold(tt, a.calc, tf, a.calc_updated[t]);
        const bool eq3 = admit_eq3(tf, eq);
        const bool th_hc = th.has_count[t] != 0, c_hc = a.calc.has_count[t] != 0, r_hc = tt.reserved.has_count[t] != 0;
        const int64_t th_c = th.count[t], c_c = a.calc.count[t], r_c = tt.reserved.count[t];
        const uint32_t th_p = th.present[t], c_p = a.calc.present[t], r_p = tt.reserved.present[t];
        const unsigned long long* prow = a.partial + (size_t)t * stride;
        const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
        int64_t vp[DT], tv[DT], cv[DT], rv[DT], tot_v[DT], tot_c[DT];
        bool need[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          need[d] = false, vp[d] = tv[d] = cv[d] = rv[d] = tot_v[d] = tot_c[d] = 0;
          if (d >= D) continue;
          vp[d] = a.pg.req[p * DS + d];
          // a name the pod does not request passes every step, and so does one that neither threshold names
          need[d] = vp[d] != 0 && (((th_p | c_p) >> d) & 1u);
          if (!need[d]) continue;
          tv[d] = th.v[(size_t)t * D + d], cv[d] = a.calc.v[(size_t)t * D + d], rv[d] = tt.reserved.v[(size_t)t * D + d];
          tot_v[d] = (int64_t)prow[d], tot_c[d] = (int64_t)prow[partial_off_presence(D) + d];
        }
        if (stored) {
          const bool u_hc = tt.used.has_count[t] != 0;
          bool f = preempt_fails(1, th_hc, th_c, (tf & kThrThrottledPod) != 0, u_hc, tt.used.count[t], r_hc, r_c, eq3, eq);
          const uint32_t u_p = tt.used.present[t], flg = tt.thrl_flag[t] & tt.thrl_has[t];
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (d >= D || vp[d] == 0) continue;
            const int64_t tvd = th.v[(size_t)t * D + d];
            f |= preempt_fails(vp[d], (th_p >> d) & 1u, tvd, (flg >> d) & 1u, (u_p >> d) & 1u, tt.used.v[(size_t)t * D + d], (r_p >> d) & 1u,
                               tt.reserved.v[(size_t)t * D + d], eq3, eq);
          }
          never = f;
        } else {  // k = 0
          bool f = preempt_count_fails(th_hc, th_c, c_hc, c_c, pods_total, r_hc, r_c, eq3, eq);
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (!need[d]) continue;
            f |= preempt_name_fails(vp[d], (th_p >> d) & 1u, tv[d], (c_p >> d) & 1u, cv[d], tot_v[d], tot_c[d], (r_p >> d) & 1u, rv[d], eq3, eq);
          }
          fail0 |= f;
        }
        // every k >= 1, 64 positions at a time
        int64_t car_v[DT], car_pods = 0;
        uint32_t car_c[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) car_v[d] = 0, car_c[d] = 0u;
        for (int64_t q0 = 0; q0 < m_eff && !never; q0 += kWave) {
          const int64_t q = q0 + lane;
          const PreemptCand L = preempt_cand(a, t, q, m_eff);
          bool f = false;
          if (!stored) {
            const int64_t pre_pods = preempt_scan_pods(L, lane, car_pods);
            f = preempt_count_fails(th_hc, th_c, c_hc, c_c, pods_total - pre_pods, r_hc, r_c, eq3, eq);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (!need[d]) continue;  // (wave-uniform)
              int64_t pre_v;
              uint32_t pre_c;
              preempt_scan_name(a, L, d, lane, car_v[d], car_c[d], &pre_v, &pre_c);
              f |= preempt_name_fails(vp[d], (th_p >> d) & 1u, tv[d], (c_p >> d) & 1u, cv[d], tot_v[d] - pre_v, tot_c[d] - (int64_t)pre_c, (r_p >> d) & 1u,
                                      rv[d], eq3, eq);
            }
          }
          if (L.in && (L.contrib || f)) vic[q] |= (uint8_t)((L.contrib ? 1u : 0u) | (f ? 2u : 0u));
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    const int64_t ans = preempt_answer(vic, m, m_eff, !err && !never, fail0, lane);
    if (lane == 0) a.prefix[i] = ans;
  }
}

void launch_preempt(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int T, bool on_equal, const uint8_t* status,
                    const uint64_t* summary, const unsigned long long* partial, const AmountTab& calc, const uint8_t* calc_updated,
                    const uint8_t* error, int64_t* prefix, uint8_t* victims, hipStream_t s) {
  if (n <= 0) return;
  PreemptArgs a{};
  a.pg = pg, a.rows = rows_dev, a.n = n, a.m = m, a.status = status, a.summary = summary, a.partial = partial, a.calc = calc;
  a.calc_updated = calc_updated, a.error = error, a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  const int blocks = (int)(n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_preempt<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_preempt<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_preempt<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
