// kt_kernels_preempt_gangs.hip — the shortest victim prefix that lets a whole gang through (kt_preempt_gangs_launch), gfx950.
//
// The gang form of kt_preempt (kt_kernels_preempt.hip), with the same inputs.  Gang g is the queue positions [gang_off[g],
// gang_off[g + 1]); its members get PreFilter in order and every admitted member reserves (plugin.go:217-239 ->
// reservedResourceAmounts.addPod) on the throttles that affect it, so member j meets, on throttle t, the stored reserved amounts
// plus the amounts of the members before it that t affects.  The verdict is two-dimensional and in closed form: deleting a prefix
// lowers `used` by a prefix sum over the CANDIDATES (per lane, as in kt_preempt), being admitted raises `reserved` by a prefix sum
// over the MEMBERS (wave-uniform) — and the gang passes in S_k iff every (member, affecting throttle, amount) passes its four steps
// against used_k and the reserved prefix of that member.  Judging member j with the reservations of ALL earlier members is exact:
// the gang passes only if every member does, and the first member that fails has met exact sums.
//
//   per gang (one wave, the grid strides) the UNION of the members' affecting throttles chunk by chunk through the 4 KiB LDS list;
//           per throttle the candidates 64 at a time: the wave scans of kt_preempt run ONCE per throttle and block (over the names
//           some affected member requests and a threshold names), then the member loop — wave-uniform: the member's matrix byte,
//           request row and presence are uniform loads — carries the reserved prefix (values, presence word, count, has_count,
//           starting from the stored row) and calls preempt_fails per amount with the lane's `used`, then adds the member's amounts
//           exactly as kt_admit's Reserve does (values of the names it carries, presence of ALL names it carries, count + 1).
//           A row that keeps its stored status depends on the member only: a failing one ends the gang with NONE.  k = 0 is
//           judged once, wave-uniform, and yields the blocker: the first member (lowest queue position over all throttles) that
//           does not pass in S_0 — an Error or invalid member is one.  Nothing is bisected, sums are formed in 128 bits.
//   output  prefix[g] and victims[g][j] as kt_preempt derives them; blocker[g]: queue position, -1 when prefix[g] == 0.
#include "kt_admit_common.h"

namespace kt {

struct PreemptGangArgs {
  const int64_t* gang_off;  // [n_gangs + 1] queue positions
  int64_t n_gangs;
  int64_t* blocker;         // [n_gangs] out
};

// (GangUsed, GangThr and gang_walk are kt_admit_common.h's: the gang reprieve judges with them too)

template <int DT>
__global__ __launch_bounds__(kWave) void kt_preempt_gangs(const PreemptArgs a, const PreemptGangArgs ga) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  const int stride = partial_stride(D);
  const int64_t m = a.m;
  const int64_t m_eff = preempt_m_eff(a, lane);
  for (int64_t gi = blockIdx.x; gi < ga.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = ga.gang_off[gi], i1 = ga.gang_off[gi + 1];
    uint8_t* vic = a.victims + gi * m;
    for (int64_t q = lane; q < m; q += kWave) vic[q] = 0;
    // the first member whose PreFilter is an error or whose row is invalid: the gang has no prefix, and it is not Success in S_0
    int64_t block0 = i1;  // the first member that is not Success when the gang is walked in S_0
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(a.pg.pod_flags[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        block0 = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    bool never = block0 < i1;  // no S_k lets the gang through
    bool fail0 = false;        // some (member, throttle, amount) stops the gang in S_0
    for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      never |= __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        const uint32_t tf = tt.flags[t];
        const bool stored = preempt_row_stored(tf, a.error[t]);
        const AmountTab& th = preempt_threshold(tt, a.calc, tf, a.calc_updated[t]);
        GangThr<DT> g;
        g.eq = eq, g.eq3 = admit_eq3(tf, eq);
        g.th_hc = th.has_count[t] != 0, g.r_hc = tt.reserved.has_count[t] != 0;
        g.th_c = th.count[t], g.r_c = tt.reserved.count[t];
        g.th_p = th.present[t], g.r_p = tt.reserved.present[t];
        const bool c_hc = a.calc.has_count[t] != 0;
        const int64_t c_c = a.calc.count[t];
        const uint32_t c_p = a.calc.present[t];
        const unsigned long long* prow = a.partial + (size_t)t * stride;
        const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
        // the names some affected member requests and a threshold names: the others pass every step of every member
        uint32_t need = 0;
        for (int64_t i = i0; i < i1; ++i) {
          if (a.status[i * (int64_t)T + t] == 0) continue;
          const int64_t p = a.rows[i];
          for (int d = 0; d < D; ++d) need |= a.pg.req[p * DS + d] != 0 ? 1u << d : 0u;
        }
        need &= g.th_p | c_p;
        int64_t cv[DT], tot_v[DT], tot_c[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          g.tv[d] = g.rv[d] = cv[d] = tot_v[d] = tot_c[d] = 0;
          if (d >= D) continue;
          g.tv[d] = th.v[(size_t)t * D + d], g.rv[d] = tt.reserved.v[(size_t)t * D + d];
          if (!((need >> d) & 1u)) continue;
          cv[d] = a.calc.v[(size_t)t * D + d];
          tot_v[d] = (int64_t)prow[d], tot_c[d] = (int64_t)prow[partial_off_presence(D) + d];
        }
        GangUsed<DT> u;
        if (stored) {  // the stored status, in every S_k
          u.c_flag = (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
          u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
#pragma unroll
          for (int d = 0; d < DT; ++d) u.u_v[d] = d < D ? tt.used.v[(size_t)t * D + d] : 0;
          const int64_t first = gang_walk<DT>(a, t, i0, i1, g, u);
          never |= first < i1;
          block0 = first < block0 ? first : block0;
        } else {  // k = 0
          u.u_hc = pods_total > 0, u.u_c = pods_total, u.c_flag = c_hc && u.u_hc && pods_total >= c_c;
          u.flag_m = u.pr_m = 0u;
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            u.u_v[d] = tot_v[d];
            if (!((need >> d) & 1u)) continue;
            const bool u_pr = tot_c[d] > 0;
            u.pr_m |= u_pr ? 1u << d : 0u;
            u.flag_m |= (((c_p >> d) & 1u) && u_pr && tot_v[d] >= cv[d]) ? 1u << d : 0u;
          }
          const int64_t first = gang_walk<DT>(a, t, i0, i1, g, u);
          fail0 |= first < i1;
          block0 = first < block0 ? first : block0;
        }
        // every k >= 1, 64 positions at a time: the scans once, then the members
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
            GangUsed<DT> uk;
            uk.u_c = pods_total - pre_pods, uk.u_hc = uk.u_c > 0, uk.c_flag = c_hc && uk.u_hc && uk.u_c >= c_c;
            uk.flag_m = uk.pr_m = 0u;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              uk.u_v[d] = 0;
              if (!((need >> d) & 1u)) continue;  // (wave-uniform)
              int64_t pre_v;
              uint32_t pre_c;
              preempt_scan_name(a, L, d, lane, car_v[d], car_c[d], &pre_v, &pre_c);
              // presence is exact: the name stays in `used` only while a remaining counted pod carries it
              const bool u_pr = tot_c[d] - (int64_t)pre_c > 0;
              uk.u_v[d] = tot_v[d] - pre_v;
              uk.pr_m |= u_pr ? 1u << d : 0u;
              uk.flag_m |= (((c_p >> d) & 1u) && u_pr && uk.u_v[d] >= cv[d]) ? 1u << d : 0u;
            }
            f = gang_walk<DT>(a, t, i0, i1, g, uk) < i1;
          }
          if (L.in && (L.contrib || f)) vic[q] |= (uint8_t)((L.contrib ? 1u : 0u) | (f ? 2u : 0u));
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    const int64_t ans = preempt_answer(vic, m, m_eff, !never, fail0, lane);
    if (lane == 0) {
      a.prefix[gi] = ans;
      ga.blocker[gi] = (ans == 0 || block0 >= i1) ? -1 : block0;
    }
  }
}

void launch_preempt_gangs(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev, int T,
                          bool on_equal, const uint8_t* status, const uint64_t* summary, const unsigned long long* partial, const AmountTab& calc,
                          const uint8_t* calc_updated, const uint8_t* error, int64_t* prefix, uint8_t* victims, int64_t* blocker, hipStream_t s) {
  if (n_gangs <= 0) return;
  PreemptArgs a{};
  a.pg = pg, a.rows = rows_dev, a.n = n, a.m = m, a.status = status, a.summary = summary, a.partial = partial, a.calc = calc;
  a.calc_updated = calc_updated, a.error = error, a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  const PreemptGangArgs ga{gang_off_dev, n_gangs, blocker};
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_preempt_gangs<4>, dim3(blocks), dim3(kWave), 0, s, a, ga);
  else if (DT == 8) hipLaunchKernelGGL(kt_preempt_gangs<8>, dim3(blocks), dim3(kWave), 0, s, a, ga);
  else hipLaunchKernelGGL(kt_preempt_gangs<16>, dim3(blocks), dim3(kWave), 0, s, a, ga);
}

}  // namespace kt
